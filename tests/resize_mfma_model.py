"""A plain restatement of the integer arithmetic of csrc/resize_mfma.hip (lanczosResize on the i8 matrix pipe), shared by
tests/test_resize_fixed_point.py (CPU) and tests/test_resize_mfma_planted_gpu.py.

The library's part is fennec_amd.resize_fixed_point: S, G and the integer weights Wq of a tap table, as the plan builder
quantises them.  Everything else is restated here in numpy integers and fp64:

    u       = sum_k Wq_k (R_k - 128) + (192 << S) + 2^(S-1) + G       (= sum_k Wq_k R_k + (64 << S) + ...: sum Wq = 2^S)
    flagged = u & (2^S - 1) < 2 G
    byte    = clamp((u >> S) - 64, 0, 255)                             ("unfixed": what the kernel writes before its fix-up)
    ref     = clampF(r * inv), r = r + R_k * fl(255 w_k), taps ascending (resize.go:95-112) -- a flagged sample gets this

on single windows, on whole passes of an image (with the maps of flagged samples), and counted per set of the kernel: an H
set is 16 outputs x one 16-row source slot of one plane, a lane one output x 4 rows; a V set is 16 output rows x 16 outputs
of one plane, a lane one row x 4 px.  A set with more than DENSE flagged lanes makes its workgroup hand its region back.
Searches for windows the guard flags, and for flagged windows whose unfixed byte is not the reference's, are here too."""
from dataclasses import dataclass

import numpy as np

import fennec_amd

DENSE = 16          # RM_DENSE
MAXTAPS = 16        # RM_MAXTAPS


@dataclass
class Plan:
    S: int
    G: int
    first: np.ndarray       # (nout,) first source index
    count: np.ndarray       # (nout,) taps
    wq: np.ndarray          # (nout, 16) int64, zeros behind the taps
    aw: np.ndarray          # (nout, 16) float64: fl(255 w), +0.0 behind the taps (RmEx::aw)
    inv: np.ndarray         # (nout,) 1.0 / a, a = the sum of aw in tap order
    nout: int
    src_n: int
    table: tuple

    @property
    def one(self):
        return 1 << self.S

    @property
    def bias(self):
        """u - sum_k Wq_k R_k"""
        return (64 << self.S) + (1 << (self.S - 1)) + self.G


def plan(table, src_n):
    """the kernel's fixed point of a CSR tap table (off, idx, wt), or None when the library says it is not the kernel's"""
    got = fennec_amd.resize_fixed_point(table, src_n)
    if got is None:
        return None
    S, G, first, count, wq = got
    off, idx, wt = (np.asarray(t) for t in table)
    nout = len(off) - 1
    aw = np.zeros((nout, MAXTAPS), np.float64)
    inv = np.zeros(nout, np.float64)
    for d in range(nout):
        a = 0.0
        for k in range(off[d], off[d + 1]):
            aw[d, k - off[d]] = 255.0 * float(wt[k])
            a += 255.0 * float(wt[k])
        inv[d] = 1.0 / a
    return Plan(S, G, first.astype(np.int64), count.astype(np.int64), wq, aw, inv, nout, int(src_n), (off, idx, wt))


def lanczos_plan(dst, src):
    return plan(fennec_amd.precomputeWeights(dst, src), src)


def make_table(rows):
    """CSR tap table from [(first index, [weights]), ...]"""
    off, idx, wt = [0], [], []
    for first, w in rows:
        idx += list(range(first, first + len(w)))
        wt += list(w)
        off.append(len(idx))
    return np.array(off, np.int32), np.array(idx, np.int32), np.array(wt, np.float64)


def lobe_table(n, x):
    """n outputs over n + 2 source px, taps (-0.3 x, 1 + x, -0.7 x) at d, d + 1, d + 2: with 255 x just under 63 the
    heaviest negative lobes the kernel accepts -- sums from below -60 to above 300.  (Unequal lobes: with two of 31.5 / 255
    every 0/255 window with one lobe lit would be an exact tie, and every set dense.)"""
    return make_table([(d, [-0.3 * x, 1.0 + x, -0.7 * x]) for d in range(n)])


LOBE_X = (63.0 - 1e-6) / 255.0


def clampf(x):
    """clampF (convert.go:149-158) of an fp64 array"""
    x = np.asarray(x, np.float64)
    t = np.trunc(x)
    t = np.where(np.abs(x - t) >= 0.5, t + np.copysign(1.0, x), t)
    return np.clip(t, 0.0, 255.0).astype(np.int64)


def u_of(p, d, win):
    """u of windows (..., 16) of bytes for output d (bytes behind the taps meet zero weights)"""
    return (np.asarray(win, np.int64) * p.wq[d]).sum(axis=-1) + p.bias


def flagged_u(p, u):
    return (u & (p.one - 1)) < 2 * p.G


def unfixed_u(p, u):
    return np.clip((u >> p.S) - 64, 0, 255)


def ref_of(p, d, win):
    """clampF of the reference's fp64 chain for windows (..., 16), always 16 taps as rm_exact_u runs it"""
    win = np.asarray(win)
    r = np.zeros(win.shape[:-1], np.float64)
    for t in range(MAXTAPS):
        r = r + win[..., t].astype(np.float64) * p.aw[d, t]
    return clampf(r * p.inv[d])


def kernel_bytes(p, d, win):
    """(flagged, unfixed byte, reference byte, the byte the kernel leaves) of windows (..., 16)"""
    u = u_of(p, d, win)
    fl, raw, ref = flagged_u(p, u), unfixed_u(p, u), ref_of(p, d, win)
    return fl, raw, ref, np.where(fl, ref, raw)


# -- the "exact uint32" claim: the sum as the matrix pipe forms it -------------------------------------------------------
def digits3(v):
    """rm_digits: three signed base-256 digits, least significant first"""
    out = []
    v = int(v)
    for _ in range(3):
        lo = v % 256
        if lo >= 128:
            lo -= 256
        out.append(lo)
        v = (v - lo) // 256
    assert v == 0, "a fourth digit"
    return out


def _wrap32(v):
    v &= 0xFFFFFFFF
    return v - (1 << 32) if v >= (1 << 31) else v


def u_from_digits(p, d, win):
    """one window's u the way the kernel builds it: three int32 sums of digit x (R - 128), the seed in the lowest, joined by
    rm_comb3 in wrapped int32 arithmetic and read as a uint32"""
    seed = _wrap32((192 << p.S) + (1 << (p.S - 1)) + p.G)
    c = [0, 0, seed]                                    # c2 (hi), c1 (mid), c0 (lo)
    for k in range(int(p.count[d])):
        lo, mid, hi = digits3(p.wq[d, k])
        x = int(win[k]) - 128
        c[0] = _wrap32(c[0] + hi * x)
        c[1] = _wrap32(c[1] + mid * x)
        c[2] = _wrap32(c[2] + lo * x)
    t = _wrap32(c[0] * 256 + c[1])
    return _wrap32(t * 256 + c[2]) & 0xFFFFFFFF


# -- searches -----------------------------------------------------------------------------------------------------------
def near_boundary(p, d, rng, lo_units=8, hi_units=6):
    """Nudged windows of output d: a random window with every value of two of its bytes tried (65 536 nudges), those kept
    whose fraction lies below lo_units G or within hi_units G of 2^S -- the flagged ones and their unflagged neighbours on both
    sides of the rounding boundary.  (n, 16) int64."""
    n = int(p.count[d])
    base = rng.integers(0, 256, MAXTAPS, dtype=np.int64)
    base[n:] = 0
    if n >= 2:
        j, k = (int(v) for v in rng.choice(n, 2, replace=False))
    else:
        j = k = 0
    v = np.arange(256, dtype=np.int64)
    u0 = int(u_of(p, d, base))
    if j != k:
        u = u0 + (p.wq[d, j] * (v - base[j]))[:, None] + (p.wq[d, k] * (v - base[k]))[None, :]
    else:
        u = (u0 + p.wq[d, j] * (v - base[j]))[:, None]
    fr = u & (p.one - 1)
    a, b = np.nonzero((fr < lo_units * p.G) | (fr >= p.one - hi_units * p.G))
    win = np.repeat(base[None, :], len(a), axis=0)
    win[:, j] = v[a]
    if j != k:
        win[:, k] = v[b]
    return win


def find_window(p, d, rng, wrong=True, tries=64):
    """one window (count[d] bytes) of output d that the guard flags -- and, with `wrong`, whose unfixed byte differs from the
    reference's: only the fix-up gives the right byte"""
    for _ in range(tries):
        win = near_boundary(p, d, rng, lo_units=2, hi_units=0)
        if len(win) == 0:
            continue
        fl, raw, ref, _ = kernel_bytes(p, d, win)
        ok = fl & (raw != ref) if wrong else fl
        hit = np.nonzero(ok)[0]
        if len(hit):
            return win[hit[int(rng.integers(0, len(hit)))], :int(p.count[d])].astype(np.uint8)
    raise AssertionError(f"no {'wrong ' if wrong else ''}flagged window found for output {d}")


def extend_profile(p, prof, d, rng):
    """V density: `prof` maps source index -> byte for a run of consecutive indices that ends inside output d's window; the
    missing bytes at the window's end (at most two are searched, the others drawn) are chosen so that output d is flagged.
    Returns the extended dict, or None when no choice flags it."""
    f, n = int(p.first[d]), int(p.count[d])
    free = [s for s in range(f, f + n) if s not in prof]
    assert free and free == list(range(free[0], f + n)), "the profile must end inside the window"
    prof = dict(prof)
    for s in free[:-2]:
        prof[s] = int(rng.integers(0, 256))
    free = free[-2:]
    base = np.zeros(MAXTAPS, np.int64)
    for s in range(f, f + n):
        base[s - f] = prof.get(s, 0)
    v = np.arange(256, dtype=np.int64)
    u = int(u_of(p, d, base)) + (p.wq[d, free[0] - f] * v)[:, None]
    u = u + (p.wq[d, free[-1] - f] * v)[None, :] if len(free) == 2 else u
    a, b = np.nonzero(flagged_u(p, u))
    if len(a) == 0:
        return None
    i = int(rng.integers(0, len(a)))
    prof[free[0]] = int(v[a[i]])
    if len(free) == 2:
        prof[free[1]] = int(v[b[i]])
    return prof


# -- whole passes ---------------------------------------------------------------------------------------------------------
def run_pass(p, a):
    """One pass over a (src_n, M) uint8 array, resampled along axis 0.  Returns (out, flag, wrong): the kernel's bytes
    (nout, M) with the flagged samples recomputed in the reference's arithmetic, the map of flagged samples, and the map of
    flagged samples whose unfixed byte differs."""
    assert a.shape[0] == p.src_n and a.dtype == np.uint8
    dense = np.zeros((p.nout, p.src_n), np.float64)
    for d in range(p.nout):
        dense[d, p.first[d]:p.first[d] + p.count[d]] = p.wq[d, :p.count[d]]
    # products below 2^31, sums below 2^53: the fp64 matrix product is the exact integer one
    u = (dense @ a.astype(np.float64)).astype(np.int64) + p.bias
    flag = flagged_u(p, u)
    out = unfixed_u(p, u)
    wrong = np.zeros_like(flag)
    for d, m in zip(*np.nonzero(flag)):
        win = np.zeros(MAXTAPS, np.int64)
        win[:p.count[d]] = a[p.first[d]:p.first[d] + p.count[d], m]
        ref = int(ref_of(p, d, win))
        wrong[d, m] = ref != out[d, m]
        out[d, m] = ref
    return out.astype(np.uint8), flag, wrong


@dataclass
class Image:
    out: np.ndarray         # (dstH, dstW, 4) what the kernel must leave (alpha 255)
    tmp: np.ndarray         # (srcH, dstW, 3) the intermediate
    flag_h: np.ndarray      # (srcH, dstW, 3)
    wrong_h: np.ndarray
    flag_v: np.ndarray      # (dstH, dstW, 3)
    wrong_v: np.ndarray
    sets_h: np.ndarray      # (H groups of 16 outputs, source slots, 3) flagged lanes per H set; slots from slot0 on
    sets_v: np.ndarray      # (V groups of 16 rows, groups of 16 outputs, 3) flagged lanes per V set
    slot0: int


def run_image(ph, pv, img):
    """both passes of an opaque (srcH, srcW, 4) image with the plans of its H and V tables, and the flagged lanes of every set"""
    sh, sw = img.shape[:2]
    assert (img[..., 3] == 255).all() and sw == ph.src_n and sh == pv.src_n
    t, fh, wh = run_pass(ph, np.ascontiguousarray(img[..., :3].transpose(1, 0, 2)).reshape(sw, sh * 3))
    dw, dh = ph.nout, pv.nout
    tmp = np.ascontiguousarray(t.reshape(dw, sh, 3).transpose(1, 0, 2))
    fh = fh.reshape(dw, sh, 3).transpose(1, 0, 2)
    wh = wh.reshape(dw, sh, 3).transpose(1, 0, 2)
    o, fv, wv = run_pass(pv, tmp.reshape(sh, dw * 3))
    out = np.full((dh, dw, 4), 255, np.uint8)
    out[..., :3] = o.reshape(dh, dw, 3)
    fv, wv = fv.reshape(dh, dw, 3), wv.reshape(dh, dw, 3)
    # H sets: every source slot a V group needs (vb .. need of the plan's groups), rows clamped to srcH - 1 as hload does
    slot0 = int(pv.first.min()) >> 4
    slot1 = int((pv.first + pv.count - 1).max()) >> 4
    rows = np.minimum(16 * np.arange(slot0, slot1 + 1)[:, None] + np.arange(16)[None, :], sh - 1)
    ng = (dw + 15) // 16
    padded = np.zeros((rows.shape[0], 16, 16 * ng, 3), bool)
    padded[:, :, :dw] = fh[rows]
    lanes = padded.reshape(rows.shape[0], 4, 4, ng, 16, 3).any(axis=2)            # slot, 4-row group, H group, output, plane
    sets_h = lanes.sum(axis=(1, 3)).transpose(1, 0, 2)
    # V sets
    nvg = (dh + 15) // 16
    padded = np.zeros((16 * nvg, 16 * ng, 3), bool)
    padded[:dh, :dw] = fv
    lanes = padded.reshape(nvg, 16, ng, 4, 4, 3).any(axis=4)                      # V group, row, H group, 4-px group, plane
    sets_v = lanes.sum(axis=(1, 3))
    return Image(out, tmp, fh, wh, fv, wv, sets_h, sets_v, slot0)
