"""The crafted files that hold the JPEG decoder's BACK half -- the DC sums, the dequantisation, the IDCT, the clamp, the placement
of blocks in the planes -- where its int32 arithmetic leaves the range every ordinary file stays in (tests/jpeg_craft.py writes
them, tests/jpeg_backend_ref.py says what image/jpeg makes of them).  One place for test_jpeg_backend.py (the reference, the
oracle) and test_jpeg_backend_gpu.py (the device).  Groups:
  a  DC chains that leave 16 bits (one component; Cb only, Cr only at 4:2:0), one that goes on until the IDCT wraps, and restart
     intervals that do not divide the MCU row, for one component and the six samplings
  b  DC x 255 of a chain near 2047 k with AC beside it, the DCs chosen so that the wrapped block lands inside 0 .. 255
  c  4160 blocks of +2047 under a quantiser of 255: the product itself passes 2^31
  d  quantisers up to 255, |AC| <= 1023: blocks in which the IDCT wraps
  e  AC sizes 11 .. 15, among them rows whose only entry is their first, of 2^20 and more after dequantisation
  f  samples as far beyond the clamp as int32 >> 14 can be, in both directions
A wrapped sample is as good as random in +-2^17, so blind blocks saturate and a comparison of them shows little: the blocks of
(b), (d) and (e) are FOUND, by a seeded search with the reference -- large coefficients first, then the DC that brings the level
most samples share inside the clamp, then a small coefficient for texture -- and kept when the reference says that an operation
wrapped and that 16 or more of the 64 samples are neither 0 nor 255 (the tests assert both again)."""
from __future__ import annotations

import functools

import numpy as np

import jpeg_backend_ref as ref
import jpeg_craft as jc
from jpeg_craft_cases import K_AC, K_DC, K_DC_C, _bits, grey_dims

ZIG = jc.ZIG
SAMPLINGS = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "440": (1, 2), "411": (4, 1), "410": (4, 2)}
MIN_UNSATURATED = 16

# (e) every (run, size) pair up to size 15, EOB and ZRL: fifteen codes of 4 bits (EOB, ZRL, the runs 0 .. 12 at size 15), the
# other 227 behind the prefix 1111 at 12 bits (the all-ones code stays free)
_E_SHORT = [0x00, 0xf0] + [(r << 4) | 15 for r in range(13)]
E_AC = jc.Table(_bits(L4=15, L12=227), _E_SHORT + [(r << 4) | s for s in range(1, 16) for r in range(16) if ((r << 4) | s) not in _E_SHORT])

Q_ONES = [1] * 64
Q_DC255 = [255] + [1] * 63
Q_255 = [255] * 64
# (d) both tables large, neither flat (zig-zag order)
Q_D_Y = [255 - (7 * k) % 64 for k in range(64)]
Q_D_C = [255 - (11 * k) % 32 for k in range(64)]
Q_D_Y[0] = Q_D_C[0] = 255


def natural_q(q_zig):
    q = np.zeros(64, np.int64)
    q[ZIG] = q_zig
    return q


def to_zigzag(nat):
    return np.asarray(nat)[..., ZIG]


def dc_only_block_wraps(dcq):
    """a block of nothing but a dequantised DC: row 0 takes the shortcut (dcq << 3), the column pass forms (that << 8) + 8192 and
    only shifts afterwards -- it wraps exactly when dcq * 2048 + 8192 leaves int32"""
    v = np.asarray(dcq, np.int64) * 2048
    return (v + 8192 > 2**31 - 1) | (v < -2**31)


class Case:
    """cr: the Crafted file; zz: (blocks, 64) as coded, zig-zag order, position 0 the DC difference; kept: the blocks the
    unsaturated-sample condition is asserted for; leaves16: a DC of the file lies beyond int16"""

    def __init__(self, name, coef, w, h, dc_tabs, ac_tabs, sampling=None, qtabs=None, restart=0, kept=(), max_ac_size=10):
        coef = np.asarray(coef, np.int64)
        self.name, self.group = name, name[0]
        self.cr = jc.encode(coef, w, h, dc_tabs, ac_tabs, sampling=sampling, qtabs=qtabs, restart=restart, max_ac_size=max_ac_size)
        self.data = self.cr.data
        self.zz = coef.copy()
        self.zz[:, 0] = self.cr.dcdiff
        self.coef = coef
        self.w, self.h, self.sampling, self.restart = w, h, sampling, restart
        self.qtabs = [list(q) for q in (qtabs or [Q_ONES])]
        self.kept = np.asarray(kept, np.int64)
        self.leaves16 = bool(np.abs(coef[:, 0]).max() > 32767)

    @functools.cached_property
    def ref(self):
        return ref.decode(self.zz, self.qtabs, self.w, self.h, self.sampling, self.restart)


# ------------------------------------------------------------------------------------------------------------ the search
def _sign(rng, n):
    return np.where(rng.integers(0, 2, n) == 1, 1, -1)


def _tune(nat, q_nat, rng, dc_max=1023, keep_row=None):
    """nat: (n, 64) candidates in natural order with their large coefficients set and the DC free.  Sets the DC that brings the
    level most samples share to the middle of 0 .. 255 and a coefficient of +-1 or +-2 where there was none (outside row
    keep_row); returns the candidates (with and without that texture) and which of them hold the condition."""
    n = len(nat)
    pre = ref.idct(nat * q_nat)[0]
    srt = np.sort(pre, axis=1)
    # per candidate: the window of 200 levels that holds most samples
    cnt = np.stack([((srt >= srt[:, j:j + 1]) & (srt <= srt[:, j:j + 1] + 200)).sum(axis=1) for j in range(64)], axis=1)
    best = cnt.argmax(axis=1)
    level = srt[np.arange(n), best] + 100
    dc = np.rint(-8.0 * level / q_nat[0]).astype(np.int64)
    nat = nat.copy()
    nat[:, 0] = np.clip(dc, -dc_max, dc_max)
    tex = nat.copy()
    for i in range(n):
        free = np.flatnonzero((tex[i] == 0) & (np.arange(64) // 8 != keep_row))
        tex[i, int(rng.choice(free))] = int(rng.choice([-2, -1, 1, 2]))
    out = []
    for cand in (tex, nat):
        p, hit = ref.idct(cand * q_nat)
        out.append((cand, hit & (ref.unsaturated(ref.level_shift(p)) >= MIN_UNSATURATED) & (np.abs(dc) <= dc_max)))
    return out


def search(seed, want, q_zig, vmin, vmax, first_of_row=None, batch=1500):
    """`want` blocks (natural order, absolute DC within +-1023) under the tables q_zig whose one or two large coefficients lie in
    vmin .. vmax by magnitude.  first_of_row: the natural position 8 r that must be the only entry of its row, at 2^20 or more
    after dequantisation."""
    rng = np.random.default_rng(seed)
    q_nat = natural_q(q_zig)
    found = []
    for _ in range(40):
        nat = np.zeros((batch, 64), np.int64)
        k1 = np.full(batch, first_of_row) if first_of_row else rng.integers(1, 64, batch)
        lo = np.maximum(vmin, -(-(1 << 20) // q_nat[k1])) if first_of_row else np.full(batch, vmin)
        nat[np.arange(batch), k1] = rng.integers(lo, vmax + 1) * _sign(rng, batch)
        k2 = rng.integers(1, 64, batch)
        two = (rng.random(batch) < 0.5) & (k2 // 8 != k1 // 8)
        nat[np.flatnonzero(two), k2[two]] = (rng.integers(vmin, vmax + 1, batch) * _sign(rng, batch))[two]
        (tex, ok_tex), (plain, ok_plain) = _tune(nat, q_nat, rng, keep_row=first_of_row // 8 if first_of_row else None)
        for i in range(batch):
            if ok_tex[i] or ok_plain[i]:
                found.append(tex[i] if ok_tex[i] else plain[i])
                if len(found) == want:
                    return np.array(found)
    raise AssertionError(f"the search found {len(found)} of {want} blocks")


# ---------------------------------------------------------------------------------------------------------------- (a)
def _grey_chain(name, diffs, **kw):
    coef = np.zeros((len(diffs), 64), np.int64)
    coef[:, 0] = np.cumsum(diffs)
    w, h = grey_dims(len(diffs))
    return Case(name, coef, w, h, [K_DC], [K_AC], **kw)


def _distinct_dcs(n, seed, step=16):
    """n distinct DCs, odd multiples of step / 2 inside +-n step / 2: as samples under a quantiser of 1 they are step / 8 levels
    apart; none is 0, so a prediction carried over a restart boundary always shows"""
    return (np.random.default_rng(seed).permutation(n) - n // 2) * step + step // 2


@functools.lru_cache(None)
def group_a():
    out = {}
    out["a_up_40"] = _grey_chain("a_up_40", [2047] * 40)
    out["a_down_40"] = _grey_chain("a_down_40", [-2047] * 40)
    out["a_cross_and_back"] = _grey_chain("a_cross_and_back", [2047] * 20 + [-2047] * 40 + [2047] * 20)
    out["a_until_the_idct_wraps"] = _grey_chain("a_until_the_idct_wraps", [2047] * 640)
    # 4:2:0, 8 x 5 MCUs: one chroma component crosses +-32767 and comes back, Y and the other one stay quiet
    for name, loud in (("a_cb_only", 4), ("a_cr_only", 5)):
        coef = np.zeros((40 * 6, 64), np.int64)
        slot = np.arange(240) % 6
        coef[slot < 4, 0] = _distinct_dcs(160, 11, step=8)
        coef[slot == 9 - loud, 0] = 8 * (np.arange(40) % 7) - 24
        coef[slot == loud, 0] = np.cumsum([2047] * 20 + [-2047] * 20) * (1 if loud == 4 else -1)
        out[name] = Case(name, coef, 128, 80, [K_DC, K_DC_C], [K_AC], sampling=(2, 2))
    # 3 x 3 MCUs, an interval of 2: boundaries inside an MCU row and across its end
    for tag, samp in [("grey", None)] + list(SAMPLINGS.items()):
        hy, vy = samp or (1, 1)
        per = hy * vy + (2 if samp else 0)
        coef = np.zeros((9 * per, 64), np.int64)
        coef[:, 0] = _distinct_dcs(9 * per, per)
        name = "a_rst_" + tag
        out[name] = Case(name, coef, 24 * hy - 3, 24 * vy - 5, [K_DC, K_DC_C], [K_AC], sampling=samp, restart=2)
    return out


# ---------------------------------------------------------------------------------------------------------------- (b)
def _b_chain(name, sign, seed, per_cluster=2):
    """255 x DC wraps in the IDCT's << 11 once it reaches 2^20 -- from 2047 x 3 on -- and what is left of it is the product's low
    21 bits, an eighth of them as the sample's level: the DCs of this chain are those up to 2047 x 40 whose product lies within
    800 of a multiple of 2^21 (they cluster every 8224.5, about 2047 x 4), two of each cluster, with two AC values beside them
    under a quantiser of 1; plain steps of 2047 lead from one to the next"""
    rng = np.random.default_rng(seed)
    q_nat = natural_q(Q_DC255)
    dc = np.arange(3 * 2047, 40 * 2047 + 1)
    low = (dc * 255 + 2**20) % 2**21 - 2**20
    dc = sign * np.repeat(dc[np.abs(low) <= 800], 4)                      # four draws of the AC values each
    nat = np.zeros((len(dc), 64), np.int64)
    nat[:, 0] = dc
    for _ in range(2):
        nat[np.arange(len(dc)), rng.integers(1, 64, len(dc))] = rng.integers(1, 1024, len(dc)) * _sign(rng, len(dc))
    pre, hit = ref.idct(nat * q_nat)
    ok = np.flatnonzero(hit & (ref.unsaturated(ref.level_shift(pre)) >= MIN_UNSATURATED))
    ok = ok[np.unique(dc[ok], return_index=True)[1]]                      # one draw per DC
    ok = ok[np.argsort(np.abs(dc[ok]), kind="stable")]                    # outward from 0
    cluster = np.rint(np.abs(dc[ok]) / 8224.5).astype(int)
    pick = [i for n, i in enumerate(ok) if (cluster[:n] == cluster[n]).sum() < per_cluster]
    assert len(set(cluster.tolist())) == 9 and len(pick) == 9 * per_cluster, (cluster, len(pick))
    blocks, kept, cur = [], [], 0
    for i in pick:
        while abs(int(dc[i]) - cur) > 2047:                                # climb there in plain steps
            cur += 2047 * sign
            blocks.append(np.concatenate([[cur], np.zeros(63, np.int64)]))
        cur = int(dc[i])
        kept.append(len(blocks))
        blocks.append(nat[i])
    coef = to_zigzag(np.array(blocks))
    w, h = grey_dims(len(coef))
    return Case(name, coef, w, h, [K_DC], [K_AC], qtabs=[Q_DC255], kept=kept)


@functools.lru_cache(None)
def group_b():
    return {"b_up": _b_chain("b_up", 1, 21), "b_down": _b_chain("b_down", -1, 22)}


# ---------------------------------------------------------------------------------------------------------------- (c)
@functools.lru_cache(None)
def group_c():
    coef = np.zeros((65 * 64, 64), np.int64)
    coef[:, 0] = 2047 * np.arange(1, 65 * 64 + 1)
    return {"c_product_wraps": Case("c_product_wraps", coef, 520, 512, [K_DC], [K_AC], qtabs=[Q_DC255])}


# ---------------------------------------------------------------------------------------------------------------- (d)
@functools.lru_cache(None)
def group_d():
    out = {}
    nat = search(31, 24, Q_D_Y, 512, 1023)
    out["d_grey"] = Case("d_grey", to_zigzag(nat), 8 * 24, 8, [K_DC], [K_AC], qtabs=[Q_D_Y], kept=range(24))
    y, c = search(32, 16, Q_D_Y, 512, 1023), search(33, 8, Q_D_C, 512, 1023)
    blocks = []
    for m in range(4):
        blocks += [y[4 * m + j] for j in range(4)] + [c[m], c[4 + m]]
    out["d_420"] = Case("d_420", to_zigzag(np.array(blocks)), 32, 32, [K_DC, K_DC_C], [K_AC], sampling=(2, 2), qtabs=[Q_D_Y, Q_D_C],
                        kept=range(24))
    return out


# ---------------------------------------------------------------------------------------------------------------- (e)
E_PER_SIZE = 4                             # blocks whose large coefficients are of size 11, of size 12 .. 15
E_FIRST_OF_ROW = 2                         # blocks per natural position 8, 16 .. 56


@functools.lru_cache(None)
def group_e():
    nat = [search(40 + size, E_PER_SIZE, Q_255, 1 << (size - 1), (1 << size) - 1) for size in range(11, 16)]
    for r in range(1, 8):
        nat.append(search(50 + r, E_FIRST_OF_ROW, Q_255, 1024, 32767, first_of_row=8 * r))
    nat = np.concatenate(nat)
    return {"e_grey": Case("e_grey", to_zigzag(nat), 8 * len(nat), 8, [K_DC], [E_AC], qtabs=[Q_255], kept=range(len(nat)), max_ac_size=15)}


def e_first_of_row_blocks():
    """(index in e_grey, natural position) of the blocks whose row holds its first entry only"""
    return [(5 * E_PER_SIZE + E_FIRST_OF_ROW * (r - 1) + j, 8 * r) for r in range(1, 8) for j in range(E_FIRST_OF_ROW)]


# ---------------------------------------------------------------------------------------------------------------- (f)
FAR = 1 << 16                              # half of what int32 >> 14 can hold: see test_f_*


@functools.lru_cache(None)
def group_f():
    rng = np.random.default_rng(61)
    q_nat = natural_q(Q_255)
    nat = np.zeros((400, 64), np.int64)
    for _ in range(3):
        nat[np.arange(400), rng.integers(0, 64, 400)] = rng.integers(512, 1024, 400) * _sign(rng, 400)
    nat[:, 0] = np.clip(nat[:, 0], -1023, 1023)
    pre = ref.idct(nat * q_nat)[0]
    far = np.flatnonzero((pre.min(axis=1) < -FAR) & (pre.max(axis=1) > FAR) & (ref.unsaturated(ref.level_shift(pre)) == 0))[:6]
    assert len(far) == 6
    return {"f_far_clamp": Case("f_far_clamp", to_zigzag(nat[far]), 48, 8, [K_DC], [K_AC], qtabs=[Q_255])}


def all_cases():
    out = {}
    for g in (group_a, group_b, group_c, group_d, group_e, group_f):
        out.update(g())
    return out
