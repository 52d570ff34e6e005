"""The arithmetic of the matrix-pipe resize (csrc/resize_mfma.hip) on the CPU: what fnx_resize_fixed_point says the plan
builder makes of a tap table (S, G, the integer weights), the bound the rounding guard rests on recomputed in exact
fractions, the claim that the sum is an exact uint32, and -- replayed in integers (tests/resize_mfma_model.py) -- the claim
that a sample the guard does not flag is the byte of the reference's clampF(fp64 chain) (resize.go:95-112).  No GPU.

S / G as measured here: 320 <- 640: 23 / 426; 301 <- 641: 23 / 617; 460 <- 1000: 23 / 585; 1280 <- 640: 22 / 206; 400 <- 1000:
23 / 432; 512 <- 640: 23 / 250.  1000 <- 479 and 195 <- 130 quantise to 22 / 350 and 22 / 277, but the library REFUSES both, and
rightly: a non-integer upscale has phases whose negative lobes sum to 69.3 / 255, past the 63 / 255 the sums' offset of 64
allows (test_two_upscales_are_refused_for_their_lobes).  Flagged share on uniform bytes: 2.7e-5 (1280 <- 640) .. 1.5e-4 (301 <- 641),
2 G / 2^S being 6.0e-5 .. 1.5e-4; about half of the flagged nudged windows have a wrong unfixed byte."""
from fractions import Fraction

import numpy as np
import pytest

import fennec_amd
import resize_mfma_model as M

# dst <- src: the issue's pairs the kernel covers, 2.5:1 (15 taps), 1.25:1, and two whose nout is no multiple of 16
PAIRS = [(320, 640), (301, 641), (460, 1000), (1280, 640), (400, 1000), (512, 640), (203, 450), (1034, 517)]
KNOWN = {(320, 640): (23, 426), (301, 641): (23, 617), (460, 1000): (23, 585), (1280, 640): (22, 206)}
REFUSED = {(1000, 479): (22, 350), (195, 130): (22, 277)}
NWIN = 20000

_plans = {}


def _plan(pair):
    if pair not in _plans:
        p = M.lanczos_plan(*pair)
        assert p is not None, pair
        _plans[pair] = p
    return _plans[pair]


def _real_weights(p, d):
    """W_k 2^S of output d as exact fractions: W_k = fl(255 w_k) * inv"""
    return [Fraction(float(p.aw[d, k])) * Fraction(float(p.inv[d])) * p.one for k in range(int(p.count[d]))]


def _restated_S_G(table):
    """the quantisation alone, restated in x86 long double: no domain check.  (S, G, largest 255 x negative lobes)"""
    L = np.longdouble
    off, idx, wt = table
    W, lobes = [], L(0)
    for d in range(len(off) - 1):
        aw = [255.0 * float(w) for w in wt[off[d]:off[d + 1]]]
        a = 0.0
        for v in aw:
            a += v
        W.append(np.array([L(v) * L(1.0 / a) for v in aw], dtype=L))
        lobes = max(lobes, 255 * -W[-1][W[-1] < 0].sum())
    S = 23 if max(np.abs(w).max() for w in W) * L(8388608) <= L(8355000) else 22
    emax = L(0)
    for w in W:
        ws = w * L(2) ** S
        q = np.floor(ws)
        rem = (1 << S) - int(q.sum())
        q[np.argsort(-(ws - q), kind="stable")[:rem]] += 1
        dl = q - ws
        emax = max(emax, 255 * max(dl[dl > 0].sum(), -dl[dl < 0].sum()))
    return S, int(np.ceil(emax)) + 2, float(lobes)


@pytest.mark.parametrize("pair", PAIRS)
def test_plan_values(pair):
    p = _plan(pair)
    if pair in KNOWN:
        assert (p.S, p.G) == KNOWN[pair]
    assert (p.S, p.G) == _restated_S_G(p.table)[:2]
    off, idx, _ = p.table
    assert np.array_equal(p.first, idx[off[:-1]]) and np.array_equal(p.count, np.diff(off))
    assert (p.wq.sum(axis=1) == p.one).all() and int(np.abs(p.wq).max()) <= 8355711
    assert (p.wq[np.arange(16)[None, :] >= p.count[:, None]] == 0).all()
    wmax, worst = Fraction(0), Fraction(0)
    for d in range(p.nout):
        W = _real_weights(p, d)
        wmax = max(wmax, max(abs(w) for w in W))
        diffs = [Fraction(int(q)) - w for q, w in zip(p.wq[d], W)]
        assert all(abs(x) < 1 for x in diffs)                     # each Wq is W 2^S rounded down or up
        worst = max(worst, sum(x for x in diffs if x > 0), -sum(x for x in diffs if x < 0))
    assert (p.S == 23) == (wmax * (1 << 23) / p.one <= 8355000)
    e = 255 * worst
    assert p.G == (e.numerator + e.denominator - 1) // e.denominator + 2


@pytest.mark.parametrize("pair", sorted(REFUSED))
def test_two_upscales_are_refused_for_their_lobes(pair):
    """quantised alone these tables give the S and G an earlier restatement listed; the library refuses them because an
    output's negative lobes pass 63 / 255: its sum could fall below -64, and u would not be a uint32"""
    table = fennec_amd.precomputeWeights(*pair)
    S, G, lobes = _restated_S_G(table)
    assert (S, G) == REFUSED[pair] and lobes > 63.0
    assert fennec_amd.resize_fixed_point(table, pair[1]) is None


@pytest.mark.parametrize("pair", PAIRS)
def test_the_sum_is_an_exact_uint32(pair):
    """the all-0/255 windows with the smallest and the largest sum: u lies in [0, 2^32), and three signed digits joined in
    wrapped int32 arithmetic (rm_digits, rm_comb3) give the same number"""
    p = _plan(pair)
    for d in range(p.nout):
        for win in (np.where(p.wq[d] < 0, 255, 0), np.where(p.wq[d] > 0, 255, 0)):
            u = int(M.u_of(p, d, win))
            assert 0 <= u < 1 << 32
            assert M.u_from_digits(p, d, win) == u
    rng = np.random.default_rng(5)
    for d in rng.integers(0, p.nout, 64):
        win = rng.integers(0, 256, 16)
        assert M.u_from_digits(p, d, win) == int(M.u_of(p, d, win))


def _sweep(p, win):
    """every output of the plan against the same windows (n, 16): an unflagged sample must be the reference's byte.
    Returns how many samples were flagged."""
    wf = win.astype(np.float64)
    nflag = 0
    for c0 in range(0, p.nout, 256):
        sl = slice(c0, min(c0 + 256, p.nout))
        u = (wf @ p.wq[sl].T.astype(np.float64)).astype(np.int64) + p.bias       # exact: sums below 2^53
        fl, raw = M.flagged_u(p, u), M.unfixed_u(p, u)
        r = np.zeros(u.shape)
        for t in range(16):                                   # r = r + R * aw, taps ascending (resize.go:101)
            r = r + wf[:, t:t + 1] * p.aw[sl, t][None, :]
        ref = M.clampf(r * p.inv[sl][None, :])
        bad = np.nonzero(~fl & (raw != ref))
        assert len(bad[0]) == 0, (c0 + bad[1][:3], win[bad[0][:3]])
        nflag += int(fl.sum())
    return nflag


def _adversarial(p, d):
    """R = 255 where Wq > W 2^S, else 0 (the integer sum as far above the real one as bytes allow), and its complement"""
    up = np.zeros(16, np.int64)
    for k, w in enumerate(_real_weights(p, d)):
        up[k] = 255 if Fraction(int(p.wq[d, k])) > w else 0
    down = 255 - up
    down[int(p.count[d]):] = 0
    return np.stack([up, down])


@pytest.mark.parametrize("pair", PAIRS)
def test_unflagged_samples_are_the_reference_s(pair):
    p = _plan(pair)
    rng = np.random.default_rng(p.nout * 4099 + p.src_n)
    nflag = _sweep(p, rng.integers(0, 256, (NWIN, 16), dtype=np.int64))
    share = nflag / (NWIN * p.nout)
    print(f"{pair}: S {p.S} G {p.G}, flagged share {share:.3e} on uniform bytes, 2G/2^S = {2 * p.G / p.one:.3e}")
    assert nflag >= 1 and share <= 4 * 2 * p.G / p.one
    _sweep(p, 255 * rng.integers(0, 2, (4096, 16), dtype=np.int64))
    nudged = flagged = wrong = 0
    for d in range(p.nout):
        win = np.concatenate([_adversarial(p, d), M.near_boundary(p, d, rng)])
        fl, raw, ref, _ = M.kernel_bytes(p, d, win)
        bad = np.nonzero(~fl & (raw != ref))[0]
        assert len(bad) == 0, (d, win[bad[:3]])
        nudged += len(win) - 2
        flagged += int(fl[2:].sum())
        wrong += int((fl[2:] & (raw[2:] != ref[2:])).sum())
    print(f"{pair}: {nudged} nudged windows, {flagged} flagged, {wrong} of them with a wrong unfixed byte")
    assert flagged >= 1 and wrong >= 1 and nudged > 2 * flagged, "both sides of the boundary must be in the set"


def test_the_model_s_image_is_the_oracle_s(orc):
    """the model the GPU test plants with, both passes and the fix-ups, on noise: down, up, and an odd geometry"""
    from fennec_amd import synth
    for (w, h, dw, dh) in ((160, 120, 80, 60), (96, 64, 192, 128), (211, 97, 101, 47)):
        img = synth.noise_image(w, h, w + dh, alpha=True)
        img[..., 3] = 255
        r = M.run_image(M.lanczos_plan(dw, w), M.lanczos_plan(dh, h), img)
        assert np.array_equal(r.out, orc.lanczos_resize(img, dw, dh))
        assert r.sets_h.max() <= M.DENSE and r.sets_v.max() <= M.DENSE


# -- hand-made tables on both sides of each limit ------------------------------------------------------------------------
def _filled(special, n=16, src_n=32):
    """n outputs, `special` (first, weights) as output 3, two taps of 1/2 elsewhere"""
    rows = [(min(d, src_n - 2), [0.5, 0.5]) for d in range(n)]
    rows[3] = special
    return M.make_table(rows), src_n


def _w_for(target):
    """the smallest double w with fl(255 w) >= target, and its predecessor"""
    w = target / 255.0
    while 255.0 * w < target:
        w = np.nextafter(w, np.inf)
    while 255.0 * np.nextafter(w, -np.inf) >= target:
        w = np.nextafter(w, -np.inf)
    return float(w), float(np.nextafter(w, -np.inf))


def test_domain_limits():
    fp = fennec_amd.resize_fixed_point
    assert fp(*_filled((0, [1 / 16] * 16))) is not None
    assert fp(*_filled((0, [1 / 17] * 17))) is None                                    # 17 taps
    gap = M.make_table([(min(d, 29), [0.25, 0.5, 0.25]) for d in range(16)])
    assert fp(gap, 32) is not None
    gap[1][3 * 3 + 2] += 1                                                                # output 3: indices 3, 4, 6
    assert fp(gap, 32) is None
    lo_in, lo_out = _w_for(254.5)
    hi_out, hi_in = _w_for(255.5)
    assert 255.0 * lo_in >= 254.5 > 255.0 * lo_out and 255.0 * hi_in < 255.5 <= 255.0 * hi_out
    for w, ok in ((lo_in, True), (lo_out, False), (hi_in, True), (hi_out, False)):       # a in [254.5, 255.5): clampF(a) == 255
        assert (fp(*_filled((5, [w]))) is not None) == ok, w
    for x, ok in (((63.0 - 1e-6) / 255.0, True), ((63.0 + 1e-6) / 255.0, False)):         # 255 x negative lobes against 63
        assert (fp(*_filled((5, [-x / 2, 1.0 + x, -x / 2]))) is not None) == ok, x
    # a weight three signed digits do not reach (|Wq| > 8355711 at S = 22: W > 1.992).  The weights of an output sum to one, so
    # such a weight brings negative lobes of at least 0.99 with it: the lobe limit refuses the table first, and does
    assert fp(*_filled((5, [-0.5, 2.0, -0.5]))) is None
    assert fp(*_filled((5, [-0.12, 1.24, -0.12]))) is not None
    # S: 23 up to |W| 2^23 = 8355000, 22 beyond
    w = 8355000 / 8388608
    assert fp(*_filled((5, [w - 1e-9, 1 - w + 1e-9])))[0] == 23 and fp(*_filled((5, [w + 1e-9, 1 - w - 1e-9])))[0] == 22
    for n, src_n, ok in ((16, 16, True), (15, 16, False), (16, 15, False), (15, 15, False)):
        rows = [(min(d, src_n - 2), [0.5, 0.5]) for d in range(n)]
        assert (fp(M.make_table(rows), src_n) is not None) == ok, (n, src_n)
    with pytest.raises(fennec_amd.FennecError):                                          # an index outside the source
        fp(M.make_table([(d, [0.5, 0.5]) for d in range(16)]), 16)


def test_lobe_heavy_table_near_the_offset_and_the_saturation():
    """taps (-0.3 x, 1 + x, -0.7 x) with 255 x just under 63: sums from below -60 to above 300 -- the only table here whose u comes
    near 0 and near 2^32 / 2, and whose bytes saturate at both ends"""
    p = M.plan(M.lobe_table(64, M.LOBE_X), 66)
    assert p is not None and p.S == 22
    d = 20
    lo, hi = np.where(p.wq[d] < 0, 255, 0), np.where(p.wq[d] > 0, 255, 0)
    xs = [(int(M.u_of(p, d, w)) >> p.S) - 64 for w in (lo, hi)]
    assert xs[0] < -60 and xs[1] > 300, xs
    for dd in range(p.nout):
        for w in (np.where(p.wq[dd] < 0, 255, 0), np.where(p.wq[dd] > 0, 255, 0)):
            u = int(M.u_of(p, dd, w))
            assert 0 <= u < 1 << 32 and M.u_from_digits(p, dd, w) == u
    rng = np.random.default_rng(63)
    nflag = _sweep(p, rng.integers(0, 256, (NWIN, 16), dtype=np.int64))
    assert nflag >= 1              # (no cap: three taps of n / 2550 put many more sums next to a tie than a Lanczos table does)
    _sweep(p, 255 * rng.integers(0, 2, (4096, 16), dtype=np.int64))
    # every 0/255 window of the three taps, and windows next to the boundary
    cube = 255 * np.array([[a, b, c] + [0] * 13 for a in (0, 1) for b in (0, 1) for c in (0, 1)], dtype=np.int64)
    sat = set()
    for dd in range(p.nout):
        win = np.concatenate([cube, _adversarial(p, dd), M.near_boundary(p, dd, rng)])
        fl, raw, ref, _ = M.kernel_bytes(p, dd, win)
        assert not (~fl & (raw != ref)).any(), dd
        sat |= set(ref[:8].tolist())
    assert {0, 255} <= sat
