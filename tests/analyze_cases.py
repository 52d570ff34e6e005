"""Crafted inputs for Analyze (fennec_amd/csrc/analyze.hip, both of its routes) and an exact classifier of what they plant.

analyze.hip promises exact integers: every histogram bin (int(lum + 0.5) of an fp64 luminance in the reference's operation
order), the Sobel edge count (sqrt(gx^2 + gy^2) > 30 in fp64), the sampled colour count (a device hash set), and the sizes of
its three sampling grids.  Photographs and noise put next to nothing on the values where those promises can break.  The images
here do:

    lum_ties()           every colour whose luminance is k + 1/2 in real arithmetic -- only the rounding of the fp64 chain
                         decides its bin, and every other evaluation (contracted, reassociated, fp32, integer) decides
                         thousands of them differently
    sobel_ties()         3 x 3 neighbourhoods whose Sobel magnitude is exactly 30 in real arithmetic
    colour_grid()        colours planted on the first, the last and chosen sampled indices of the colour walk, decoys on
                         unsampled ones, counts that end at 1023, 1024 and 1025, before and after the staged route's hand-over
    colliding_colours()  pixels inverted from the slot function so that they share one home slot at the table's end: one probe
                         chain that wraps through slot 0, merged with the chains of two neighbouring homes
    contrast_grid()      0 / 255 outliers on the last row and column of the contrast grid and one pixel off it
    edge_grid()          isolated white pixels around the last sampled Sobel centre and the first unsampled one

What each image must give is stated here from the definitions alone, in integers and fractions.Fraction.  IEEE 754 rounding is
stated once, rn(); no floating-point operation of numpy or Python decides a planted quantity (floats only PROPOSE candidates
in the search for Sobel neighbourhoods, and each proposal is then decided by rn()).  Nothing here is shared with
np_restatement or the oracle: tests/test_analyze_cases.py holds both to these values before a GPU is involved.
"""
from __future__ import annotations

import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

# analyze.hip's own numbers (tests/test_analyze_cases.py reads them from the source text and compares)
HASH_MULT = 2654435761
HASH_BITS = 17
HASH_CAP = 1 << HASH_BITS
FIRST_COLOR_BLOCKS, COLOR_BLOCK = 8, 256
FIRST_SAMPLES = FIRST_COLOR_BLOCKS * COLOR_BLOCK      # the staged route's first colour launch
COLOR_SAMPLES = 50000
CONTRAST_DIV = 100
EDGE_DIV = 200
COLOR_CAP = 1024


# ------------------------------------------------------------------ what the GPU tests hold every result to
def _serial_sum_tol(n):
    """brightSum is ONE serial fp64 chain over all n pixels in the reference (analyze.go:63): its
    own rounding error is bounded by (n-1)*2^-53 relative (1.1e-12 observed at 4K, against the
    exact sum); the device's fixed-tree sum is closer to exact, so the bar is the chain's bound."""
    return max(1e-12, n * 2.0 ** -53)


def _check_analysis(raw, st, want):
    """raw = fnx_analyze's accumulators, st = ImageStats dict, want = oracle."""
    assert np.array_equal(raw["histogram"].astype(np.float64), want["histogram"])      # exact
    for k in ("has_alpha", "is_grayscale", "unique_colors", "sample_count", "edge_count", "edge_total"):
        assert raw[k] == want[k], k
    rel = _serial_sum_tol(want["width"] * want["height"])
    assert abs(raw["bright_sum"] - want["bright_sum"]) <= rel * abs(want["bright_sum"])
    # (lum - mean)^2 terms inherit the mean's last-bit difference: absolute floor for flat images
    assert abs(raw["variance_sum"] - want["variance_sum"]) <= 1e-9 * abs(want["variance_sum"]) + 1e-6
    assert (st["Width"], st["Height"]) == (want["width"], want["height"])
    assert (st["HasAlpha"], st["IsGrayscale"], st["UniqueColors"]) == (want["has_alpha"], want["is_grayscale"], want["unique_colors"])
    assert abs(st["Entropy"] - want["entropy"]) <= 1e-12
    assert st["EdgeDensity"] == want["edge_density"]
    assert abs(st["MeanBrightness"] - want["mean_brightness"]) <= rel * max(1.0, want["mean_brightness"])
    assert abs(st["Contrast"] - want["contrast"]) <= 1e-9
    assert (st["RecommendedFormat"], st["RecommendedQuality"]) == (want["recommended_format"], want["recommended_quality"])
    assert st["EstimatedCompression"] == want["estimated_compression"]


# ------------------------------------------------------------------ IEEE 754 round-to-nearest, stated once
def rn(x, p=53):
    """the rational x rounded to the nearest number of p significant bits, ties to the even one: what one fp64 (p = 53) or
    fp32 (p = 24) operation returns for the exact result x.  (No value here reaches the overflow or the subnormal range.
    For p = 53 this is Fraction(float(x)): CPython's float(Fraction) is correctly rounded -- the CPU tests compare the two.)"""
    x = Fraction(x)
    if x == 0:
        return x
    n, d = abs(x.numerator), x.denominator
    e = n.bit_length() - d.bit_length() - p              # n / (d 2^e) is in [2^(p-1), 2^(p+1))
    a, b = (n << -e, d) if e < 0 else (n, d << e)
    if a >= b << p:
        e += 1
        a, b = (n << -e, d) if e < 0 else (n, d << e)
    q, r = divmod(a, b)
    if 2 * r > b or (2 * r == b and (q & 1)):
        q += 1
    v = Fraction(q << e) if e >= 0 else Fraction(q, 1 << -e)
    return -v if x < 0 else v


HALF = Fraction(1, 2)


@lru_cache(maxsize=None)
def _products(p):
    """the three constants as the compiler reads their decimal literals, and their rounded products with 0..255"""
    c = tuple(rn(Fraction(k, 1000), p) for k in (299, 587, 114))
    return c, tuple(tuple(rn(ci * v, p) for v in range(256)) for ci in c)


def milli(r, g, b):
    """1000 x the luminance, an integer (works on Python integers and on numpy integer arrays)"""
    return 299 * r + 587 * g + 114 * b


def lum_chain(r, g, b, variant="ref"):
    """the luminance of (r, g, b) as a rational, under the reference's evaluation or one of the evaluations a compiler flag, a
    transcription slip or a narrower type would make of it:
        ref        (0.299 R + 0.587 G) + 0.114 B in fp64, every product and sum rounded: analyze.go:62, devutil.hpp's lum601
        fma_all    fma(0.114, B, fma(0.587, G, 0.299 R))      -- contraction of both sums
        fma_inner  fma(0.299, R, 0.587 G) + 0.114 B           -- contraction of the inner sum only
        reassoc    0.299 R + (0.587 G + 0.114 B)
        fp32       the reference's order in fp32"""
    p = 24 if variant == "fp32" else 53
    (c299, c587, c114), (pr, pg, pb) = _products(p)
    if variant in ("ref", "fp32"):
        return rn(rn(pr[r] + pg[g], p) + pb[b], p)
    if variant == "fma_all":
        return rn(c114 * b + rn(c587 * g + pr[r]))
    if variant == "fma_inner":
        return rn(rn(c299 * r + pg[g]) + pb[b])
    if variant == "reassoc":
        return rn(pr[r] + rn(pg[g] + pb[b]))
    raise ValueError(variant)


VARIANTS = ("fma_all", "fma_inner", "reassoc", "fp32", "int_half_up")


def lum_bin(r, g, b, variant="ref"):
    """the histogram bin of a colour: int(lum + 0.5), the sum rounded like every other operation (analyze.go:64)"""
    if variant == "int_half_up":
        return (milli(r, g, b) + 500) // 1000
    return math.floor(rn(lum_chain(r, g, b, variant) + HALF, 24 if variant == "fp32" else 53))


# ------------------------------------------------------------------ lum_ties
@lru_cache(maxsize=None)
def tie_triples():
    """every (r, g, b) with 299 r + 587 g + 114 b == 500 (mod 1000), in integers, as an (n, 3) array in (r, g, b) order"""
    r, g, b = np.meshgrid(np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), np.arange(256, dtype=np.int64), indexing="ij")
    sel = milli(r, g, b) % 1000 == 500
    out = np.stack([r[sel], g[sel], b[sel]], axis=1)
    out.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def tie_bins(variant="ref"):
    """the bin of every tie triple under `variant`, a tuple of Python integers in tie_triples() order"""
    return tuple(lum_bin(r, g, b, variant) for r, g, b in tie_triples().tolist())


def lum_tie_sensitivity():
    """{variant: how many ties it bins differently from the reference's chain}, and the reference's own split (up, down)"""
    ref = tie_bins("ref")
    moved = {v: sum(1 for a, b in zip(ref, tie_bins(v)) if a != b) for v in VARIANTS}
    up = sum(1 for (r, g, b), k in zip(tie_triples().tolist(), ref) if k == (milli(r, g, b) + 500) // 1000)
    return moved, (up, len(ref) - up)


TIES_W, TIES_H = 129, 131
PAD_COLOUR = (10, 20, 30)                          # 16 150 on the milli-luminance: no tie


def _histogram(bins):
    h = np.zeros(256, np.uint64)
    for k in bins:
        h[k] += 1
    return h


def lum_ties(alpha="mixed", order="spread"):
    """129 x 131: every tie triple once (16 782 of the 16 899 pixels), the rest PAD_COLOUR.  alpha "mixed": values below 255
    on every third pixel (has_alpha == 1); "opaque": 255 throughout (has_alpha == 0).  order "spread": the triples in a stride
    permutation, so that neighbours in a 4-pixel unit land in distant bins; "sorted": by luminance, neighbours mostly in one bin
    -> (image, {planted quantity: value})"""
    t = tie_triples()
    n, total = len(t), TIES_W * TIES_H
    assert n <= total and milli(*PAD_COLOUR) % 1000 != 500
    perm = (np.arange(n, dtype=np.int64) * 7919) % n if order == "spread" else np.argsort(milli(t[:, 0], t[:, 1], t[:, 2]), kind="stable")
    assert len(set(perm.tolist())) == n
    rgb = np.empty((total, 3), np.int64)
    rgb[:n] = t[perm]
    rgb[n:] = PAD_COLOUR
    img = np.empty((total, 4), np.uint8)
    img[:, :3] = rgb
    i = np.arange(total)
    img[:, 3] = 255 if alpha == "opaque" else np.where(i % 3 == 0, (i * 37) % 255, 255)
    ref = tie_bins("ref")
    hist = _histogram(ref)
    hist[lum_bin(*PAD_COLOUR)] += total - n
    expect = {"histogram": hist, "has_alpha": 0 if alpha == "opaque" else 1, "is_grayscale": 0, "unique_colors": COLOR_CAP}
    return img.reshape(TIES_H, TIES_W, 4), expect


def lum_ties_histogram_under(variant):
    """the histogram lum_ties() would have if the bins were taken under `variant`"""
    hist = _histogram(tie_bins(variant))
    hist[lum_bin(*PAD_COLOUR, variant)] += TIES_W * TIES_H - len(tie_triples())
    return hist


# ------------------------------------------------------------------ the sampling grids, restated
def colour_walk(total):
    """(step, number of samples, last sampled index) of the colour walk over `total` pixels (analyze.go:46-50, 73): every
    index that is a multiple of step"""
    step = total // COLOR_SAMPLES if total > COLOR_SAMPLES else 1
    idx = range(0, total, step)
    return step, len(idx), idx[-1]


def contrast_axis(n):
    """the contrast grid's coordinates along an axis of n pixels (analyze.go:93-109): step ceil(n / 100)"""
    return range(0, n, max(1, -(-n // CONTRAST_DIV)))


def edge_axis(n):
    """the Sobel centres along an axis of n >= 3 pixels (analyze.go:150-156): step int(max(1, n / 200)), from 1 to n - 2.
    (n / 200 in fp64 is an integer exactly when n is a multiple of 200, and further than 2^-40 from one otherwise: the
    truncation is the integer quotient)"""
    return range(1, n - 1, max(1, n // EDGE_DIV))


# ------------------------------------------------------------------ sobel_ties
# milli-luminance pairs with a^2 + b^2 == 15000^2: right-middle and bottom-middle pixels moved by (a, b) give gx == 2a / 1000,
# gy == 2b / 1000, magnitude exactly 30
PAIRS = ((0, 15000), (4200, 14400), (5280, 14040), (8064, 12648), (9000, 12000))
DELTA_MAX = 60


@lru_cache(maxsize=None)
def _delta_table():
    """{D: every (dr, dg, db) within +-DELTA_MAX with 299 dr + 587 dg + 114 db == D} for the D of PAIRS, both signs"""
    ds = sorted({s * v for p in PAIRS for v in p for s in (1, -1)})
    out = {d: [] for d in ds}
    for dr in range(-DELTA_MAX, DELTA_MAX + 1):
        for dg in range(-DELTA_MAX, DELTA_MAX + 1):
            for d in ds:
                rest = d - 299 * dr - 587 * dg
                if rest % 114 == 0 and abs(rest // 114) <= DELTA_MAX:
                    out[d].append((dr, dg, rest // 114))
    assert all(out.values())
    return out


@lru_cache(maxsize=None)
def _lum_ref(rgb):
    return lum_chain(*rgb)


def _g_chain(a, b, c, d, e, f):
    """a - b + 2 c - 2 d + e - f, left to right, every sum rounded (the doublings are exact)"""
    return rn(rn(rn(rn(rn(a - b) + 2 * c) - 2 * d) + e) - f)


def sobel_gradients(win):
    """win[dy][dx]: the 3 x 3 colours around a centre -> (gx, gy) as analyze.go:158-171 and analyze.hip evaluate them"""
    l = [[_lum_ref(tuple(c)) for c in row] for row in win]
    gx = _g_chain(l[0][2], l[0][0], l[1][2], l[1][0], l[2][2], l[2][0])
    gy = _g_chain(l[2][0], l[0][0], l[2][1], l[0][1], l[2][2], l[0][2])
    return gx, gy


def sobel_m(gx, gy, contract=None):
    """gx*gx + gy*gy: None -- both products rounded, then the sum (the reference); "x" -- fma(gx, gx, gy*gy); "y" -- fma(gy, gy, gx*gx)"""
    if contract is None:
        return rn(rn(gx * gx) + rn(gy * gy))
    if contract == "x":
        return rn(gx * gx + rn(gy * gy))
    assert contract == "y"
    return rn(rn(gx * gx) + gy * gy)


def is_edge(m):
    """sqrt(m) > 30.0 for a double m >= 0, decided as m > 900.  The two are the same decision: IEEE sqrt is correctly rounded,
    hence monotone, and sqrt(900) == 30 exactly, so m <= 900 gives sqrt(m) <= 30; the next double above 900 is 900 + 2^-43,
    whose root is 30 + 2^-43 / 60 - ... = 30 + 0.533 ulp(30) (ulp(30) == 2^-48), which rounds to 30 + 2^-48 > 30, and
    every larger m gives at least that."""
    return m > 900


M30 = 30000 * 30000                               # the threshold on 1000 gx, 1000 gy in integers
NEAR = 1000                                       # |M - M30| <= NEAR (1e-3 on m): decided by the fp64 chain, not by the integers


class SobelCount:
    """edge_count / edge_total of an image; near: {(x, y): (gx, gy)} of the sampled centres whose exact magnitude is within
    1e-3 of the threshold squared -- the only ones that rounding can decide.  (The chain's error: each luminance carries at most
    4 roundings of values under 256, the gradient 8 of those and 5 roundings of values under 2048 -- under 2^-39 --, m then
    2 (|gx| + |gy|) 2^-39 and three roundings of values under 2^23: under 2^-26 in all, five orders below 1e-3.)"""

    def count(self, contract=None):
        return self.far_edges + sum(1 for g in self.near.values() if is_edge(sobel_m(*g, contract)))


def sobel_classify(img):
    h, w = img.shape[:2]
    out = SobelCount()
    out.near, out.far_edges, out.total = {}, 0, 0
    if w < 3 or h < 3:
        return out
    xs, ys = edge_axis(w), edge_axis(h)
    a = img.astype(np.int64)
    L = milli(a[..., 0], a[..., 1], a[..., 2])
    X, Y = np.asarray(xs)[None, :], np.asarray(ys)[:, None]
    at = lambda dx, dy: L[Y + dy, X + dx]
    GX = at(1, -1) - at(-1, -1) + 2 * at(1, 0) - 2 * at(-1, 0) + at(1, 1) - at(-1, 1)
    GY = at(-1, 1) - at(-1, -1) + 2 * at(0, 1) - 2 * at(0, -1) + at(1, 1) - at(1, -1)
    M = GX * GX + GY * GY
    near = np.abs(M - M30) <= NEAR
    out.total = len(xs) * len(ys)
    out.far_edges = int(((M > M30) & ~near).sum())
    for j, i in zip(*(v.tolist() for v in np.nonzero(near))):
        x, y = xs[i], ys[j]
        out.near[(x, y)] = sobel_gradients(img[y - 1:y + 2, x - 1:x + 2, :3].tolist())
    return out


def _propose(rng, n):
    """random members of the family, those of n draws whose colours stay inside 0..255: background, right-middle and
    bottom-middle colours, (k, 3) integer arrays each.  (Dark backgrounds matter: their luminances have the finer ulp, the
    gradients the longer mantissas, and only those products lose enough in rounding for contraction to show.)"""
    tab = _delta_table()
    bg = rng.integers(0, 256, (n, 3))
    pair = rng.integers(0, len(PAIRS), n)
    swap, sa, sb = rng.integers(0, 2, n), rng.integers(0, 2, n) * 2 - 1, rng.integers(0, 2, n) * 2 - 1
    pick = rng.integers(0, 1 << 30, (n, 2))
    right, below = np.empty((n, 3), np.int64), np.empty((n, 3), np.int64)
    for k in range(n):
        a, b = PAIRS[pair[k]][::-1] if swap[k] else PAIRS[pair[k]]
        ta, tb = tab[int(sa[k]) * a], tab[int(sb[k]) * b]
        right[k] = bg[k] + ta[pick[k, 0] % len(ta)]
        below[k] = bg[k] + tb[pick[k, 1] % len(tb)]
    ok = ((right >= 0) & (right <= 255) & (below >= 0) & (below <= 255)).all(axis=1)
    return bg[ok], right[ok], below[ok]


def _screen(bg, right, below):
    """floats PROPOSE: which members could round differently once gx*gx + gy*gy is contracted.  The product's rounding error
    is recovered exactly (Veltkamp / Dekker) and compared with the sum's; members where the two cannot carry the sum over a
    rounding boundary are dropped.  What passes is decided by member_flips() -- a wrong proposal costs time, never a result."""
    f = lambda c: (0.299 * c[:, 0].astype(np.float64) + 0.587 * c[:, 1].astype(np.float64)) + 0.114 * c[:, 2].astype(np.float64)
    l0, lr, lb = f(bg), f(right), f(below)
    g = lambda v: ((((l0 - l0) + 2 * v) - 2 * l0) + l0) - l0
    gx, gy = g(lr), g(lb)

    def sq(a):
        p = a * a
        c = 134217729.0 * a
        hi = c - (c - a)
        lo = a - hi
        return p, ((hi * hi - p) + 2 * hi * lo) + lo * lo

    (px, ex), (py, ey) = sq(gx), sq(gy)
    s = px + py
    bb = s - px
    t = (px - (s - bb)) + (py - bb)
    ulp = 2.0 ** -43
    close = np.abs(s - 900.0) <= 2 * ulp
    return np.nonzero(close & ((np.abs(t + ex) >= 0.45 * ulp) | (np.abs(t + ey) >= 0.45 * ulp)))[0]


def member_window(bg, right, below):
    """the 3 x 3 colours around the member's centre"""
    bg, right, below = tuple(bg), tuple(right), tuple(below)
    return [[bg, bg, bg], [bg, bg, right], [bg, below, bg]]


def member_flips(bg, right, below):
    """(edge by the reference, edge under fma(gx, gx, gy*gy), edge under fma(gy, gy, gx*gx)) of the member's centre"""
    g = sobel_gradients(member_window(bg, right, below))
    return tuple(is_edge(sobel_m(*g, c)) for c in (None, "x", "y"))


FLIPS_WANTED = 10
SEARCH_BATCH = 60000


@lru_cache(maxsize=None)
def flip_members():
    """members whose centre the reference calls an edge and fma(gx, gx, gy*gy) does not, or the other way round -- the more
    frequent direction only, so that their count cannot cancel in edge_count.  -> (members, members examined)"""
    rng = np.random.default_rng(20240517)
    found = {True: [], False: []}
    seen = 0
    for _ in range(40):
        bg, right, below = _propose(rng, SEARCH_BATCH)
        seen += len(bg)
        for k in _screen(bg, right, below).tolist():
            m = (tuple(bg[k].tolist()), tuple(right[k].tolist()), tuple(below[k].tolist()))
            ref, cx, _ = member_flips(*m)
            if ref != cx and m not in found[ref]:
                found[ref].append(m)
        if max(len(v) for v in found.values()) >= FLIPS_WANTED:
            break
    best = max(found.values(), key=len)
    return tuple(best), seen


def grey_members():
    """the grey sub-family: steps of 15, and of 9 and 12, on a grey background (0.299 v + 0.587 v + 0.114 v is not v in fp64)"""
    out = []
    for v in range(20, 236, 3):
        for a, b in ((0, 15), (15, 0), (9, 12), (12, 9), (-9, 12), (12, -9), (0, -15), (-9, -12)):
            out.append(((v, v, v), (v + a,) * 3, (v + b,) * 3))
    return out


CELL = 5


def sobel_ties(w=307, h=227, seed=1, flips=True):
    """w x h (at most 399 each: the edge step is 1, every interior pixel is a sample) tiled with 5 x 5 cells, each with its own
    background and one member of the family at its centre: planted pixels of two cells are at least 4 apart, so no 3 x 3
    window holds pixels of two members.  The margin right and below the last cell repeats the cell's edge.
    The members: the contraction flips first (flips=True), the grey sub-family, then random ones.
    -> (image, {planted quantity: value}, SobelCount)"""
    assert 3 <= w <= 399 and 3 <= h <= 399
    nx, ny = w // CELL, h // CELL
    members = (list(flip_members()[0]) if flips else []) + grey_members()
    rng = np.random.default_rng(1000 + seed)
    order = rng.permutation(nx * ny)
    while len(members) < nx * ny:
        bg, right, below = _propose(rng, 2 * (nx * ny - len(members)) + 16)
        members += [(tuple(bg[k].tolist()), tuple(right[k].tolist()), tuple(below[k].tolist())) for k in range(len(bg))]
    img = np.empty((ny * CELL, nx * CELL, 4), np.uint8)
    img[..., 3] = 255
    for cell, (bg, right, below) in zip(order.tolist(), members):
        cx, cy = CELL * (cell % nx), CELL * (cell // nx)
        img[cy:cy + CELL, cx:cx + CELL, :3] = bg
        img[cy + 2, cx + 3, :3] = right
        img[cy + 3, cx + 2, :3] = below
    img = np.pad(img, ((0, h - ny * CELL), (0, w - nx * CELL), (0, 0)), mode="edge")
    cl = sobel_classify(img)
    return img, {"edge_count": cl.count(), "edge_total": cl.total}, cl


# ------------------------------------------------------------------ colour_grid
TOTALS = (50000, 50001, 99999, 100000, 100001, 149999, 150000)
BACKGROUND = 0xFF203040


def grid_dims(total):
    """total == w * h with w the divisor nearest below sqrt(total) that is no multiple of 4 (where the number has one)"""
    for need_odd in (True, False):
        for w in range(math.isqrt(total), 2, -1):
            if total % w == 0 and (w % 4 or not need_odd):
                return w, total // w
    raise ValueError(total)


def _words(n, mult, add, avoid):
    out, k = [], 0
    while len(out) < n:
        k += 1
        v = (k * mult + add) & 0xffffffff
        if v not in avoid:
            out.append(v)
    return out


def _image_of_words(words, w, h):
    """pixel words (R in the low byte: the little-endian RGBA word the kernels load) -> (h, w, 4) uint8"""
    return np.asarray(words, dtype="<u4").view(np.uint8).reshape(h, w, 4)


def colour_grid(total, truth, layout="spread"):
    """one background colour; truth - 1 planted colours, all distinct, on sampled indices of the colour walk; where the step
    leaves unsampled indices, further distinct colours on those (they must not count).
        spread  the planted colours over the whole walk, index 0 and the last sampled index among them
        late    every planted colour at sample FIRST_SAMPLES or later (the last sampled index among them): the staged route's
                first launch counts 1, the second has to run
        split   1022 planted colours before sample FIRST_SAMPLES -- 1023 with the background, so the hand-over must not skip --
                and truth - 1023 after it, the last sampled index among them
    -> (image, {"unique_colors": min(truth, 1024)})"""
    w, h = grid_dims(total)
    step, n, last = colour_walk(total)
    k = truth - 1
    if layout == "spread":
        ranks = sorted({(j * (n - 1)) // (k - 1) for j in range(k)}) if k > 1 else [n - 1]
    elif layout == "late":
        lo = FIRST_SAMPLES
        ranks = sorted({lo + (j * (n - 1 - lo)) // (k - 1) for j in range(k)}) if k > 1 else [n - 1]
    else:
        assert layout == "split" and truth > 1023
        before, after = 1022, truth - 1023
        ranks = [(j * (FIRST_SAMPLES - 1)) // (before - 1) for j in range(before)]
        ranks += [n - 1 - (j * (n - 1 - FIRST_SAMPLES)) // max(after, 2) for j in range(after)]
        ranks = sorted(set(ranks))
    assert len(ranks) == k and ranks[-1] == n - 1 and 0 <= ranks[0], (len(ranks), k)
    words = [BACKGROUND] * total
    planted = _words(k, 0x9E3779B1, 0, {BACKGROUND})
    for r, v in zip(ranks, planted):
        words[r * step] = v
    decoys = 0
    if step > 1:
        spots = sorted({r * step + 1 for r in range(0, n, max(1, n // 300))} | {last + 1, last - 1, total - 1, step - 1, step + 1})
        spots = [i for i in spots if 0 <= i < total and i % step]
        for i, v in zip(spots, _words(len(spots), 0x85EBCA6B, 0x1234567, set(planted) | {BACKGROUND})):
            words[i] = v
        decoys = len(spots)
    img = _image_of_words(words, w, h)
    return img, {"unique_colors": min(truth, COLOR_CAP)}, dict(step=step, samples=n, last=last, ranks=ranks, decoys=decoys, truth=truth)


# ------------------------------------------------------------------ colliding_colours
HASH_INV = pow(HASH_MULT, -1, 1 << 32)


def home_slot(p):
    """the slot a pixel word starts probing at"""
    return ((p * HASH_MULT) & 0xffffffff) >> (32 - HASH_BITS)


def pixels_homed_at(slot, n, with_zero=False):
    """n distinct pixel words whose home slot is `slot`: the multiplier is odd, hence invertible mod 2^32"""
    out = [0] if with_zero else []
    j = 0
    while len(out) < n:
        j += 1
        out.append((((slot << (32 - HASH_BITS)) | (j * 17 + 3)) * HASH_INV) & 0xffffffff)
    assert len(set(out)) == n and all(home_slot(p) == slot for p in out)
    return out


COLLIDING = {5: (3, 1, 1), 1023: (723, 150, 150), 1024: (724, 150, 150), 1500: (1200, 150, 150), 2100: (1500, 300, 300)}


def colliding_colours(truth, w=53, h=47):
    """w x h (under 50 000 pixels: every pixel is sampled) holding exactly `truth` distinct pixel words: COLLIDING[truth] of
    them homed at the table's last slot, at the one before it and at slot 0 -- the pixel 0x00000000 among the latter -- each
    repeated through the image in a shuffled order.  A smaller truth's words are a subset of a larger one's: after a table that
    was not cleared, the smaller image would find its colours present and count none.  -> (image, {"unique_colors": min(truth, 1024)}, the words)"""
    n_last, n_prev, n_zero = COLLIDING[truth]
    words = pixels_homed_at(HASH_CAP - 1, n_last) + pixels_homed_at(HASH_CAP - 2, n_prev) + pixels_homed_at(0, n_zero, with_zero=True)
    assert len(set(words)) == truth == len(words) and w * h >= truth and w * h <= COLOR_SAMPLES
    order = np.random.default_rng(truth).permutation(truth).tolist()
    seq = [words[order[i % truth]] for i in range(w * h)]
    return _image_of_words(seq, w, h), {"unique_colors": min(truth, COLOR_CAP)}, words


def simulate_probe(words):
    """insert the words in order into a table of HASH_CAP slots, linear probing -> (entries, longest probe, inserts that
    stepped from the last slot to slot 0, the occupied slots as a sorted list)"""
    table, longest, wrapped = {}, 0, 0
    for p in words:
        s, steps, wrap = home_slot(p), 0, False
        while s in table and table[s] != p:
            if s == HASH_CAP - 1:
                wrap = True
            s = (s + 1) & (HASH_CAP - 1)
            steps += 1
        if s not in table:
            table[s] = p
            wrapped += wrap
        longest = max(longest, steps)
    return len(table), longest, wrapped, sorted(table)


# ------------------------------------------------------------------ contrast_grid
CONTRAST_SIZES = (99, 100, 101, 200, 201, 301)
GREY = (120, 120, 120)


def contrast_grid(w, h, variant=0):
    """a flat grey image with black and white outliers: on grid points of the contrast grid -- the last grid row and column
    always -- and, where the step leaves room, one pixel off the grid.
    -> (image, {"sample_count": n}, info) with info["variance"] the exact sum of (lum - mean)^2 over the grid (a Fraction; lum
    and mean in real arithmetic) and info["teeth"] the smallest relative change of it that wrongly including or dropping any single
    outlier would make"""
    xs, ys = contrast_axis(w), contrast_axis(h)
    img = np.empty((h, w, 4), np.uint8)
    img[..., :3] = GREY
    img[..., 3] = 255
    on = {(xs[-1], ys[-1]), (xs[-1], ys[0]), (xs[0], ys[-1]), (xs[len(xs) // 2], ys[len(ys) // 2]), (xs[-1], ys[len(ys) // 2]),
          (xs[len(xs) // 3], ys[-1]), (xs[1 % len(xs)], ys[1 % len(ys)])}
    off = set()
    sx, sy = xs.step, ys.step
    if sx > 1:
        off |= {(x, ys[j % len(ys)]) for j, x in enumerate((xs[-1] + 1, xs[-1] - 1, xs[1] - 1, xs[0] + 1, w - 1)) if 0 <= x < w and x % sx}
    if sy > 1:
        off |= {(xs[j % len(xs)], y) for j, y in enumerate((ys[-1] + 1, ys[-1] - 1, ys[1] - 1, ys[0] + 1, h - 1)) if 0 <= y < h and y % sy}
    assert not (on & off) and all(x % sx == 0 and y % sy == 0 for x, y in on) and all(x % sx or y % sy for x, y in off)
    for j, (x, y) in enumerate(sorted(on) + sorted(off)):
        img[y, x, :3] = 255 if (j + variant) % 2 else 0
    # exact: 1000 lum is an integer per pixel
    a = img.astype(np.int64)
    L = milli(a[..., 0], a[..., 1], a[..., 2])
    mean = Fraction(int(L.sum()), 1000 * w * h)
    dev2 = lambda v: (Fraction(int(v), 1000) - mean) ** 2
    var = sum(dev2(L[y, x]) for y in ys for x in xs)
    bg = dev2(milli(*GREY))
    teeth = min(min(dev2(L[y, x]), abs(dev2(L[y, x]) - bg)) for x, y in on | off) / var
    assert teeth > Fraction(1, 10 ** 6)                    # three orders above the 1e-9 the results are held to
    info = dict(variance=var, teeth=teeth, on=sorted(on), off=sorted(off), xs=xs, ys=ys)
    return img, {"sample_count": len(xs) * len(ys)}, info


# ------------------------------------------------------------------ edge_grid
EDGE_SIZES = (3, 4, 5, 399, 400, 401, 402, 599, 600, 601)


def edge_grid(w, h, variant=0):
    """black, with isolated white pixels (at least 4 apart in both directions' maximum, so no 3 x 3 window holds two) around the
    last sampled Sobel centre of each axis and the first unsampled one.  A white pixel beside or diagonal to a centre gives
    |gx| or |gy| of 255 or 510: every sampled centre at Chebyshev distance 1 of a white pixel is one edge, no other centre is.
    -> (image, {"edge_count": n, "edge_total": centres})"""
    xs, ys = edge_axis(w), edge_axis(h)
    lx, ly = xs[-1], ys[-1]
    cand = []
    for dx in (1, 0, -1, xs.step, xs.step - 1, xs.step + 1, -xs.step + 1, 2):
        for y in (ly + 1, ly, 1, 0, ys[len(ys) // 2], h - 1):
            cand.append((lx + dx, y))
    for dy in (1, 0, -1, ys.step, ys.step - 1, ys.step + 1, -ys.step + 1, 2):
        for x in (lx + 1, lx, 1, 0, xs[len(xs) // 2], w - 1):
            cand.append((x, ly + dy))
    cand += [(w - 1, h - 1), (0, 0), (w - 1, 0), (0, h - 1), (xs[0], ys[0])]
    cand = cand[variant:] + cand[:variant]
    white = []
    for x, y in cand:
        if 0 <= x < w and 0 <= y < h and all(max(abs(x - p), abs(y - q)) >= 4 for p, q in white):
            white.append((x, y))
    img = np.zeros((h, w, 4), np.uint8)
    img[..., 3] = 255
    for x, y in white:
        img[y, x, :3] = 255
    sx, sy = set(xs), set(ys)
    count = sum(1 for x, y in white for cx in (x - 1, x, x + 1) for cy in (y - 1, y, y + 1)
                if (cx, cy) != (x, y) and cx in sx and cy in sy)
    return img, {"edge_count": count, "edge_total": len(xs) * len(ys)}, dict(white=white, xs=xs, ys=ys)


# ------------------------------------------------------------------ the cases
class Case:
    """name, kind, the image (made once, read-only), expect {key of fnx_analyze's accumulators: planted value}, info"""

    def __init__(self, name, kind, make):
        self.name, self.kind, self._make, self._made = name, kind, make, None

    def _get(self):
        if self._made is None:
            made = self._make()
            img = np.ascontiguousarray(made[0])
            img.setflags(write=False)
            self._made = (img, made[1], made[2] if len(made) > 2 else None)
        return self._made

    img = property(lambda self: self._get()[0])
    expect = property(lambda self: self._get()[1])
    info = property(lambda self: self._get()[2])

    def __repr__(self):
        return self.name


MIXED_W, MIXED_H = TIES_W, TIES_H                 # lum_ties' size: colliding_colours and sobel_ties are made at it for the mixed batch


def _cases():
    c = []
    add = lambda name, kind, make: c.append(Case(name, kind, make))
    add("lum_ties_mixed", "lum_ties", lambda: lum_ties("mixed", "spread"))
    add("lum_ties_opaque", "lum_ties", lambda: lum_ties("opaque", "spread"))
    add("lum_ties_sorted", "lum_ties", lambda: lum_ties("mixed", "sorted"))
    add("sobel_ties", "sobel_ties", lambda: sobel_ties(307, 227, 1))
    add("sobel_ties_b", "sobel_ties", lambda: sobel_ties(307, 227, 2, flips=False))
    add("sobel_ties_129x131", "sobel_ties", lambda: sobel_ties(MIXED_W, MIXED_H, 3))
    for total in TOTALS:
        for truth in (5, 1023, 1024, 1025):
            add(f"colour_grid_{total}_{truth}", "colour_grid", lambda total=total, truth=truth: colour_grid(total, truth))
    for total in (50001, 100001, 150000):
        add(f"colour_grid_{total}_late_1023", "colour_grid", lambda total=total: colour_grid(total, 1023, "late"))
        add(f"colour_grid_{total}_late_1024", "colour_grid", lambda total=total: colour_grid(total, 1024, "late"))
        add(f"colour_grid_{total}_split_1024", "colour_grid", lambda total=total: colour_grid(total, 1024, "split"))
        add(f"colour_grid_{total}_split_1025", "colour_grid", lambda total=total: colour_grid(total, 1025, "split"))
    for truth in COLLIDING:
        add(f"colliding_{truth}", "colliding", lambda truth=truth: colliding_colours(truth))
    add("colliding_2100_129x131", "colliding", lambda: colliding_colours(2100, MIXED_W, MIXED_H))
    for n in CONTRAST_SIZES:
        add(f"contrast_grid_{n}x7", "contrast_grid", lambda n=n: contrast_grid(n, 7))
        add(f"contrast_grid_7x{n}", "contrast_grid", lambda n=n: contrast_grid(7, n))
    for v in (1, 2):
        add(f"contrast_grid_201x7_v{v}", "contrast_grid", lambda v=v: contrast_grid(201, 7, v))
    for n in EDGE_SIZES:
        add(f"edge_grid_{n}x7", "edge_grid", lambda n=n: edge_grid(n, 7))
        add(f"edge_grid_7x{n}", "edge_grid", lambda n=n: edge_grid(7, n))
    for v in (5, 11):
        add(f"edge_grid_401x7_v{v}", "edge_grid", lambda v=v: edge_grid(401, 7, v))
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}

# one case of every kind for the four presentations: widths that are no multiple of 4 (vector loads with row tails)
PRESENTED = ("lum_ties_mixed", "sobel_ties", "colour_grid_100001_1024", "colliding_1500", "contrast_grid_201x7", "edge_grid_401x7")
# batches of equal-sized cases; the first is the mixed one, at lum_ties' size
BATCHES = {
    "mixed": ("lum_ties_mixed", "colliding_2100_129x131", "sobel_ties_129x131", "lum_ties_opaque", "lum_ties_sorted"),
    "sobel_ties": ("sobel_ties", "sobel_ties_b"),
    "colour_grid": ("colour_grid_100001_1024", "colour_grid_100001_5", "colour_grid_100001_split_1025", "colour_grid_100001_late_1023", "colour_grid_100001_1023"),
    "colliding": ("colliding_1500", "colliding_1023", "colliding_1024", "colliding_2100"),
    "contrast_grid": ("contrast_grid_201x7", "contrast_grid_201x7_v1", "contrast_grid_201x7_v2"),
    "edge_grid": ("edge_grid_401x7", "edge_grid_401x7_v5", "edge_grid_401x7_v11"),
}


def batch_names(group, n):
    """n case names of a batch group; one of them appears twice (and the tests pass the SAME tensor for both)"""
    names = BATCHES[group]
    distinct = min(len(names), n - 1)
    picked = list(names[:distinct])
    k = 0
    while len(picked) < n:
        picked.append(names[k % distinct])
        k += 1
    return picked
