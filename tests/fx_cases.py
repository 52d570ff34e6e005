"""Crafted inputs for Sharpen / AdaptiveSharpen (fennec_amd/csrc/effects.hip) and an exact classifier of what they reach.

The kernels are bit-exact by argument: Sharpen through a table R[d], AdaptiveSharpen through an fp32 chain under a rounding
guard whose flagged pixels go to a fix list (per tile or per wave) and are recomputed in fp64; a list that overflows recomputes
its whole tile or segment; surely saturated pixels (|Sobel| > 400) take the table when the amount is tie-prone.  Photographs and
noise execute next to none of that.  The images here are built so that most samples ARE exact half-integers in real arithmetic,
so that the Sobel magnitude sits on and around 400, and so that a list is filled exactly to its cap and one past it.

classify() states, per interior sample and in integers only (numpy integer arrays, Python big integers, math.isqrt -- no
floating point decides anything, and nothing here is shared with np_restatement or the oracle):

    d = orig - blur3x3,  M = gx^2 + gy^2 of the Sobel sums over I = 299 R + 587 G + 114 B,
    V = orig + (p / q) * min(1, sqrt(M) / 400000) * d        (adaptive; e == 1 for Sharpen)

the exact rounding clampF(V), and V's exact distance from the nearest rounding boundary (sqrt(M) is bracketed by isqrt of
M * 10^30: the distance is known to 1e-17).
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

# the geometry of effects.hip's two marching forms (tests/test_fx_cases.py reads the kernel's own constants and compares)
TILE_W, TILE_H, TILE_CAP = 64, 24, 512          # fx_march_kernel: FX_TW, FX_TH, FX_FIX_CAP
STRIP_W, SEG_H, SEG_CAP = 62, 16, 64            # fx_stream_kernel: FXS_COLS, the segment floor of launch_fx, FXS_FIX
SOBEL_ONE = 400000                              # |Sobel| = 400 on the milli-luminance: e == 1 from here on
M_ONE = SOBEL_ONE * SOBEL_ONE                   # 1.6e11
# classes of a pixel by its exact M, around the kernel's own bound 1.6000016e11f for "saturated for certain"
SAT_CLASSES = ("at", "band", "below", "above")
UNCERTAIN = 0.01                                # a boundary nearer than this (and not on it) could be flagged or not: 2G + E is ~1.2e-3 at amount 2.5

_S = 10 ** 15                                   # sqrt(M) * _S is bracketed by [isqrt(M _S^2), isqrt(M _S^2) + 1]


def sat_class(m: int):
    if m == M_ONE:
        return "at"
    if M_ONE < m <= M_ONE + 140000:
        return "band"
    if 159900000000 <= m < M_ONE:
        return "below"
    if M_ONE + 180000 <= m <= 160100000000:
        return "above"
    return None


# ------------------------------------------------------------------ generators
def _image(v, offsets=(0, 0, 0), alpha=255):
    """R, G, B = v + a constant per channel, alpha constant"""
    v = np.asarray(v, dtype=np.int64)
    out = np.empty(v.shape + (4,), np.uint8)
    for c in range(3):
        ch = v + offsets[c]
        assert ch.min() >= 0 and ch.max() <= 255, (int(ch.min()), int(ch.max()))
        out[..., c] = ch
    out[..., 3] = alpha
    return out


def ramp_rows(w, h, s, amp, base=20, wrap=200, offsets=(0, 0, 0)):
    """v = base + (s x mod wrap) + amp [y even]: gy == 0, gx == 8000 s, d == +-1 (amp 2) or d in {0, -1} (amp 1) away from the wraps"""
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    return _image(base + (s * x) % wrap + amp * ((y + 1) % 2), offsets)


def pythagorean(w, h, k=2, base=20, wrap=192, offsets=(0, 0, 0)):
    """v = base + (3k x + 4k y mod wrap) + 2 [y even]: gx : gy == 3 : 4, |Sobel| == 40000 k on the milli-luminance (e == k / 10), d == +-1"""
    x = np.arange(w)[None, :]
    y = np.arange(h)[:, None]
    return _image(base + (3 * k * x + 4 * k * y) % wrap + 2 * ((y + 1) % 2), offsets)


def step_edges(w, h, seed, lo=80, hi=180, offsets=(0, 0, 0)):
    """grey plateaus three columns wide that step by +-100: beside an edge gx == +-400000 exactly (M == 1.6e11) and d == +-25;
    single +-1 / +-2 changes of one channel on a sparse lattice move M into the classes around that"""
    rng = np.random.default_rng(seed)
    x = np.arange(w)[None, :]
    v = np.where((x // 3) % 2 == 0, lo, hi) + np.zeros((h, 1), np.int64)
    img = _image(v, offsets)
    k = 0
    for yy in range(2, h - 1, 4):
        for xx in range(2 + (yy // 4) % 5, w - 1, 7):
            ch = (2, 0, 2, 1, 2, 0)[k % 6]                      # mostly blue and red: 2 * 114 and 299 keep gy^2 inside the band
            delta = (1, -1, 2, -2)[int(rng.integers(4))]
            img[yy, xx, ch] = int(img[yy, xx, ch]) + delta
            k += 1
    return img


def soft(w, h, seed):
    """noise under two passes of the integer binomial [1 4 6 4 1]^2: Sobel magnitudes spread below 400, nothing crafted"""
    rng = np.random.default_rng(seed)
    out = np.empty((h, w, 4), np.uint8)
    for c in range(3):
        v = rng.integers(0, 256, (h, w)).astype(np.int64)
        for _ in range(2):
            p = np.pad(v, 2, mode="edge")
            t = p[:, :-4] + 4 * p[:, 1:-3] + 6 * p[:, 2:-2] + 4 * p[:, 3:-1] + p[:, 4:]
            v = (t[:-4] + 4 * t[1:-3] + 6 * t[2:-2] + 4 * t[3:-1] + t[4:] + 128) >> 8
        out[..., c] = v
    out[..., 3] = rng.integers(0, 256, (h, w))
    return out


def flat(w, h, value=(90, 120, 60, 255)):
    out = np.empty((h, w, 4), np.uint8)
    out[...] = value
    return out


def half_and_half(dense, other, side):
    """`dense` in the left / right / top / bottom half, `other` in the rest: an overflowing and a quiet tile, strip and segment side by side"""
    h, w = dense.shape[:2]
    assert other.shape == dense.shape
    out = other.copy()
    if side == "left":
        out[:, :w // 2] = dense[:, :w // 2]
    elif side == "right":
        out[:, w // 2:] = dense[:, w // 2:]
    elif side == "top":
        out[:h // 2] = dense[:h // 2]
    else:
        assert side == "bottom"
        out[h // 2:] = dense[h // 2:]
    return out


def _triangle(w, h, offsets):
    """a ramp of +-10 per column that turns every 20 columns instead of wrapping: gx == +-80000 (e == 0.2) but for the turning
    columns (gx == 0), gy == 0 and d == 0 but there -- at amount 2.5 no sample is a tie, none is near one, no pixel is saturated"""
    x = np.arange(w)[None, :]
    t = x % 40
    return (30 + 10 * np.where(t <= 20, t, 40 - t) + np.zeros((h, 1), np.int64)), offsets


def _count_region(cl, x0, x1, y0, y1):
    """(surely flagged, uncertain, saturated) pixels of the image region [x0, x1) x [y0, y1) (interior pixels only)"""
    ys, xs = slice(max(y0, 1) - 1, max(min(y1, cl.h - 1) - 1, 0)), slice(max(x0, 1) - 1, max(min(x1, cl.w - 1) - 1, 0))
    return int(cl.tie_px[ys, xs].sum()), int(cl.uncertain_px[ys, xs].sum()), int((cl.M[ys, xs] >= M_ONE).sum())


def _cap_image(w, h, region, n, band, offsets):
    """the triangle ramp with exactly n surely flagged pixels in region (x0, x1, y0, y1) at amount 5/2, and no uncertain one:
    `band` (xa, xb) -- columns that carry +2 on every even row over the whole height: d == +-1 inside it (a tie each), columns
    xa and xb - 1 at e == 0.21 (0.025 from a boundary); then single +2 bumps three apart (one tie each: the bump's own d == 1,
    its neighbours' d == 0) until the count is n"""
    v, offsets = _triangle(w, h, offsets)
    v = v.copy()
    if band:
        v[0::2, band[0]:band[1]] += 2
    x0, x1, y0, y1 = region
    sites = [(xx, yy) for yy in range(max(y0, 1) + 1, min(y1, h - 1) - 1, 3) for xx in range(max(x0, 1) + 1, min(x1, w - 1) - 1, 3)
             if xx % 20 not in (19, 0, 1) and not (band and band[0] - 3 <= xx < band[1] + 3)]
    have = _count_region(classify(_image(v, offsets), 5, 2), *region)[0]
    assert have <= n <= have + len(sites), (have, n, len(sites))
    for xx, yy in sites[:n - have]:
        v[yy, xx] += 2
    img = _image(v, offsets)
    ties, unc, sat = _count_region(classify(img, 5, 2), *region)
    assert (ties, unc, sat) == (n, 0, 0), (ties, unc, sat, n)
    return img


CAP_W, CAP_H = 130, 50                           # one interior tile (1, 1), strips 0..2, segments 0..3


def cap_tile(n, tile=(1, 1), offsets=(0, 0, 0)):
    """130 x 50: tile `tile` of fx_march_kernel holds exactly n surely flagged pixels at amount 5/2 and no uncertain one"""
    bx, by = tile
    x0 = bx * TILE_W
    band = (x0 + 2, x0 + 25)
    return _cap_image(CAP_W, CAP_H, (x0, x0 + TILE_W, by * TILE_H, (by + 1) * TILE_H), n, band, offsets)


def cap_segment(n, strip=1, seg=1, offsets=(0, 0, 0)):
    """130 x 50: the wave of fx_stream_kernel that owns strip `strip`, segment `seg` lists exactly n pixels"""
    return _cap_image(CAP_W, CAP_H, (strip * STRIP_W, (strip + 1) * STRIP_W, seg * SEG_H, (seg + 1) * SEG_H), n, None, offsets)


# ------------------------------------------------------------------ the exact classifier
class Classified:
    """per interior sample (arrays of shape (h - 2, w - 2, 3) unless noted):
    d, M (h - 2, w - 2), result (the exact rounding), dist (float: to the nearest boundary that clampF can still cross, exact to
    1e-17), raw (float: to the nearest half-integer of V, clamped or not -- what a fract() test sees), tie (raw is exactly 0)"""

    def __init__(self, w, h):
        self.w, self.h = w, h

    @property
    def tie_px(self):                            # a surely flagged pixel: some channel is an exact tie
        return self.tie.any(axis=2)

    @property
    def uncertain_px(self):                      # some channel is near a boundary without being on it
        return ((self.raw > 0) & (self.raw < UNCERTAIN)).any(axis=2)

    def tie_share(self):
        return float(self.tie.mean())

    def sat_counts(self):
        """pixels with some d != 0 per saturation class"""
        live = (self.d != 0).any(axis=2)
        out = dict.fromkeys(SAT_CLASSES, 0)
        for m in self.M[live].tolist():
            c = sat_class(m)
            if c:
                out[c] += 1
        return out

    def tile_counts(self):
        """{(bx, by): (surely flagged, uncertain)} per tile of fx_march_kernel"""
        return {(bx, by): _count_region(self, bx * TILE_W, (bx + 1) * TILE_W, by * TILE_H, (by + 1) * TILE_H)[:2]
                for by in range((self.h + TILE_H - 1) // TILE_H) for bx in range((self.w + TILE_W - 1) // TILE_W)}

    def segment_counts(self):
        """{(strip, seg): (surely flagged, uncertain)} per wave of fx_stream_kernel (images this small march 16-row segments)"""
        return {(s, g): _count_region(self, s * STRIP_W, (s + 1) * STRIP_W, g * SEG_H, (g + 1) * SEG_H)[:2]
                for g in range((self.h + SEG_H - 1) // SEG_H) for s in range((self.w + STRIP_W - 1) // STRIP_W)}

    def describe(self, y, x, ch):
        """of the image's pixel (x, y), channel ch: what a failure message says"""
        j, i = y - 1, x - 1
        m = int(self.M[j, i])
        return (f"pixel ({x}, {y}) channel {ch}: d = {int(self.d[j, i, ch])}, M = {m} (saturation class {sat_class(m)}), exact result "
                f"{int(self.result[j, i, ch])}, {self.dist[j, i, ch]:.3e} from a rounding boundary")


def _one(orig, d, m, p, q, adaptive):
    """(exact rounding, distance to the nearest live boundary, distance to the nearest half-integer, on a half-integer) of
    V = orig + (p / q) e d"""
    if d == 0:
        return orig, 0.5, 0.5, False
    if not adaptive or m >= M_ONE:
        den = 2 * q
        nums = ((2 * orig + 1) * q + 2 * p * d,)                 # U = V + 1/2 over den
    else:
        r = math.isqrt(m * _S * _S)
        den = 2 * q * SOBEL_ONE * _S
        base = (2 * orig + 1) * q * SOBEL_ONE * _S
        nums = (base + 2 * p * d * r,) if r * r == m * _S * _S else (base + 2 * p * d * r, base + 2 * p * d * (r + 1))
    fl = [n // den for n in nums]
    exact = len(nums) == 1
    if not exact and fl[0] != fl[1]:                             # a boundary inside the bracket of an irrational: within 1e-17, never seen
        return min(max(max(fl), 0), 255), 0.0, 0.0, False
    num = nums[0]
    f = fl[0]
    near = f + 1 if 2 * (num - f * den) >= den else f            # the nearest integer to U: the boundary V = near - 1/2
    raw = abs(num - near * den)
    live = min(max(near, 1), 255)                                # clampF crosses only the boundaries 0.5 .. 254.5
    dist = abs(num - live * den)
    return min(max(f, 0), 255), float(Fraction(dist, den)), float(Fraction(raw, den)), exact and raw == 0


def classify(img, p, q=1, adaptive=True):
    """img (h, w, 4) uint8, amount p / q (integers, or p a Fraction) -> Classified"""
    if isinstance(p, Fraction):
        p, q = p.numerator, p.denominator
    h, w = img.shape[:2]
    assert h >= 3 and w >= 3
    a = img.astype(np.int64)
    c = a[..., :3]
    s = np.zeros((h - 2, w - 2, 3), np.int64)
    for dy in range(3):
        for dx in range(3):
            s += (1, 2, 1)[dy] * (1, 2, 1)[dx] * c[dy:h - 2 + dy, dx:w - 2 + dx]
    orig = c[1:h - 1, 1:w - 1]
    d = orig - ((s + 8) >> 4)
    lum = 299 * a[..., 0] + 587 * a[..., 1] + 114 * a[..., 2]
    at = lambda dx, dy: lum[1 + dy:h - 1 + dy, 1 + dx:w - 1 + dx]
    gx = -at(-1, -1) + at(1, -1) - 2 * at(-1, 0) + 2 * at(1, 0) - at(-1, 1) + at(1, 1)
    gy = -at(-1, -1) - 2 * at(0, -1) - at(1, -1) + at(-1, 1) + 2 * at(0, 1) + at(1, 1)
    m = gx * gx + gy * gy
    key = (m[..., None] << 17) | ((d + 255) << 8) | orig
    uniq, inv = np.unique(key.reshape(-1), return_inverse=True)
    res = np.empty(len(uniq), np.int64)
    dist = np.empty(len(uniq))
    raw = np.empty(len(uniq))
    tie = np.empty(len(uniq), bool)
    for i, k in enumerate(uniq.tolist()):
        res[i], dist[i], raw[i], tie[i] = _one(k & 255, ((k >> 8) & 511) - 255, k >> 17, p, q, adaptive)
    out = Classified(w, h)
    shape = (h - 2, w - 2, 3)
    out.d, out.M = d, m
    out.result, out.dist, out.raw, out.tie = res[inv].reshape(shape), dist[inv].reshape(shape), raw[inv].reshape(shape), tie[inv].reshape(shape)
    return out


# ------------------------------------------------------------------ the cases
class Case:
    def __init__(self, name, make, strength, kind, **kw):
        self.name, self._make, self.strength, self.kind = name, make, strength, kind
        self.amount = Fraction(strength) * 2 + 1                 # AdaptiveSharpen's amount (effects.go:63); strengths here are dyadic
        self.__dict__.update(kw)
        self._img = self._cl = None

    @property
    def img(self):
        if self._img is None:
            self._img = self._make()
            self._img.setflags(write=False)
        return self._img

    @property
    def cl(self):
        if self._cl is None:
            self._cl = classify(self.img, self.amount)
        return self._cl

    def __repr__(self):
        return self.name


RGB = (0, 3, 1)                                                  # channel offsets: 1000 * luminance differs, the gradients do not


def _cases():
    c = []
    add = lambda *a, **k: c.append(Case(*a, **k))
    # kind "ties": at least 40 % of the interior samples are exact ties; "control": none is; "sat": the classes around |Sobel| = 400;
    # "half": a dense and a quiet half; "cap": a list filled to its cap (n == cap) or one past it; "soft": nothing crafted
    for off, tag in (((0, 0, 0), "grey"), (RGB, "rgb")):
        add(f"ramp10_amp2_{tag}", lambda off=off: ramp_rows(64, 24, 10, 2, offsets=off), 0.75, "ties")
        add(f"ramp10_amp1_{tag}", lambda off=off: ramp_rows(64, 24, 10, 1, offsets=off), 0.75, "ties")
        add(f"ramp20_{tag}", lambda off=off: ramp_rows(130, 50, 20, 2, offsets=off), 0.125, "ties")
        add(f"ramp25_{tag}", lambda off=off: ramp_rows(125, 49, 25, 2, offsets=off), 1.0, "ties")
        add(f"ramp10_control_{tag}", lambda off=off: ramp_rows(64, 24, 10, 2, offsets=off), 0.25, "control")
        add(f"pyth_{tag}", lambda off=off: pythagorean(130, 50, offsets=off), 0.75, "ties")
        add(f"steps_2.5_{tag}", lambda off=off: step_edges(64, 24, 5, offsets=off), 0.75, "sat")
        add(f"steps_3.0_{tag}", lambda off=off: step_edges(64, 24, 5, offsets=off), 1.0, "sat")
    add("steps_2.0_big", lambda: step_edges(200, 150, 9), 0.5, "sat")
    add("steps_2.5_big", lambda: step_edges(200, 150, 9), 0.75, "sat")
    for side in ("left", "right", "top", "bottom"):
        add(f"half_{side}", lambda side=side: half_and_half(ramp_rows(200, 150, 10, 2, offsets=RGB), soft(200, 150, 31), side), 0.75, "half", side=side)
    add("half_pyth_right", lambda: half_and_half(pythagorean(200, 150), soft(200, 150, 32), "right"), 0.75, "half", side="right")
    for n in (TILE_CAP, TILE_CAP + 1):
        add(f"cap_tile_inner_{n}", lambda n=n: cap_tile(n, (1, 1)), 0.75, "cap", n=n, where=("tile", (1, 1)))
        add(f"cap_tile_edge_{n}", lambda n=n: cap_tile(n, (0, 0), RGB), 0.75, "cap", n=n, where=("tile", (0, 0)))
    for n in (SEG_CAP, SEG_CAP + 1):
        add(f"cap_segment_{n}", lambda n=n: cap_segment(n, 1, 1, RGB), 0.75, "cap", n=n, where=("segment", (1, 1)))
    add("soft_64x48", lambda: soft(64, 48, 3), 0.75, "soft")
    add("soft_131x77", lambda: soft(131, 77, 4), 0.5, "soft")
    return c


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


# ------------------------------------------------------------------ Sharpen amounts
def sharpen_amounts():
    """{name: amount}: amounts of Sharpen's table whose products A d come within build_rtab's 1e-6 of a half-integer without
    being one -- the fp64 kernel's share -- and the exact ties beside them"""
    inf = math.inf
    return {
        "1.5": 1.5, "2.5": 2.5,
        "1.5+ulp": math.nextafter(1.5, inf), "1.5-ulp": math.nextafter(1.5, -inf),
        "2.5+ulp": math.nextafter(2.5, inf), "2.5-ulp": math.nextafter(2.5, -inf),
        "1.5+1e-9": 1.5 + 1e-9, "1.5-1e-9": 1.5 - 1e-9,
        # 251 A == 502.5 + 1e-8, and d / 502 is at least 1 / 502 from 1/2 (mod 1) for every other |d| <= 255: the only near-tie is at
        # |d| == 251, which no image reaches (|orig - blur| <= 191: the centre weighs a quarter)
        "far_d": (502.5 + 1e-8) / 251.0,
    }


NEAR_TIE = ("1.5+ulp", "1.5-ulp", "2.5+ulp", "2.5-ulp", "1.5+1e-9", "1.5-1e-9", "far_d")


def table_rule(img, amount):
    """Sharpen as effects.hip's table states it: clamp(orig + floor(fl(A d) + 0.5)) on the interior -- in Python floats, one product each"""
    h, w = img.shape[:2]
    cl = classify(img, 1, 1, adaptive=False)
    tab = {d: math.floor(amount * float(d)) + (1 if amount * float(d) - math.floor(amount * float(d)) >= 0.5 else 0) for d in range(-255, 256)}
    lut = np.array([tab[d] for d in range(-255, 256)], np.int64)
    out = img.copy()
    out[1:h - 1, 1:w - 1, :3] = np.clip(img[1:h - 1, 1:w - 1, :3].astype(np.int64) + lut[cl.d + 255], 0, 255)
    return out


def strength_for_amount(target):
    """a public strength s with 1.0 + s * 1.5 == target in fp64 (effects.go:24), by search around (target - 1) / 1.5; None if there is none"""
    s = (target - 1.0) / 1.5
    lo = s
    for _ in range(16):
        lo = math.nextafter(lo, -math.inf)
    for _ in range(33):
        if 0.0 < lo <= 1.0 and 1.0 + lo * 1.5 == target:
            return lo
        lo = math.nextafter(lo, math.inf)
    return None
