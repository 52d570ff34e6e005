"""medianCut (targetsize.go:352-486) restated in numpy under the library's tie rule, and the cases every median-cut test shares.

The rule (include/fennec_hip.h, above fnx_median_cut): samples are the R, G, B of every step-th flat 4-byte group; a split takes
the FIRST box of the largest score among those with two samples or more, the reference's axis, and orders the box by
(value on the axis, sample number j); the first count // 2 replace the box, the rest are appended.  Go's sort.Slice leaves tied
samples in whatever order pdqsort produces, so any tie order is a reference answer; the library fixes ascending j.

median_cut() caches each box's minima, maxima and sums (a naive restatement took seconds on the largest case) and keeps the
score in Python ints.  It also counts the splits whose median straddles a tie -- the sorted box's elements mid - 1 and mid carry
the same axis value -- which are the only splits where another tie order gives other halves."""
from __future__ import annotations

import numpy as np

LEVELS = (16, 32, 64, 128, 256)
MAX_SAMPLES = 100000


def sample_step(w: int, h: int) -> int:
    n = int(w) * int(h)
    return n // MAX_SAMPLES if n > MAX_SAMPLES else 1


def samples(img: np.ndarray) -> np.ndarray:
    """(ns, 3) uint8: the flat group at byte 4 j step for j step < w h (targetsize.go:426-441: `off := i*4` into Pix)"""
    h, w = img.shape[:2]
    flat = np.ascontiguousarray(img).reshape(-1, 4)
    return flat[::sample_step(w, h), :3]


class _Box:
    __slots__ = ("idx", "mn", "mx", "sums")

    def __init__(self, px: np.ndarray, idx: np.ndarray):
        self.idx = idx
        sub = px[idx]
        self.mn = sub.min(axis=0)
        self.mx = sub.max(axis=0)
        self.sums = sub.sum(axis=0)

    def score(self) -> int:
        r = [int(self.mx[c]) - int(self.mn[c]) + 1 for c in range(3)]
        return r[0] * r[1] * r[2] * len(self.idx)

    def axis(self) -> int:
        r, g, b = (int(self.mx[c]) - int(self.mn[c]) for c in range(3))
        if r >= g and r >= b:
            return 0
        return 1 if g >= b else 2

    def entry(self):
        n = len(self.idx)
        return (int(self.sums[0]) // n, int(self.sums[1]) // n, int(self.sums[2]) // n, 255)


def median_cut(img: np.ndarray, levels=LEVELS, trace: list | None = None):
    """-> (palettes: one (ncolors, 4) uint8 array per level, straddles: splits whose median falls inside a run of equal values).
    trace, when given, receives per split (axis, left values on the axis, right values on the axis, count)."""
    levels = [int(c) for c in levels]
    assert levels and all(1 <= c <= 256 for c in levels) and all(a < b for a, b in zip(levels, levels[1:]))
    h, w = img.shape[:2]
    if w * h == 0:
        return [np.array([[0, 0, 0, 255]], dtype=np.uint8) for _ in levels], 0
    px = samples(img).astype(np.int64)
    boxes = [_Box(px, np.arange(len(px)))]
    out, straddles = [], 0

    def palette():
        return np.array([b.entry() for b in boxes], dtype=np.uint8).reshape(-1, 4)

    for want in levels:
        while len(boxes) < want:
            best, best_score = -1, -1
            for i, b in enumerate(boxes):
                if len(b.idx) < 2:
                    continue
                s = b.score()
                if s > best_score:
                    best, best_score = i, s
            if best < 0:
                break
            b = boxes[best]
            axis = b.axis()
            vals = px[b.idx, axis]
            order = np.lexsort((b.idx, vals))           # by value, then by sample number: the library's tie rule
            mid = len(order) // 2
            svals = vals[order]
            straddles += int(svals[mid - 1] == svals[mid])
            if trace is not None:
                trace.append((axis, svals[:mid].copy(), svals[mid:].copy(), len(order)))
            sidx = b.idx[order]
            boxes[best] = _Box(px, sidx[:mid])
            boxes.append(_Box(px, sidx[mid:]))
        out.append(palette())
    return out, straddles


def median_cut_other_ties(img: np.ndarray, max_colors: int) -> np.ndarray:
    """targetsize.go:422-486 line by line, one call per palette size, on Python lists, with sorted(key=value) over the box in
    REVERSED order: tied samples come out in descending sample number -- another tie order than median_cut()'s."""
    h, w = img.shape[:2]
    pix = np.ascontiguousarray(img).reshape(-1)
    max_samples = 100000
    step = 1
    if w * h > max_samples:
        step = (w * h) // max_samples
        if step < 1:
            step = 1
    pixels = []
    for i in range(0, w * h, step):
        off = i * 4
        if off + 3 < len(pix):
            pixels.append((int(pix[off]), int(pix[off + 1]), int(pix[off + 2])))
    if not pixels:
        return np.array([[0, 0, 0, 255]], dtype=np.uint8)

    def rng(box, c):
        return max(p[c] for p in box) - min(p[c] for p in box)

    boxes = [pixels]
    while len(boxes) < max_colors:
        best_idx, best_score = -1, -1
        for i, box in enumerate(boxes):
            if len(box) < 2:
                continue
            score = (rng(box, 0) + 1) * (rng(box, 1) + 1) * (rng(box, 2) + 1) * len(box)
            if score > best_score:
                best_score, best_idx = score, i
        if best_idx == -1:
            break
        box = boxes[best_idx]
        r, g, b = rng(box, 0), rng(box, 1), rng(box, 2)
        axis = 0 if (r >= g and r >= b) else (1 if g >= b else 2)
        box = sorted(reversed(box), key=lambda p: p[axis])
        mid = len(box) // 2
        boxes[best_idx] = box[:mid]
        boxes.append(box[mid:])
    pal = []
    for box in boxes:
        n = len(box)
        pal.append((sum(p[0] for p in box) // n, sum(p[1] for p in box) // n, sum(p[2] for p in box) // n, 255))
    return np.array(pal, dtype=np.uint8)


# ---- the cases: the smallest shapes at which each step can go wrong ----------------------------------------------------
def _rgb(rows, alpha=255):
    a = np.array(rows, dtype=np.uint8)
    return np.concatenate([a, np.full(a.shape[:2] + (1,), alpha, np.uint8)], axis=2)


def _noise(w, h, seed, alpha=None):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha is not None:
        img[:, :, 3] = alpha
    return img


def tie_free_16x16():
    """R, G and B planes are three independent permutations of 0..255, alpha random: no two samples share a value on any axis,
    so the reference's answer is unique"""
    rng = np.random.default_rng(20260)
    img = np.empty((16, 16, 4), dtype=np.uint8)
    for c in range(3):
        img[:, :, c] = rng.permutation(256).astype(np.uint8).reshape(16, 16)
    img[:, :, 3] = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    return img


def _two_colours():
    rng = np.random.default_rng(7)
    img = np.empty((64, 64, 4), dtype=np.uint8)
    pick = rng.integers(0, 2, (64, 64)).astype(bool)
    img[pick] = (200, 30, 40, 255)
    img[~pick] = (10, 220, 90, 255)
    return img


def _build_cases():
    c = {}
    c["1x1"] = (_rgb([[(9, 8, 7)]]), LEVELS)
    c["2x1"] = (_rgb([[(1, 2, 3), (200, 100, 50)]]), LEVELS)
    c["5x2_random"] = (_noise(5, 2, 1), LEVELS)
    c["score_tie_8x1"] = (_rgb([[(r, 0, 0) for r in (0, 0, 10, 10, 100, 100, 110, 110)]]), (2, 3))
    c["range_tie_2x2"] = (_rgb([[(0, 0, 0), (10, 10, 0)], [(0, 10, 0), (10, 0, 0)]]), (2,))
    c["median_tie_3x2"] = (_rgb([[(5, 0, 0), (5, 9, 0), (5, 0, 9)], [(5, 9, 9), (0, 4, 4), (10, 4, 4)]]), (2,))
    c["flat_16x16"] = (np.full((16, 16, 4), (37, 99, 200, 255), dtype=np.uint8), LEVELS)
    c["two_colours_64x64"] = (_two_colours(), LEVELS)
    c["tie_free_16x16"] = (tie_free_16x16(), LEVELS)
    c["noise_64x64"] = (_noise(64, 64, 31), LEVELS)     # this seed: 75 splits straddle a tie
    c["noise_alpha0_40x30"] = (_noise(40, 30, 3, alpha=0), LEVELS)
    c["noise_317x317"] = (_noise(317, 317, 4), LEVELS)
    c["noise_448x447"] = (_noise(448, 447, 5), LEVELS)
    c["noise_447x447"] = (_noise(447, 447, 6), LEVELS)
    # the partition's tile of 8192 samples: a first box of exactly one tile; one sample more; and a box of fewer samples than a tile
    # that still straddles two (16381 samples: the right half starts at sample 8190, two past a 16-byte group, and holds 8191)
    c["noise_128x64"] = (_noise(128, 64, 8), LEVELS)
    c["noise_8193x1"] = (_noise(8193, 1, 9), LEVELS)
    c["noise_16381x1"] = (_noise(16381, 1, 10), LEVELS)
    return c


CASES = _build_cases()
_WANT = {}


def want(name):
    """(palettes, straddles) of a case: computed once, shared by every test that needs it"""
    if name not in _WANT:
        img, levels = CASES[name]
        _WANT[name] = median_cut(img, levels)
    return _WANT[name]
