"""Pairs that differ in one place: the per-window net under the windowed-SSIM kernels (helpers, no tests).

If `b` equals `a` except inside a small region, every window that does not overlap the region has
2 mu_a mu_b == mu_a^2 + mu_b^2 and 2 sigma_ab == sigma_aa + sigma_bb term for term: its value is exactly 1.0.  Then

    D = N * (1 - mean) = sum over the K affected windows of (1 - s_w)           (N = (w - 8) * (h - 8) windows)

is a sum over K windows only.  A window dropped or counted twice ANYWHERE in the plane moves D by about s_w ~ 1; a wrong
value in an affected window shows undiluted.  The reference D_ref needs no full-plane run: a window's value depends on its
own 8 x 8 pixels only, so `np_restatement.ssim_map` on a crop that holds every affected window gives the same K values.

Geometry (ssim.go:110-111): window (wx, wy), wx < w - 8, wy < h - 8, covers pixels [wx, wx + 8) x [wy, wy + 8).  The image's
last column and last row are sampled by no window, so the "corners" of the probes are the corners of the SAMPLED area:
(0, 0), (w - 2, 0), (0, h - 2), (w - 2, h - 2) -- each seen by exactly one window.
"""
from __future__ import annotations

import math

import numpy as np

import np_restatement as npr
from fennec_amd import synth

DELTA = 170          # what an alteration adds to R, G and B (clipped): >= 120 of luminance on every background() pixel
FP64_BAR = 1e-9      # SURVEY Appendix A, SSIM_TOL: the fp64 routes' tolerance, held per window here


# ---------------------------------------------------------------------------------------------- inputs
def background(w: int, h: int, seed: int) -> np.ndarray:
    """Non-flat opaque content: makeTestImage's two gradients at half amplitude plus a few levels of seeded noise per
    channel.  Every pixel differs from its neighbours (a window read from the wrong place does not pass for the right
    one) while the local variance stays far below C2 = 58.5, so that ONE altered pixel seen through the window's
    smallest weight (5.8e-5, the corner probes) still moves its window by more than 1e-2."""
    g = synth.make_test_image(w, h)
    n = synth.noise_image(w, h, seed)
    img = np.empty((h, w, 4), dtype=np.uint8)
    img[..., 0] = g[..., 0] // 2 + (n[..., 0] >> 5)
    img[..., 1] = g[..., 1] // 2 + (n[..., 1] >> 5)
    img[..., 2] = 40 + (n[..., 2] >> 4)
    img[..., 3] = 255
    return img


def tiled_background(w: int, h: int, seed: int, tw: int = 2601, th: int = 1703) -> np.ndarray:
    """background(tw, th, seed) repeated to w x h: 8K planes without half a gigabyte of index grids"""
    t = background(min(tw, w), min(th, h), seed)
    return np.ascontiguousarray(np.tile(t, (-(-h // t.shape[0]), -(-w // t.shape[1]), 1))[:h, :w])


def sparse(probes):
    """A probe list without the one-pixel sweeps over the first seam and the plane's last columns and rows (big planes
    of a route whose sweeps another case runs): corners, edges, lines, the far pixel and the sweep over the LAST strip stay."""
    return [p for p in probes if not p[0].startswith(("seam", "last_cols", "last_rows"))]


def altered_block(a: np.ndarray, box, delta: int = DELTA) -> np.ndarray:
    """The pixels of `a` inside box = (x0, y0, x1, y1) (inclusive) with `delta` added to R, G, B (clipped)."""
    x0, y0, x1, y1 = box
    blk = a[y0:y1 + 1, x0:x1 + 1].copy()
    blk[..., :3] = np.clip(blk[..., :3].astype(np.int32) + delta, 0, 255).astype(np.uint8)
    return blk


def _with(a, box, delta):
    x0, y0, x1, y1 = box
    b = a.copy()
    b[y0:y1 + 1, x0:x1 + 1] = altered_block(a, box, delta)
    return b


def patch_box(x, y, pw, ph):
    return (x, y, x + pw - 1, y + ph - 1)


def patch(a, x, y, pw, ph, delta: int = DELTA):
    return _with(a, patch_box(x, y, pw, ph), delta)


def row_line(a, y, delta: int = DELTA):
    return _with(a, (0, y, a.shape[1] - 1, y), delta)


def col_line(a, x, delta: int = DELTA):
    return _with(a, (x, 0, x, a.shape[0] - 1), delta)


def pixel(a, x, y, delta: int = DELTA):
    return _with(a, (x, y, x, y), delta)


# ---------------------------------------------------------------------------------------------- the reference
def diff_box(a, b):
    """Bounding box (x0, y0, x1, y1), inclusive, of the pixels where a != b (RGB: alpha is not read by toLuminance); None: equal."""
    ne = (a[..., :3] != b[..., :3]).any(axis=2)
    ys = np.flatnonzero(ne.any(axis=1))
    if ys.size == 0:
        return None
    xs = np.flatnonzero(ne.any(axis=0))
    return (int(xs[0]), int(ys[0]), int(xs[-1]), int(ys[-1]))


def crop_of(box, w, h):
    """The pixel rectangle [cx0, cx1) x [cy0, cy1) whose window grid is exactly the windows that overlap `box`: 7 px more
    to the left and above, 8 px more to the right and below (a plane's last column and row are sampled by no window),
    clipped to the image."""
    x0, y0, x1, y1 = box
    return max(x0 - 7, 0), max(y0 - 7, 0), min(x1 + 9, w), min(y1 + 9, h)


def ref_map(a, b, box, kernel=None):
    """ssim_map of the crop around `box`, fp64, and the crop's origin: -> (map, cx0, cy0)"""
    h, w = a.shape[:2]
    cx0, cy0, cx1, cy1 = crop_of(box, w, h)
    k = npr.gaussian_kernel() if kernel is None else np.asarray(kernel, dtype=np.float64).ravel()
    la = npr.to_luminance(a[cy0:cy1, cx0:cx1])
    lb = npr.to_luminance(b[cy0:cy1, cx0:cx1])
    return npr.ssim_map(la, lb, k), cx0, cy0


def d_of_map(m) -> float:
    return math.fsum((1.0 - m).ravel().tolist())


def d_ref(a, b, kernel=None, box=None):
    """-> (D_ref, K): the sum of (1 - s_w) over the K windows that overlap the bounding box of a != b (`box`: the caller
    knows it already), every s_w from ssim_map on the crop, summed with math.fsum."""
    if box is None:
        box = diff_box(a, b)
    if box is None:
        return 0.0, 0
    m, _, _ = ref_map(a, b, box, kernel)
    return d_of_map(m), int(m.size)


def windows(w: int, h: int) -> int:
    return max(w - 8, 0) * max(h - 8, 0)


def d_of(mean: float, w: int, h: int) -> float:
    """N * (1 - mean)"""
    return windows(w, h) * (1.0 - mean)


def fast_planes(orc, a, b):
    """The planes SSIMFast's windows run over (ssim.go:52-58), through the oracle's own functions."""
    h, w = a.shape[:2]
    ds, nw, nh = orc.ssim_fast_dims(w, h)
    if ds:
        return orc.box_downsample(a, nw, nh), orc.box_downsample(b, nw, nh)
    return a, b


def msssim_planes(orc, a, b, levels: int = 5):
    """Per MSSSIM level (ssim.go:344-362): the SSIMFast planes of the level's 2 x 2 pyramid images."""
    out = []
    ac, bc = np.ascontiguousarray(a), np.ascontiguousarray(b)
    for i in range(levels):
        out.append(fast_planes(orc, ac, bc))
        nw, nh = ac.shape[1] // 2, ac.shape[0] // 2
        if nw < 8 or nh < 8:
            break
        ac, bc = orc.box_downsample(ac, nw, nh), orc.box_downsample(bc, nw, nh)
    return out


# ---------------------------------------------------------------------------------------------- the bound
def floor(n: float, adds: int, local=(), background_ulps: float = 0.0) -> float:
    """What fp64 summation alone may move D by -- derived, not tuned.

    Every partial sum is <= N, so an fp64 addition with a non-integer operand rounds by at most ulp(N) / 2; `adds` is the
    longest chain of such additions between a workgroup's result and the mean.  `local` = ((count, bound), ...) are the
    additions BEFORE that, inside a lane, wave or workgroup, whose partial sums cannot exceed `bound` (the windows the
    unit owns): each rounds by at most ulp(bound) / 2 -- stricter than charging them ulp(N) / 2.  Plus N * 2^-53 each for
    the library's division sum / N and the test's 1 - mean.  `background_ulps`: routes whose UNaffected windows may
    return 1 only to the last bit are granted that many units of N * 2^-52 (windowed_ssim_march2_kernel: four windows
    share one division, P / Q, ssim.hip:1407-1416).

    Chains, read off ssim.hip / devutil.hpp (block_sum_256, devutil.hpp:126-137: 6 shuffle steps + 3 = 9):
      finish (all routes)   finish_sum_256, ssim.hip:1071-1082: ceil(items / 2048) per accumulator, 3 for the eight
                            accumulators, 9 for block_sum_256                         -> `finish_adds(items)`
      windowed_ssim_kernel  one window per lane; block_sum_256 (ssim.hip:581), sums <= 256 windows         local (9, 256)
      sep / sep_multi       2 windows per lane (ssim.hip:763), 6 shuffles + 3 waves (ssim.hip:769-776)     local (11, 512)
      sep24                 3 windows per lane (ssim.hip:1000), 6 + 3 (ssim.hip:1005-1011)                 local (12, 768)
      march, march2(f)      a lane adds one window per row of its segment (ssim.hip:1224, 1404-1415, 1657-1667: <= h
                            additions of sums <= 2 h), then 6 shuffles over the wave's <= 121 columns (ssim.hip:1091)
                                                                                      local (h + 1, 2 h), (6, 128 h)
    """
    n = float(n)
    if n <= 0:
        return 0.0
    t = adds * math.ulp(n) / 2
    for count, bound in local:
        t += count * math.ulp(float(bound)) / 2
    return t + 2 * n * 2.0 ** -53 + background_ulps * n * 2.0 ** -52


def finish_adds(items: int) -> int:
    return -(-int(items) // 2048) + 3 + 9


def agrees(d_gpu: float, d_want: float, k: int, bar: float, flo: float) -> bool:
    """The comparison every probe test makes: |D_gpu - D_ref| <= K * bar + floor"""
    return abs(d_gpu - d_want) <= k * bar + flo


# ---------------------------------------------------------------------------------------------- probe sets
def overlap_count(box, w, h) -> int:
    """Closed form of K: the windows (wx < w - 8, wy < h - 8) whose 8 x 8 pixels meet `box`."""
    x0, y0, x1, y1 = box
    nx = min(x1, w - 9) - max(x0 - 7, 0) + 1
    ny = min(y1, h - 9) - max(y0 - 7, 0) + 1
    return max(nx, 0) * max(ny, 0)


def probe_boxes(w: int, h: int, xpitch: int, ypitch=()):
    """[(name, box)] for one w x h plane of a route whose strips / tiles are `xpitch` window columns wide and (tile
    kernels) whose tile rows and inner rounds start every `ypitch` window rows:
      corners and mid-edges of the sampled area, one pixel each; a pixel row and a pixel column through the middle and one
      each across the first seam; an 8 x 8 patch stepped one
      pixel at a time over x = c - 9 .. c + 1 for c = xpitch and for c = the last strip's first column, over the plane's
      last columns, over y = c - 9 .. c + 1 for every c of ypitch and over the plane's last rows; one far pixel."""
    xm, ym = w // 2 + 3, h // 2 + 5
    out = [("corner_tl", (0, 0, 0, 0)), ("corner_tr", (w - 2, 0, w - 2, 0)), ("corner_bl", (0, h - 2, 0, h - 2)),
           ("corner_br", (w - 2, h - 2, w - 2, h - 2)), ("unsampled_br", (w - 1, h - 1, w - 1, h - 1)),
           ("edge_t", (xm, 0, xm, 0)), ("edge_b", (xm, h - 2, xm, h - 2)), ("edge_l", (0, ym, 0, ym)), ("edge_r", (w - 2, ym, w - 2, ym)),
           ("row_line", (0, ym, w - 1, ym)), ("col_line", (xm, 0, xm, h - 1)),
           ("far_pixel", ((2 * w) // 3 + 1, (3 * h) // 4 + 2, (2 * w) // 3 + 1, (3 * h) // 4 + 2))]
    if xpitch + 3 < w - 1:                                # a pixel column / row whose 8 window columns / rows straddle the first seam
        out.append(("col_line_seam", (xpitch + 3, 0, xpitch + 3, h - 1)))
    if ypitch and ypitch[0] + 3 < h - 1:
        out.append(("row_line_seam", (0, ypitch[0] + 3, w - 1, ypitch[0] + 3)))
    ww = w - 8
    last = ((ww - 1) // xpitch) * xpitch                  # first window column of the last strip
    ysw = min(ym, h - 9)
    for tag, c in (("seam_x", xpitch), ("last_strip_x", last)):
        if c - 9 < 0 or c + 1 + 8 > w:
            continue
        for x in range(c - 9, c + 2):
            out.append((f"{tag}{c}@{x}", patch_box(x, ysw, 8, 8)))
    for x in range(w - 19, w - 8 + 1):                    # up to the last column
        out.append((f"last_cols@{x}", patch_box(x, ysw, 8, 8)))
    xsw = min(xm, w - 9)
    for c in ypitch:
        if c - 9 < 0 or c + 1 + 8 > h:
            continue
        for y in range(c - 9, c + 2):
            out.append((f"seam_y{c}@{y}", patch_box(xsw, y, 8, 8)))
    for y in range(h - 19, h - 8 + 1):
        out.append((f"last_rows@{y}", patch_box(xsw, y, 8, 8)))
    seen, uniq = set(), []
    for name, box in out:                                 # (sweeps overlap on small planes)
        if box not in seen:
            seen.add(box)
            uniq.append((name, box))
    return uniq
