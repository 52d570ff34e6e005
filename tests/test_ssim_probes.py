"""The probe method of tests/ssim_probe.py held against the reference before any kernel is judged by it (no GPU):
the crop reference equals the full-plane reference, unaffected windows are exactly 1.0, every probe the GPU file uses
moves its windows by enough, K has its closed form, and the comparison the GPU tests make REJECTS a reference with one
window removed, one counted twice or one value moved by 1e-6."""
import math

import numpy as np
import pytest

import np_restatement as npr
import ssim_probe as sp

# the planes of tests/test_ssim_probes_gpu.py whose size does not depend on the device (the sep24 plane is 1400 wide and
# about 920 high: its probes are those of 1400 x 923, the height 256 CUs give)
GPU_PLANES = [("windowed_ssim_kernel small", 301, 203, 32, (8,)), ("windowed_ssim_sep_kernel", 641, 483, 32, (16,)),
              ("windowed_ssim_sep24_kernel", 1400, 923, 32, (24, 16, 24 + 16)), ("windowed_ssim_march_kernel", 1921, 1083, 57, ()),
              ("windowed_ssim_march2(f)_kernel / 64-tap big", 2601, 1703, 121, (8,)), ("batch", 1025, 771, 57, ()),
              ("two-column kernels at 8K", 7680, 4320, 121, ())]


def _full_map(a, b):
    return npr.ssim_map(npr.to_luminance(a), npr.to_luminance(b), npr.gaussian_kernel())


@pytest.mark.parametrize("kind", ["patch", "row_line", "col_line"])
def test_crop_reference_is_the_full_plane_reference(orc, kind):
    w, h = 700, 500
    a = sp.background(w, h, 1)
    b = {"patch": lambda: sp.patch(a, 311, 207, 9, 5), "row_line": lambda: sp.row_line(a, 133),
         "col_line": lambda: sp.col_line(a, 402)}[kind]()
    d, k = sp.d_ref(a, b)
    box = sp.diff_box(a, b)
    assert k == sp.overlap_count(box, w, h)
    assert k == {"patch": (9 + 7) * (5 + 7), "row_line": 8 * (w - 8), "col_line": 8 * (h - 8)}[kind]
    # the same K values, bit for bit, as the full plane's; every other window is exactly 1.0
    full = _full_map(a, b)
    m, cx0, cy0 = sp.ref_map(a, b, box)
    assert np.array_equal(full[cy0:cy0 + m.shape[0], cx0:cx0 + m.shape[1]], m)
    rest = full.copy()
    rest[cy0:cy0 + m.shape[0], cx0:cx0 + m.shape[1]] = 1.0
    assert np.all(rest == 1.0)
    assert np.all(m != 1.0)
    n = sp.windows(w, h)
    # the oracle sums N values one after the other (procs = 1) or in 8 chains: N additions charged at ulp(N) / 2
    for procs in (1, 8):
        got = n * (1.0 - orc.ssim(a, b, procs=procs))
        assert sp.agrees(got, d, k, 0.0, sp.floor(n, n)), (procs, got, d)
    assert sp.d_of(orc.ssim(a, b), w, h) == n * (1.0 - orc.ssim(a, b))


def test_identical_pair_and_unsampled_pixel():
    a = sp.background(120, 90, 2)
    assert sp.d_ref(a, a.copy()) == (0.0, 0)
    b = sp.pixel(a, 119, 89)                                   # the last column and row: no window samples them
    assert sp.d_ref(a, b) == (0.0, 0) and np.all(_full_map(a, b) == 1.0)
    b = a.copy()
    b[40:50, 30:40, 3] = 7                                     # alpha is not read
    assert sp.d_ref(a, b) == (0.0, 0)


@pytest.mark.parametrize("name,w,h,xpitch,ypitch", GPU_PLANES, ids=[p[0] for p in GPU_PLANES])
def test_probes_move_their_windows(name, w, h, xpitch, ypitch):
    """Every probe of the GPU file: K is the closed form and the mean of (1 - s_w) over its windows is >= 1e-2 (by the
    reference); the corners of the sampled area are seen by exactly one window."""
    a = sp.background(w, h, 3) if w < 4000 else sp.tiled_background(w, h, 3)
    b = a.copy()
    probes = sp.probe_boxes(w, h, xpitch, ypitch)
    assert len({box for _, box in probes}) == len(probes)
    if w >= 4000:
        probes = sp.sparse(probes)
        assert {"corner_tl", "corner_br", "row_line", "col_line", "col_line_seam", "far_pixel"} <= {n for n, _ in probes}
        assert sum(n.startswith("last_strip_x") for n, _ in probes) == 11
    for pname, box in probes:
        x0, y0, x1, y1 = box
        b[y0:y1 + 1, x0:x1 + 1] = sp.altered_block(a, box)
        d, k = sp.d_ref(a, b, box=box)
        b[y0:y1 + 1, x0:x1 + 1] = a[y0:y1 + 1, x0:x1 + 1]
        bw, bh = x1 - x0 + 1, y1 - y0 + 1
        assert k == sp.overlap_count(box, w, h), pname
        if pname.startswith("corner"):
            assert k == 1
        elif pname == "unsampled_br":
            assert k == 0 and d == 0.0
        elif pname.startswith("row_line"):
            assert k == 8 * (w - 8)
        elif pname.startswith("col_line"):
            assert k == 8 * (h - 8)
        elif pname == "far_pixel":
            assert k == 64
        elif not pname.startswith(("edge", "last_")):
            assert k == (bw + 7) * (bh + 7), pname             # seam patches lie inside the plane
        if k:
            assert d / k >= 1e-2, (name, pname, d / k)
    assert np.array_equal(a, b)


# D of a route's plane at the two sizes the fast-moment tests and config 4 run at: 2600 x 1700 (4.4 M windows), 7680 x 4320
# (33 M).  Floors as the GPU file builds them for the two-column kernels.
@pytest.mark.parametrize("w,h", [(2600, 1700), (7680, 4320)])
@pytest.mark.parametrize("bar,ulps", [(sp.FP64_BAR, 1.0), (1e-6, 0.0)], ids=["fp64", "fp32_moments"])
def test_a_wrong_reference_is_rejected(w, h, bar, ulps):
    n = sp.windows(w, h)
    a = sp.background(600, 400, 4)
    b = sp.patch(a, 200, 150, 8, 8)                            # K = 225 windows, as a seam probe's
    box = sp.diff_box(a, b)
    m, _, _ = sp.ref_map(a, b, box)
    k = int(m.size)
    assert k == 225
    d = sp.d_of_map(m)
    items = -(-(w - 8) // 121) * max(1, (h - 8) // 32)
    flo = sp.floor(n, sp.finish_adds(items), local=((h + 1, 2 * h), (6, 128 * h)), background_ulps=ulps)
    assert flo < 1e-6 / 4                                      # the summation floor is far below one moved value
    # what a GPU returns: a mean, rounded; D taken from it as the tests do
    mean = (n - d) / n
    assert sp.agrees(n * (1.0 - mean), d, k, bar, flo)
    flat = m.ravel()
    j = int(np.argmin(flat))
    gone = math.fsum((1.0 - np.delete(flat, j)).tolist())                 # one window removed from the map
    removed = gone + 1.0                                                  # ... as a kernel loses it: the count stays N
    twice = d - flat[j]                                                   # its value added once more
    far_removed, far_twice = d + 1.0, d - 1.0                             # the same to a window of value 1 anywhere in the plane
    for wrong in (gone, removed, twice, far_removed, far_twice):
        assert not sp.agrees(n * (1.0 - mean), wrong, k, bar, flo), (wrong, d)
    if bar == sp.FP64_BAR:
        for moved in (d + 1e-6, d - 1e-6):
            assert not sp.agrees(n * (1.0 - mean), moved, k, bar, flo)
    # ... and through the mean, as every earlier test compares, all of them pass: |delta mean| <= 1 / N
    tol = 1e-9 if bar == sp.FP64_BAR else 1e-6
    if bar != sp.FP64_BAR:
        assert abs(((n - far_removed) / n) - mean) <= tol and abs(((n - twice) / n) - mean) <= tol
    assert abs(((n - (d + 1e-6)) / n) - mean) <= 1e-9


def test_fast_and_pyramid_planes_follow_the_oracle(orc):
    """SSIMFast / MSSSIM probes take D_ref on the planes the reference derives: the mean over those planes is the oracle's."""
    w, h = 1360, 752
    a = sp.background(w, h, 5)
    b = sp.patch(a, 600, 300, 40, 36)
    pa, pb = sp.fast_planes(orc, a, b)
    d, k = sp.d_ref(pa, pb)
    n = sp.windows(pa.shape[1], pa.shape[0])
    assert k > 0 and d / k >= 1e-2
    assert sp.agrees(n * (1.0 - orc.ssim_fast(a, b)), d, k, 0.0, sp.floor(n, n))
    _, lv = orc.msssim(a, b, per_level=True)
    planes = sp.msssim_planes(orc, a, b)
    assert len(planes) == int(np.sum(~np.isnan(lv)))
    for (qa, qb), s in zip(planes, lv):
        n = sp.windows(qa.shape[1], qa.shape[0])
        d, k = sp.d_ref(qa, qb)
        assert sp.agrees(n * (1.0 - s), d, k, 0.0, sp.floor(n, n))
