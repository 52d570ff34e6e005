"""Every windowed-SSIM route of launch_windowed_ssim (csrc/ssim.hip) held PER WINDOW, on pairs that differ in one place.

The other GPU tests of these kernels compare one number per plane -- the mean over all windows -- on pairs that differ
everywhere; a mean over N windows divides every local error by N.  Here `b` equals `a` except inside a small region, so
every unaffected window is exactly 1.0 and

    D = N * (1 - mean) = sum over the K affected windows of (1 - s_w)

is compared with the reference's D (tests/ssim_probe.py: np_restatement.ssim_map on the crop that holds the K windows):

    |D_gpu - D_ref| <= K * bar + floor(N, additions of the route's reduction)

A window dropped or counted twice anywhere in the plane moves D by about 1; a wrong value in an affected window shows
undiluted.  bar = 1e-9 for the fp64 routes (now per window); for the fp32-moment route see
FAST_BAR below.  Every case first asserts the route by name (`ctx.last_kernel(PROF_SSIM)`) and SSIM(a, a) == 1.0 on it.

Tile and strip pitches, stated here from the source and not imported from the library (csrc/ssim.hip):
  WS_TX 32, WS_TY 8 (:513)   WSS_TX 32, WSS_TY 16 (:590)   W24_TY 24, W24_R1 16 (:895)   WM_COLS 57 (:1035)   WM2_COLS 121 (:1252)
Thresholds (:1703-1714): rank-1 windows take the marching kernels from 1.5 M windows x images (two columns per lane from
4 M windows of ONE plane), the 32 x 24 tile kernel from 4096 x CUs, the 32 x 16 one below; other windows the 64-tap kernel.

That the file bites: three mutants of ssim.hip that change arithmetic only (built aside, nothing of them is kept), each run
once on an MI355X against the 100 SSIM / config tests the suite had (`-k "ssim or SSIM or config"`) and against this file:

  mutant                                                              the 100 earlier tests                this file
  (a) march2f: a segment's last window row left out of the sum        16 fail (every 4.4 M / 8K fast-mode   test_march2f_kernel, _at_8k: the first check,
                                                                      case: the pairs differ everywhere)   SSIM(a, a) == 1.0, gives 0.9693
  (b) march2: one column weight x (1 + 1e-5) in the lane on a         14 fail (1e-9 on the mean sees it:    test_march2_kernel, _at_8k, test_batch_enqueue[2601-1703-2]:
      strip's last column                                             every 121st column is off)           22 probes named, seam_x121@113 .. @121, row_line
  (c) sep24: a tile's first window row added twice                    1 fails: test_ssim_and_sharpen_       test_sep24_kernel, test_batch_enqueue[641-483-4]
                                                                      batches[640-480], whose batch of 5   (SSIM(a, a) = 1.0426)
                                                                      (1.49 M windows) takes sep24
  (d) march2f: as (a), but ONE lane of ONE wave: two windows per      1 fails: the 8K case's SSIM(img, img) test_march2f_kernel, _at_8k (SSIM(a, a) =
      plane                                                           == 1.0 in fast mode; all eleven      0.99999954 and 0.99999994: D = 2.0 both times)
                                                                      4.4 M-window cases pass (2 / N < 1e-6)

(b) was expected to pass the earlier tests and (c) to meet none of their shapes; the run says otherwise for both: a relative
weight error of 1e-5 moves the windows of a pair that differs everywhere by far more than 1e-9 x 121, and n = 5 images of
640 x 480 lie inside sep24's band.  (d) is the case the mean cannot see at 4.4 M windows; the earlier suite holds it only where
it asserts SSIM(img, img) == 1.0 on that route.  What the earlier tests cannot do is NAME the place: here (b) fails at
seam_x121@113 .. @121 and nowhere else.

Cost on one MI355X, one run, the same library: this file's 19 tests 3.2 s of test calls (5.95 s with start-up);
test_ssim_fast_moments, all 11 cases, 4.0 s (6.4 s).
"""
import numpy as np
import pytest

import fennec_amd
import ssim_probe as sp

pytestmark = pytest.mark.gpu

MARCH_MIN, MARCH2_MIN = 1_500_000, 4_000_000        # ssim.hip:1703, :1711

# The fp32-moment route (windowed_ssim_march2f_kernel).  Its stated tolerance, 1e-6 (fennec_hip.h), was
# only ever measured on the MEAN, where per-window errors average out.  Measured here per window, against the reference
# (never against the fp64 kernel): max |D_gpu - D_ref| / K over all probes of this file = FAST_MEASURED (the 8 x 8 patch over
# the plane's last columns, last_cols@2592, K = 120; single windows -- the corners -- are within 2e-8, the far pixel's 64
# within 2.6e-8 each, a whole pixel row within 8.6e-8).  It is <= 1e-6, so the stated tolerance holds per window and is the bar.
FAST_MEASURED = 5.35e-7
FAST_BAR = 1e-6


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


@pytest.fixture(scope="module")
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _non_rank1_window():
    """gaussianKernel(8, 1.5) with weight moved between two taps: still sums to 1, no longer a product row x col"""
    k = sp.npr.gaussian_kernel().copy()
    k[9] += 0.004
    k[18] -= 0.004
    assert k.min() > 0
    return k


def _tiles(w, h, tx, ty):
    return -(-(w - 8) // tx) * -(-(h - 8) // ty)


def _march_items(w, h, cols):
    return -(-(w - 8) // cols) * max(1, (h - 8) // 32)         # segments are never shorter than 32 rows (ssim.hip:1725)


def _floor(route, w, h):
    """ssim_probe.floor with the chains of the route's reduction (read off in floor's docstring)"""
    n = sp.windows(w, h)
    if route == "windowed_ssim_kernel":
        return sp.floor(n, sp.finish_adds(_tiles(w, h, 32, 8)), local=((9, 256),))
    if route in ("windowed_ssim_sep_kernel", "windowed_ssim_sep_multi_kernel"):
        return sp.floor(n, sp.finish_adds(_tiles(w, h, 32, 16)), local=((11, 512),))
    if route == "windowed_ssim_sep24_kernel":
        return sp.floor(n, sp.finish_adds(_tiles(w, h, 32, 24)), local=((12, 768),))
    local = ((h + 1, 2 * h), (6, 128 * h))
    if route == "windowed_ssim_march_kernel":
        return sp.floor(n, sp.finish_adds(_march_items(w, h, 57)), local=local)
    if route == "windowed_ssim_march2_kernel":
        return sp.floor(n, sp.finish_adds(_march_items(w, h, 121)), local=local, background_ulps=1.0)
    assert route == "windowed_ssim_march2f_kernel"
    return sp.floor(n, sp.finish_adds(_march_items(w, h, 121)), local=local)


def _pitched(host, left, right):
    import torch
    w = host.shape[1]
    return torch.from_numpy(np.ascontiguousarray(np.pad(host, ((0, 0), (left, right), (0, 0))))).cuda()[:, left: left + w]


def _run_route(ctx, route, entry, w, h, xpitch, ypitch, call, bar, kernel=None, host_call=None, seed=7, probes=None, a=None,
               pitched=True):
    """All probes of one route through `call(xa, xb) -> mean` (device tensors), one through host arrays (`host_call`) and one
    through pitched device views.  Every failing probe is named in the assertion: its position names the seam."""
    import torch
    a = sp.background(w, h, seed) if a is None else a
    b = a.copy()
    da = torch.from_numpy(a).cuda()
    db = da.clone()
    flo = _floor(route, w, h)
    # the route, and SSIM(a, a) == 1.0 on it
    assert call(da, db) == 1.0
    assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
    bad, worst, worst_name = [], 0.0, ""
    probes = sp.probe_boxes(w, h, xpitch, ypitch) if probes is None else probes
    for name, box in probes:
        x0, y0, x1, y1 = box
        blk = sp.altered_block(a, box)
        b[y0:y1 + 1, x0:x1 + 1] = blk
        db[y0:y1 + 1, x0:x1 + 1] = torch.from_numpy(blk).cuda()
        want, k = sp.d_ref(a, b, kernel=kernel, box=box)
        got = [("device", sp.d_of(call(da, db), w, h))]
        assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
        if name == "far_pixel" and host_call is not None:
            got.append(("host", sp.d_of(host_call(a, b), w, h)))
            assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
        if name == "row_line" and pitched:
            got.append(("pitched", sp.d_of(call(_pitched(a, 2, 1), _pitched(b, 1, 3)), w, h)))
            assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
        for how, d in got:
            err = abs(d - want)
            print(f"{route} {entry} {w}x{h} {name} {how}: K={k} D_ref={want:.12g} D_gpu={d:.12g} err={err:.3g} floor={flo:.3g}")
            if k and err / k > worst:
                worst, worst_name = err / k, name
            if not sp.agrees(d, want, k, bar, flo):
                bad.append((name, how, k, want, d, err))
        b[y0:y1 + 1, x0:x1 + 1] = a[y0:y1 + 1, x0:x1 + 1]
        db[y0:y1 + 1, x0:x1 + 1] = da[y0:y1 + 1, x0:x1 + 1]
    print(f"SUMMARY {route} {entry} {w}x{h}: {len(probes)} probes, worst |D_gpu - D_ref| / K = {worst:.3g} ({worst_name}), floor {flo:.3g}")
    assert not bad, f"{route} via {entry}, {w}x{h}: {len(bad)} probes off (name, how, K, D_ref, D_gpu, |diff|): {bad[:12]}"
    return worst


def _enqueue(ctx, window=None):
    def call(xa, xb):
        ctx.ssim_enqueue(xa, xb, window=window)
        return ctx.fetch_result()
    return call


def test_sep_kernel(ctx, cus):
    w, h = 641, 483
    assert sp.windows(w, h) < 4096 * cus
    _run_route(ctx, "windowed_ssim_sep_kernel", "SSIM", w, h, 32, (16,), ctx.SSIM, sp.FP64_BAR, host_call=ctx.SSIM)


def test_sep24_kernel(ctx, cus):
    """the band 4096 x CUs <= windows < 1.5 M that no other SSIM test's shape is inside"""
    lo = 4096 * cus
    assert lo < MARCH_MIN, "no band on this device"
    w = 1400
    h = 8 + -(-((lo + MARCH_MIN) // 2) // (w - 8))
    assert lo <= sp.windows(w, h) < MARCH_MIN
    _run_route(ctx, "windowed_ssim_sep24_kernel", "SSIM", w, h, 32, (24, 16, 24 + 16), ctx.SSIM, sp.FP64_BAR, host_call=ctx.SSIM)


def test_march_kernel_blocking(ctx):
    """windowed_ssim_march_kernel<false>: fnx_ssim"""
    w, h = 1921, 1083
    assert MARCH_MIN <= sp.windows(w, h) < MARCH2_MIN
    _run_route(ctx, "windowed_ssim_march_kernel", "SSIM", w, h, 57, (), ctx.SSIM, sp.FP64_BAR, host_call=ctx.SSIM)


def test_march_kernel_enqueued(ctx):
    """windowed_ssim_march_kernel<true> (the <= 96-register build, ctx->partial_slot >= 0): fnx_ssim_enqueue on the second
    stream -- against the reference, not against the blocking form"""
    w, h = 1921, 1083
    _run_route(ctx, "windowed_ssim_march_kernel", "ssim_enqueue", w, h, 57, (), _enqueue(ctx), sp.FP64_BAR)


def test_march2_kernel(ctx):
    """two pixel columns per lane; odd width: the last lane pair of the last strip re-reads two columns"""
    w, h = 2601, 1703
    assert sp.windows(w, h) >= MARCH2_MIN
    _run_route(ctx, "windowed_ssim_march2_kernel", "SSIM", w, h, 121, (), ctx.SSIM, sp.FP64_BAR, host_call=ctx.SSIM)
    _run_route(ctx, "windowed_ssim_march2_kernel", "ssim_enqueue", 2600, 1700, 121, (), _enqueue(ctx), sp.FP64_BAR,
               probes=sp.sparse(sp.probe_boxes(2600, 1700, 121)))


def test_march2f_kernel(ctx):
    """fp32 moments: no window dropped or repeated (the far pixel and the lines need no bar: a shift of ~1 against
    <= K * 1e-6), and the per-window bar FAST_BAR = 1e-6, the route's stated tolerance: measured max |D_gpu - D_ref| / K =
    5.35e-7 over this file's probes, against the reference"""
    w, h = 2601, 1703
    ctx.set_ssim_mode(True)
    try:
        _run_route(ctx, "windowed_ssim_march2f_kernel", "SSIM", w, h, 121, (), ctx.SSIM, FAST_BAR, host_call=ctx.SSIM)
        _run_route(ctx, "windowed_ssim_march2f_kernel", "ssim_enqueue", 2600, 1700, 121, (), _enqueue(ctx), FAST_BAR,
                   probes=sp.sparse(sp.probe_boxes(2600, 1700, 121)))
    finally:
        ctx.set_ssim_mode(False)


def test_two_column_kernels_at_8k(ctx):
    """config 4's plane: 7680 x 4320, 33 M windows -- one lost window is 3e-8 of the mean there, under both bars.  fp64 and
    fp32 moments, the segment geometry an 8K launch has"""
    w, h = 7680, 4320
    a = sp.tiled_background(w, h, 9)
    probes = sp.sparse(sp.probe_boxes(w, h, 121))
    _run_route(ctx, "windowed_ssim_march2_kernel", "ssim_enqueue", w, h, 121, (), _enqueue(ctx), sp.FP64_BAR, probes=probes, a=a, pitched=False)
    ctx.set_ssim_mode(True)
    try:
        _run_route(ctx, "windowed_ssim_march2f_kernel", "ssim_enqueue", w, h, 121, (), _enqueue(ctx), FAST_BAR, probes=probes, a=a,
                   pitched=False)
    finally:
        ctx.set_ssim_mode(False)


@pytest.mark.parametrize("w,h", [(301, 203), (2601, 1703)])
def test_64_tap_kernel(ctx, w, h):
    """a window table that is not rank-1 (windowed_ssim_kernel, whatever the size): a small plane and one of >= 4 M windows"""
    k = _non_rank1_window()
    probes = sp.probe_boxes(w, h, 32, (8,))
    if w > 1000:                                              # (this kernel is 20 x slower per window: thinner sweeps on the big plane)
        probes = [p for i, p in enumerate(probes) if not p[0].startswith(("seam", "last_")) or i % 3 == 0]
        assert sp.windows(w, h) >= MARCH2_MIN
    _run_route(ctx, "windowed_ssim_kernel", "ssim_enqueue(window)", w, h, 32, (8,), _enqueue(ctx, k), sp.FP64_BAR, kernel=k, probes=probes)


def _expected_batch_route(w, h, n, cus):
    total = sp.windows(w, h) * n
    if total >= MARCH_MIN:
        return "windowed_ssim_march2_kernel" if sp.windows(w, h) >= MARCH2_MIN else "windowed_ssim_march_kernel"
    return "windowed_ssim_sep24_kernel" if total >= 4096 * cus else "windowed_ssim_sep_kernel"


@pytest.mark.parametrize("w,h,n", [(1025, 771, 2), (1025, 771, 5), (641, 483, 2), (641, 483, 4), (641, 483, 5), (2601, 1703, 2)])
def test_batch_enqueue(ctx, cus, w, h, n):
    """fnx_ssim_batch_enqueue: the image is a grid dimension and n moves both thresholds and the segment length.  Every image
    of the batch has its own background and carries a different probe in each round."""
    import torch
    route = _expected_batch_route(w, h, n, cus)
    xp = {"windowed_ssim_march2_kernel": 121, "windowed_ssim_march_kernel": 57}.get(route, 32)
    yp = {"windowed_ssim_sep24_kernel": (24, 16), "windowed_ssim_sep_kernel": (16,)}.get(route, ())
    A = [sp.background(w, h, 20 + i) for i in range(n)]
    B = [x.copy() for x in A]
    da = [torch.from_numpy(x).cuda() for x in A]
    db = [t.clone() for t in da]
    ctx.ssim_batch_enqueue(da, db)
    assert np.all(ctx.fetch_results(n) == 1.0)
    assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
    flo = _floor(route, w, h)
    probes = sp.probe_boxes(w, h, xp, yp)
    if w > 2000:
        probes = sp.sparse(probes)
    bad = []
    worst = 0.0
    for r in range(0, len(probes), n):
        mine = [probes[(r + i) % len(probes)] for i in range(n)]
        for i, (name, box) in enumerate(mine):
            x0, y0, x1, y1 = box
            blk = sp.altered_block(A[i], box)
            B[i][y0:y1 + 1, x0:x1 + 1] = blk
            db[i][y0:y1 + 1, x0:x1 + 1] = torch.from_numpy(blk).cuda()
        ctx.ssim_batch_enqueue(da, db)
        means = ctx.fetch_results(n)
        assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
        for i, (name, box) in enumerate(mine):
            x0, y0, x1, y1 = box
            want, k = sp.d_ref(A[i], B[i], box=box)
            d = sp.d_of(means[i], w, h)
            err = abs(d - want)
            print(f"batch n={n} {route} {w}x{h} image {i} {name}: K={k} D_ref={want:.12g} D_gpu={d:.12g} err={err:.3g} floor={flo:.3g}")
            if k:
                worst = max(worst, err / k)
            if not sp.agrees(d, want, k, sp.FP64_BAR, flo):
                bad.append((i, name, k, want, d, err))
            B[i][y0:y1 + 1, x0:x1 + 1] = A[i][y0:y1 + 1, x0:x1 + 1]
            db[i][y0:y1 + 1, x0:x1 + 1] = da[i][y0:y1 + 1, x0:x1 + 1]
    print(f"SUMMARY batch n={n} {route} {w}x{h}: {len(probes)} probes, worst |D_gpu - D_ref| / K = {worst:.3g}, floor {flo:.3g}")
    assert not bad, f"batch of {n}, {route}, {w}x{h}: (image, name, K, D_ref, D_gpu, |diff|) {bad[:12]}"


def _plane_probes(w, h):
    """patches large enough to survive the 2 x 2 pyramid and the <= 512 px box planes, at the image's corners, edges, middle"""
    s = max(24, w // 64)
    xs, ys = (0, w // 2 - s // 2 + 1, w - s), (0, h // 2 - s // 2 + 3, h - s)
    return [(f"patch{s}@{x},{y}", sp.patch_box(x, y, s, s)) for y in ys for x in xs] + [("row_band", (0, h // 3, w - 1, h // 3 + s // 2)),
                                                                                 ("col_band", (w // 3, 0, w // 3 + s // 2, h - 1))]


@pytest.mark.parametrize("w,h,route", [(1024, 768, "windowed_ssim_sep_multi_kernel"), (2048, 1024, "windowed_ssim_sep_multi_kernel"),
                                       (1000, 600, "windowed_ssim_sep_kernel")])
def test_msssim_levels(ctx, orc, w, h, route):
    """fnx_msssim level by level: launch_msssim_fused (five levels in one windowed_ssim_sep_multi_kernel launch) and the
    level loop (shapes whose halvings are not all 2 x 2), each level's D against the reference's own planes"""
    import torch
    a = sp.background(w, h, 31)
    b = a.copy()
    da = torch.from_numpy(a).cuda()
    db = da.clone()
    got, lv = ctx.msssim_levels(da, db)
    assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
    assert got == 1.0 and np.all(lv[~np.isnan(lv)] == 1.0)
    bad = []
    worst = 0.0
    every = _plane_probes(w, h)
    for name, box in every[0:9:2] + every[9:]:                # the corners, the middle, both bands (the reference's pyramid is the cost)
        x0, y0, x1, y1 = box
        blk = sp.altered_block(a, box)
        b[y0:y1 + 1, x0:x1 + 1] = blk
        db[y0:y1 + 1, x0:x1 + 1] = torch.from_numpy(blk).cuda()
        planes = sp.msssim_planes(orc, a, b)
        runs = [("device", ctx.msssim_levels(da, db)[1])]
        assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
        if name.startswith("row"):
            runs.append(("host", ctx.msssim_levels(a, b)[1]))
            assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
        for how, lv in runs:
            assert int(np.sum(~np.isnan(lv))) == len(planes)
            for i, (pa, pb) in enumerate(planes):
                pw, ph = pa.shape[1], pa.shape[0]
                want, k = sp.d_ref(pa, pb)
                if i == 0:
                    assert k > 0 and want / k >= 1e-2                     # (the input condition, by the reference)
                d = sp.d_of(lv[i], pw, ph)
                flo = _floor("windowed_ssim_sep_kernel", pw, ph)
                err = abs(d - want)
                print(f"msssim {route} {w}x{h} {name} {how} level {i} ({pw}x{ph}): K={k} D_ref={want:.12g} D_gpu={d:.12g} err={err:.3g} floor={flo:.3g}")
                if k:
                    worst = max(worst, err / k)
                if not sp.agrees(d, want, k, sp.FP64_BAR, flo):
                    bad.append((name, how, i, k, want, d, err))
        b[y0:y1 + 1, x0:x1 + 1] = a[y0:y1 + 1, x0:x1 + 1]
        db[y0:y1 + 1, x0:x1 + 1] = da[y0:y1 + 1, x0:x1 + 1]
    print(f"SUMMARY msssim {route} {w}x{h}: worst |D_gpu - D_ref| / K = {worst:.3g}")
    assert not bad, f"msssim_levels {w}x{h} via {route}: (name, how, level, K, D_ref, D_gpu, |diff|) {bad[:12]}"


def test_ssim_fast_4k(ctx, orc):
    """SSIMFast at 4K: box planes of 512 x 288, then the 32 x 16 tile kernel -- device tensors, host arrays, a pitched view,
    and the prepared form (fnx_ssim_fast_prepare / _against)"""
    import torch
    w, h = 3840, 2160
    route = "windowed_ssim_sep_kernel"
    a = sp.background(w, h, 41)
    b = a.copy()
    da = torch.from_numpy(a).cuda()
    db = da.clone()
    assert ctx.SSIMFast(da, db) == 1.0
    assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
    prep = ctx.ssim_fast_prepare(da)
    assert prep.against(db) == 1.0
    pa = orc.box_downsample(a, 512, 288)
    assert orc.ssim_fast_dims(w, h) == (True, 512, 288)
    flo = _floor(route, 512, 288)
    bad = []
    worst = 0.0
    for name, box in _plane_probes(w, h):
        x0, y0, x1, y1 = box
        blk = sp.altered_block(a, box)
        b[y0:y1 + 1, x0:x1 + 1] = blk
        db[y0:y1 + 1, x0:x1 + 1] = torch.from_numpy(blk).cuda()
        pb = orc.box_downsample(b, 512, 288)
        want, k = sp.d_ref(pa, pb)
        assert k > 0 and want / k >= 1e-2
        runs = [("device", ctx.SSIMFast(da, db))]
        assert ctx.last_kernel(fennec_amd.PROF_SSIM) == route
        runs.append(("prepared", prep.against(db)))
        if name.startswith("row"):
            runs.append(("host", ctx.SSIMFast(a, b)))
            runs.append(("pitched", ctx.SSIMFast(_pitched(a, 4, 4), _pitched(b, 8, 0))))
        for how, mean in runs:
            d = sp.d_of(mean, 512, 288)
            err = abs(d - want)
            print(f"ssim_fast {name} {how}: K={k} D_ref={want:.12g} D_gpu={d:.12g} err={err:.3g} floor={flo:.3g}")
            worst = max(worst, err / k)
            if not sp.agrees(d, want, k, sp.FP64_BAR, flo):
                bad.append((name, how, k, want, d, err))
        b[y0:y1 + 1, x0:x1 + 1] = a[y0:y1 + 1, x0:x1 + 1]
        db[y0:y1 + 1, x0:x1 + 1] = da[y0:y1 + 1, x0:x1 + 1]
    prep.close()
    print(f"SUMMARY ssim_fast 4K: worst |D_gpu - D_ref| / K = {worst:.3g}")
    assert not bad, f"SSIMFast 4K: (name, how, K, D_ref, D_gpu, |diff|) {bad[:12]}"
