"""Resize, then score, in one call: fnx_lanczos_box_downsample, fnx_ssim_fast_resized, fnx_ssim_resized, fnx_msssim_resized and
fennec_computeSSIMNRGBA against the CPU oracle's composites (lanczos_resize, then box_downsample / ssim_fast / ssim / msssim).

Bounds: plane bytes are integers and must be equal; scores are within 1e-9 of the oracle (the project's bar for the SSIM
family: fp64 sums in another order); two routes of the library that hand the same planes to the same scoring launch must
agree with ==.

The fused kernel is opt-in (form "resize_box" "1"); "0" and the default take the composed route."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import fennec_amd
from fennec_amd import FNX_TS_QUALITY_SCALE, PROF_RESIZE, synth
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

FUSED = "resize_box_kernel"


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


# ---- content ---------------------------------------------------------------------------------------------------------
def _photo(w, h, seed=1):
    """photograph-like and blocky: smooth gradients, 50 x 40 px blocks, grain; opaque"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 127 + 90 * np.sin(x / 37.0 + seed) * np.cos(y / 23.0) + 30 * ((x // 50 + y // 40) % 2)
    img = np.empty((h, w, 4), np.uint8)
    for c in range(3):
        img[..., c] = np.clip(base + 15 * c + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)
    img[..., 3] = 255
    return img


def _content(kind, w, h):
    if kind == "photo":
        return _photo(w, h)
    if kind == "ramp":                       # dense rounding ties
        return synth.large_photo(w, h, 3)
    if kind == "alpha":                      # random alpha: the premultiplied arithmetic and some al <= 0.5 zero pixels
        return synth.noise_image(w, h, 11, alpha=True)
    assert kind == "holes"                   # fully transparent regions beside opaque ones
    img = _photo(w, h, 2)
    img[h // 5: h // 2, w // 7: w // 2, 3] = 0
    img[-(h // 6):, : w // 3] = 0
    img[: h // 9, -(w // 4):, 3] = 1
    return img


PAIRS = [(1280, 720, 640, 360), (1280, 720, 960, 540), (1000, 600, 333, 217), (1920, 1080, 1919, 1079), (720, 1280, 360, 640),
         (1001, 603, 97, 61), (3840, 2160, 1920, 1080), (3840, 2160, 2880, 1620)]
CONTENTS = ["photo", "ramp", "alpha", "holes"]


@functools.lru_cache(maxsize=4)
def _upscaled(kind, aw, ah, bw, bh):
    b = _content(kind, bw, bh)
    return b, orc.lanczos_resize(b, aw, ah, procs=8)


def _tables(aw, ah, bw, bh):
    return fennec_amd.precomputeWeights(aw, bw), fennec_amd.precomputeWeights(ah, bh)


def _dev(img):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    torch.cuda.synchronize()
    return t


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


# ---- plane bytes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", CONTENTS)
@pytest.mark.parametrize("aw,ah,bw,bh", PAIRS)
def test_plane_bytes(ctx, aw, ah, bw, bh, kind):
    """boxDownsample(lanczosResize(b, aw, ah), SSIMFast's dims) byte for byte, in both spaces, from the fused kernel (every
    pair here lies in its domain: the route is asserted) and from the composed form"""
    b, up = _upscaled(kind, aw, ah, bw, bh)
    down, pw, ph = ctx.ssimFastDims(aw, ah)
    assert down
    want = orc.box_downsample(up, pw, ph)
    for src in (b, _dev(b)):
        with ctx.forms(resize_box=1):
            got = ctx.lanczosBoxDownsample(src, aw, ah, pw, ph)
            ctx.sync()
            assert ctx.last_kernel(PROF_RESIZE) == FUSED
        assert np.array_equal(_host(got), want), f"fused, {type(src).__name__}: {(_host(got) != want).sum()} bytes differ"
        for form in (0, None):
            with ctx.forms(resize_box=form):
                got = ctx.lanczosBoxDownsample(src, aw, ah, pw, ph)
                ctx.sync()
                assert ctx.last_kernel(PROF_RESIZE) != FUSED
            assert np.array_equal(_host(got), want), f"composed ({form}), {type(src).__name__}"


@pytest.mark.parametrize("kind", ["photo", "alpha"])
def test_plane_bytes_pitched(ctx, kind):
    """pitched views on both sides of the call: a source cut out of wider rows (host and device), a destination inside a wider
    plane (device); the bytes outside the destination stay untouched"""
    import ctypes as C
    import torch
    aw, ah, bw, bh = 1000, 600, 333, 217
    b, up = _upscaled(kind, aw, ah, bw, bh)
    _, pw, ph = ctx.ssimFastDims(aw, ah)
    want = orc.box_downsample(up, pw, ph)
    wide = np.full((bh, bw + 7, 4), 0x5A, np.uint8)
    wide[:, 3: 3 + bw] = b
    for src in (wide[:, 3: 3 + bw], _dev(wide)[:, 3: 3 + bw]):
        for form in (1, 0):
            with ctx.forms(resize_box=form):
                got = ctx.lanczosBoxDownsample(src, aw, ah, pw, ph, to_host=True)
                assert (ctx.last_kernel(PROF_RESIZE) == FUSED) == (form == 1)
            assert np.array_equal(got, want), (type(src).__name__, form)
    # pitched destination through the C ABI
    th, tv = _tables(aw, ah, bw, bh)
    keep = [np.ascontiguousarray(t[0], np.int32) for t in (th, tv)] + [np.ascontiguousarray(t[1], np.int32) for t in (th, tv)] + \
           [np.ascontiguousarray(t[2], np.float64) for t in (th, tv)]
    i32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_double)
    ptr = lambda a, t: a.ctypes.data_as(t)
    dsrc = _dev(wide)
    plane = torch.full((ph + 2, pw + 9, 4), 0xC3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    u8 = C.POINTER(C.c_uint8)
    for form in (1, 0):
        plane.fill_(0xC3)
        torch.cuda.synchronize()
        with ctx.forms(resize_box=form):
            rc = ctx._lib.fnx_lanczos_box_downsample(
                ctx._h, fennec_amd.FNX_DEVICE, C.cast(dsrc.data_ptr() + 12, u8), (bw + 7) * 4, bw, bh,
                ptr(keep[0], i32), ptr(keep[2], i32), ptr(keep[4], f64), ptr(keep[1], i32), ptr(keep[3], i32), ptr(keep[5], f64),
                aw, ah, C.cast(plane.data_ptr() + (pw + 9) * 4 + 8, u8), (pw + 9) * 4, pw, ph)
            assert rc == 0, ctx._err()
            ctx.sync()
        got = plane.cpu().numpy()
        assert np.array_equal(got[1: 1 + ph, 2: 2 + pw], want), form
        frame = got.copy()
        frame[1: 1 + ph, 2: 2 + pw] = 0xC3
        assert (frame == 0xC3).all(), "bytes outside the destination were written"


# ---- scores ------------------------------------------------------------------------------------------------------------
def _pair_for_score(kind, aw, ah, bw, bh):
    """a and a smaller b that resembles it (non-trivial scores: 0.9 .. 0.999)"""
    if kind == "alpha":
        a = _photo(aw, ah)
        b = orc.box_downsample(a, bw, bh)
        b[..., 3] = synth.noise_image(bw, bh, 5, alpha=True)[..., 3]
        return a, b
    a = _photo(aw, ah)
    return a, orc.box_downsample(a, bw, bh)


@pytest.mark.parametrize("aw,ah,bw,bh,kind", [(1280, 720, 640, 360, "photo"), (1280, 720, 960, 540, "photo"), (1000, 600, 333, 217, "photo"),
                                              (1280, 720, 640, 360, "alpha"), (3840, 2160, 1920, 1080, "photo")])
def test_ssim_fast_resized(ctx, aw, ah, bw, bh, kind):
    a, b = _pair_for_score(kind, aw, ah, bw, bh)
    want = orc.ssim_fast(a, orc.lanczos_resize(b, aw, ah, procs=8))
    tabs = _tables(aw, ah, bw, bh)
    vals = {}
    for name, (x, y) in (("host", (a, b)), ("device", (_dev(a), _dev(b)))):
        with ctx.forms(resize_box=1):
            fused = ctx.ssim_fast_resized(x, y, tabs)
            assert ctx.last_kernel(PROF_RESIZE) == FUSED
            assert ctx.ssim_fast_resized(x, y, tabs) == fused      # scratch reuse: a second identical call
            assert ctx.computeSSIMNRGBA(x, y) == fused
        with ctx.forms(resize_box=0):
            composed = ctx.ssim_fast_resized(x, y, tabs)
            assert ctx.last_kernel(PROF_RESIZE) != FUSED
        mirror = ctx.computeSSIMNRGBA(x, y)
        print(f"{aw}x{ah} <- {bw}x{bh} {kind} {name}: fused {fused!r} composed {composed!r} oracle {want!r}")
        assert abs(fused - want) <= 1e-9
        assert fused == composed == mirror
        assert ctx.ssim_fast_resized(x, y, tabs) == composed       # the default, and scratch reuse: a second identical call
        vals[name] = fused
    assert vals["host"] == vals["device"]
    assert want < 1.0 - 1e-5, "the pair is too alike to test anything"


RESIZED_PAIRS = [("upscale", 700, 520, 350, 260), ("downscale", 700, 520, 1400, 1040), ("mixed", 700, 520, 1000, 300)]


@pytest.mark.parametrize("name,aw,ah,bw,bh", RESIZED_PAIRS)
def test_ssim_and_msssim_resized(ctx, name, aw, ah, bw, bh):
    a = _photo(aw, ah)
    b = orc.lanczos_resize(_photo(2 * aw, 2 * ah, 1)[::2, ::2].copy(), bw, bh, procs=8)     # a's relative: same seed, resampled
    want_s = orc.ssim(a, b, procs=8)
    want_m, want_lv = orc.msssim(a, b, procs=8, per_level=True)
    tabs = _tables(aw, ah, bw, bh)
    for x, y in ((a, b), (_dev(a), _dev(b))):
        s = ctx.ssim_resized(x, y, tabs)
        m, lv = ctx.msssim_resized(x, y, tabs)
        print(f"{name}: SSIM {s!r} (oracle {want_s!r}), MSSSIM {m!r} (oracle {want_m!r})")
        assert abs(s - want_s) <= 1e-9
        assert abs(m - want_m) <= 1e-9
        assert np.array_equal(np.isnan(lv), np.isnan(want_lv))
        ok = ~np.isnan(want_lv)
        assert np.abs(lv[ok] - want_lv[ok]).max() <= 1e-9
        assert s == ctx.SSIM(x, y) and m == ctx.MSSSIM(x, y)          # fennec_SSIM / fennec_MSSSIM: the same code path


# ---- edges -------------------------------------------------------------------------------------------------------------
def test_equal_dims_need_no_tables(ctx):
    a, b = _photo(800, 600), _photo(800, 600, 3)
    none = ((None, None, None), (None, None, None))
    for x, y in ((a, b), (_dev(a), _dev(b))):
        assert ctx.ssim_fast_resized(x, y, none) == ctx.SSIMFast(x, y)
        assert ctx.ssim_resized(x, y, none) == ctx.SSIM(x, y)
        m, lv = ctx.msssim_resized(x, y, none)
        want, want_lv = ctx.msssim_levels(x, y)
        assert m == want and np.array_equal(lv, want_lv, equal_nan=True)
        assert ctx.computeSSIMNRGBA(x, y) == ctx.SSIMFast(x, y)


@pytest.mark.parametrize("aw,ah,bw,bh", [(512, 300, 256, 150), (400, 512, 133, 170), (300, 200, 450, 300)])
def test_small_a_is_composed(ctx, aw, ah, bw, bh):
    """SSIMFast does not downsample an `a` of at most 512 px: the whole resized image is needed"""
    a, b = _pair_for_score("photo", aw, ah, bw, bh) if bw < aw else (_photo(aw, ah), _photo(bw, bh))
    want = orc.ssim_fast(a, orc.lanczos_resize(b, aw, ah))
    for x, y in ((a, b), (_dev(a), _dev(b))):
        got = ctx.computeSSIMNRGBA(x, y)
        assert ctx.last_kernel(PROF_RESIZE) != FUSED
        assert abs(got - want) <= 1e-9


def test_downscale_is_composed(ctx):
    """a downscale on either axis lies outside the fused kernel's domain: same bytes from the composed route"""
    for (bw, bh) in ((2000, 1200), (500, 1200), (2000, 300)):
        aw, ah = 1000, 600
        b = _content("alpha", bw, bh)
        _, pw, ph = ctx.ssimFastDims(aw, ah)
        want = orc.box_downsample(orc.lanczos_resize(b, aw, ah, procs=8), pw, ph)
        got = ctx.lanczosBoxDownsample(_dev(b), aw, ah, pw, ph, to_host=True)
        assert ctx.last_kernel(PROF_RESIZE) != FUSED
        assert np.array_equal(got, want), (bw, bh)


def test_tables_with_gaps_are_composed(ctx):
    """a caller's table whose tap indices are not consecutive (a zero weight dropped from the middle of a list)"""
    aw, ah, bw, bh = 1000, 600, 500, 300
    b = _content("photo", bw, bh)
    (oh, ih, wh), tv = _tables(aw, ah, bw, bh)
    oh, ih, wh = oh.copy(), ih.copy(), wh.copy()
    t0 = int(oh[400])
    keep = np.ones(len(ih), bool)
    keep[t0 + 2] = False                               # output 400 loses its third tap: its indices now skip one
    ih, wh = ih[keep], wh[keep]
    oh[401:] -= 1
    _, pw, ph = ctx.ssimFastDims(aw, ah)
    want = orc.box_downsample(orc.resize_v(orc.resize_h(b, aw, table=(oh, ih, wh)), ah), pw, ph)
    got = ctx.lanczosBoxDownsample(b, aw, ah, pw, ph, tables=((oh, ih, wh), tv))
    assert ctx.last_kernel(PROF_RESIZE) != FUSED
    assert np.array_equal(got, want)


def test_tiny_a_takes_pixel_ssim(ctx):
    a = synth.noise_image(6, 5, 1)
    b = synth.noise_image(13, 11, 2)
    want = orc.ssim_fast(a, orc.lanczos_resize(b, 6, 5))
    for x, y in ((a, b), (_dev(a), _dev(b))):
        assert abs(ctx.computeSSIMNRGBA(x, y) - want) <= 1e-9
        assert abs(ctx.ssim_resized(x, y) - orc.ssim(a, b)) <= 1e-9


def test_empty_images_and_missing_tables(ctx):
    empty = np.zeros((0, 0, 4), np.uint8)
    a, b = _photo(600, 400), _photo(300, 200)
    assert ctx.computeSSIMNRGBA(empty, b) == 1.0
    assert ctx.ssim_fast_resized(empty, b) == 1.0
    assert ctx.ssim_resized(empty, b) == 1.0
    assert ctx.msssim_resized(empty, b)[0] == ctx.msssim_levels(empty, empty)[0]
    none = ((None, None, None), (None, None, None))
    half = (fennec_amd.precomputeWeights(600, 300), (None, None, None))
    for call in (ctx.ssim_fast_resized, ctx.ssim_resized, ctx.msssim_resized):
        with pytest.raises(fennec_amd.FennecError, match=r"\(-1\)"):      # FNX_ERR_INVALID: the reference panics
            call(a, empty)
        for tabs in (none, half):
            with pytest.raises(fennec_amd.FennecError, match=r"\(-1\).*tap table is null"):
                call(a, b, tabs)
    with pytest.raises(fennec_amd.FennecError, match=r"\(-1\)"):
        ctx.computeSSIMNRGBA(a, empty)
    with pytest.raises(fennec_amd.FennecError, match=r"\(-1\).*tap table is null"):
        ctx.lanczosBoxDownsample(b, 600, 400, 512, 341, tables=none)
    assert ctx.lanczosBoxDownsample(empty, 600, 400, 512, 341).size == 0


# ---- target-size mode ----------------------------------------------------------------------------------------------------
def test_target_size_scores_through_the_fused_kernel(ctx):
    """strategy 3's candidate (a Lanczos-scaled image, scored by computeSSIMNRGBA against the 1280 x 720 source): the upscale
    back is never stored, and the score is the composed form's to the bit"""
    src = orc.gaussian_blur(synth.noise_image(1280, 720, 7), 2.0)
    with ctx.forms(resize_box=1):
        fused = ctx.jpeg_target_size(src, 60000, FNX_TS_QUALITY_SCALE)
        assert ctx.last_kernel(PROF_RESIZE) == FUSED
    c = fused["candidates"][1]
    assert c["strategy"] == FNX_TS_QUALITY_SCALE and (c["final_w"], c["final_h"]) != (1280, 720), c
    with ctx.forms(resize_box=0):
        composed = ctx.jpeg_target_size(src, 60000, FNX_TS_QUALITY_SCALE)
        assert ctx.last_kernel(PROF_RESIZE) != FUSED
    assert composed["candidates"][1] == c
    assert composed["data"] == fused["data"]
    want = orc.ssim_fast(src, orc.lanczos_resize(np.ascontiguousarray(fused["image"]), 1280, 720, procs=8))
    assert abs(c["ssim"] - want) <= 1e-9
