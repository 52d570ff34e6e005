"""fnx_jpeg_compress_batch (Context.jpeg_compress_batch): n device images of one geometry searched in lockstep and
entropy-coded together.  Per item, the result must be fnx_jpeg_compress's: file bytes, quality, ssim (bit for bit) and
steps -- over the synthetic contents, every route of the search (SSIMFast downsampled from the candidate's planes, from
its decoded image, not downsampled, pixelSSIM), strided sources, per-item targets, small buffers, 65 535 tiny images
and refused arguments."""
from __future__ import annotations

import ctypes as C
import random

import numpy as np
import pytest

import fennec_amd
from fennec_amd import synth

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PRESETS = [1.0, 0.99, 0.97, 0.94, 0.90, 0.85]


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def _contents(w, h):
    return [
        synth.large_photo(w, h, 0),
        synth.make_test_image(w, h),
        synth.make_striped_image(w, h, 7),
        synth.noise_image(w, h, 3),
        synth.make_solid_image(w, h, (200, 120, 40, 255)),
        synth.make_test_image_with_alpha(w, h),          # translucent: the premultiplied colour conversion
    ]


def _dev(imgs, pad=0, offset=0):
    """device copies; pad > 0: rows of (w + pad) px with the image at column `offset` (a strided view)"""
    out = []
    for im in imgs:
        h, w = im.shape[:2]
        if pad == 0:
            out.append(torch.from_numpy(np.ascontiguousarray(im)).cuda())
        else:
            big = torch.zeros((h, w + pad, 4), dtype=torch.uint8, device="cuda")
            big[:, offset:offset + w] = torch.from_numpy(np.ascontiguousarray(im)).cuda()
            out.append(big[:, offset:offset + w])
    torch.cuda.synchronize()
    return out


def _singles(ctx, imgs, targets, window=None):
    return [ctx.jpeg_compress(im, t, window=window) for im, t in zip(imgs, targets)]


def _check(got, want):
    assert len(got) == len(want)
    for i, (g, e) in enumerate(zip(got, want)):
        assert g[1:] == e[1:], f"item {i}: (quality, ssim, steps) {g[1:]} != {e[1:]}"
        assert np.float64(g[2]).tobytes() == np.float64(e[2]).tobytes(), f"item {i}: ssim bits differ"
        assert g[0] == e[0], f"item {i}: file bytes differ ({len(g[0])} vs {len(e[0])})"
        assert g == e


ROUTES = [
    (640, 480),      # downsampled, candidate planes box-summed straight from the YCbCr planes
    (333, 517),      # odd, downsampled on one side only
    (100, 100),      # no downsample: the decoded candidate itself
    (4000, 40),      # SSIMFast plane on the 8-px floor on one side
    (4000, 5),       # the floor above the source's height: an upscale, decoded image + box downsample
    (7, 9),          # pixelSSIM
]


@pytest.mark.parametrize("w,h", ROUTES, ids=[f"{w}x{h}" for w, h in ROUTES])
def test_parity_with_single_calls(ctx, w, h):
    imgs = _dev(_contents(w, h))
    targets = [PRESETS[i % len(PRESETS)] for i in range(len(imgs))]
    _check(ctx.jpeg_compress_batch(imgs, targets), _singles(ctx, imgs, targets))


def test_parity_1080p_per_item_targets(ctx):
    w, h = 1920, 1080
    imgs = _dev(_contents(w, h) + [synth.large_photo(w, h, 1), synth.large_photo(w, h, 2)])
    targets = [0.99, 0.97, 0.94, 0.90, 0.85, 1.0, 0.94, 0.97]
    _check(ctx.jpeg_compress_batch(imgs, targets), _singles(ctx, imgs, targets))


def test_parity_4k(ctx):
    w, h = 3840, 2160
    imgs = _dev([synth.large_photo(w, h, 0), synth.make_test_image(w, h), synth.noise_image(w, h, 5)])
    targets = [0.94, 0.99, 0.90]
    _check(ctx.jpeg_compress_batch(imgs, targets), _singles(ctx, imgs, targets))


def test_unreachable_target_on_noise(ctx):
    imgs = _dev([synth.noise_image(640, 480, s) for s in range(3)] + [synth.large_photo(640, 480, 0)])
    targets = [0.9999, 0.9999, 0.85, 0.9999]
    got = ctx.jpeg_compress_batch(imgs, targets)
    _check(got, _singles(ctx, imgs, targets))
    assert got[0][1] == 100 and got[0][2] == 1.0


@pytest.mark.parametrize("w,h,pad,offset", [(640, 480, 16, 0), (640, 480, 5, 1), (100, 100, 3, 2), (7, 9, 4, 1), (4000, 5, 8, 3)])
def test_strided_sources(ctx, w, h, pad, offset):
    host = _contents(w, h)
    imgs = _dev(host, pad=pad, offset=offset)
    targets = [PRESETS[(i + 2) % len(PRESETS)] for i in range(len(imgs))]
    got = ctx.jpeg_compress_batch(imgs, targets)
    _check(got, _singles(ctx, imgs, targets))
    _check(got, _singles(ctx, _dev(host), targets))          # a strided view compresses as its tight copy


def test_one_target_for_all_and_a_window(ctx):
    imgs = _dev(_contents(333, 517))
    _check(ctx.jpeg_compress_batch(imgs, 0.94), _singles(ctx, imgs, [0.94] * len(imgs)))
    # a window that is not rank-1: SSIMFast's 64-tap kernel instead of the separable one
    win = np.asarray(ctx.gaussianKernel(), dtype=np.float64).copy()
    win[9] += 0.004
    win[54] -= 0.004
    _check(ctx.jpeg_compress_batch(imgs, 0.97, window=win), _singles(ctx, imgs, [0.97] * len(imgs), window=win))


def test_n1_equals_jpeg_compress(ctx):
    for w, h in [(640, 480), (100, 100), (7, 9)]:
        im = _dev([synth.large_photo(w, h, 0)])
        assert ctx.jpeg_compress_batch(im, [0.94]) == [ctx.jpeg_compress(im[0], 0.94)]


def test_order_independence(ctx):
    imgs = _dev(_contents(640, 480))
    targets = [0.99, 0.85, 0.94, 0.9999, 1.0, 0.90]
    base = ctx.jpeg_compress_batch(imgs, targets)
    perm = [3, 0, 5, 1, 4, 2]
    got = ctx.jpeg_compress_batch([imgs[p] for p in perm], [targets[p] for p in perm])
    assert got == [base[p] for p in perm]
    for i in range(len(imgs)):                 # alone, each item is what it was in the batch: nothing leaks between items
        assert ctx.jpeg_compress_batch([imgs[i]], [targets[i]]) == [base[i]]


def _raw(ctx, imgs, targets, caps, window=None, srcs=None, sstride=None, w=None, h=None, n=None):
    lib = ctx._lib
    v0 = fennec_amd._Img(imgs[0])
    n = len(imgs) if n is None else n
    m = max(n, 1)
    win = np.asarray(ctx.gaussianKernel() if window is None else window, dtype=np.float64)
    def fill(xs):                               # m entries (the refused counts only need the arrays to exist)
        return (list(xs) + [xs[0]] * m)[:m]

    tg = np.asarray(fill(targets), dtype=np.float64)
    bufs = [np.zeros(max(int(c), 1), dtype=np.uint8) for c in caps]
    ptrs = [fennec_amd._Img(t).ptr for t in imgs] if srcs is None else srcs
    srcs_a = (C.c_void_p * m)(*fill(ptrs))
    outs = (C.c_void_p * m)(*fill([b.ctypes.data for b in bufs]))
    caps_a = (C.c_size_t * m)(*fill(caps))
    nb, q, st, status = (C.c_size_t * m)(), (C.c_int * m)(), (C.c_int * m)(), (C.c_int * m)()
    v = (C.c_double * m)()
    wp = None if window is False else win.ctypes.data_as(C.POINTER(C.c_double))
    rc = lib.fnx_jpeg_compress_batch(ctx._h, n, srcs_a, v0.stride if sstride is None else sstride, v0.w if w is None else w,
                                     v0.h if h is None else h, tg.ctypes.data_as(C.POINTER(C.c_double)), wp, outs, caps_a, nb, q, v, st,
                                     status)
    return rc, bufs, list(nb), list(q), list(v), list(st), list(status)


def test_small_buffer(ctx):
    imgs = _dev(_contents(640, 480)[:4])
    targets = [0.94, 0.99, 0.90, 0.97]
    want = _singles(ctx, imgs, targets)
    caps = [len(want[0][0]) + 10, 100, len(want[2][0]), 1 << 20]
    rc, bufs, nb, q, v, st, status = _raw(ctx, imgs, targets, caps)
    assert rc == fennec_amd.FNX_OK
    assert status == [fennec_amd.FNX_OK, fennec_amd.FNX_ERR_INVALID, fennec_amd.FNX_OK, fennec_amd.FNX_OK]
    assert nb[1] == len(want[1][0]) and q[1] == want[1][1] and v[1] == want[1][2] and st[1] == want[1][3]
    assert ctx.jpeg_encode(imgs[1], q[1]) == want[1][0]       # the file without a new search
    for i in (0, 2, 3):
        assert bufs[i][:nb[i]].tobytes() == want[i][0] and (q[i], v[i], st[i]) == want[i][1:]


def test_small_buffer_through_python(ctx):
    # every cap too small: the method finishes each item with fnx_jpeg_encode at the reported quality, no new search
    imgs = _dev([synth.noise_image(100, 100, 1), synth.large_photo(100, 100, 0)])
    want = _singles(ctx, imgs, [0.9999, 0.94])
    real = ctx._lib
    calls = []

    def small(h, n, srcs, sstride, w, hh, tg, win, outs, caps, nb, q, v, st, status):
        for i in range(n):
            caps[i] = 64
        rc = real.fnx_jpeg_compress_batch(h, n, srcs, sstride, w, hh, tg, win, outs, caps, nb, q, v, st, status)
        calls.append(list(status))
        return rc

    class Lib:
        def __getattr__(self, name):
            return small if name == "fnx_jpeg_compress_batch" else getattr(real, name)

    ctx._lib = Lib()
    try:
        got = ctx.jpeg_compress_batch(imgs, [0.9999, 0.94])
    finally:
        ctx._lib = real
    assert calls == [[fennec_amd.FNX_ERR_INVALID] * 2]
    assert got == want


def test_many_tiny_images(ctx):
    n = 65535                                   # FNX_BATCH_MAX
    rng = np.random.default_rng(7)
    host = rng.integers(0, 256, size=(n, 16, 16, 4), dtype=np.uint8)
    host[: n // 2, ..., 3] = 255
    ramp = (np.arange(16, dtype=np.uint8) * 16)[None, None, :, None]
    host[n // 4: n // 2] = (host[n // 4: n // 2] // 4 + ramp // 2).astype(np.uint8)
    dev = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    imgs = [dev[i] for i in range(n)]
    targets = [PRESETS[i % len(PRESETS)] if i % 11 else 0.9999 for i in range(n)]
    got = ctx.jpeg_compress_batch(imgs, targets)
    assert len(got) == n
    sample = sorted(random.Random(2026).sample(range(n), 64))
    for i in sample:
        assert got[i] == ctx.jpeg_compress(imgs[i], targets[i]), i


def test_bad_arguments_are_refused(ctx):
    imgs = _dev(_contents(100, 100)[:2])
    caps = [1 << 16, 1 << 16]
    inv = fennec_amd.FNX_ERR_INVALID
    assert _raw(ctx, imgs, [0.94, 0.94], caps, n=0)[0] == inv
    assert _raw(ctx, imgs, [0.94, 0.94], caps, n=65536)[0] == inv
    p = fennec_amd._Img(imgs[0]).ptr
    assert _raw(ctx, imgs, [0.94, 0.94], caps, srcs=[p, None])[0] == inv
    assert _raw(ctx, imgs, [0.94, 0.94], caps, sstride=4 * 100 - 4)[0] == inv
    assert _raw(ctx, imgs, [0.94, 0.94], caps, w=0)[0] == inv
    assert _raw(ctx, imgs, [0.94, 0.94], caps, window=False)[0] == inv
    # the same ctx then compresses normally
    _check(ctx.jpeg_compress_batch(imgs, [0.94, 0.97]), _singles(ctx, imgs, [0.94, 0.97]))
