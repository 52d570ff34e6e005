"""fnx_median_cut and fnx_quantize on the GPU: the palettes equal the numpy restatement (tests/median_cut_ref.py) byte for byte
on every shared case in both spaces, two calls return identical bytes, the kernel is named, and fnx_quantize's outputs `==` the
three existing calls composed."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
import median_cut_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_palettes_equal_the_restatement(ctx, name, space):
    import torch
    img, levels = ref.CASES[name]
    want, _ = ref.want(name)
    src = img if space == "host" else torch.from_numpy(img).cuda()
    got = ctx.median_cut(src, levels)
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == "median_cut_kernel"
    for level, g, w in zip(levels, got, want):
        print(name, space, level, "ncolors", len(g), "want", len(w), "differing entries", int((g != w).any(axis=1).sum()) if g.shape == w.shape else -1)
        assert g.shape == w.shape, (name, space, level, g.shape, w.shape)
        assert np.array_equal(g, w), (name, space, level, np.argwhere(g != w)[:4])
    again = ctx.median_cut(src, levels)
    assert all(np.array_equal(a, b) for a, b in zip(got, again)), "two calls differ"


def test_empty_image(ctx):
    for shape in ((0, 5, 4), (5, 0, 4)):
        assert [p.tolist() for p in ctx.median_cut(np.zeros(shape, np.uint8), (2, 16))] == [[[0, 0, 0, 255]]] * 2


def _composed(ctx, img, max_colors):
    """fnx_median_cut, fnx_apply_palette and fnx_ssim_fast one after the other, in the image's own space"""
    pal = ctx.median_cut(img, (max_colors,))[0]
    idx, q = ctx.applyPalette(img, pal, want_quantized=True)
    v, qv = fennec_amd._Img(img), fennec_amd._Img(q)
    win = ctx.gaussianKernel()
    out = C.c_double()
    with ctx._ordered(img, q):
        rc = ctx._lib.fnx_ssim_fast(ctx._h, v.space, v.ptr, v.stride, qv.ptr, qv.stride, v.w, v.h, win.ctypes.data_as(fennec_amd._f64p), C.byref(out))
    assert rc == 0
    return pal, idx, q, out.value


def _np(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


# 64 x 64: windowed SSIM on the images themselves; 5 x 2: pixelSSIM; 600 x 520: box-downsampled, the palette grid (>= 256 k pixels)
@pytest.mark.parametrize("space", ["host", "device"])
@pytest.mark.parametrize("max_colors", [256, 16])
@pytest.mark.parametrize("shape", [(64, 64), (5, 2), (600, 520)])
def test_quantize_equals_the_three_calls_composed(ctx, shape, max_colors, space):
    import torch
    w, h = shape
    img = fennec_amd.synth.large_photo(w, h, 3) if w >= 64 else ref.CASES["5x2_random"][0]
    src = img if space == "host" else torch.from_numpy(img).cuda()
    pal, idx, q, s = _composed(ctx, src, max_colors)
    gp, gi, gq, gs = ctx.quantize(src, max_colors)
    ctx.sync()
    print(shape, max_colors, space, "ncolors", len(gp), len(pal), "ssim", gs, s)
    assert np.array_equal(gp, pal) and np.array_equal(_np(gi), _np(idx)) and np.array_equal(_np(gq), _np(q))
    assert gs == s
    # without the optional outputs
    p2, i2, q2, s2 = ctx.quantize(src, max_colors, want_indices=False, want_quantized=False)
    assert i2 is None and q2 is None and np.array_equal(p2, pal) and s2 == s
    p3, i3, q3, s3 = ctx.quantize(src, max_colors, want_quantized=False, want_ssim=False)
    ctx.sync()
    assert q3 is None and s3 is None and np.array_equal(p3, pal) and np.array_equal(_np(i3), _np(idx))
    p4, i4, q4, s4 = ctx.quantize(src, max_colors, want_indices=False, want_ssim=False)
    ctx.sync()
    assert i4 is None and s4 is None and np.array_equal(p4, pal) and np.array_equal(_np(q4), _np(q))
