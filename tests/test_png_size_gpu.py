"""fnx_png_encoded_size on the GPU: the size-only forms of the deflate kernels behind the row stage.  The size is the length of
the file fnx_png_encode writes for the same arguments on the same ctx -- every kind, every bit depth, with and without tRNS, a
width of 1, of 7, and streams of several chunks -- under both deflate levels, from host and device sources."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
import png_filter_ref as ref
from fennec_amd import FNX_DEFLATE_CHUNK as CH, FNX_PNG_GRAY, FNX_PNG_NRGBA, FNX_PNG_PALETTED

pytestmark = pytest.mark.gpu

SIZES = [(1, 5), (7, 3), (181, 181)]                                  # 181 x 181 RGB: 98 464 stream bytes, four chunks
KINDS = ["rgb", "rgba", "gray", "pal2", "pal4", "pal16", "pal17", "pal256"]


@pytest.fixture(scope="module", params=["fast", "dense"])
def ctx(request):
    c = fennec_amd.Context(0)
    c.set_deflate_level(request.param)
    c.level_name = request.param
    return c


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def content(kind, w, h, seed):
    """-> (source, FNX_PNG_* kind, ncolors, palette): noise above, smooth content below: stored and coded chunks"""
    half = (h + 1) // 2
    if kind in ("rgb", "rgba"):
        img = ref.smooth_rgba(w, h, seed, opaque=kind == "rgb")
        img[:half] = ref.noise_rgba(w, half, seed + 1, opaque=kind == "rgb")
        if kind == "rgba":
            img[-1, -1, 3] = 17
        return img, FNX_PNG_NRGBA, 0, None
    if kind == "gray":
        g = ref.smooth_rgba(w, h, seed)[..., 0].copy()
        g[:half] = ref.noise_rgba(w, half, seed + 1)[..., 0]
        return g, FNX_PNG_GRAY, 0, None
    n = int(kind[3:])
    rng = np.random.default_rng(seed)
    idx = (ref.smooth_rgba(w, h, seed)[..., 0].astype(np.int32) * n // 256).astype(np.uint8)
    idx[:half] = rng.integers(0, n, size=(half, w), dtype=np.uint8)
    pal = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    pal[:, 3] = 255
    if n != 4:
        pal[n // 2, 3] = 40                                           # tRNS up to and including entry n / 2; pal4: no tRNS chunk
    return idx, FNX_PNG_PALETTED, n, pal


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", SIZES)
def test_size_is_the_files_length(ctx, kind, w, h):
    src, k, ncolors, pal = content(kind, w, h, 1000 * w + h)
    file = ctx.png_encode(src, k, ncolors, -1, pal)
    assert ctx.last_kernel() == ("deflate_dense_chunk_kernel" if ctx.level_name == "dense" else "deflate_chunk_kernel")
    sizes = [ctx.png_encoded_size(src, k, ncolors, -1, pal), ctx.png_encoded_size(dev(src), k, ncolors, -1, pal),
             ctx.png_encoded_size(src, k, ncolors, -1, pal)]
    assert ctx.last_kernel() == ("deflate_dense_chunk_size_kernel" if ctx.level_name == "dense" else "deflate_chunk_size_kernel")
    print(f"{ctx.level_name} {kind} {w}x{h}: file {len(file)}, sizes {sizes}")
    assert sizes == [len(file)] * 3
    assert np.array_equal(ref.decode_png(file), src if k == FNX_PNG_NRGBA else pal[src] if k == FNX_PNG_PALETTED
                          else np.dstack([src, src, src, np.full_like(src, 255)]))
    if (w, h) == (181, 181) and kind == "rgb":
        assert ref.png_stream(src, k, ncolors)[0].size > 3 * CH
    # the opacity stated beforehand: the same size without the alpha scan's wait
    if k == FNX_PNG_NRGBA:
        assert ctx.png_encoded_size(src, k, 0, 1 if kind == "rgb" else 0) == len(file)


def test_the_file_still_comes_out_after_a_size_query(ctx):
    """the size-only form shares the token words with the emitting form and nothing else: a file made between two queries is whole"""
    src, k, ncolors, pal = content("rgb", 181, 181, 5)
    want = ctx.png_encode(src, k)
    assert ctx.png_encoded_size(src, k) == len(want)
    assert ctx.png_encode(src, k) == want
    small, _, _, _ = content("rgb", 7, 3, 6)
    assert ctx.png_encoded_size(small, k) == len(ctx.png_encode(small, k))
    assert ctx.png_encoded_size(src, k) == len(want)


def test_refusals(ctx):
    lib = fennec_amd.load_library()
    bad = fennec_amd.FNX_ERR_INVALID
    nb = C.c_size_t(7)
    idx = np.zeros((9, 67), np.uint8)
    # a paletted image without its palette, as fnx_png_encode refuses it
    assert lib.fnx_png_encoded_size(ctx._h, fennec_amd.FNX_HOST, FNX_PNG_PALETTED, idx.ctypes.data, 67, 67, 9, 4, -1, None, C.byref(nb)) == bad
    assert lib.fnx_png_encoded_size(ctx._h, fennec_amd.FNX_HOST, FNX_PNG_GRAY, idx.ctypes.data, 66, 67, 9, 0, -1, None, C.byref(nb)) == bad
    assert lib.fnx_png_encoded_size(ctx._h, fennec_amd.FNX_HOST, FNX_PNG_GRAY, idx.ctypes.data, 67, 67, 9, 0, -1, None, None) == bad
    assert nb.value == 7
