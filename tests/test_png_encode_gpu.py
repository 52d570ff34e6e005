"""fnx_png_encode / fennec_CompressFilePNG on the GPU: whole PNG files from the device deflate.  The file's chunks are held
against fennec_amd.png_file's (every chunk but IDAT byte for byte), IDAT must inflate to the numpy restatement's stream, and
Pillow must read the source's pixels back."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest

import fennec_amd
import jpeg_mini
import png_filter_ref as ref
from fennec_amd import FNX_PNG_GRAY, FNX_PNG_NRGBA, FNX_PNG_PALETTED, synth

pytestmark = pytest.mark.gpu

KINDS = ["rgb", "rgba", "gray", "pal8", "pal4", "pal2", "pal1"]


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def palette_of(n, seed):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    pal[:, 3] = 255
    if n > 2:
        pal[1, 3] = 40                                               # tRNS: up to and including entry 1
    return pal


def check_file(data, src, kind, ncolors, pal):
    wstream, wct, wdepth = ref.png_stream(src, kind, ncolors)
    h, w = src.shape[:2]
    got = ref.chunks(data)                                           # CRCs checked
    want = ref.chunks(fennec_amd.png_file(wstream, w, h, wct, wdepth, pal))
    assert [t for t, _ in got] == [t for t, _ in want]
    for (tag, body), (_, wbody) in zip(got, want):
        if tag != b"IDAT":
            assert body == wbody, tag
    idat = dict(got)[b"IDAT"]
    assert zlib.decompress(idat) == np.ascontiguousarray(wstream).tobytes()
    pixels = ref.decode_png(data)
    if kind == FNX_PNG_NRGBA:
        assert np.array_equal(pixels, src)
    elif kind == FNX_PNG_GRAY:
        assert np.array_equal(pixels[..., 0], src) and np.array_equal(pixels[..., 1], src) and (pixels[..., 3] == 255).all()
    else:
        assert np.array_equal(pixels, pal[src])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", [(5, 3), (67, 7), (1031, 37)])
def test_files(ctx, kind, w, h):
    import test_png_filter_gpu as filter_tests
    src, k, ncolors = filter_tests.content(kind, w, h, 100 * w + h)
    pal = palette_of(ncolors, w) if k == FNX_PNG_PALETTED else None
    files = [ctx.png_encode(src, k, ncolors, -1, pal), ctx.png_encode(filter_tests.dev(src), k, ncolors, -1, pal)]
    files.append(ctx.png_encode(src, k, ncolors, -1, pal))
    assert files[0] == files[1] == files[2], "host and device source, first and second call: the same file"
    check_file(files[0], src, k, ncolors, pal)


@pytest.mark.parametrize("kind", ["rgba", "gray", "pal4"])
def test_strided_and_misaligned_views(ctx, kind):
    import test_png_filter_gpu as filter_tests
    w, h = 67, 7
    if kind == "rgba":
        big = ref.noise_rgba(w + 6, h, 21, opaque=False)
        view, k, ncolors, pal = big[:, 1:w + 1], FNX_PNG_NRGBA, 0, None
    else:
        ncolors = 16 if kind == "pal4" else 0
        plane = np.random.default_rng(22).integers(0, 16 if ncolors else 256, size=(h, w + 9), dtype=np.uint8)
        view, k = plane[:, 3:3 + w], FNX_PNG_PALETTED if ncolors else FNX_PNG_GRAY
        pal = palette_of(ncolors, 3) if ncolors else None
    a = ctx.png_encode(view, k, ncolors, -1, pal)
    b = ctx.png_encode(filter_tests._same_view_on_device(view), k, ncolors, -1, pal)
    assert a == b
    check_file(a, np.ascontiguousarray(view), k, ncolors, pal)


def test_short_capacity_reports_the_size(ctx):
    src = ref.smooth_rgba(67, 9, 3)
    data = ctx.png_encode(src)
    lib = fennec_amd.load_library()
    nb = C.c_size_t(0)
    out = np.full(len(data) + 32, 0xAB, np.uint8)
    args = (ctx._h, fennec_amd.FNX_HOST, FNX_PNG_NRGBA, src.ctypes.data, src.strides[0], 67, 9, 0, -1, None, out.ctypes.data)
    assert lib.fnx_png_encode(*args, len(data) - 1, C.byref(nb)) == fennec_amd.FNX_ERR_INVALID
    assert nb.value == len(data) and (out == 0xAB).all()
    assert lib.fnx_png_encode(*args, len(out), C.byref(nb)) == 0
    assert out[:nb.value].tobytes() == data and (out[nb.value:] == 0xAB).all()
    assert ctx.last_kernel() == "deflate_chunk_kernel"
    # a paletted image without its palette is refused
    idx = np.zeros((9, 67), np.uint8)
    assert lib.fnx_png_encode(ctx._h, fennec_amd.FNX_HOST, FNX_PNG_PALETTED, idx.ctypes.data, 67, 67, 9, 4, -1, None, out.ctypes.data,
                              len(out), C.byref(nb)) == fennec_amd.FNX_ERR_INVALID


# ---- compressPNG end to end -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["two_colour", "translucent_gray", "photograph"])
def test_compress_png_with_the_device_deflate(ctx, name):
    import test_png_filter_gpu as filter_tests
    img = {"two_colour": lambda: filter_tests.two_colour(67, 33), "translucent_gray": lambda: filter_tests.translucent_gray(67, 33),
           "photograph": lambda: synth.large_photo(320, 240, 5)}[name]()
    files = [ctx.compress_png(img, device_deflate=True), ctx.compress_png(filter_tests.dev(img), device_deflate=True)]
    assert files[0] == files[1], "host and device images give the same file"
    got = ref.decode_png(files[0])
    if name == "translucent_gray":                                   # toGray drops alpha (convert.go:96): the reference's behaviour
        assert np.array_equal(got[..., 0], img[..., 0]) and (got[..., 3] == 255).all()
    else:
        assert np.array_equal(got, img)
    # the default route is what it was: png_reduce, png_filter, then zlib level 9 and the chunks on the host
    kind, pal, plane = ctx.png_reduce(img)
    stream, ct, bd = ctx.png_filter(img if kind == FNX_PNG_NRGBA else plane, kind, len(pal))
    parent = fennec_amd.png_file(stream, img.shape[1], img.shape[0], ct, bd, pal if kind == FNX_PNG_PALETTED else None, 9)
    assert ctx.compress_png(img) == parent == ctx.compress_png(img, device_deflate=False)
    host_chunks, dev_chunks = ref.chunks(parent), ref.chunks(files[0])
    assert [c for c in host_chunks if c[0] != b"IDAT"] == [c for c in dev_chunks if c[0] != b"IDAT"]
    assert zlib.decompress(dict(dev_chunks)[b"IDAT"]) == zlib.decompress(dict(host_chunks)[b"IDAT"])


# ---- the file route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("orient,max_w", [(1, 0), (6, 0), (3, 40)])
def test_compress_file_png(ctx, orient, max_w):
    img = synth.large_photo(96, 64, 7)
    data = jpeg_mini.encode(img, 2, 2, quality=90)
    kind, pal, stream, ct, depth, d0, d1 = ctx.compress_file_png_stream(data, orient, max_w, 0)
    want = fennec_amd.png_file(stream, d1[0], d1[1], ct, depth, pal if kind == FNX_PNG_PALETTED else None)
    file, kind2, e0, e1 = ctx.compress_file_png(data, orient, max_w, 0)
    assert (kind2, e0, e1) == (kind, d0, d1)
    assert np.array_equal(ref.decode_png(file), ref.decode_png(want))
    got, wanted = ref.chunks(file), ref.chunks(want)
    assert [c for c in got if c[0] != b"IDAT"] == [c for c in wanted if c[0] != b"IDAT"]
    assert zlib.decompress(dict(got)[b"IDAT"]) == np.ascontiguousarray(stream).tobytes()
    assert ctx.last_kernel() == "deflate_chunk_kernel"
    assert ctx.compress_file_png(data, orient, max_w, 0, cap=64)[0] == file      # a short first buffer: asked again with the size
