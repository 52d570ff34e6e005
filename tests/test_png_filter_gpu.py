"""fnx_png_filter / fennec_CompressFilePNGStream on the GPU: the PNG encoder's row stage against the numpy restatement in
tests/png_filter_ref.py (anchored by tests/test_png_filter_ref.py).  Every comparison is of the WHOLE stream, byte for byte,
in the host and in the device space, and a second call must return the same bytes."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
import png_filter_ref as ref
from fennec_amd import FNX_PNG_GRAY, FNX_PNG_NRGBA, FNX_PNG_PALETTED, synth

pytestmark = pytest.mark.gpu

KINDS = ["rgb", "rgba", "gray", "pal8", "pal4", "pal2", "pal1"]
NCOLORS = {"pal8": 256, "pal4": 16, "pal2": 4, "pal1": 2}


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def content(kind, w, h, seed):
    """-> (source array, FNX_PNG_* kind, ncolors): noise in the upper rows, smooth content below, so that several filters win"""
    if kind in ("rgb", "rgba"):
        img = ref.smooth_rgba(w, h, seed, opaque=kind == "rgb")
        img[: (h + 1) // 2] = ref.noise_rgba(w, (h + 1) // 2, seed + 1, opaque=kind == "rgb")
        if kind == "rgba":
            img[0, 0, 3] = 17                                        # translucent whatever the noise drew
        return img, FNX_PNG_NRGBA, 0
    if kind == "gray":
        g = ref.smooth_rgba(w, h, seed)[..., 0].copy()
        g[: (h + 1) // 2] = ref.noise_rgba(w, (h + 1) // 2, seed + 1)[..., 0]
        return g, FNX_PNG_GRAY, 0
    n = NCOLORS[kind]
    return np.random.default_rng(seed).integers(0, n, size=(h, w), dtype=np.uint8), FNX_PNG_PALETTED, n


def check(ctx, src, kind, ncolors=0, opaque=-1, want=None, spaces=("host", "device")):
    """one source (numpy, possibly a strided view) through the host and the device space, twice each, against the restatement"""
    wstream, wct, wdepth = ref.png_stream(src, kind, ncolors, opaque) if want is None else want
    for space in spaces:
        arg = src if space == "host" else _same_view_on_device(src)
        for _ in range(2):
            stream, ct, depth = ctx.png_filter(arg, kind, ncolors, opaque)
            ctx.sync()
            assert (ct, depth) == (wct, wdepth), (space, ct, depth)
            got = host(stream)
            assert got.shape == wstream.shape, (space, got.shape, wstream.shape)
            if not np.array_equal(got, wstream):
                bad = np.argwhere(got != wstream)
                raise AssertionError(f"{space}: {len(bad)} bytes differ, first at row {bad[0][0]} byte {bad[0][1]}: "
                                     f"types {got[bad[0][0], 0]} / {wstream[bad[0][0], 0]}")
    return wstream, wct, wdepth


def _same_view_on_device(a):
    """the array's base buffer on the device, and the same window into it: padding and misalignment travel along"""
    base = a
    while base.base is not None and isinstance(base.base, np.ndarray):
        base = base.base
    d = dev(base)
    if base is a:
        return d
    off = a.__array_interface__["data"][0] - base.__array_interface__["data"][0]
    import torch
    return torch.as_strided(d.view(-1), a.shape, a.strides, off)


# ---- sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w", [1, 2, 3, 5, 67, 256, 1031])
def test_small_shapes(ctx, kind, w):
    """w = 1: no left neighbour; h = 1: the row above is zeros; odd n: output rows at every alignment"""
    for h in (1, 2, 7):
        src, k, n = content(kind, w, h, 100 * w + h)
        check(ctx, src, k, n)


@pytest.mark.parametrize("kind", KINDS)
def test_many_workgroups_and_the_row_above(ctx, kind):
    src, k, n = content(kind, 1031, 517, 7)
    stream, _, _ = check(ctx, src, k, n)
    if k != FNX_PNG_PALETTED:
        assert len(set(stream[:, 0].tolist())) >= 3, "the content no longer exercises several filters"


def test_full_hd_rgb(ctx):
    img = synth.large_photo(1920, 1080, 3)
    img[..., 3] = 255
    check(ctx, img, FNX_PNG_NRGBA)


def test_all_five_types_are_chosen_on_the_device(ctx):
    img = ref.noise_rgba(64, 67, 1)
    stream, ct, _ = ctx.png_filter(img)
    assert ct == 2 and set(stream[:, 0].tolist()) == {0, 1, 2, 3, 4}
    check(ctx, img, FNX_PNG_NRGBA)


# ---- strides, alignment, capacity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(5, 3), (67, 9), (1031, 3)])
def test_padded_source_with_other_colours_in_the_padding(ctx, w, h):
    big = ref.noise_rgba(w + 6, h, 21, opaque=False)                 # translucent noise left and right of the window
    big[:, 1:w + 1, 3] = 255
    check(ctx, big[:, 1:w + 1], FNX_PNG_NRGBA)                       # 4 bytes off a 16-byte boundary
    check(ctx, big[:, 4:w + 4], FNX_PNG_NRGBA)
    plane = np.random.default_rng(22).integers(0, 256, size=(h, w + 9), dtype=np.uint8)
    plane4 = plane & 3
    for off in (0, 1, 2, 3):                                         # byte planes start anywhere
        check(ctx, plane[:, off:off + w], FNX_PNG_GRAY)
        check(ctx, plane4[:, off:off + w], FNX_PNG_PALETTED, 4)
    check(ctx, plane[:, 1:1 + w], FNX_PNG_PALETTED, 256)


@pytest.mark.parametrize("kind", ["rgb", "rgba", "gray", "pal2"])
def test_spare_capacity_keeps_its_sentinel(ctx, kind):
    src, k, n = content(kind, 67, 9, 31)
    want, wct, wdepth = ref.png_stream(src, k, n)
    for space in ("host", "device", "device_src"):
        arg = src if space == "host" else dev(src)
        out = np.full(want.size + 64, 0xAB, np.uint8)
        out = dev(out) if space == "device" else out
        stream, ct, depth = ctx.png_filter(arg, k, n, -1, out)
        ctx.sync()
        assert (ct, depth) == (wct, wdepth) and np.array_equal(host(stream), want), space
        assert (host(out)[want.size:] == 0xAB).all(), f"{space}: bytes behind the stream were written"


def test_short_capacity_reports_the_size(ctx):
    src, k, n = content("rgb", 67, 9, 32)
    lib = fennec_amd.load_library()
    nb, ct, bd = C.c_size_t(0), C.c_int(0), C.c_int(0)
    need = 9 * (1 + 3 * 67)
    out = np.full(need, 0xAB, np.uint8)
    rc = lib.fnx_png_filter(ctx._h, fennec_amd.FNX_HOST, k, src.ctypes.data, src.strides[0], 67, 9, 0, -1, out.ctypes.data, need - 1,
                            C.byref(nb), C.byref(ct), C.byref(bd))
    assert rc == fennec_amd.FNX_ERR_INVALID and (nb.value, ct.value, bd.value) == (need, 2, 8)
    assert (out == 0xAB).all()
    # arguments that are refused with a live ctx: nothing is launched, nothing written
    for args in ((FNX_PNG_PALETTED, src.strides[0], 67, 9, 0), (FNX_PNG_PALETTED, src.strides[0], 67, 9, 257), (FNX_PNG_GRAY, 66, 67, 9, 0),
                 (FNX_PNG_NRGBA, 4 * 67 - 4, 67, 9, 0), (FNX_PNG_NRGBA, src.strides[0], 65536, 9, 0), (7, src.strides[0], 67, 9, 0)):
        kind, stride, w, h, ncol = args
        assert lib.fnx_png_filter(ctx._h, fennec_amd.FNX_HOST, kind, src.ctypes.data, stride, w, h, ncol, -1, out.ctypes.data, need,
                                  C.byref(nb), C.byref(ct), C.byref(bd)) == fennec_amd.FNX_ERR_INVALID, args
    assert (out == 0xAB).all()


# ---- opacity ------------------------------------------------------------------------------------------------------------
def test_opacity_is_decided_on_visible_pixels(ctx):
    w, h = 67, 9
    big = ref.smooth_rgba(w + 3, h, 41)
    view = big[:, :w]
    big[h - 1, w, 3] = 254                                           # row padding: image.NRGBA.Opaque() does not look there
    assert check(ctx, view, FNX_PNG_NRGBA)[1] == 2
    big[h - 1, w - 1, 3] = 254                                       # the last visible pixel
    assert check(ctx, view, FNX_PNG_NRGBA)[1] == 6
    big[h - 1, w - 1, 3] = 255
    big[0, 0, 3] = 0                                                 # and the first
    assert check(ctx, view, FNX_PNG_NRGBA)[1] == 6


def test_stated_opacity_agrees_with_the_decision(ctx):
    for kind in ("rgb", "rgba"):
        src, k, _ = content(kind, 67, 9, 42)
        decided = check(ctx, src, k)
        stated = check(ctx, src, k, 0, 1 if kind == "rgb" else 0)
        assert decided[1:] == stated[1:] and np.array_equal(decided[0], stated[0])
        # the caller's word is taken: RGBA rows for an opaque image, alpha dropped from a translucent one
        other = check(ctx, src, k, 0, 0 if kind == "rgb" else 1)
        assert other[1] == (6 if kind == "rgb" else 2)


# ---- paletted -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ncolors", [1, 2, 3, 4, 5, 16, 17, 256])
def test_paletted_depths_and_spare_bits(ctx, ncolors):
    depth = ref.depth_of(ncolors)
    for w in (1, 2, 3, 4, 5, 6, 7, 8, 9, 31, 33, 250, 1027):          # 1 .. 7 spare bits in the last byte at every depth
        idx = np.random.default_rng(w + ncolors).integers(0, ncolors, size=(3, w), dtype=np.uint8)
        stream, ct, d = check(ctx, idx, FNX_PNG_PALETTED, ncolors)
        assert (ct, d) == (3, depth) and stream.shape[1] == 1 + (w * depth + 7) // 8 and not stream[:, 0].any()


# ---- ties and abs8 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ref.tie_cases(), ids=lambda c: c[0])
def test_ties_go_to_the_filter_tried_first(ctx, case):
    _, img, types = case
    stream, _, _ = check(ctx, img, FNX_PNG_NRGBA)
    assert stream[:, 0].tolist() == types
    got, _, _ = ctx.png_filter(img)
    assert got[:, 0].tolist() == types


@pytest.mark.parametrize("case", ref.abs8_cases(), ids=lambda c: c[0])
def test_abs8_at_127_128_129(ctx, case):
    _, g, _, want = case
    check(ctx, g, FNX_PNG_GRAY)
    assert ctx.png_filter(g)[0][:, 0].tolist() == [want]
    # the same residuals at every lane position of a wide row: the row repeated, Sub and Paeth still differ from Up only at the seam
    wide = np.tile(g, (2, 300))
    check(ctx, wide, FNX_PNG_GRAY)


# ---- end to end -----------------------------------------------------------------------------------------------------------
def two_colour(w, h):
    cell = (np.add.outer(np.arange(h) // 5, np.arange(w) // 7) % 2).astype(np.uint8)
    return np.ascontiguousarray(np.where(cell[..., None] == 1, np.array([200, 40, 40, 255], np.uint8), np.array([20, 60, 180, 255], np.uint8)).astype(np.uint8))


def translucent_gray(w, h, seed=0):
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    return np.ascontiguousarray(np.stack([v, v, v, rng.integers(0, 256, size=(h, w), dtype=np.uint8)], axis=-1))


@pytest.mark.parametrize("name", ["two_colour", "translucent_gray", "photograph"])
def test_compress_png_decodes_to_the_source(ctx, name):
    img = {"two_colour": lambda: two_colour(67, 33), "translucent_gray": lambda: translucent_gray(67, 33),
           "photograph": lambda: synth.large_photo(320, 240, 5)}[name]()
    want_ihdr = {"two_colour": (3, 1), "translucent_gray": (0, 8), "photograph": (2 if ref.visible_opaque(img) else 6, 8)}[name]
    files = [ctx.compress_png(img), ctx.compress_png(dev(img))]
    assert files[0] == files[1], "host and device images give the same file"
    got = ref.decode_png(files[0])
    ihdr = dict(ref.chunks(files[0]))[b"IHDR"]
    assert (ihdr[9], ihdr[8]) == want_ihdr
    if name == "translucent_gray":                                   # toGray drops alpha (convert.go:96): the reference's behaviour
        assert np.array_equal(got[..., 0], img[..., 0]) and (got[..., 3] == 255).all()
    else:
        assert np.array_equal(got, img)


# ---- the file route -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gray", "two_colour", "photograph"])
def test_file_route(ctx, orc, name):
    import test_png_reduce_gpu as reduce_tests
    data = {"gray": reduce_tests.gray_jpeg, "two_colour": reduce_tests.two_colour_jpeg,
            "photograph": lambda: orc.jpeg_encode(synth.large_photo(320, 240, 4), 90)}[name]()
    dec = orc.jpeg_decode(data)
    for orient, max_w, max_h in ((1, 0, 0), (6, 0, 0), (3, 160, 0)):
        img = dec if orient == 1 else orc.apply_orientation(dec, orient)
        orig = (img.shape[1], img.shape[0])
        img = np.ascontiguousarray(orc.smart_resize(img, max_w, max_h) if (max_w or max_h) else img)
        wkind, wpal, wplane = reduce_tests.restate(img)
        want, wct, wdepth = ref.png_stream(img if wplane is None else wplane, wkind, len(wpal))
        kind, pal, stream, ct, depth, d0, d1 = ctx.compress_file_png_stream(data, orient, max_w, max_h)
        assert (d0, d1) == (orig, (img.shape[1], img.shape[0]))
        assert kind == wkind and np.array_equal(pal, wpal) and (ct, depth) == (wct, wdepth)
        assert np.array_equal(stream, want)
        file = fennec_amd.png_file(stream, d1[0], d1[1], ct, depth, pal if kind == FNX_PNG_PALETTED else None)
        assert np.array_equal(ref.decode_png(file), img)             # a JPEG decodes opaque: toGray loses nothing
    # the reduced entry's answer is what it was
    kind2, pal2, out2, _, _ = ctx.compress_file_png_reduce(data)
    wkind, wpal, wplane = reduce_tests.restate(dec)
    assert kind2 == wkind and np.array_equal(pal2, wpal) and np.array_equal(out2, dec if wplane is None else wplane)


def test_file_route_short_cap(ctx, orc):
    data = orc.jpeg_encode(synth.large_photo(320, 240, 4), 90)
    lib = fennec_amd.load_library()
    src = np.frombuffer(data, np.uint8)
    o = fennec_amd.FileOptions(1, 0, 0, 0, 0.0)
    k, nc, ct, bd, n = C.c_int(0), C.c_int(-1), C.c_int(0), C.c_int(0), C.c_size_t(0)
    palbuf = np.zeros((256, 4), np.uint8)
    dims = (C.c_int * 4)()
    need = 240 * (1 + 3 * 320)
    buf = np.full(need, 0xAB, np.uint8)
    rc = lib.fennec_CompressFilePNGStream(ctx._h, src.ctypes.data, len(data), C.byref(o), C.byref(k), palbuf.ctypes.data, C.byref(nc),
                                          C.byref(ct), C.byref(bd), buf.ctypes.data, need - 1, C.byref(n), dims)
    assert rc == fennec_amd.FNX_ERR_INVALID
    assert (n.value, k.value, nc.value, ct.value, bd.value, list(dims)) == (need, FNX_PNG_NRGBA, 0, 2, 8, [320, 240, 320, 240])
    assert (buf == 0xAB).all()


# ---- routes -----------------------------------------------------------------------------------------------------------------
def test_last_kernel_names_the_new_kernels(ctx):
    ctx.png_filter(ref.noise_rgba(9, 3, 1))
    assert ctx.last_kernel() == "png_filter_kernel"
    ctx.png_filter(np.zeros((3, 9), np.uint8), FNX_PNG_PALETTED, 4)
    assert ctx.last_kernel() == "png_pack_kernel"
    ctx.png_filter(np.zeros((3, 9), np.uint8))
    assert ctx.last_kernel() == "png_filter_kernel"
