"""fnx_png_decode on the GPU: whole images, ==, against tests/png_decode_ref.py -- in the host and the device space, twice each,
the second call returning the first one's bytes.  The shapes are the ones png_unfilter_kernel can break at: around the wave
(64 rows) and the workgroup's rows in flight (R), widths around one pixel and one 16-byte load, chains of every length.

Large cases take their expectation from the samples the file was written from (png_decode_ref.expected: the pixel rule over
the raw rows) instead of the reference's byte-by-byte unfilter; tests/test_png_decode_ref.py holds the two against each
other on every colour type and filter."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
import png_decode_ref as ref
from fennec_amd import FNX_PNG_DECODE_ROWS as R
from fennec_amd import FNX_PNG_GRAY, FNX_PNG_NRGBA, FNX_PNG_PALETTED

pytestmark = pytest.mark.gpu

KERNELS = "png_unfilter_kernel, png_expand_kernel"
HEIGHTS = [1, 2, 63, 64, 65, 129, R - 1, R, R + 1, 2 * R + 3]
WIDTHS = [1, 2, 3, 5, 67, 1031]


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def expected(samples, color_type, depth, plte=None, trns=None):
    s = np.asarray(samples)
    return ref.expand(ref.pack_rows(s, color_type, depth), s.shape[1], color_type, depth, plte, trns)


def check(ctx, data, want):
    """host and device space, twice each: every result is the whole expected image"""
    import torch
    for _ in range(2):
        host = ctx.png_decode(data, "host")
        assert ctx.last_kernel() == KERNELS
        dev = ctx.png_decode(data, "device")
        assert ctx.last_kernel() == KERNELS
        assert isinstance(dev, torch.Tensor) and dev.is_cuda
        assert host.shape == want.shape and np.array_equal(host, want)
        assert np.array_equal(dev.cpu().numpy(), want)


def plan(name, h, seed=0):
    rng = np.random.default_rng(seed)
    if name.startswith("all"):
        return [int(name[3:])] * h
    if name.startswith("first"):                       # the type on row 0 alone (the row above is zeros), Up below
        return [int(name[5:])] + [2] * (h - 1)
    if name == "random":
        return rng.integers(0, 5, size=h).tolist()
    raise KeyError(name)


# ---- rows and widths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", HEIGHTS)
def test_heights_and_widths_rgb(ctx, h):
    for w in WIDTHS:
        s = ref.random_samples(w, h, 2, 8, 1000 * h + w)
        # chains as long as the image: Average and Paeth alternate below row 0, which takes each type in turn
        filters = [(h + w) % 5] + [3 + (y & 1) for y in range(1, h)]
        check(ctx, ref.write_png(s, 2, 8, filters=filters), expected(s, 2, 8))


@pytest.mark.parametrize("depth", [1, 2, 4])
def test_sub_byte_widths(ctx, depth):
    for w in (1, 7, 8, 9, 17):
        for ct in (0, 3):
            for h in (1, 65, R + 1):
                s = ref.random_samples(w, h, ct, depth, 10 * w + depth)
                pal = ref.random_palette(1 << depth, w) if ct == 3 else None
                data = ref.write_png(s, ct, depth, filters=plan("random", h, w), palette=pal)
                check(ctx, data, expected(s, ct, depth, pal))


# ---- filter plans ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["all0", "all1", "all2", "all3", "all4", "first0", "first1", "first2", "first3", "first4", "random"])
@pytest.mark.parametrize("ct,depth", [(2, 8), (6, 16), (0, 8)])
def test_filter_plans(ctx, name, ct, depth):
    w, h = 67, R + 1
    s = ref.random_samples(w, h, ct, depth, 7)
    data = ref.write_png(s, ct, depth, filters=plan(name, h, 3))
    assert ref.filter_types(data) == plan(name, h, 3)
    check(ctx, data, expected(s, ct, depth))


def test_small_images_against_the_byte_by_byte_reference(ctx):
    """the reference's own unfilter, not the writer's samples"""
    for ct, depth in ref.PAIRS:
        s = ref.random_samples(19, 70, ct, depth, ct * 16 + depth)
        pal = ref.random_palette(1 << min(depth, 8), 9) if ct == 3 else None
        data = ref.write_png(s, ct, depth, filters=plan("random", 70, depth), palette=pal)
        check(ctx, data, ref.decode(data))


@pytest.mark.parametrize("seg", [1, 2, 64, 65, R + 1])
def test_segment_lengths(ctx, seg):
    """None / Sub rows every `seg` rows: chain segments of exactly that length, Paeth and Average inside"""
    w, h = 37, 2 * R + 3
    filters = [(y // seg) % 2 if y % seg == 0 else 3 + (y & 1) for y in range(h)]
    s = ref.random_samples(w, h, 6, 8, seg)
    check(ctx, ref.write_png(s, 6, 8, filters=filters), expected(s, 6, 8))


def test_tall_narrow_and_short_wide_paeth(ctx):
    s = ref.random_samples(3, 2 * R + 3, 2, 8, 1)
    check(ctx, ref.write_png(s, 2, 8, filters=[4] * (2 * R + 3)), expected(s, 2, 8))
    s = ref.random_samples(5000, 3, 2, 8, 2)
    check(ctx, ref.write_png(s, 2, 8, filters=[4] * 3), expected(s, 2, 8))


# ---- conversions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct,depth", ref.PAIRS)
def test_every_pair(ctx, ct, depth):
    w, h = 33, 66
    s = ref.random_samples(w, h, ct, depth, 5)
    pal = ref.random_palette(1 << min(depth, 8), 4) if ct == 3 else None
    data = ref.write_png(s, ct, depth, filters=plan("random", h, 8), palette=pal, idat_sizes=[1, 1, 1, 7, 100])
    check(ctx, data, expected(s, ct, depth, pal))


@pytest.mark.parametrize("ct,depth", [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16)])
def test_trns_for_grey_and_truecolour(ctx, ct, depth):
    w, h = 21, 9
    s = ref.random_samples(w, h, ct, depth, 6)
    key = [int(v) for v in s[4, 5]]
    s[::2, ::3] = key                                   # matches all over the image
    if depth == 16:
        s[1, 1] = [v ^ 0x0100 for v in key]             # the low bytes match, the samples do not
    hi = 0xa5 if depth < 16 else None                   # at depth <= 8 only the LOW byte of a tRNS sample counts
    trns = b"".join(bytes([(v >> 8) if hi is None else hi, v & 255]) for v in key)
    data = ref.write_png(s, ct, depth, filters=plan("random", h, 2), trns=trns)
    want = expected(s, ct, depth, None, trns)
    assert (want[..., 3] == 0).any() and (want[..., 3] == 255).any()
    check(ctx, data, want)
    check(ctx, data, ref.decode(data))


@pytest.mark.parametrize("depth", [1, 2, 4, 8])
def test_palette_with_trns_and_short_palette(ctx, depth):
    w, h = 23, 11
    top = 1 << depth
    npal = max(1, top - 1 - top // 4)                     # shorter than the largest index
    s = ref.random_samples(w, h, 3, depth, 9)
    assert s.max() >= npal
    pal = ref.random_palette(npal, depth)
    alphas = bytes(([0, 255, 128, 1, 254, 77] * 43)[:max(1, npal - 1 if depth < 8 else npal + 5)])
    for trns in (None, alphas):
        data = ref.write_png(s, 3, depth, filters=[0] * h, palette=pal, trns=trns)
        want = expected(s, 3, depth, pal, trns)
        check(ctx, data, want)
        assert np.array_equal(ref.decode(data), want)


def test_alpha_zero_full_and_partial(ctx):
    for ct, depth in [(4, 8), (4, 16), (6, 8), (6, 16)]:
        s = ref.random_samples(29, 13, ct, depth, 3)
        full = (1 << depth) - 1
        a = s[..., -1]
        assert (a == 0).any() and (a == full).any() and ((a > 0) & (a < full)).any()
        data = ref.write_png(s, ct, depth, filters=plan("random", 13, 1))
        check(ctx, data, ref.decode(data))


def test_strided_destination(ctx):
    import torch
    w, h = 67, 70
    s = ref.random_samples(w, h, 6, 8, 12)
    data = ref.write_png(s, 6, 8, filters=plan("random", h, 5))
    want = expected(s, 6, 8)
    for _ in range(2):
        big = np.full((h, w + 5, 4), 0xAB, np.uint8)
        ctx.png_decode(data, "host", out=big[:, 2:w + 2])
        assert np.array_equal(big[:, 2:w + 2], want) and (big[:, :2] == 0xAB).all() and (big[:, w + 2:] == 0xAB).all()
        dbig = torch.full((h, w + 5, 4), 0xAB, dtype=torch.uint8, device="cuda:0")
        ctx.png_decode(data, "device", out=dbig[:, 2:w + 2])
        got = dbig.cpu().numpy()
        assert np.array_equal(got[:, 2:w + 2], want) and (got[:, :2] == 0xAB).all() and (got[:, w + 2:] == 0xAB).all()
        assert ctx.last_kernel() == KERNELS


def test_dimensions_only(ctx):
    s = ref.random_samples(67, 41, 2, 8, 1)
    data = ref.write_png(s, 2, 8)
    assert ctx.png_decode_config(data) == (67, 41)
    assert fennec_amd.png_info(data) == (67, 41, 2, 8, 0)


# ---- round trip with the project's own encoder ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rgb", "rgba", "gray", "pal8", "pal4", "pal2", "pal1"])
def test_round_trip_with_png_encode(ctx, kind):
    import test_png_filter_gpu as filter_tests
    w, h = 131, 77
    src, k, ncolors = filter_tests.content(kind, w, h, 17)
    pal = None
    if k == FNX_PNG_PALETTED:
        pal = np.random.default_rng(3).integers(0, 256, size=(ncolors, 4), dtype=np.uint8)
        pal[:, 3] = 255
        if ncolors > 2:
            pal[1, 3] = 40
            pal[0, 3] = 0
    data = ctx.png_encode(src, k, ncolors, -1, pal)
    if k == FNX_PNG_NRGBA:
        want = src
    elif k == FNX_PNG_GRAY:
        want = np.stack([src, src, src, np.full_like(src, 255)], -1)
    else:
        table = np.array([ref.palette_pixel(*(int(v) for v in e)) for e in pal], np.uint8)      # toNRGBA of the plane's meaning
        want = table[src]
    check(ctx, data, want)
    assert np.array_equal(ref.decode(data), want)


# ---- damaged files: host-side refusals, nothing is launched ---------------------------------------------------------------
def test_damaged_files_are_refused_before_any_launch(ctx):
    s = ref.random_samples(9, 5, 2, 8, 1)
    good = ref.write_png(s, 2, 8, filters=[0, 1, 2, 3, 4])
    ctx.png_decode(good, "host")
    img = fennec_amd.synth.large_photo(64, 48, 1)
    ctx.GaussianBlur(img, 1.0)
    before = ctx.last_kernel()
    assert before != KERNELS
    bad_filter = ref.write_png(s, 2, 8, filters=[0, 1, 5, 3, 4])
    flipped = bytearray(good)
    flipped[len(good) - 20] ^= 0x40                     # inside the last IDAT: its CRC no longer matches
    import zlib
    short = ref.SIG + ref.ihdr(9, 5, 8, 2) + ref.chunk(b"IDAT", zlib.compress(b"\0" * (5 * 28 - 1))) + ref.chunk(b"IEND", b"")
    long = ref.SIG + ref.ihdr(9, 5, 8, 2) + ref.chunk(b"IDAT", zlib.compress(b"\0" * (5 * 28 + 1))) + ref.chunk(b"IEND", b"")
    for data in (bad_filter, bytes(flipped), short, long, good[:-30]):
        with pytest.raises(fennec_amd.FennecError) as e:
            ctx.png_decode(data, "host")
        assert not isinstance(e.value, fennec_amd.FennecUnsupported)
        assert ctx.last_kernel() == before
    with pytest.raises(fennec_amd.FennecUnsupported):
        ctx.png_decode(ref.write_png(s, 2, 8, interlace=1), "device")
    # a header that promises 14 GB over an IDAT of a few bytes: refused from the file's own size (a deflate stream grows at most
    # 1032-fold), before any memory is sized by the header
    huge = ref.SIG + ref.ihdr(60000, 60000, 8, 6) + ref.chunk(b"IDAT", zlib.compress(b"\0" * 1000)) + ref.chunk(b"IEND", b"")
    assert ctx.png_decode_config(huge) == (60000, 60000)
    import torch
    view = torch.empty(4, dtype=torch.uint8, device="cuda:0")
    buf = np.frombuffer(huge, np.uint8)
    w, h = C.c_int(), C.c_int()
    rc = ctx._lib.fnx_png_decode(ctx._h, buf.ctypes.data, len(huge), fennec_amd.FNX_DEVICE, view.data_ptr(), 4 * 60000, C.byref(w), C.byref(h))
    assert rc == fennec_amd.FNX_ERR_INVALID and b"not enough pixel data" in ctx._lib.fnx_last_error()
    assert (w.value, h.value) == (60000, 60000) and ctx.last_kernel() == before
    # the space is checked also where only the dimensions are asked for
    assert ctx._lib.fnx_png_decode(ctx._h, buf.ctypes.data, len(huge), 7, None, 0, C.byref(w), C.byref(h)) == fennec_amd.FNX_ERR_INVALID


# ---- fennec_CompressFile* with PNG bytes -----------------------------------------------------------------------------------
def _sources():
    rng = np.random.default_rng(4)
    photo = fennec_amd.synth.large_photo(96, 64, 3)
    translucent = rng.integers(0, 256, size=(41, 67, 4), dtype=np.int64)
    return {"translucent": ref.write_png(translucent, 6, 8, filters=plan("random", 41, 1)),
            "opaque": ref.write_png(photo[..., :3].astype(np.int64), 2, 8, filters=plan("random", 64, 2))}


@pytest.mark.parametrize("name", ["translucent", "opaque"])
def test_compress_file_entries_take_png_bytes(ctx, name):
    data = _sources()[name]
    dec = ctx.png_decode(data, "host")
    assert np.array_equal(dec, ref.decode(data))
    dims = (dec.shape[1], dec.shape[0])
    # CompressFileJPEG, Format: JPEG and Format: Auto
    out, q, s, steps, od, fd = ctx.compress_file_jpeg(data, 0.94, auto_format=False)
    assert (out, q, s, steps) == ctx.jpeg_compress(dec, 0.94) and od == fd == dims
    out, q, s, steps, od, fd = ctx.compress_file_jpeg(data, 0.94, auto_format=True)
    if name == "translucent":
        assert out is None and od == fd == dims          # analyzeFormat picks PNG for a translucent source
    else:
        assert (out, q, s, steps) == ctx.jpeg_compress(dec, 0.94)
    # the stages in between: orientation and smartResize on the decoded pixels
    turned = ctx.ApplyOrientation(dec, 6)
    out, q, s, steps, od, fd = ctx.compress_file_jpeg(data, 0.94, orient=6, auto_format=False)
    assert (out, q, s, steps) == ctx.jpeg_compress(turned, 0.94) and od == (dims[1], dims[0])
    # PNGReduce, PNGStream, PNG
    kind, pal, plane = ctx.png_reduce(dec)
    k2, pal2, out2, d0, d1 = ctx.compress_file_png_reduce(data)
    assert k2 == kind and np.array_equal(pal2, pal) and d0 == d1 == dims
    assert np.array_equal(out2, dec if kind == FNX_PNG_NRGBA else plane)
    stream, ct, bd = ctx.png_filter(dec if kind == FNX_PNG_NRGBA else plane, kind, len(pal))
    k3, pal3, stream3, ct3, bd3, e0, e1 = ctx.compress_file_png_stream(data)
    assert (k3, ct3, bd3, e0, e1) == (kind, ct, bd, dims, dims) and np.array_equal(stream3, stream)
    file, k4, f0, f1 = ctx.compress_file_png(data)
    assert (k4, f0, f1) == (kind, dims, dims)
    assert file == ctx.png_encode(dec if kind == FNX_PNG_NRGBA else plane, kind, len(pal), -1, pal if kind == FNX_PNG_PALETTED else None)
    assert np.array_equal(ref.decode(file), dec)         # and the library reads its own file back


def test_mixed_batch_of_jpeg_and_png_files(ctx):
    import jpeg_mini
    fa = fennec_amd
    L = fa.load_library()
    src = _sources()
    files = [jpeg_mini.encode(fa.synth.large_photo(96, 64, 7), 2, 2, quality=90), src["opaque"], src["translucent"],
             jpeg_mini.encode(fa.synth.large_photo(80, 48, 8), 1, 1, quality=85)]
    n = len(files)
    default = fa.FileOptions(1, 0, 0, 1, 0.94)
    per = (C.POINTER(fa.FileOptions) * n)()
    arrs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    srcs = (C.c_void_p * n)(*[a.ctypes.data for a in arrs])
    sizes = (C.c_size_t * n)(*[len(f) for f in files])
    bufs = [np.empty(4 * len(f) + 65536, dtype=np.uint8) for f in files]
    outs = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    caps = (C.c_size_t * n)(*[b.size for b in bufs])
    res = (fa.NativeBatchResult * n)()
    dims = (C.c_int * (4 * n))()
    assert L.fennec_CompressBatchJPEGOpts(0, 2, n, srcs, sizes, C.byref(default), per, outs, caps, res, dims, None, None, None) == fa.FNX_OK
    for i in range(n):
        out, q, s, steps, od, fd = ctx.compress_file_jpeg(files[i], 0.94, auto_format=True)
        assert tuple(dims[4 * i:4 * i + 4]) == od + fd, i
        if out is None:
            assert res[i].status == fa.FNX_NOOP, i          # analyzeFormat picked PNG: the caller's compressPNG
            continue
        assert res[i].status == fa.FNX_OK and not res[i].failed, i
        assert (res[i].quality, res[i].ssim, res[i].steps, res[i].compressed_size) == (q, s, steps, len(out)), i
        assert bufs[i][:res[i].compressed_size].tobytes() == out, i
    assert res[2].status == fa.FNX_NOOP and res[1].status == fa.FNX_OK
