"""fnx_png_reduce / fennec_CompressFilePNGReduce on the GPU: compressPNG's decision and reduced image (compress.go:90-153,
convert.go:76-100) against a numpy restatement that lives here.

The restatement: pack the w visible pixels of every row to uint32, np.unique(..., return_index=True); PALETTED iff the count is
<= max_colors, the palette is the unique colours sorted by first index, the plane each pixel's rank; else GRAY iff every
pixel of the FLAT byte range (row padding included) has r == g == b.  Every comparison is integer equality."""
from __future__ import annotations

import ctypes as C
import io

import numpy as np
import pytest

import fennec_amd
from fennec_amd import FNX_PNG_GRAY, FNX_PNG_NRGBA, FNX_PNG_PALETTED, synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


# ---- the restatement ------------------------------------------------------------------------------------------------
def pack(img):
    a = img.astype(np.uint32)
    return a[..., 0] | (a[..., 1] << 8) | (a[..., 2] << 16) | (a[..., 3] << 24)


def unpack(words):
    w = np.asarray(words, dtype=np.uint32)
    return np.stack([w & 255, (w >> 8) & 255, (w >> 16) & 255, w >> 24], axis=-1).astype(np.uint8)


def flat_is_gray(img):
    """isGrayscale (convert.go:76-84) over the Pix slice of a (sub)image: (h-1)*stride + 4w bytes from its first pixel."""
    h, w = img.shape[:2]
    stride = img.strides[0] if h > 1 else 4 * w
    n = (h - 1) * stride + 4 * w
    flat = np.lib.stride_tricks.as_strided(img, shape=(n // 4, 4), strides=(4, 1))
    return bool(np.all((flat[:, 0] == flat[:, 1]) & (flat[:, 1] == flat[:, 2])))


def restate(img, max_colors=256):
    """-> (kind, palette (n, 4), plane (h, w) or None)"""
    h, w = img.shape[:2]
    words = pack(img).ravel()
    u, first, inv = np.unique(words, return_index=True, return_inverse=True)
    if len(u) <= max_colors:
        order = np.argsort(first, kind="stable")
        rank = np.empty(len(u), dtype=np.int64)
        rank[order] = np.arange(len(u))
        return FNX_PNG_PALETTED, unpack(u[order]), rank[inv.ravel()].reshape(h, w).astype(np.uint8)
    if flat_is_gray(img):
        return FNX_PNG_GRAY, np.zeros((0, 4), np.uint8), np.ascontiguousarray(img[..., 0])
    return FNX_PNG_NRGBA, np.zeros((0, 4), np.uint8), None


def host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def check(ctx, src, max_colors=256, want=None, **kw):
    """one call (src: numpy or a device tensor) against the restatement; every PALETTED answer also meets the order-free
    property that is the parity with the reference: palette[plane] is the source and the palette has no duplicates"""
    kind, pal, plane = ctx.png_reduce(src, max_colors, **kw)
    ctx.sync()
    img = host(src)
    wkind, wpal, wplane = restate(img, max_colors) if want is None else want
    assert kind == wkind, (kind, wkind)
    assert pal.shape == wpal.shape and np.array_equal(pal, wpal), "palette"
    if kind == FNX_PNG_NRGBA:
        assert plane is None
        return kind, pal, plane
    got = host(plane)[:, :img.shape[1]]
    assert np.array_equal(got, wplane), "plane"
    if kind == FNX_PNG_PALETTED:
        assert np.array_equal(pal[got], img), "palette[plane] != source"
        assert len(np.unique(pack(pal))) == len(pal), "duplicate palette entries"
    return kind, pal, plane


def colors(n, seed):
    """n distinct random colours (n, 4)"""
    rng = np.random.default_rng(seed)
    words = rng.integers(0, 1 << 32, size=4 * n + 16, dtype=np.uint64).astype(np.uint32)
    c = unpack(words)
    _, keep = np.unique(pack(c), return_index=True)
    return c[np.sort(keep)[:n]]


def image_of(w, h, pal, seed):
    """a w x h image in which every colour of pal occurs (w*h >= len(pal)), in random places"""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, len(pal), size=w * h)
    idx[rng.permutation(w * h)[:len(pal)]] = np.arange(len(pal))
    return np.ascontiguousarray(pal[idx].reshape(h, w, 4))


def translucent_gray(w, h, seed=0):
    """grey pixels with more than 256 (v, a) pairs: tryPalettize gives up, isGrayscale holds"""
    rng = np.random.default_rng(seed)
    v = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    a = rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    img = np.stack([v, v, v, a], axis=-1)
    assert len(np.unique(pack(img))) > 256
    return np.ascontiguousarray(img)


# ---- sizes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 2, 3, 5, 67, 256, 1031])
def test_small_shapes(ctx, w):
    for h in (1, 2, 7):
        n = min(9, w * h)
        kind, pal, _ = check(ctx, image_of(w, h, colors(n, 10 * w + h), w + h))
        assert kind == FNX_PNG_PALETTED and len(pal) == n


@pytest.mark.parametrize("w,h", [(1031, 517), (1920, 1080)])
def test_many_workgroups_and_the_fold(ctx, w, h):
    kind, pal, _ = check(ctx, image_of(w, h, colors(256, 5), 6))
    assert kind == FNX_PNG_PALETTED and len(pal) == 256


# ---- strides ----------------------------------------------------------------------------------------------------------
def test_row_padding_is_not_counted(ctx):
    w, h, pad = 67, 33, 5
    buf = image_of(w + pad, h, colors(256, 1), 2)
    buf[:, :w] = image_of(w, h, colors(256, 3), 4)               # 256 colours inside, up to 256 others in the padding
    img = buf[:, :w]
    assert len(np.unique(pack(buf))) > 256
    kind, pal, _ = check(ctx, img)
    assert kind == FNX_PNG_PALETTED and len(pal) == 256
    check(ctx, torch_of(img_buf=buf)[:, :w], want=restate(img))


def test_row_padding_counts_for_isGrayscale(ctx):
    w, h, pad = 67, 33, 3
    buf = np.zeros((h, w + pad, 4), np.uint8)
    buf[:, :, :] = translucent_gray(w + pad, h, 7)
    img = buf[:, :w]
    assert check(ctx, img)[0] == FNX_PNG_GRAY
    buf[h // 2, w + 1, 1] ^= 1                                    # one non-grey pixel in the padding of a middle row
    assert restate(img)[0] == FNX_PNG_NRGBA
    assert check(ctx, img)[0] == FNX_PNG_NRGBA
    buf[h // 2, w + 1, 1] ^= 1
    buf[h - 1, w + 1, 1] ^= 1                                     # behind the last row's pixels: outside the Pix slice
    assert check(ctx, img)[0] == FNX_PNG_GRAY


def torch_of(img_buf):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(img_buf)).cuda()
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("w,h", [(5, 3), (67, 9), (256, 4), (1031, 3)])
def test_unaligned_source_view_and_wide_plane(ctx, w, h):
    buf = image_of(w + 2, h, colors(min(40, (w + 2) * h), w), h)
    img = buf[:, 1:1 + w]                                         # the first pixel is 4 bytes off a 16-byte boundary
    want = restate(img)
    for src in (img, torch_of(buf)[:, 1:1 + w]):
        plane = np.full((h, w + 7), 0xAB, np.uint8)               # pstride > w: what lies beyond w stays
        kind, _, got = check(ctx, src, want=want, plane=plane)
        assert kind == FNX_PNG_PALETTED and got is plane
        assert np.all(plane[:, w:] == 0xAB)
    import torch
    dplane = torch.full((h, w + 7), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    kind, pal, got = ctx.png_reduce(torch_of(buf)[:, 1:1 + w], plane=dplane)
    ctx.sync()
    got = got.cpu().numpy()
    assert np.array_equal(got[:, :w], want[2]) and np.all(got[:, w:] == 0xAB) and np.array_equal(pal, want[1])


# ---- the threshold ----------------------------------------------------------------------------------------------------
def test_exactly_256_colours(ctx):
    kind, pal, _ = check(ctx, image_of(67, 61, colors(256, 11), 12))
    assert kind == FNX_PNG_PALETTED and len(pal) == 256


@pytest.mark.parametrize("where", ["last", "first", "middle_of_last_row"])
@pytest.mark.parametrize("w,h", [(67, 61), (1031, 517)])
def test_257th_colour_in_one_pixel(ctx, w, h, where):
    pal = colors(257, 13)
    img = image_of(w, h, pal[:256], 14)
    y, x = {"last": (h - 1, w - 1), "first": (0, 0), "middle_of_last_row": (h - 1, w // 2)}[where]
    if where == "first":                                          # the colour that sat there must still occur
        img[1, 1] = img[0, 0]
    else:
        img[0, 0] = img[y, x]
    img[y, x] = pal[256]
    assert len(np.unique(pack(img))) == 257
    assert check(ctx, img)[0] == FNX_PNG_NRGBA
    img[y, x] = img[h // 2, w // 3]
    assert check(ctx, img)[0] == FNX_PNG_PALETTED


@pytest.mark.parametrize("max_colors", [1, 2, 16])
def test_max_colors_below_256(ctx, max_colors):
    for w, h in ((67, 9), (1031, 40)):
        kind, pal, _ = check(ctx, image_of(w, h, colors(max_colors, max_colors), 3), max_colors)
        assert kind == FNX_PNG_PALETTED and len(pal) == max_colors
        assert check(ctx, image_of(w, h, colors(max_colors + 1, max_colors), 3), max_colors)[0] == FNX_PNG_NRGBA


# ---- keys -------------------------------------------------------------------------------------------------------------
def test_alpha_is_part_of_the_key(ctx):
    pal = np.tile(np.array([[10, 20, 30, 0]], np.uint8), (200, 1))
    pal[:, 3] = np.arange(200)
    kind, got, _ = check(ctx, image_of(67, 31, pal, 1))
    assert kind == FNX_PNG_PALETTED and len(got) == 200
    assert check(ctx, image_of(67, 31, pal[:3], 1), 2)[0] == FNX_PNG_NRGBA


def test_sentinel_colours(ctx):
    pal = np.array([[0, 0, 0, 0], [255, 255, 255, 255], [0, 0, 0, 255], [255, 255, 255, 0], [1, 0, 0, 0]], np.uint8)
    for n in (2, 5):
        kind, got, _ = check(ctx, image_of(67, 31, pal[:n], n))
        assert kind == FNX_PNG_PALETTED and len(got) == n
    assert check(ctx, np.zeros((5, 3, 4), np.uint8))[1].tolist() == [[0, 0, 0, 0]]
    assert check(ctx, np.full((5, 3, 4), 255, np.uint8))[1].tolist() == [[255, 255, 255, 255]]


@pytest.mark.parametrize("keys", ["byte0", "byte1", "byte2", "byte3", "multiples_of_2048", "multiples_of_2_to_24"])
def test_adversarial_keys(ctx, keys):
    k = np.arange(256, dtype=np.uint32)
    words = {"byte0": 0x11223300 | k, "byte1": 0x11220033 | (k << 8), "byte2": 0x11002233 | (k << 16), "byte3": 0x00112233 | (k << 24),
             "multiples_of_2048": k * 2048, "multiples_of_2_to_24": k << 24}[keys]
    pal = unpack(words)
    for w, h in ((67, 31), (1031, 64)):
        kind, got, _ = check(ctx, image_of(w, h, pal, 9))
        assert kind == FNX_PNG_PALETTED and len(got) == 256


# ---- first-occurrence order across workgroups -------------------------------------------------------------------------
ORDER_W, ORDER_H = 1031, 517


def test_order_random_everywhere(ctx):
    check(ctx, image_of(ORDER_W, ORDER_H, colors(256, 21), 22))


def test_order_blocks_in_descending_address_order(ctx):
    """colour k fills block 255 - k: the colours' first pixels descend as the colour number (and any hash of it) ascends"""
    n = ORDER_W * ORDER_H
    pal = colors(256, 23)
    pal = pal[np.argsort(pack(pal))]                                # colour numbers ascending with the packed value
    idx = 255 - (np.arange(n) * 256 // n)
    img = np.ascontiguousarray(pal[idx].reshape(ORDER_H, ORDER_W, 4))
    _, got, _ = check(ctx, img)
    assert np.array_equal(got, pal[::-1])


def test_order_colour_k_first_at_pixel_k_times_2089(ctx):
    n = ORDER_W * ORDER_H
    assert 255 * 2089 < n
    pal = colors(256, 24)
    rng = np.random.default_rng(25)
    idx = np.zeros(n, np.int64)
    for k in range(1, 256):
        lo, hi = k * 2089, (k + 1) * 2089 if k < 255 else n
        idx[lo:hi] = rng.integers(0, k + 1, size=hi - lo)           # only colours that have appeared
        idx[lo] = k
    img = np.ascontiguousarray(pal[idx].reshape(ORDER_H, ORDER_W, 4))
    _, got, _ = check(ctx, img)
    assert np.array_equal(got, pal)


# ---- gray -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(67, 33), (1031, 517)])
def test_translucent_gray(ctx, w, h):
    img = translucent_gray(w, h, 3)
    kind, pal, plane = check(ctx, img)
    assert kind == FNX_PNG_GRAY and len(pal) == 0 and np.array_equal(plane, img[..., 0])
    img[h - 1, w - 1, 1] += 1                                       # G + 1 in the very last pixel
    keep = np.full((h, w), 0x5A, np.uint8)
    kind, pal, plane = ctx.png_reduce(img, plane=keep)
    assert kind == FNX_PNG_NRGBA and plane is None and len(pal) == 0 and np.all(keep == 0x5A)


def test_opaque_gray_ramp_is_paletted(ctx):
    v = (np.arange(300 * 40) % 256).astype(np.uint8).reshape(40, 300)
    img = np.ascontiguousarray(np.stack([v, v, v, np.full_like(v, 255)], axis=-1))
    kind, pal, _ = check(ctx, img)
    assert kind == FNX_PNG_PALETTED and len(pal) == 256


# ---- early exit, classify only, spaces ----------------------------------------------------------------------------------
def test_photograph_leaves_early(ctx):
    rng = np.random.default_rng(31)
    img = rng.integers(0, 256, size=(1080, 1920, 4), dtype=np.uint8)
    img[..., 3] = 255
    keep = np.full((1080, 1920), 7, np.uint8)
    kind, pal, plane = ctx.png_reduce(img, plane=keep)
    assert kind == FNX_PNG_NRGBA and plane is None and len(pal) == 0 and np.all(keep == 7)
    assert ctx.last_kernel() == "png_colors_kernel"


def test_classify_only(ctx):
    for img in (image_of(67, 31, colors(100, 41), 42), translucent_gray(67, 31, 43), image_of(67, 31, colors(300, 44), 45)):
        kind, pal, _ = ctx.png_reduce(img)
        k2, p2, none = ctx.png_reduce(img, want_plane=False)
        assert none is None and k2 == kind and np.array_equal(p2, pal)


@pytest.mark.parametrize("make", [lambda: image_of(1031, 64, colors(256, 51), 52), lambda: translucent_gray(257, 33, 53),
                                  lambda: image_of(257, 33, colors(300, 54), 55)], ids=["paletted", "gray", "nrgba"])
def test_spaces_agree_and_calls_repeat(ctx, make):
    img = make()
    h, w = img.shape[:2]
    want = restate(img)
    answers = []
    for _ in range(2):
        answers.append(check(ctx, img, want=want))
        k, p, pl = check(ctx, torch_of(img), want=want)
        answers.append((k, p, None if pl is None else host(pl)))
        answers.append(check(ctx, torch_of(img), want=want, plane=np.zeros((h, w), np.uint8)))     # device source, host plane
    for k, p, pl in answers[1:]:
        assert k == answers[0][0] and p.tobytes() == answers[0][1].tobytes()
        assert (pl is None) == (answers[0][2] is None) and (pl is None or pl.tobytes() == answers[0][2].tobytes())
    got = ctx.tryPalettize(img)
    assert (got is None) == (want[0] != FNX_PNG_PALETTED)
    if got is not None:
        assert np.array_equal(got[0], want[1]) and np.array_equal(got[1], want[2])


# ---- the file route ---------------------------------------------------------------------------------------------------
def _jpeg(arr, mode, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr, mode).save(buf, "JPEG", **kw)
    return buf.getvalue()


def gray_jpeg():
    v = (np.arange(320) // 8 * 6 + 10).astype(np.uint8)            # 40 levels, one per 8-px column of blocks
    return _jpeg(np.ascontiguousarray(np.tile(v, (240, 1))), "L", quality=95)


def two_colour_jpeg():
    cell = (np.add.outer(np.arange(240) // 16, np.arange(320) // 16) % 2).astype(np.uint8)
    rgb = np.where(cell[..., None] == 1, np.array([200, 40, 40], np.uint8), np.array([20, 60, 180], np.uint8)).astype(np.uint8)
    return _jpeg(np.ascontiguousarray(rgb), "RGB", quality=95, subsampling=0)


@pytest.fixture(scope="module")
def files():
    return {"gray": gray_jpeg(), "two_colour": two_colour_jpeg()}


@pytest.mark.parametrize("name", ["gray", "two_colour"])
def test_file_route_closes_the_hole(ctx, orc, files, name):
    data = files[name]
    assert ctx.compress_file_jpeg(data, 0.94, auto_format=True)[0] is None      # analyzeFormat: PNG -- the image was thrown away
    dec = orc.jpeg_decode(data)
    for orient, max_w, max_h in ((1, 0, 0), (6, 0, 0), (3, 160, 0)):
        img = dec if orient == 1 else orc.apply_orientation(dec, orient)
        orig = (img.shape[1], img.shape[0])
        img = orc.smart_resize(img, max_w, max_h) if (max_w or max_h) else img
        wkind, wpal, wplane = restate(np.ascontiguousarray(img))
        kind, pal, out, d0, d1 = ctx.compress_file_png_reduce(data, orient, max_w, max_h)
        assert (d0, d1) == (orig, (img.shape[1], img.shape[0]))
        assert kind == wkind and np.array_equal(pal, wpal)
        assert np.array_equal(out, img if wplane is None else wplane)
    assert restate(dec)[0] == FNX_PNG_PALETTED


def test_file_route_photograph_and_short_cap(ctx, orc):
    data = orc.jpeg_encode(synth.large_photo(320, 240, 4), 90)
    dec = orc.jpeg_decode(data)
    kind, pal, out, d0, d1 = ctx.compress_file_png_reduce(data)
    assert kind == FNX_PNG_NRGBA and len(pal) == 0 and d0 == d1 == (320, 240)
    assert out.shape == dec.shape and np.array_equal(out, dec)
    # one byte short: FNX_ERR_INVALID, and everything the caller needs to call again is set
    lib = fennec_amd.load_library()
    src = np.frombuffer(data, np.uint8)
    o = fennec_amd.FileOptions(1, 0, 0, 0, 0.0)
    k, nc, n = C.c_int(0), C.c_int(-1), C.c_size_t(0)
    palbuf = np.zeros((256, 4), np.uint8)
    dims = (C.c_int * 4)()
    cap = 320 * 240 * 4 - 1
    buf = np.zeros(cap, np.uint8)
    rc = lib.fennec_CompressFilePNGReduce(ctx._h, src.ctypes.data, len(data), C.byref(o), C.byref(k), palbuf.ctypes.data, C.byref(nc),
                                          buf.ctypes.data, cap, C.byref(n), dims)
    assert rc == fennec_amd.FNX_ERR_INVALID
    assert n.value == cap + 1 and k.value == FNX_PNG_NRGBA and nc.value == 0 and list(dims) == [320, 240, 320, 240]
    gray = gray_jpeg()
    cap = 320 * 240 - 1
    rc = lib.fennec_CompressFilePNGReduce(ctx._h, np.frombuffer(gray, np.uint8).ctypes.data, len(gray), C.byref(o), C.byref(k),
                                          palbuf.ctypes.data, C.byref(nc), buf.ctypes.data, cap, C.byref(n), dims)
    assert rc == fennec_amd.FNX_ERR_INVALID
    assert n.value == cap + 1 and k.value == FNX_PNG_PALETTED and 1 <= nc.value <= 256 and list(dims) == [320, 240, 320, 240]
