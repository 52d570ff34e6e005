"""fnx_png_compress_batch and fnx_png_recompress_batch on the GPU.  Every file is compared with the single route
(Context.compress_png(device_deflate=True): fnx_png_reduce + fnx_png_encode) BYTE FOR BYTE, and decoded by another reader
(Pillow through png_filter_ref.decode_png; png_decode_ref.decode for the recompressed sources) back to the source's pixels, so
that two equal wrong files do not pass.  The batches are the ones the batched kernels can break at: every kind and row form
in one chunk, streams that end with a deflate chunk or one row into the next among one-chunk streams, strided views whose
padding would change the decision if it were looked at the wrong way, more images than a chunk, refused items between good
ones.  Every image is small; the single route's files are made once."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
import png_decode_ref as ref
import png_filter_ref as pf
from fennec_amd import (FNX_ERR_INVALID, FNX_ERR_UNSUPPORTED, FNX_OK, FNX_PNG_COMPRESS_CHUNK, FNX_PNG_GRAY, FNX_PNG_NRGBA,
                        FNX_PNG_PALETTED)

pytestmark = pytest.mark.gpu

BATCH_KERNELS = ("png_colors_batch_kernel, png_finish_batch_kernel, png_flags_batch_kernel, png_plane_batch_kernel, "
                 "png_filter_batch_kernel, png_pack_batch_kernel, deflate_chunk_batch_kernel, deflate_gather_batch_kernel")
SENTINEL = 0xAB


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- images by what compressPNG makes of them --------------------------------------------------------------------------------
def few_colours(w, h, n, seed, alpha=False):
    """n distinct colours (non-grey), every one present when w h >= n, in an order that is not the order of first occurrence"""
    rng = np.random.default_rng(seed)
    pal = np.zeros((n, 4), np.uint8)
    pal[:, 0] = np.arange(n) & 255
    pal[:, 1] = (np.arange(n) * 7 + 3) & 255
    pal[:, 2] = 200 - (np.arange(n) >> 8) * 100
    pal[:, 3] = rng.integers(0, 256, n) if alpha else 255
    idx = rng.integers(0, n, w * h)
    idx[:min(n, w * h)] = rng.permutation(n)[:min(n, w * h)]
    return pal[rng.permutation(idx)].reshape(h, w, 4)


def noise(w, h, seed, opaque=True):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    if opaque:
        img[..., 3] = 255
    return img


def smooth(w, h, seed, opaque=True):
    return pf.smooth_rgba(w, h, seed, opaque)


def translucent_grey(w, h, seed):
    """r == g == b, more than 256 (v, a) pairs: not paletted, grey -> toGray's plane (the alpha is dropped, convert.go:96)"""
    rng = np.random.default_rng(seed)
    img = np.empty((h, w, 4), np.uint8)
    img[..., 0] = img[..., 1] = img[..., 2] = rng.integers(0, 256, (h, w))
    img[..., 3] = rng.integers(0, 256, (h, w))
    assert len(np.unique(img.reshape(-1, 4), axis=0)) > 256
    return img


def expected_pixels(img, kind):
    if kind != FNX_PNG_GRAY:
        return img
    out = img.copy()
    out[..., 1] = out[..., 2] = img[..., 0]
    out[..., 3] = 255
    return out


def check_files(ctx, imgs, files, kinds, want_kinds=None):
    """imgs: numpy images or device views; every file against the single route and against Pillow's decode"""
    for i, img in enumerate(imgs):
        host = img if isinstance(img, np.ndarray) else img.cpu().numpy()
        single = ctx.compress_png(img if not isinstance(img, np.ndarray) else dev(img), device_deflate=True)
        assert files[i] == single, f"image {i} ({host.shape[1]} x {host.shape[0]}): {len(files[i])} bytes, the single route {len(single)}"
        assert np.array_equal(pf.decode_png(files[i]), expected_pixels(host, kinds[i])), i
        if want_kinds is not None:
            assert kinds[i] == want_kinds[i], (i, kinds[i])


# ---- 1: every kind side by side in one chunk -----------------------------------------------------------------------------------
def kinds_set():
    exactly_256 = few_colours(260, 130, 256, 11)
    just_over = few_colours(260, 130, 257, 12)
    assert len(np.unique(exactly_256.reshape(-1, 4), axis=0)) == 256 and len(np.unique(just_over.reshape(-1, 4), axis=0)) == 257
    P, G, N = FNX_PNG_PALETTED, FNX_PNG_GRAY, FNX_PNG_NRGBA
    return [
        (few_colours(1, 1, 1, 1), P), (few_colours(5, 3, 2, 2), P), (few_colours(5, 3, 4, 3, alpha=True), P), (few_colours(67, 7, 16, 4), P),
        (few_colours(260, 130, 200, 5, alpha=True), P), (exactly_256, P), (just_over, N),
        (noise(67, 7, 6), N), (noise(67, 7, 7, opaque=False), N), (smooth(260, 130, 8), N), (smooth(1031, 37, 9, opaque=False), N),
        (translucent_grey(260, 130, 10), G), (translucent_grey(1031, 37, 13), G), (few_colours(1031, 37, 3, 14), P), (few_colours(67, 7, 17, 15), P),
    ]


def test_every_kind_side_by_side(ctx):
    imgs = [a for a, _ in kinds_set()]
    files, kinds = ctx.png_compress_batch([dev(a) for a in imgs])
    assert ctx.last_kernel() == BATCH_KERNELS
    check_files(ctx, imgs, files, kinds, [k for _, k in kinds_set()])
    depths = [f[24] for f, k in zip(files, kinds) if k == FNX_PNG_PALETTED]
    assert sorted(set(depths)) == [1, 2, 4, 8]                              # every pack kernel ran
    assert sorted({f[25] for f in files}) == [0, 2, 3, 6]                   # IHDR colour types: gray, RGB, paletted, RGBA


# ---- 2: deflate chunk edges ----------------------------------------------------------------------------------------------------
def test_streams_that_end_at_and_behind_a_deflate_chunk(ctx):
    imgs = [few_colours(5, 3, 4, 20), translucent_grey(127, 256, 21), noise(9, 5, 22), translucent_grey(127, 257, 23), smooth(1031, 37, 24),
            few_colours(9, 5, 2, 25), translucent_grey(127, 255, 26)]
    files, kinds = ctx.png_compress_batch([dev(a) for a in imgs])
    assert kinds[1] == kinds[3] == kinds[6] == FNX_PNG_GRAY and kinds[4] == FNX_PNG_NRGBA
    # 128 x 256 = 32768 bytes: one chunk; 257 rows: a second chunk of 128 bytes; 37 x 3094 = 114478: four chunks
    for i, blocks in ((1, 1), (3, 2), (4, 4), (6, 1)):
        z = dict(pf.chunks(files[i]))[b"IDAT"]
        assert len(fennec_amd.inflate(z)) == imgs[i].shape[0] * (1 + imgs[i].shape[1] * (3 if i == 4 else 1))
        import inflate_probe
        assert len(inflate_probe.probe(z).blocks) == 2 * blocks - 1, i      # every chunk but the last is closed by an empty stored block
    check_files(ctx, imgs, files, kinds)


# ---- 3: strided and offset views -----------------------------------------------------------------------------------------------
def test_padding_is_looked_at_as_the_single_route_does(ctx):
    rng = np.random.default_rng(30)
    views, hosts, want = [], [], []

    def view_of(img, pad_left, pad_right, fill):
        h, w = img.shape[:2]
        base = np.empty((h + 1, pad_left + w + pad_right, 4), np.uint8)
        base[...] = fill(base.shape)
        base[1:, pad_left:pad_left + w] = img
        t = dev(base)
        views.append(t[1:, pad_left:pad_left + w])
        hosts.append(img)

    colour = lambda shape: rng.integers(0, 256, shape, dtype=np.uint8)          # non-grey, translucent
    # grey pixels, colour in the padding: the flat walk meets it -> NOT gray (RGBA rows: the visible alphas differ)
    view_of(translucent_grey(61, 9, 31), 3, 2, colour)
    want.append(FNX_PNG_NRGBA)
    # the same with grey, translucent padding: gray
    view_of(translucent_grey(61, 9, 32), 3, 2, lambda shape: np.repeat(rng.integers(0, 256, shape[:2] + (1,), dtype=np.uint8), 4, axis=2))
    want.append(FNX_PNG_GRAY)
    # opaque photograph, translucent padding: Opaque() looks at visible pixels only -> RGB rows
    view_of(noise(33, 11, 33), 1, 6, colour)
    want.append(FNX_PNG_NRGBA)
    # few colours, many more in the padding: the colour set is the visible pixels'
    view_of(few_colours(35, 6, 5, 34), 2, 1, colour)
    want.append(FNX_PNG_PALETTED)
    # odd row lengths one after another: the zlib streams start at every alignment of the area they come down in
    for k, w in enumerate((7, 9, 10, 11, 13)):
        view_of(translucent_grey(w + 20, 16, 40 + k), k, 3 - k % 3, colour if k == 4 else lambda shape: np.full(shape, 77, np.uint8))
        want.append(FNX_PNG_NRGBA if k == 4 else FNX_PNG_GRAY)
    files, kinds = ctx.png_compress_batch(views)
    assert kinds == want
    assert files[0][25] == 6 and files[2][25] == 2                          # RGBA rows; RGB rows
    for i, v in enumerate(views):
        assert v.stride(0) > 4 * v.shape[1] and np.array_equal(v.cpu().numpy(), hosts[i])
    check_files(ctx, views, files, kinds)
    # the zlib streams come down back to back at their true sizes: five gray images of 6 rows of 61 noise bytes -- 366 bytes that
    # deflate can only store, 377 with the block's and the stream's framing -- start at every alignment of that area
    views, hosts = [], []
    for k in range(5):
        view_of(translucent_grey(60, 6, 80 + k), 1 + k, 2, lambda shape: np.full(shape, 99, np.uint8))
    files, kinds = ctx.png_compress_batch(views)
    assert kinds == [FNX_PNG_GRAY] * 5
    zsizes = [len(dict(pf.chunks(f))[b"IDAT"]) for f in files]
    assert {sum(zsizes[:k]) % 4 for k in range(5)} == {0, 1, 2, 3}, zsizes
    check_files(ctx, views, files, kinds)


# ---- 4: more images than a chunk; order does not show ----------------------------------------------------------------------------
def test_more_images_than_a_chunk(ctx):
    n = 2 * FNX_PNG_COMPRESS_CHUNK + 6
    assert n == 70
    imgs = [noise(9, 5, 100 + i, opaque=i % 3 != 0) if i % 2 else few_colours(9, 5, 2 + i % 40, 100 + i) for i in range(n)]
    devs = [dev(a) for a in imgs]
    files, kinds = ctx.png_compress_batch(devs)
    assert len(set(files)) == n
    check_files(ctx, imgs, files, kinds)
    back, kinds_back = ctx.png_compress_batch(devs[::-1])
    assert back == files[::-1] and kinds_back == kinds[::-1]
    for i in (0, 33, 69):
        assert ctx.png_compress_batch([devs[i]]) == ([files[i]], [kinds[i]])


# ---- 5: refusals stay items ----------------------------------------------------------------------------------------------------
def raw_batch(ctx, ptrs, strides, ws, hs, caps, outs=None):
    n = len(ptrs)
    bufs = [np.full(max(c, 1), SENTINEL, np.uint8) for c in caps]
    po = (C.c_void_p * n)(*[b.ctypes.data for b in bufs]) if outs is None else (C.c_void_p * n)(*outs)
    nb, kinds, status = (C.c_size_t * n)(*[99] * n), (C.c_int * n)(*[-7] * n), (C.c_int * n)(*[77] * n)
    rc = ctx._lib.fnx_png_compress_batch(ctx._h, n, (C.c_void_p * n)(*ptrs), (C.c_int * n)(*strides), (C.c_int * n)(*ws), (C.c_int * n)(*hs), po,
                                         (C.c_size_t * n)(*caps), nb, kinds, status)
    return rc, list(nb), list(kinds), list(status), bufs


def test_a_cap_too_small_in_the_middle(ctx):
    imgs = [few_colours(9, 5, 3, 50), smooth(40, 30, 51), translucent_grey(40, 30, 52)]
    devs = [dev(a) for a in imgs]
    ctx.sync()
    want, want_kinds = ctx.png_compress_batch(devs)
    caps = [fennec_amd.png_file_bound(a.shape[1], a.shape[0]) for a in imgs]
    caps[1] = len(want[1]) - 1
    rc, nb, kinds, status, bufs = raw_batch(ctx, [t.data_ptr() for t in devs], [t.stride(0) for t in devs], [9, 40, 40], [5, 30, 30], caps)
    assert rc == FNX_OK and status == [FNX_OK, FNX_ERR_INVALID, FNX_OK]
    assert nb == [len(f) for f in want] and kinds == want_kinds
    assert b"image 1" in ctx._lib.fnx_last_error() and b"cap" in ctx._lib.fnx_last_error()
    assert (bufs[1] == SENTINEL).all()
    for i in (0, 2):
        assert bufs[i][:nb[i]].tobytes() == want[i] and (bufs[i][nb[i]:] == SENTINEL).all()
    # exactly enough is enough; a size query (no buffer, cap 0) answers the same way
    caps[1] += 1
    rc, nb, kinds, status, bufs = raw_batch(ctx, [t.data_ptr() for t in devs], [t.stride(0) for t in devs], [9, 40, 40], [5, 30, 30], caps)
    assert status == [FNX_OK] * 3 and bufs[1].tobytes() == want[1]
    rc, nb, kinds, status, _ = raw_batch(ctx, [t.data_ptr() for t in devs], [t.stride(0) for t in devs], [9, 40, 40], [5, 30, 30], [0, 0, 0], outs=[None] * 3)
    assert rc == FNX_OK and status == [FNX_ERR_INVALID] * 3 and nb == [len(f) for f in want] and kinds == want_kinds


def test_argument_refusals_stay_items(ctx):
    good = smooth(12, 10, 60)
    t = dev(good)
    ctx.sync()
    want = ctx.compress_png(t, device_deflate=True)
    p, cap = t.data_ptr(), fennec_amd.png_file_bound(12, 10)
    #          pointer  stride  w      h      why
    items = [(p,       48,     12,    10,    None),
             (None,    48,     12,    10,    b"NULL"),
             (p,       48,     0,     10,    b"dims"),
             (p,       48,     12,    65536, b"dims"),
             (p,       44,     12,    10,    b"stride"),
             (p,       50,     12,    10,    b"stride"),
             (p + 2,   48,     11,    9,     b"aligned"),
             (p,       48,     12,    10,    None)]
    rc, nb, kinds, status, bufs = raw_batch(ctx, [i[0] for i in items], [i[1] for i in items], [i[2] for i in items], [i[3] for i in items], [cap] * len(items))
    assert rc == FNX_OK
    for k, it in enumerate(items):
        if it[4] is None:
            assert status[k] == FNX_OK and bufs[k][:nb[k]].tobytes() == want and kinds[k] == FNX_PNG_PALETTED   # 120 pixels: at most 120 colours
        else:
            assert (status[k], nb[k], kinds[k]) == (FNX_ERR_INVALID, 0, 0) and (bufs[k] == SENTINEL).all(), k
    assert b"srcs[1]" in ctx._lib.fnx_last_error()                            # the lowest-indexed refused item's message
    # a missing buffer with a cap that is not 0
    rc, nb, kinds, status, bufs = raw_batch(ctx, [p, p], [48, 48], [12, 12], [10, 10], [cap, cap], outs=[None, None])
    assert rc == FNX_OK and status == [FNX_ERR_INVALID] * 2 and nb == [0, 0] and b"outs[0]" in ctx._lib.fnx_last_error()


# ---- 6: files in, files out ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sources():
    """(file, how it decodes: 'png', 'jpeg', the status that refuses it, or 'refused' where the JPEG decoder picks the status)"""
    import jpeg_mini
    out = []
    for k, (ct, depth, w, h) in enumerate([(0, 8, 31, 9), (2, 8, 40, 33), (3, 4, 17, 21), (4, 8, 64, 5), (6, 8, 33, 40), (6, 16, 9, 9), (3, 8, 120, 90), (0, 1, 70, 3)]):
        s = ref.random_samples(w, h, ct, depth, 200 + k)
        pal = ref.random_palette(min(256, 1 << depth), k) if ct == 3 else None
        trns = bytes([0, 128, 255, 7]) if ct == 3 and depth == 4 else None
        out.append((ref.write_png(s, ct, depth, filters=np.random.default_rng(k).integers(0, 5, size=h).tolist(), palette=pal, trns=trns), "png"))
    good = out[1][0]
    photo = pf.smooth_rgba(64, 16, 3)
    out.insert(2, (jpeg_mini.encode(photo, 2, 2, 88, 0), "jpeg"))
    out.insert(4, (good[:len(good) // 2], FNX_ERR_INVALID))
    out.insert(6, (ref.write_png(ref.random_samples(9, 5, 2, 8, 1), 2, 8, interlace=1), FNX_ERR_UNSUPPORTED))
    out.append((b"neither a PNG nor a JPEG file", "refused"))
    return out


def test_recompress_batch(ctx, sources):
    files = [f for f, _ in sources]
    results = [ctx.png_recompress_batch(files, workers=w) for w in (1, 3, 8, 0)]
    assert ctx.last_kernel() == BATCH_KERNELS
    for r in results[1:]:
        assert r == results[0]
    out, kinds, statuses = results[0]
    for i, (f, how) in enumerate(sources):
        if how not in ("png", "jpeg"):
            assert (statuses[i] == how or (how == "refused" and statuses[i] < 0)) and out[i] is None, i
            continue
        assert statuses[i] == FNX_OK, i
        img = ctx.png_decode(f) if how == "png" else ctx.jpeg_decode(f, device=True)
        assert out[i] == ctx.compress_png(img, device_deflate=True), i
        host = img.cpu().numpy()
        if how == "png":
            assert np.array_equal(host, ref.decode(f))
        assert np.array_equal(pf.decode_png(out[i]), expected_pixels(host, kinds[i])), i
        assert np.array_equal(ref.decode(out[i]), expected_pixels(host, kinds[i])) or kinds[i] == FNX_PNG_PALETTED, i


def test_recompress_reports_dimensions_and_sizes(ctx, sources):
    files = [f for f, _ in sources]
    n = len(files)
    bufs = [np.frombuffer(f, np.uint8) for f in files]
    outs = [np.full(1 << 16, SENTINEL, np.uint8) for _ in files]
    nb, kinds, ws, hs, status = (C.c_size_t * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    rc = ctx._lib.fnx_png_recompress_batch(ctx._h, n, (C.c_void_p * n)(*[b.ctypes.data for b in bufs]), (C.c_size_t * n)(*[len(f) for f in files]), 2,
                                           (C.c_void_p * n)(*[o.ctypes.data for o in outs]), (C.c_size_t * n)(*[1 << 16] * n), nb, kinds, ws, hs, status)
    assert rc == FNX_OK
    for i, (f, how) in enumerate(sources):
        if how == "png" or how == FNX_ERR_UNSUPPORTED:
            assert (ws[i], hs[i]) == fennec_amd.png_info(f)[:2], i
        if how in ("png", "jpeg"):
            assert status[i] == FNX_OK and nb[i] > 57 and (outs[i][nb[i]:] == SENTINEL).all()
        else:
            assert (status[i] == how or (how == "refused" and status[i] < 0)) and nb[i] == 0 and (outs[i] == SENTINEL).all(), i


# ---- 7: which kernels ran ------------------------------------------------------------------------------------------------------
def test_last_kernel(ctx):
    t = dev(smooth(40, 30, 70))
    ctx.sync()
    ctx.png_compress_batch([t])
    assert ctx.last_kernel() == BATCH_KERNELS
    ctx.png_encode(t)
    assert ctx.last_kernel() == "deflate_chunk_kernel"
    rc, _, _, status, _ = raw_batch(ctx, [None, t.data_ptr()], [160, 158], [40, 40], [30, 30], [1 << 16] * 2)      # refused items only
    assert rc == FNX_OK and status == [FNX_ERR_INVALID] * 2
    assert ctx.last_kernel() == "deflate_chunk_kernel"
    ctx.compress_png(t, device_deflate=True)
    assert ctx.last_kernel() == "deflate_chunk_kernel"
    ctx.png_compress_batch([t, t])
    assert ctx.last_kernel() == BATCH_KERNELS
