"""fnx_png_decode_batch on the GPU: every image ==, against tests/png_decode_ref.py (ref.decode) AND against the single call
(Context.png_decode) on the same file.  The batches are the ones the batched kernels can break at: several bpp groups and
descriptor rows in one chunk, chains of every shape side by side, files of one bpp with different geometry, refused items
between good ones, more files than a chunk, strided destinations.  Every file is small; the references are computed once."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest

import fennec_amd
import png_decode_ref as ref
from fennec_amd import FNX_ERR_INVALID, FNX_ERR_UNSUPPORTED, FNX_OK, FNX_PNG_DECODE_CHUNK
from fennec_amd import FNX_PNG_DECODE_ROWS as R

pytestmark = pytest.mark.gpu

BATCH_KERNELS = "png_unfilter_batch_kernel, png_expand_batch_kernel"
SINGLE_KERNELS = "png_unfilter_kernel, png_expand_kernel"
SENTINEL = 0xAB
DST_BYTES = 8192                 # test_refusals_stay_items: every item's destination; its largest image is 21 x 66
FNX_BATCH_MAX = 65535            # include/fennec_hip.h


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def random_plan(h, seed):
    return np.random.default_rng(seed).integers(0, 5, size=h).tolist()


def every_pair_files():
    """all 15 colour type / depth pairs: widths 1..37 and heights 1..70, different per file, random filter plans; paletted
    files with tRNS and a palette shorter than the largest index, types 0 and 2 with a tRNS key that occurs in the image"""
    files = []
    widths = [1, 2, 3, 5, 7, 8, 9, 13, 16, 17, 21, 31, 32, 33, 37]
    heights = [70, 1, 65, 2, 64, 33, 63, 17, 66, 5, 69, 9, 3, 47, 68]
    for k, (ct, depth) in enumerate(ref.PAIRS):
        w, h = widths[k], heights[k]
        s = ref.random_samples(w, h, ct, depth, 100 + k)
        pal = trns = None
        if ct == 3:
            top = 1 << depth
            npal = max(1, top - 1 - top // 4)
            pal = ref.random_palette(npal, k)
            trns = bytes(([0, 255, 128, 1, 254, 77] * 43)[:max(1, npal - 1)])
        elif ct in (0, 2):
            key = [int(v) for v in s[h // 2, w // 2]]
            s[::2, ::3] = key
            trns = b"".join(bytes([v >> 8, v & 255]) for v in key)
        files.append(ref.write_png(s, ct, depth, filters=random_plan(h, k), palette=pal, trns=trns, idat_sizes=[1, 7, 100] if k % 3 == 0 else None))
    return files


def chain_files():
    files = []
    s = ref.random_samples(5, R + 1, 2, 8, 1)                                   # one chain of R + 1 rows: the band march reads
    files.append(ref.write_png(s, 2, 8, filters=[4] * (R + 1)))                 # the last row of the first band back
    s = ref.random_samples(11, 200, 2, 8, 2)                                    # all Sub: 200 segments sharing units
    files.append(ref.write_png(s, 2, 8, filters=[1] * 200))
    for seg in (1, 2, 64, 65):                                                  # None / Sub every `seg` rows, Average and Paeth inside
        h = 2 * 65 + 7
        s = ref.random_samples(9, h, 6, 8, 10 + seg)
        files.append(ref.write_png(s, 6, 8, filters=[(y // seg) % 2 if y % seg == 0 else 3 + (y & 1) for y in range(h)]))
    s = ref.random_samples(1, 130, 6, 8, 3)
    files.append(ref.write_png(s, 6, 8, filters=random_plan(130, 3)))            # w = 1
    s = ref.random_samples(300, 1, 2, 8, 4)
    files.append(ref.write_png(s, 2, 8, filters=[4]))                            # h = 1, more than one tile of the expand kernel
    return files


def same_bpp_files():
    return [ref.write_png(ref.random_samples(w, 70, 2, 8, 20 + w), 2, 8, filters=random_plan(70, w)) for w in (3, 16, 67)]


@pytest.fixture(scope="module")
def pairs():
    files = every_pair_files()
    return files, [ref.decode(f) for f in files]


def check_against_both(ctx, files, want, images, statuses):
    assert statuses == [FNX_OK] * len(files)
    for i, f in enumerate(files):
        assert images[i].shape == want[i].shape and np.array_equal(images[i], want[i]), i
        assert np.array_equal(ctx.png_decode(f, "host"), want[i]), i


def raw_batch(ctx, files, dsts, strides, workers=0, n=None, null_status=False):
    """fnx_png_decode_batch through ctypes: dsts are device tensors (flat uint8) or None"""
    m = len(files)
    bufs = [np.frombuffer(f, np.uint8) if len(f) else np.zeros(1, np.uint8) for f in files]
    pf = (C.c_void_p * m)(*[b.ctypes.data for b in bufs])
    ps = (C.c_size_t * m)(*[len(f) for f in files])
    pd = (C.c_void_p * m)(*[None if t is None else t.data_ptr() for t in dsts])
    pst = (C.c_int * m)(*strides)
    ws, hs, status = (C.c_int * m)(*[-7] * m), (C.c_int * m)(*[-7] * m), (C.c_int * m)(*[77] * m)
    with ctx._ordered(*[t for t in dsts if t is not None]):
        rc = ctx._lib.fnx_png_decode_batch(ctx._h, m if n is None else n, pf, ps, pd, pst, workers, ws, hs, None if null_status else status)
    return rc, list(ws), list(hs), list(status)


def single_status(ctx, data, dst, stride):
    buf = np.frombuffer(data, np.uint8) if len(data) else np.zeros(1, np.uint8)
    w, h = C.c_int(), C.c_int()
    with ctx._ordered(dst):
        rc = ctx._lib.fnx_png_decode(ctx._h, buf.ctypes.data, len(data), fennec_amd.FNX_DEVICE, dst.data_ptr(), stride, C.byref(w), C.byref(h))
    return rc, ctx._lib.fnx_last_error()


# ---- 1, 6: every pair in one batch; workers do not change a byte ----------------------------------------------------------
def test_every_pair_in_one_batch(ctx, pairs):
    files, want = pairs
    assert len(files) == 15 and len({ref.bpp_of(ct, d) for ct, d in ref.PAIRS}) == 6
    images, statuses = ctx.png_decode_batch(files)
    assert ctx.last_kernel() == BATCH_KERNELS
    check_against_both(ctx, files, want, images, statuses)


def test_workers_do_not_change_a_byte(ctx, pairs):
    files, want = pairs
    for workers in (1, 2, 8):
        for _ in range(2):                               # twice in a row on one ctx: staging and scratch reused
            images, statuses = ctx.png_decode_batch(files, workers=workers)
            assert statuses == [FNX_OK] * len(files)
            for i in range(len(files)):
                assert np.array_equal(images[i], want[i]), (workers, i)


def test_device_images_are_tensors(ctx, pairs):
    import torch
    files, want = pairs
    images, statuses = ctx.png_decode_batch(files[:4], device=True)
    for i in range(4):
        assert isinstance(images[i], torch.Tensor) and images[i].is_cuda and np.array_equal(images[i].cpu().numpy(), want[i])


# ---- 2, 3: chains of every shape; one bpp, different geometry ------------------------------------------------------------
def test_chains_of_every_shape_side_by_side(ctx):
    files = chain_files()
    assert ref.filter_types(files[0]) == [4] * (R + 1)
    images, statuses = ctx.png_decode_batch(files)
    check_against_both(ctx, files, [ref.decode(f) for f in files], images, statuses)


def test_same_bpp_different_geometry(ctx):
    files = same_bpp_files()
    images, statuses = ctx.png_decode_batch(files, workers=1)
    check_against_both(ctx, files, [ref.decode(f) for f in files], images, statuses)


# ---- 4: refusals stay items ------------------------------------------------------------------------------------------------
def test_refusals_stay_items(ctx):
    import torch
    s = ref.random_samples(9, 5, 2, 8, 1)
    good = ref.write_png(s, 2, 8, filters=[0, 1, 2, 3, 4])
    good2 = ref.write_png(ref.random_samples(21, 66, 3, 4, 2), 3, 4, filters=random_plan(66, 2), palette=ref.random_palette(16, 2))
    flipped = bytearray(good)
    flipped[len(good) - 20] ^= 0x40
    items = [
        ("good", good, FNX_OK),
        ("truncated", good[:-30], FNX_ERR_INVALID),
        ("bad CRC", bytes(flipped), FNX_ERR_INVALID),
        ("good paletted", good2, FNX_OK),
        ("filter type 5", ref.write_png(s, 2, 8, filters=[0, 1, 5, 3, 4]), FNX_ERR_INVALID),
        ("Adam7", ref.write_png(s, 2, 8, interlace=1), FNX_ERR_UNSUPPORTED),
        ("JPEG bytes", b"\xff\xd8\xff\xe0\x00\x10JFIF\x00" + bytes(range(200)), FNX_ERR_INVALID),
        ("zero length", b"", FNX_ERR_INVALID),
        ("not enough pixel data", ref.SIG + ref.ihdr(9, 5, 8, 2) + ref.chunk(b"IDAT", zlib.compress(b"\0" * 139)) + ref.chunk(b"IEND", b""),
         FNX_ERR_INVALID),
        ("too wide", ref.SIG + ref.ihdr(65536, 1, 1, 0) + ref.chunk(b"IDAT", zlib.compress(b"\0")) + ref.chunk(b"IEND", b""), FNX_ERR_UNSUPPORTED),
        ("NULL dst", good, FNX_ERR_INVALID),
        ("stride below 4w", good, FNX_ERR_INVALID),
        ("good again", good, FNX_OK),
    ]
    files = [it[1] for it in items]
    n = len(items)
    want_img = {0: ref.decode(good), 3: ref.decode(good2), n - 1: ref.decode(good)}
    assert all(img.size <= DST_BYTES for img in want_img.values())
    for workers in (1, 8):
        dsts = [torch.full((DST_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda:0") for _ in items]
        strides = []
        for name, data, _ in items:
            try:
                w = fennec_amd.png_info(data)[0]
            except fennec_amd.FennecError:
                w = 9
            strides.append(min(4 * w, 1 << 20))
        strides[n - 2] = 4 * 9 - 4
        dsts[n - 3] = None
        rc, ws, hs, status = raw_batch(ctx, files, dsts, strides, workers=workers)
        text = ctx._lib.fnx_last_error()
        assert rc == FNX_OK
        assert status == [it[2] for it in items], [it[0] for it in items]
        assert (ws[5], hs[5]) == (9, 5) and (ws[9], hs[9]) == (65536, 1)           # set whenever the IHDR parses
        assert (ws[1], hs[1]) == (9, 5) and (ws[6], hs[6]) == (0, 0) and (ws[7], hs[7]) == (0, 0)
        for i, (name, data, st) in enumerate(items):
            if dsts[i] is None:
                continue
            got = dsts[i].cpu().numpy()
            if st != FNX_OK:
                assert (got == SENTINEL).all(), name                              # a refused item leaves its destination untouched
                fresh = torch.full((DST_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda:0")
                src, _ = single_status(ctx, data, fresh, strides[i])
                assert src == st, name                                            # the single call's status
                assert (fresh.cpu().numpy() == SENTINEL).all()
            else:
                img = want_img[i]
                h, w = img.shape[:2]
                assert np.array_equal(got[:h * w * 4].reshape(h, w, 4), img), name
                assert (got[h * w * 4:] == SENTINEL).all()
        # the call's text is the lowest-indexed refused item's, whichever thread finished first
        _, single_text = single_status(ctx, files[1], torch.full((DST_BYTES,), SENTINEL, dtype=torch.uint8, device="cuda:0"), strides[1])
        assert text == single_text and b"invalid PNG" in text


# ---- 5: more files than a chunk -------------------------------------------------------------------------------------------
def test_more_files_than_a_chunk(ctx):
    n = FNX_PNG_DECODE_CHUNK + 3
    files, want = [], []
    for k in range(n):
        ct, depth = [(2, 8), (6, 8), (0, 8), (3, 8)][k % 4]
        s = ref.random_samples(8, 8, ct, depth, 300 + k)
        pal = ref.random_palette(256, k) if ct == 3 else None
        files.append(ref.write_png(s, ct, depth, filters=random_plan(8, k), palette=pal))
        want.append(ref.decode(files[-1]))
    assert len({w.tobytes() for w in want}) == n
    for workers in (0, 1):
        images, statuses = ctx.png_decode_batch(files, workers=workers)
        assert statuses == [FNX_OK] * n
        for i in range(n):
            assert np.array_equal(images[i], want[i]), i
    assert np.array_equal(ctx.png_decode(files[-1], "host"), want[-1])


# ---- 7: strided destinations ----------------------------------------------------------------------------------------------
def test_strided_destinations(ctx):
    import torch
    files = same_bpp_files() + [every_pair_files()[8]]
    want = [ref.decode(f) for f in files]
    dsts, strides = [], []
    for img in want:
        h, w = img.shape[:2]
        strides.append(4 * w + 12)
        dsts.append(torch.full((h * (4 * w + 12),), SENTINEL, dtype=torch.uint8, device="cuda:0"))
    rc, ws, hs, status = raw_batch(ctx, files, dsts, strides, workers=2)
    assert rc == FNX_OK and status == [FNX_OK] * len(files)
    for i, img in enumerate(want):
        h, w = img.shape[:2]
        assert (ws[i], hs[i]) == (w, h)
        got = dsts[i].cpu().numpy().reshape(h, 4 * w + 12)
        assert np.array_equal(got[:, :4 * w].reshape(h, w, 4), img), i
        assert (got[:, 4 * w:] == SENTINEL).all(), i


# ---- 8: the route is named ------------------------------------------------------------------------------------------------
def test_the_route_is_named(ctx):
    files = same_bpp_files()
    ctx.png_decode(files[0], "host")
    assert ctx.last_kernel() == SINGLE_KERNELS
    ctx.png_decode_batch(files)
    assert ctx.last_kernel() == BATCH_KERNELS
    ctx.png_decode(files[0], "device")
    assert ctx.last_kernel() == SINGLE_KERNELS


# ---- 9: whole-batch argument errors ---------------------------------------------------------------------------------------
def test_whole_batch_argument_errors(ctx):
    import torch
    files = same_bpp_files()[:1]
    want = ref.decode(files[0])
    h, w = want.shape[:2]
    ctx.png_decode(files[0], "host")
    before = ctx.last_kernel()
    for kw in (dict(n=0), dict(n=FNX_BATCH_MAX + 1), dict(workers=-1), dict(workers=65), dict(null_status=True)):
        dst = torch.full((h * w * 4,), SENTINEL, dtype=torch.uint8, device="cuda:0")
        rc, ws, hs, status = raw_batch(ctx, files, [dst], [4 * w], **kw)
        assert rc == FNX_ERR_INVALID, kw
        assert ws == [-7] and hs == [-7] and status == [77], kw                    # nothing written
        assert (dst.cpu().numpy() == SENTINEL).all(), kw
        assert ctx.last_kernel() == before, kw
    with pytest.raises(fennec_amd.FennecError):
        ctx.png_decode_batch([])
