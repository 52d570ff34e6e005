"""Adam7-interlaced PNG sources on the GPU (fnx_ctx_set_png_adam7): every image byte for byte against
tests/png_adam7_ref.py (decode_adam7), which is png_decode_ref's unfilter and expand per pass.  A ctx that never calls the
setter answers as before.  Every file is small; the references are computed once per test."""
from __future__ import annotations

import numpy as np
import pytest

import fennec_amd
import png_adam7_ref as a7
import png_decode_ref as ref
from fennec_amd import FNX_ERR_INVALID, FNX_ERR_UNSUPPORTED, FNX_OK
from fennec_amd import FNX_PNG_DECODE_ROWS as R

pytestmark = pytest.mark.gpu

SINGLE_KERNELS = "png_unfilter_kernel, png_expand_kernel"
ADAM7_KERNELS = "png_unfilter_batch_kernel, png_expand_adam7_kernel"
BATCH_KERNELS = "png_unfilter_batch_kernel, png_expand_batch_kernel"
ADAM7_BATCH_KERNELS = BATCH_KERNELS + ", png_expand_adam7_batch_kernel"
SIZES = [(1, 1), (3, 5), (8, 8), (9, 17), (33, 10)]


@pytest.fixture(scope="module")
def ctx():
    c = fennec_amd.Context(0)
    c.set_png_adam7(True)
    return c


@pytest.fixture(scope="module")
def plain_ctx():
    return fennec_amd.Context(0)


def pair_file(ct, depth, w, h, seed):
    s = ref.random_samples(w, h, ct, depth, seed)
    pal = ref.random_palette(1 << depth, seed) if ct == 3 else None
    return a7.write_adam7(s, ct, depth, filters=seed, palette=pal, idat_sizes=[1, 7, 100] if seed % 3 == 0 else None)


def short_stream_file():
    s = ref.random_samples(9, 5, 2, 8, 1)
    return a7.file_around(a7.adam7_stream(s, 2, 8, 5)[:-1], 9, 5, 2, 8)


def mislabelled_file():
    return ref.write_png(ref.random_samples(9, 5, 2, 8, 1), 2, 8, interlace=1)


def single(c, data):
    """(status, image or None) of Context.png_decode"""
    try:
        return FNX_OK, c.png_decode(data, "host")
    except fennec_amd.FennecUnsupported:
        return FNX_ERR_UNSUPPORTED, None
    except fennec_amd.FennecError:
        return FNX_ERR_INVALID, None


# ---- the default does not change -------------------------------------------------------------------------------------------
def test_a_default_ctx_still_refuses(plain_ctx):
    il = pair_file(2, 8, 9, 17, 1)
    with pytest.raises(fennec_amd.FennecUnsupported):
        plain_ctx.png_decode(il)
    with pytest.raises(fennec_amd.FennecUnsupported):
        plain_ctx.png_decode_config(il)
    plain = ref.write_png(ref.random_samples(9, 17, 2, 8, 1), 2, 8)
    images, statuses = plain_ctx.png_decode_batch([plain, il, plain])
    assert statuses == [FNX_OK, FNX_ERR_UNSUPPORTED, FNX_OK] and images[1] is None
    assert plain_ctx.last_kernel() == BATCH_KERNELS
    out, kinds, statuses = plain_ctx.png_recompress_batch([il])
    assert statuses == [FNX_ERR_UNSUPPORTED] and out == [None]
    with pytest.raises(fennec_amd.FennecUnsupported):
        plain_ctx.compress_file_png(il)


def test_the_setter_goes_both_ways():
    c = fennec_amd.Context(0)
    il = pair_file(6, 8, 9, 17, 2)
    want = a7.decode_adam7(il)
    for accept in (True, False, True):
        c.set_png_adam7(accept)
        if accept:
            assert c.png_decode_config(il) == (9, 17)
            assert np.array_equal(c.png_decode(il, "host"), want)
        else:
            with pytest.raises(fennec_amd.FennecUnsupported):
                c.png_decode(il)
            with pytest.raises(fennec_amd.FennecUnsupported):
                c.png_decode_config(il)
    assert c._lib.fnx_ctx_set_png_adam7(c._h, 2) == FNX_ERR_INVALID and c._lib.fnx_ctx_set_png_adam7(c._h, -1) == FNX_ERR_INVALID
    assert np.array_equal(c.png_decode(il, "host"), want)             # a refused setting leaves the ctx as it was


# ---- every pair, every small size ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct,depth", ref.PAIRS)
def test_every_pair(ctx, ct, depth):
    for k, (w, h) in enumerate(SIZES):
        il = pair_file(ct, depth, w, h, 20 * k + depth + ct)
        want = a7.decode_adam7(il)
        got = ctx.png_decode(il, "host")
        assert ctx.last_kernel() == ADAM7_KERNELS
        assert got.shape == (h, w, 4) and np.array_equal(got, want), (w, h)
        if k % 2:
            assert np.array_equal(ctx.png_decode(il, "device").cpu().numpy(), want), (w, h)


def trns_files():
    files = []
    for ct, depth in ((0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16)):      # a key that occurs in the image; 16-bit keys
        s = ref.random_samples(9, 17, ct, depth, 40 + depth)
        key = [int(v) for v in s[8, 4]]
        s[::2, ::3] = key
        if depth == 16:
            s[1, 1] = [v ^ 0x100 for v in key]                                        # the low bytes alone match: no hit at depth 16
        trns = b"".join(bytes([v >> 8, v & 255]) for v in key)
        files.append(a7.write_adam7(s, ct, depth, filters=depth, trns=trns))
    for depth in (1, 2, 4, 8):                                                        # tRNS shorter than, and longer than, PLTE
        top = 1 << depth
        npal = max(1, top - 1 - top // 4)
        s = ref.random_samples(9, 17, 3, depth, 50 + depth)                           # indices up to top - 1: behind the palette's end
        pal = ref.random_palette(npal, depth)
        files.append(a7.write_adam7(s, 3, depth, filters=depth, palette=pal, trns=bytes(([0, 255, 128, 1, 254, 77] * 43)[:max(1, npal - 1)])))
        files.append(a7.write_adam7(s, 3, depth, filters=depth + 1, palette=pal, trns=bytes(([128, 0, 255, 3] * 64)[:min(256, npal + 2)])))
    return files


def test_trns_and_indices_behind_the_palette(ctx):
    files = trns_files()
    want = [a7.decode_adam7(f) for f in files]
    assert any((w[..., 3] == 0).any() and (w[..., 3] == 255).any() for w in want)
    for f, w in zip(files, want):
        assert np.array_equal(ctx.png_decode(f, "host"), w)
    s = np.full((5, 9, 1), 200, np.int64)                                             # every index behind a palette of 3: opaque black
    f = a7.write_adam7(s, 3, 8, filters=1, palette=ref.random_palette(3, 1))
    got = ctx.png_decode(f, "host")
    assert np.array_equal(got, a7.decode_adam7(f)) and (got == np.array([0, 0, 0, 255], np.uint8)).all()


def test_host_and_device_space_and_a_strided_out(ctx):
    import torch
    il = pair_file(6, 16, 33, 10, 5)
    want = a7.decode_adam7(il)
    assert np.array_equal(ctx.png_decode(il, "host"), want)
    assert np.array_equal(ctx.png_decode(il, "device").cpu().numpy(), want)
    big = torch.full((10, 40, 4), 0xAB, dtype=torch.uint8, device="cuda:0")
    ctx.png_decode(il, "device", out=big[:, 2:35])
    got = big.cpu().numpy()
    assert np.array_equal(got[:, 2:35], want) and (got[:, :2] == 0xAB).all() and (got[:, 35:] == 0xAB).all()
    host = np.full((10, 40, 4), 0xAB, np.uint8)
    ctx.png_decode(il, "host", out=host[:, 2:35])
    assert np.array_equal(host, got)


# ---- the expand kernel's tile edge ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,h", [(300, 9), (257, 2)])
@pytest.mark.parametrize("ct,depth", [(2, 8), (0, 2)])
def test_a_second_workgroup_per_row(ctx, w, h, ct, depth):
    il = pair_file(ct, depth, w, h, w + depth)
    assert np.array_equal(ctx.png_decode(il, "host"), a7.decode_adam7(il))


# ---- the march --------------------------------------------------------------------------------------------------------------
def test_a_pass_longer_than_a_band(ctx):
    h = 2120
    counts = a7.passes(12, h, 2, 8)[1]
    assert counts[6] == 1060 and counts[6] > R
    fl = [[0] + [4 if y % 3 else 2 for y in range(1, n)] for n in counts]           # Paeth or Up everywhere but each pass's first row
    il = a7.write_adam7(ref.random_samples(12, h, 2, 8, 7), 2, 8, filters=fl)
    assert [p[:1] for p in a7.pass_filter_types(il)] == [[0]] * 7 and all(t >= 2 for p in a7.pass_filter_types(il) for t in p[1:])
    assert np.array_equal(ctx.png_decode(il, "host"), a7.decode_adam7(il))


def test_pass_rows_that_are_no_multiple_of_16_bytes(ctx):
    rb = a7.passes(70, 200, 6, 16)[2]
    assert sum(1 for b in rb if b % 16) == 5                                     # 72, 72, 144, 136, 280, 280, 560
    il = a7.write_adam7(ref.random_samples(70, 200, 6, 16, 8), 6, 16, filters=8)
    assert np.array_equal(ctx.png_decode(il, "host"), a7.decode_adam7(il))


# ---- the routes' names ------------------------------------------------------------------------------------------------------
def test_the_routes_are_named(ctx):
    il = pair_file(2, 8, 9, 17, 1)
    plain = ref.write_png(ref.random_samples(9, 17, 2, 8, 1), 2, 8, filters=[y % 5 for y in range(17)])
    ctx.png_decode(il, "host")
    assert ctx.last_kernel() == ADAM7_KERNELS
    ctx.png_decode(plain, "host")
    assert ctx.last_kernel() == SINGLE_KERNELS                       # a non-interlaced file goes the way it went, the setting on
    images, statuses = ctx.png_decode_batch([plain, plain])
    assert ctx.last_kernel() == BATCH_KERNELS and statuses == [FNX_OK, FNX_OK]
    assert np.array_equal(images[1], ref.decode(plain))
    images, statuses = ctx.png_decode_batch([plain, il])
    assert ctx.last_kernel() == ADAM7_BATCH_KERNELS and statuses == [FNX_OK, FNX_OK]
    images, statuses = ctx.png_decode_batch([il, il])                 # no non-interlaced file at all
    assert ctx.last_kernel() == ADAM7_BATCH_KERNELS and statuses == [FNX_OK, FNX_OK]
    assert np.array_equal(images[0], a7.decode_adam7(il)) and np.array_equal(images[1], images[0])


# ---- a mixed list -----------------------------------------------------------------------------------------------------------
def mixed_files():
    plain = [ref.write_png(ref.random_samples(w, 70, 2, 8, 20 + w), 2, 8, filters=np.random.default_rng(w).integers(0, 5, size=70).tolist())
             for w in (3, 67)]
    plain.append(ref.write_png(ref.random_samples(21, 66, 3, 4, 2), 3, 4, filters=[y % 5 for y in range(66)], palette=ref.random_palette(16, 2)))
    il = [pair_file(2, 8, 300, 9, 1), pair_file(6, 16, 33, 10, 2), pair_file(3, 2, 9, 17, 3), pair_file(2, 8, 1, 1, 4),
          pair_file(0, 1, 257, 2, 5), trns_files()[-1]]
    assert len({ref.bpp_of(ct, d) for ct, d in ((2, 8), (6, 16), (3, 2))}) == 3
    return [plain[0], il[0], short_stream_file(), il[1], plain[1], mislabelled_file(), il[2], b"\xff\xd8\xff\xe0\x00\x10JFIF\x00" + bytes(range(200)),
            il[3], plain[2], il[4], il[5]]


def test_a_mixed_list_equals_the_single_calls(ctx, plain_ctx):
    files = mixed_files()
    singles = [single(ctx, f) for f in files]
    assert [s for s, _ in singles] == [FNX_OK, FNX_OK, FNX_ERR_INVALID, FNX_OK, FNX_OK, FNX_ERR_INVALID, FNX_OK, FNX_ERR_INVALID, FNX_OK, FNX_OK,
                                       FNX_OK, FNX_OK]
    for i, f in enumerate(files):
        if singles[i][0] == FNX_OK:
            want = a7.decode_adam7(f) if fennec_amd.png_info(f)[4] else ref.decode(f)
            assert np.array_equal(singles[i][1], want), i
    for workers in (1, 4):
        images, statuses = ctx.png_decode_batch(files, workers=workers)
        assert ctx.last_kernel() == ADAM7_BATCH_KERNELS
        assert statuses == [s for s, _ in singles], workers
        for i in range(len(files)):
            assert (images[i] is None) == (singles[i][1] is None), (workers, i)
            if images[i] is not None:
                assert np.array_equal(images[i], singles[i][1]), (workers, i)
    # the same list on a default ctx: today's statuses
    images, statuses = plain_ctx.png_decode_batch(files, workers=4)
    today = [FNX_ERR_UNSUPPORTED if f[:8] == ref.SIG and fennec_amd.png_info(f)[4] else singles[i][0] for i, f in enumerate(files)]
    assert statuses == today and plain_ctx.last_kernel() == BATCH_KERNELS
    for i in range(len(files)):
        if today[i] == FNX_OK:
            assert np.array_equal(images[i], singles[i][1]), i
        else:
            assert images[i] is None


# ---- the entries behind the decoder -----------------------------------------------------------------------------------------
def test_recompress_batch_takes_an_adam7_file(ctx):
    il = pair_file(2, 8, 33, 10, 6)
    out, kinds, statuses = ctx.png_recompress_batch([il, short_stream_file()])
    assert statuses == [FNX_OK, FNX_ERR_INVALID] and out[1] is None
    assert out[0] == ctx.compress_png(ctx.png_decode(il), device_deflate=True)
    assert np.array_equal(ref.decode(out[0]), a7.decode_adam7(il))


def test_compress_file_png_takes_an_adam7_file(ctx):
    s = ref.random_samples(33, 10, 6, 8, 9)
    il = a7.write_adam7(s, 6, 8, filters=9)
    plain = ref.write_png(s, 6, 8, filters=[y % 5 for y in range(10)])
    got = ctx.compress_file_png(il)
    assert got == ctx.compress_file_png(plain)
    assert got[2] == (33, 10) and np.array_equal(ref.decode(got[0]), a7.decode_adam7(il))
