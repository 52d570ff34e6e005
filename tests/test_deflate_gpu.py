"""fnx_deflate on the GPU.  The decoder of record is Python's zlib: every stream must inflate to its input, in the host and
in the device space, and a second call must return the same bytes.  Sizes are held against the stored bound (derived) and
against raw deflate at zlib level 1 over the same independent chunks (measured once, see EXCESS_ALLOWED)."""
from __future__ import annotations

import ctypes as C
import zlib

import numpy as np
import pytest

import fennec_amd
import png_filter_ref as ref
from fennec_amd import FNX_DEFLATE_CHUNK as CH, FNX_DEFLATE_SUB as S

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 257, 258, 259, 260, S - 1, S, S + 1, CH - 1, CH, CH + 1, 2 * CH + 3, 5 * CH + S + 1]
ROW = 1 + 3 * 67                                                     # the row length of a 67-pixel RGB stream


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def fibonacci_shuffle():
    """21 symbols with counts 1, 1, 2, 3, 5, ... (28 656 bytes, one chunk): an unconstrained Huffman code of the BYTES is 20
    deep; the block's own histogram (match lengths, the end-of-block) is not, see test_fibonacci_takes_a_huffman_form"""
    counts = [1, 1]
    while len(counts) < 21:
        counts.append(counts[-1] + counts[-2])
    x = np.repeat(np.arange(21, dtype=np.uint8) * 11 + 3, counts)
    np.random.default_rng(5).shuffle(x)
    return x


def period(k):
    return lambda n: np.resize((np.arange(k) * 37 + 11).astype(np.uint8), n)


def pair_and_noise(n):
    """64 bytes of one byte pair, 64 bytes of noise, and so on"""
    x = np.random.default_rng(9).integers(0, 256, size=n, dtype=np.uint8)
    i = np.arange(n)
    pair = np.where(i % 2 == 0, 0xAB, 0xCD).astype(np.uint8)
    return np.where((i // 64) % 2 == 0, pair, x).astype(np.uint8)


CONTENTS = {
    "constant": (lambda n: np.full(n, 0x5A, np.uint8), 0),
    "period1": (period(1), 0), "period2": (period(2), 0), "period3": (period(3), 0), "period4": (period(4), 0), "period7": (period(7), 0),
    "period_row": (period(ROW), ROW),
    "noise": (lambda n: np.random.default_rng(n).integers(0, 256, size=n, dtype=np.uint8), 0),
    "pair_and_noise": (pair_and_noise, 0),
    "fibonacci": (lambda n: np.resize(fibonacci_shuffle(), n), 0),
    "all_bytes": (lambda n: np.resize(np.arange(256, dtype=np.uint8), n), 0),
}


def round_trip(ctx, x, row=0):
    """x through the host and the device space, twice each -> the stream (bytes)"""
    want = x.tobytes()
    d = dev(x)
    outs = []
    for _ in range(2):
        outs.append(ctx.deflate(x, row))
        t = ctx.deflate(d, row)
        ctx.sync()
        outs.append(t.cpu().numpy().tobytes())
    assert all(o == outs[0] for o in outs), "host and device space, first and second call: identical bytes"
    assert outs[0][:2] == b"\x78\x01"
    assert zlib.decompress(outs[0]) == want, f"n = {len(x)}"
    assert len(outs[0]) <= fennec_amd.deflate_bound(len(x)), (len(outs[0]), len(x))
    return outs[0]


@pytest.mark.parametrize("name", sorted(CONTENTS))
def test_round_trip(ctx, name):
    gen, row = CONTENTS[name]
    for n in LENGTHS:
        round_trip(ctx, gen(n), row)


def test_fibonacci_takes_a_huffman_form(ctx):
    """a skewed block that takes a Huffman form.  It does NOT reach the 15-bit limit: the shuffle leaves many matches, and the
    end-of-block's count of 1 beside the chain's two splits the chain, so the literal/length tree is 13 deep and the distance
    tree 11.  The limit is reached, and certified from the stream, by test_deflate_structure_gpu.py::test_the_15_bit_limit."""
    x = fibonacci_shuffle()
    assert len(x) == 28656 and len(x) <= CH
    out = round_trip(ctx, x)
    assert len(out) < len(x) // 2                                    # a Huffman block (entropy 2.6 bits a symbol), not a stored one


def test_noise_takes_the_stored_form(ctx):
    n = 2 * CH
    out = round_trip(ctx, CONTENTS["noise"][0](n))
    assert len(out) == fennec_amd.deflate_bound(n) - 5              # every chunk stored; the last carries no closing block
    assert out[2] == 0 and out[3:7] == bytes([CH & 255, CH >> 8, ~CH & 255, (~CH >> 8) & 255])


def test_single_symbol_and_no_match_blocks(ctx):
    """one distinct symbol (a run that is all one match chain), and blocks without any match: three different bytes"""
    for x in (np.zeros(S, np.uint8), np.zeros(3, np.uint8), np.array([1, 2, 3], np.uint8), np.arange(64, dtype=np.uint8),
              np.array([7], np.uint8), np.array([7, 7], np.uint8), np.resize(np.array([0, 0, 0, 1], np.uint8), 2 * S)):
        round_trip(ctx, x)


KINDS = ["rgb", "rgba", "gray", "pal8", "pal4", "pal2", "pal1"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("w,h", [(67, 7), (1031, 37)])
def test_filtered_streams(ctx, kind, w, h):
    import test_png_filter_gpu as filter_tests
    src, k, ncolors = filter_tests.content(kind, w, h, 100 * w + h)
    stream, _, _ = ref.png_stream(src, k, ncolors)
    flat = np.ascontiguousarray(stream).reshape(-1)
    assert round_trip(ctx, flat, stream.shape[1]) == round_trip(ctx, flat, stream.shape[1])
    round_trip(ctx, flat, 0)                                         # the hint changes the bytes at most, never the content


# ---- size -------------------------------------------------------------------------------------------------------------
def test_constant_mebibyte(ctx):
    """tokens are cut at most every S >= 64 bytes and a match token costs at most 15 + 5 + 15 + 13 bits = 6 bytes: 6 / 64 plus
    headers stays under 1 / 8"""
    n = 1 << 20
    out = round_trip(ctx, np.full(n, 0x33, np.uint8))
    assert len(out) < n // 8, len(out)


def chunked_level1(data: bytes) -> int:
    """the yardstick: raw deflate at zlib level 1 over the same independent chunks, Z_FULL_FLUSH behind each"""
    co = zlib.compressobj(1, zlib.DEFLATED, -15)
    total = 0
    for i in range(0, len(data), CH):
        total += len(co.compress(data[i:i + CH])) + len(co.flush(zlib.Z_FULL_FLUSH))
    return total + len(co.flush())


def stripes(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return (((x // 8) + (y // 16)) % 5).astype(np.uint8)


# The device stream's excess over chunked level 1: smooth RGB +4.4 %,
# smooth RGBA +3.4 %, striped paletted plane +54.3 % (2623 bytes against 1700 of 131 328: a flat plane is one match per lane,
# cut every S = 128 bytes, where zlib's run to 258) -- the worst of the three rounded up to the next 5 %.
# The three figures are from the kernel's source run on the host (lanes as threads); the encoder is integer arithmetic that
# does not depend on the launch, so an MI355X gives the same sizes -- the test prints them, and a first GPU run that shows
# other figures corrects this comment and the constant.
EXCESS_ALLOWED = 0.55
# Smooth content above 25 % would mean that candidates are being lost: that is a bug, not a figure to record.
EXCESS_ALLOWED_SMOOTH = 0.25

RATIO_CASES = {
    "smooth_rgb": lambda: ref.png_stream(ref.smooth_rgba(512, 256, 11, opaque=True), ref.NRGBA),
    "smooth_rgba": lambda: ref.png_stream(ref.smooth_rgba(512, 256, 12, opaque=False), ref.NRGBA),
    "stripes": lambda: ref.png_stream(stripes(512, 256), ref.PALETTED, 256),
}


@pytest.mark.parametrize("name", sorted(RATIO_CASES))
def test_ratio_against_chunked_level_1(ctx, name):
    stream = RATIO_CASES[name]()[0]
    flat = np.ascontiguousarray(stream).reshape(-1)
    out = round_trip(ctx, flat, stream.shape[1])
    yard = chunked_level1(flat.tobytes())
    best = len(zlib.compress(flat.tobytes(), 9))
    excess = len(out) / yard - 1.0
    print(f"{name}: {flat.size} bytes -> device {len(out)}, chunked level 1 {yard} (excess {100 * excess:+.1f} %), level 9 {best} "
          f"(excess {100 * (len(out) / best - 1):+.1f} %)")
    assert excess <= (EXCESS_ALLOWED_SMOOTH if name.startswith("smooth") else EXCESS_ALLOWED), (name, len(out), yard)


# ---- capacity, routes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["host", "device", "device_src"])
def test_capacity(ctx, space):
    lib = fennec_amd.load_library()
    x = CONTENTS["pair_and_noise"][0](CH + 777)
    want = round_trip(ctx, x)
    src = x if space == "host" else dev(x)
    sptr = x.ctypes.data if space == "host" else src.data_ptr()
    sp = {"host": fennec_amd.FNX_HOST, "device": fennec_amd.FNX_DEVICE, "device_src": fennec_amd.FNX_DEVICE_SRC}[space]

    def call(cap):
        out = np.full(len(want) + 64, 0xAB, np.uint8)
        out = dev(out) if space == "device" else out
        nb = C.c_size_t(0)
        rc = lib.fnx_deflate(ctx._h, sp, sptr, len(x), 0, out.data_ptr() if space == "device" else out.ctypes.data, cap, C.byref(nb))
        ctx.sync()
        return rc, nb.value, out if isinstance(out, np.ndarray) else out.cpu().numpy()
    rc, nb, out = call(len(want) - 1)                                # one byte short: the size, and nothing written
    assert rc == fennec_amd.FNX_ERR_INVALID and nb == len(want)
    assert (out == 0xAB).all()
    rc, nb, out = call(len(want))
    assert rc == 0 and nb == len(want) and out[:nb].tobytes() == want
    assert (out[nb:] == 0xAB).all(), "bytes behind the stream were written"
    rc, nb, out = call(len(want) + 64)
    assert rc == 0 and out[:nb].tobytes() == want and (out[nb:] == 0xAB).all()
    # arguments that are refused with a live ctx
    nbv = C.c_size_t(0)
    o = np.full(64, 0xAB, np.uint8)
    assert lib.fnx_deflate(ctx._h, fennec_amd.FNX_HOST, x.ctypes.data, 0, 0, o.ctypes.data, 64, C.byref(nbv)) == fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_deflate(ctx._h, fennec_amd.FNX_HOST, None, 16, 0, o.ctypes.data, 64, C.byref(nbv)) == fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_deflate(ctx._h, fennec_amd.FNX_HOST, x.ctypes.data, 16, 0, o.ctypes.data, 64, None) == fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_deflate(ctx._h, 5, x.ctypes.data, 16, 0, o.ctypes.data, 64, C.byref(nbv)) == fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_deflate(ctx._h, fennec_amd.FNX_HOST, x.ctypes.data, 16, -1, o.ctypes.data, 64, C.byref(nbv)) == fennec_amd.FNX_ERR_INVALID
    assert (o == 0xAB).all()


def test_last_kernel_names_the_kernel(ctx):
    ctx.png_filter(ref.noise_rgba(9, 3, 1))
    assert ctx.last_kernel() == "png_filter_kernel"
    ctx.deflate(b"abcabcabc")
    assert ctx.last_kernel() == "deflate_chunk_kernel"
