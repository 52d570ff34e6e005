"""The host side of fnx_png_decode without a GPU: the header's new entries, fnx_inflate against zlib (and against the streams
zlib never writes), fnx_png_info, and every rule of the chunk walk -- each damaged file is refused by the library AND by the
tests' own restatement (png_decode_ref.parse), each odd-but-legal one passes both."""
from __future__ import annotations

import ctypes as C
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import fennec_amd
import inflate_probe
import png_decode_ref as ref
from fennec_amd import FNX_ERR_INVALID, FNX_ERR_UNSUPPORTED, FNX_HOST, FNX_OK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return fennec_amd.load_library()


def inflate_rc(lib, z: bytes, cap: int):
    src = np.frombuffer(z, np.uint8) if z else np.zeros(1, np.uint8)
    out = np.full(cap + 8, 0xAB, np.uint8)
    n = C.c_size_t(0)
    rc = lib.fnx_inflate(src.ctypes.data, len(z), out.ctypes.data, cap, C.byref(n))
    assert (out[cap:] == 0xAB).all(), "fnx_inflate wrote behind cap"
    return rc, out[:n.value].tobytes()


def inflate_overflow(lib, z: bytes, cap: int):
    src = np.frombuffer(z, np.uint8)
    out = np.full(cap + 8, 0xAB, np.uint8)
    n = C.c_size_t(0)
    rc = lib.fnx_inflate(src.ctypes.data, len(z), out.ctypes.data, cap, C.byref(n))
    assert (out[cap:] == 0xAB).all(), "fnx_inflate wrote behind cap"
    return rc, n.value


def config_rc(lib, data: bytes):
    """fnx_png_decode with dst == NULL: the chunk walk alone, no ctx"""
    src = np.frombuffer(data, np.uint8) if data else np.zeros(1, np.uint8)
    w, h = C.c_int(-1), C.c_int(-1)
    return lib.fnx_png_decode(None, src.ctypes.data, len(data), FNX_HOST, None, 0, C.byref(w), C.byref(h)), (w.value, h.value)


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_header_python_and_library_agree(lib):
    names = fennec_amd.exported_symbols()
    for n in ("fnx_inflate", "fnx_png_info", "fnx_png_decode"):
        assert n in names and hasattr(C.CDLL(fennec_amd.LIB_PATH), n)
    text = open(os.path.join(ROOT, "include", "fennec_hip.h")).read()
    assert f"#define FNX_PNG_DECODE_ROWS {fennec_amd.FNX_PNG_DECODE_ROWS}" in text
    assert callable(fennec_amd.inflate) and callable(fennec_amd.png_info) and hasattr(fennec_amd.Context, "png_decode")
    out = subprocess.check_output(["nm", "-D", "--undefined-only", fennec_amd.LIB_PATH]).decode()
    assert "inflate" not in out and "crc32" not in out and "adler32" not in out, "the library links no zlib"


def test_header_is_plain_c_and_links_from_c(lib, tmp_path):
    z = zlib.compress(b"hello, hello, hello, hello", 9)
    png = ref.write_png(np.zeros((2, 3, 1), np.int64), 0, 8)
    arr = lambda b: ", ".join(str(v) for v in b)          # noqa: E731
    src = tmp_path / "png_abi.c"
    src.write_text(r'''
#include <string.h>
#include "fennec_hip.h"
static const uint8_t z[] = {%s};
static const uint8_t png[] = {%s};
int main(void) {
    uint8_t out[64];
    size_t n = 0;
    int w = 0, h = 0, ct = -1, bd = -1, il = -1;
    if (fnx_inflate(z, sizeof z, out, sizeof out, &n) != FNX_OK || n != 26 || memcmp(out, "hello, hello", 12)) return 1;
    if (fnx_inflate(z, sizeof z, out, 25, &n) != FNX_ERR_INVALID || n != 26) return 2;             /* cap + 1: too small */
    if (fnx_png_info(png, sizeof png, &w, &h, &ct, &bd, &il) != FNX_OK || w != 3 || h != 2 || ct != 0 || bd != 8 || il != 0) return 3;
    w = h = 0;
    if (fnx_png_decode(0, png, sizeof png, FNX_HOST, 0, 0, &w, &h) != FNX_OK || w != 3 || h != 2) return 4;   /* dimensions: no ctx */
    if (fnx_png_decode(0, png, sizeof png - 1, FNX_HOST, 0, 0, &w, &h) != FNX_ERR_INVALID) return 5;
    return FNX_PNG_DECODE_ROWS == 1024 ? 0 : 6;
}
''' % (arr(z), arr(png)))
    exe = tmp_path / "png_abi"
    libdir = os.path.dirname(fennec_amd.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfennec_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.call([str(exe)]) == 0


def test_null_pointers_are_refused(lib):
    n = C.c_size_t(0)
    one = np.zeros(8, np.uint8)
    assert lib.fnx_inflate(None, 0, one.ctypes.data, 8, C.byref(n)) == FNX_ERR_INVALID
    assert lib.fnx_inflate(one.ctypes.data, 8, None, 8, C.byref(n)) == FNX_ERR_INVALID
    assert lib.fnx_inflate(one.ctypes.data, 8, one.ctypes.data, 8, None) == FNX_ERR_INVALID
    v = C.c_int()
    assert lib.fnx_png_info(None, 0, C.byref(v), C.byref(v), C.byref(v), C.byref(v), C.byref(v)) == FNX_ERR_INVALID
    assert lib.fnx_png_info(one.ctypes.data, 8, None, C.byref(v), C.byref(v), C.byref(v), C.byref(v)) == FNX_ERR_INVALID
    assert lib.fnx_png_decode(None, None, 0, FNX_HOST, None, 0, C.byref(v), C.byref(v)) == FNX_ERR_INVALID
    ok = np.frombuffer(ref.write_png(np.zeros((2, 3, 1), np.int64), 0, 8), np.uint8)
    for space in (-1, 2, 7):                 # FNX_HOST or FNX_DEVICE, also for the dimensions alone
        assert lib.fnx_png_decode(None, ok.ctypes.data, ok.size, space, None, 0, C.byref(v), C.byref(v)) == FNX_ERR_INVALID
    assert lib.fnx_png_decode(None, ok.ctypes.data, ok.size, 1, None, 0, C.byref(v), C.byref(v)) == FNX_OK
    # a destination needs a context: refused, not crashed
    png = np.frombuffer(ref.write_png(np.zeros((2, 3, 1), np.int64), 0, 8), np.uint8)
    dst = np.zeros((2, 3, 4), np.uint8)
    assert lib.fnx_png_decode(None, png.ctypes.data, png.size, FNX_HOST, dst.ctypes.data, 12, C.byref(v), C.byref(v)) < 0


# ---- fnx_inflate --------------------------------------------------------------------------------------------------------------
def _inputs():
    rng = np.random.default_rng(3)
    text = (b"the quick brown fox jumps over the lazy dog; " * 400)[:17000]
    block = bytes(rng.integers(0, 256, 32000, dtype=np.uint8))
    return {"empty": b"", "one": b"x", "two": b"ab", "text": text, "noise": bytes(rng.integers(0, 256, 5000, dtype=np.uint8)),
            "far": block + block + block[:6000],                      # 70 000 bytes, matches 32 000 back
            "runs": bytes(rng.integers(0, 3, 40000, dtype=np.uint8))}


@pytest.mark.parametrize("level", [0, 1, 6, 9])
def test_inflate_against_zlib(lib, level):
    seen = set()
    for name, data in _inputs().items():
        z = zlib.compress(data, level)
        p = inflate_probe.probe(z)
        seen |= {b.btype for b in p.blocks}
        rc, out = inflate_rc(lib, z, len(data))
        assert rc == FNX_OK and out == data, (name, level)
        assert fennec_amd.inflate(z) == data
        if name == "far" and level:
            assert max(t[1] for b in p.blocks for t in b.tokens if isinstance(t, tuple)) >= 32000
        if data:
            rc, n = inflate_overflow(lib, z, len(data) - 1)             # cap too small: refused, nothing behind cap written,
            assert rc == FNX_ERR_INVALID and n == len(data), (name, level)   # and said so: *nbytes = cap + 1
    if level == 0:
        assert seen == {inflate_probe.STORED}
    else:
        assert inflate_probe.FIXED in seen and inflate_probe.DYNAMIC in seen     # short inputs take the fixed codes, text the dynamic ones


def test_all_three_block_forms_occur():
    forms = set()
    for level in (0, 1, 6, 9):
        for data in _inputs().values():
            forms |= {b.btype for b in inflate_probe.probe(zlib.compress(data, level)).blocks}
    assert forms == {inflate_probe.STORED, inflate_probe.FIXED, inflate_probe.DYNAMIC}


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, n):                     # least significant bit first (everything but Huffman codes)
        self.bits += [(v >> i) & 1 for i in range(n)]

    def code(self, v, n):                    # a Huffman code: most significant bit first
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]

    def fixed_literal(self, b):
        self.code(0x30 + b, 8) if b < 144 else self.code(0x190 + b - 144, 9)

    def bytes(self):
        return np.packbits(np.array(self.bits + [0] * (-len(self.bits) % 8), np.uint8), bitorder="little").tobytes()


def zwrap(body: bytes, out: bytes) -> bytes:
    return b"\x78\x9c" + body + struct.pack(">I", zlib.adler32(out))


def test_inflate_distance_of_exactly_32768(lib):
    data = bytes(np.random.default_rng(8).integers(0, 256, 32768, dtype=np.uint8))
    w = BitWriter()
    w.put(1, 1); w.put(1, 2)                                   # BFINAL, fixed codes
    for b in data:
        w.fixed_literal(b)
    w.code(0xc5, 8)                                             # length symbol 285: 258 bytes
    w.code(29, 5); w.put(8191, 13)                              # distance symbol 29: 24577 + 8191 = 32768
    w.code(0, 7)                                                # end of block
    want = data + data[:258]
    z = zwrap(w.bytes(), want)
    assert zlib.decompress(z) == want
    rc, out = inflate_rc(lib, z, len(want))
    assert rc == FNX_OK and out == want


def test_damaged_streams_are_refused(lib):
    data = b"abcabcabcabc" * 50
    good = zlib.compress(data, 6)
    assert inflate_rc(lib, good, len(data)) == (FNX_OK, data)
    bad = {
        "CM is not 8": b"\x79" + good[1:],
        "window above 32 KiB": bytes([0x88, 0x1c]) + good[2:],
        "header check": good[:1] + bytes([good[1] ^ 1]) + good[2:],
        "preset dictionary": bytes([0x78, 0xbb]) + good[2:],
        "Adler-32": good[:-1] + bytes([good[-1] ^ 1]),
        "truncated in the check": good[:-2],
        "truncated in the block": good[:len(good) // 2],
        "header only": good[:2],
        "empty": b"",
    }
    w = BitWriter()                                             # a match with no output behind it
    w.put(1, 1); w.put(1, 2)
    w.code(1, 7)                                                # length symbol 257: 3 bytes
    w.code(0, 5)                                                # distance 1
    w.code(0, 7)
    bad["distance too far"] = zwrap(w.bytes(), b"")
    w = BitWriter()                                             # literal 'a', then a match 2 back
    w.put(1, 1); w.put(1, 2)
    w.fixed_literal(97)
    w.code(1, 7); w.code(1, 5)
    w.code(0, 7)
    bad["distance one too far"] = zwrap(w.bytes(), b"aaaa")
    w = BitWriter()                                             # dynamic block whose code-length code has four codes of one bit
    w.put(1, 1); w.put(2, 2)
    w.put(0, 5); w.put(0, 5); w.put(0, 4)
    for _ in range(4):
        w.put(1, 3)
    w.put(0, 32)
    bad["over-subscribed code-length code"] = zwrap(w.bytes(), b"")
    w = BitWriter()                                             # code-length code: 0 and 1 get one bit each; then 257 + 1 lengths of 1
    w.put(1, 1); w.put(2, 2)
    w.put(0, 5); w.put(0, 5); w.put(14, 4)                      # HCLEN 18: ... 14, 1 are the last two in the order
    for i in range(18):
        w.put(1 if i in (3, 17) else 0, 3)                      # positions of symbols 0 and 1 in the order 16 17 18 0 8 ... 14 1
    for _ in range(258):
        w.code(1, 1)                                            # every literal/length symbol and the one distance symbol: length 1
    w.put(0, 32)
    bad["over-subscribed literal/length code"] = zwrap(w.bytes(), b"")
    w = BitWriter()
    w.put(1, 1); w.put(3, 2)
    bad["block type 3"] = zwrap(w.bytes(), b"")
    stored = zlib.compress(data, 0)
    bad["LEN / NLEN"] = stored[:5] + bytes([stored[5] ^ 1]) + stored[6:]
    for name, z in bad.items():
        with pytest.raises(zlib.error):
            zlib.decompress(z)
        rc, out = inflate_rc(lib, z, 4096)
        assert rc == FNX_ERR_INVALID and len(out) <= 4096, name         # damage, not "cap is too small" (cap + 1)
        with pytest.raises(fennec_amd.FennecError):
            fennec_amd.inflate(z)


def canonical(lengths: dict) -> dict:
    """symbol -> (code, length) of the canonical code of RFC 1951, 3.2.2, complete or not"""
    codes, code = {}, 0
    for l in range(1, 16):
        for s in sorted(k for k, v in lengths.items() if v == l):
            codes[s] = (code, l)
            code += 1
        code <<= 1
    return codes


def dynamic_stream(ll: dict, d: dict, tokens, out: bytes, hlit=None, hdist=None, cl=None) -> bytes:
    """a zlib stream of ONE dynamic block whose literal/length and distance codes have exactly the given lengths (symbol ->
    length, everything else 0), sent one length at a time through a code-length code `cl` (default: a complete one over the
    length values used).  tokens: literal/length symbols, or (length symbol, extra value, extra bits, distance symbol, extra
    value, extra bits); the end-of-block is appended."""
    hlit = hlit or max(257, max(ll) + 1)
    hdist = hdist or max(1, max(d, default=0) + 1)
    lens = [ll.get(i, 0) for i in range(hlit)] + [d.get(i, 0) for i in range(hdist)]
    if cl is None:
        used = sorted(set(lens)) if len(set(lens)) > 1 else sorted(set(lens) | {15})
        k = len(used)
        m = max(1, (k - 1).bit_length())
        short = (1 << m) - k                                   # a complete code: `short` symbols of m - 1 bits, the rest of m
        cl = {v: (m - 1 if i < short else m) for i, v in enumerate(used)}
    order = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
    w = BitWriter()
    w.put(1, 1); w.put(2, 2)
    w.put(hlit - 257, 5); w.put(hdist - 1, 5); w.put(15, 4)    # HCLEN 19: all of them
    for sym in order:
        w.put(cl.get(sym, 0), 3)
    clc, llc, dc = canonical(cl), canonical(ll), canonical(d)
    for v in lens:
        w.code(*clc.get(v, (0, 1)))                            # (a length `cl` has no code for: a refused code-length code, never read)
    for t in list(tokens) + [256]:
        if isinstance(t, tuple):
            ls, le, lb, ds, de, db = t
            w.code(*llc[ls]); w.put(le, lb)
            w.code(*dc[ds]); w.put(de, db)
        else:
            w.code(*llc[t])
    return zwrap(w.bytes(), out)


A = 97
# what zlib's inflate_table and Go's compress/flate pass although the code is incomplete: a literal/length or a distance code of
# ONE code of one bit -- and a distance code of no code at all in a block without matches.  zlib's deflate never writes
# either (it always sends two distance codes); other encoders do.
INCOMPLETE_ACCEPTED = {
    "one distance code of one bit": (dynamic_stream({A: 1, 256: 2, 285: 2}, {0: 1}, [A, (285, 0, 0, 0, 0, 0)], b"a" * 259, hlit=286), b"a" * 259),
    "one literal/length code of one bit": (dynamic_stream({256: 1}, {0: 1}, [], b""), b""),
    "no distance code, no match": (dynamic_stream({A: 1, 256: 1}, {}, [A, A], b"aa"), b"aa"),
    "both codes of one code": (dynamic_stream({256: 1}, {}, [], b""), b""),
}
INCOMPLETE_REFUSED = {
    "two distance codes of two bits": dynamic_stream({A: 1, 256: 2, 285: 2}, {0: 2, 1: 2}, [A, (285, 0, 0, 0, 0, 0)], b"a" * 259, hlit=286),
    "one distance code of two bits": dynamic_stream({A: 1, 256: 2, 285: 2}, {0: 2}, [A, (285, 0, 0, 0, 0, 0)], b"a" * 259, hlit=286),
    "one literal/length code of two bits": dynamic_stream({256: 2}, {0: 1}, [], b""),
    "two literal/length codes of two bits": dynamic_stream({A: 2, 256: 2}, {0: 1}, [A], b"a"),
    "a match through a distance code of no code": dynamic_stream({A: 1, 256: 2, 285: 2}, {}, [A, 285], b"a" * 259, hlit=286),
    # the code-length code may never be incomplete, not even in the one-code form
    "code-length code of one code of one bit": dynamic_stream({256: 1}, {0: 1}, [], b"", cl={1: 1}),
    "code-length code of two codes of two bits": dynamic_stream({256: 1}, {0: 1}, [], b"", cl={0: 2, 1: 2}),
}


@pytest.mark.parametrize("name", sorted(INCOMPLETE_ACCEPTED))
def test_incomplete_codes_zlib_takes(lib, name):
    z, want = INCOMPLETE_ACCEPTED[name]
    assert zlib.decompress(z) == want
    assert inflate_rc(lib, z, len(want) + 8) == (FNX_OK, want)


@pytest.mark.parametrize("name", sorted(INCOMPLETE_REFUSED))
def test_incomplete_codes_zlib_refuses(lib, name):
    z = INCOMPLETE_REFUSED[name]
    with pytest.raises(zlib.error):
        zlib.decompress(z)
    rc, _ = inflate_rc(lib, z, 4096)
    assert rc == FNX_ERR_INVALID, name


def test_the_complete_twins_of_those_streams_pass(lib):
    """the builder itself: the same blocks with complete codes inflate, so the refusals above are about completeness alone"""
    z = dynamic_stream({A: 1, 256: 2, 285: 2}, {0: 1, 1: 1}, [A, (285, 0, 0, 0, 0, 0)], b"a" * 259, hlit=286)
    assert zlib.decompress(z) == b"a" * 259 and inflate_rc(lib, z, 300) == (FNX_OK, b"a" * 259)
    z = dynamic_stream({A: 1, 256: 1}, {0: 1, 1: 1}, [A], b"a")
    assert zlib.decompress(z) == b"a" and inflate_rc(lib, z, 8) == (FNX_OK, b"a")


# ---- fnx_png_info -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct,depth", ref.PAIRS)
def test_png_info_on_every_pair(lib, ct, depth):
    s = ref.random_samples(5, 3, ct, depth, 1)
    data = ref.write_png(s, ct, depth, palette=ref.random_palette(2, 1) if ct == 3 else None)
    assert fennec_amd.png_info(data) == (5, 3, ct, depth, 0)
    assert config_rc(lib, data) == (FNX_OK, (5, 3))
    assert ref.parse(data)["w"] == 5
    il = ref.write_png(s, ct, depth, palette=ref.random_palette(2, 1) if ct == 3 else None, interlace=1)
    assert fennec_amd.png_info(il) == (5, 3, ct, depth, 1)
    assert config_rc(lib, il)[0] == FNX_ERR_UNSUPPORTED
    with pytest.raises(ref.Unsupported):
        ref.parse(il)


def test_oversized_files_are_unsupported(lib):
    for w, h in ((65536, 1), (1, 65536)):
        data = ref.SIG + ref.ihdr(w, h, 1, 0) + ref.chunk(b"IDAT", zlib.compress(b"\0")) + ref.chunk(b"IEND", b"")
        assert fennec_amd.png_info(data)[:2] == (w, h)
        assert config_rc(lib, data)[0] == FNX_ERR_UNSUPPORTED
        with pytest.raises(ref.Unsupported):
            ref.parse(data)
    data = ref.SIG + ref.ihdr(65535, 1, 1, 0) + ref.chunk(b"IDAT", zlib.compress(b"\0")) + ref.chunk(b"IEND", b"")
    assert config_rc(lib, data) == (FNX_OK, (65535, 1))


# ---- the chunk walk ---------------------------------------------------------------------------------------------------------
def _parts(ct=2, depth=8, w=4, h=2):
    rowbytes = (w * ref.CHANNELS[ct] * depth + 7) // 8
    return dict(ihdr=ref.ihdr(w, h, depth, ct), plte=ref.chunk(b"PLTE", bytes(range(12))), idat=ref.chunk(b"IDAT", zlib.compress(bytes(h * (1 + rowbytes)))),
                iend=ref.chunk(b"IEND", b""), text=ref.chunk(b"tEXt", b"Comment\0hello"))


def _flip_crc(c: bytes) -> bytes:
    return c[:-1] + bytes([c[-1] ^ 1])


def _flip_body(c: bytes) -> bytes:
    return c[:9] + bytes([c[9] ^ 0x10]) + c[10:]


def damaged_files():
    t, p, g = _parts(2), _parts(3), _parts(0)
    S = ref.SIG
    z = t["idat"][8:-4]
    out = {
        "signature": b"\x89PNG\r\n\x1a\r" + t["ihdr"] + t["idat"] + t["iend"],
        "too short for a signature": S[:5],
        "CRC of IHDR": S + _flip_crc(t["ihdr"]) + t["idat"] + t["iend"],
        "CRC of PLTE": S + p["ihdr"] + _flip_crc(p["plte"]) + p["idat"] + p["iend"],
        "CRC of IDAT": S + t["ihdr"] + _flip_crc(t["idat"]) + t["iend"],
        "body of IDAT": S + t["ihdr"] + _flip_body(t["idat"]) + t["iend"],
        "CRC of an ancillary chunk": S + t["ihdr"] + _flip_crc(t["text"]) + t["idat"] + t["iend"],
        "CRC of IEND": S + t["ihdr"] + t["idat"] + _flip_crc(t["iend"]),
        "IHDR is not first": S + t["text"] + t["ihdr"] + t["idat"] + t["iend"],
        "IHDR of 12 bytes": S + ref.chunk(b"IHDR", t["ihdr"][8:-5]) + t["idat"] + t["iend"],
        "a second IHDR": S + t["ihdr"] + t["ihdr"] + t["idat"] + t["iend"],
        "width 0": S + ref.ihdr(0, 2, 8, 2) + t["idat"] + t["iend"],
        "height 0": S + ref.ihdr(4, 0, 8, 2) + t["idat"] + t["iend"],
        "width 2^31": S + ref.ihdr(1 << 31, 2, 8, 2) + t["idat"] + t["iend"],
        "colour type 1": S + ref.ihdr(4, 2, 8, 1) + t["idat"] + t["iend"],
        "truecolour at depth 4": S + ref.ihdr(4, 2, 4, 2) + t["idat"] + t["iend"],
        "paletted at depth 16": S + ref.ihdr(4, 2, 16, 3) + p["plte"] + t["idat"] + t["iend"],
        "depth 3": S + ref.ihdr(4, 2, 3, 0) + t["idat"] + t["iend"],
        "compression 1": S + ref.ihdr(4, 2, 8, 2, compression=1) + t["idat"] + t["iend"],
        "filter method 1": S + ref.ihdr(4, 2, 8, 2, filt=1) + t["idat"] + t["iend"],
        "interlace 2": S + ref.ihdr(4, 2, 8, 2, interlace=2) + t["idat"] + t["iend"],
        "PLTE after IDAT": S + p["ihdr"] + p["idat"] + p["plte"] + p["iend"],
        "PLTE missing": S + p["ihdr"] + p["idat"] + p["iend"],
        "PLTE of 4 bytes": S + p["ihdr"] + ref.chunk(b"PLTE", bytes(4)) + p["idat"] + p["iend"],
        "PLTE empty": S + p["ihdr"] + ref.chunk(b"PLTE", b"") + p["idat"] + p["iend"],
        "PLTE of 257 entries": S + p["ihdr"] + ref.chunk(b"PLTE", bytes(771)) + p["idat"] + p["iend"],
        "PLTE twice": S + p["ihdr"] + p["plte"] + p["plte"] + p["idat"] + p["iend"],
        "PLTE in a greyscale file": S + g["ihdr"] + g["plte"] + g["idat"] + g["iend"],
        "PLTE longer than 2^depth": S + ref.ihdr(4, 2, 1, 3) + p["plte"] + ref.chunk(b"IDAT", zlib.compress(bytes(4))) + p["iend"],
        "tRNS before PLTE": S + p["ihdr"] + ref.chunk(b"tRNS", b"\1\2") + p["plte"] + p["idat"] + p["iend"],
        "tRNS after IDAT": S + t["ihdr"] + t["idat"] + ref.chunk(b"tRNS", bytes(6)) + t["iend"],
        "tRNS between IDATs": S + t["ihdr"] + ref.chunk(b"IDAT", z[:5]) + ref.chunk(b"tRNS", bytes(6)) + ref.chunk(b"IDAT", z[5:]) + t["iend"],
        "tRNS for colour type 4": S + ref.ihdr(4, 2, 8, 4) + ref.chunk(b"tRNS", bytes(2)) + ref.chunk(b"IDAT", zlib.compress(bytes(18))) + t["iend"],
        "tRNS for colour type 6": S + ref.ihdr(4, 2, 8, 6) + ref.chunk(b"tRNS", bytes(6)) + ref.chunk(b"IDAT", zlib.compress(bytes(34))) + t["iend"],
        "tRNS of 3 bytes for grey": S + g["ihdr"] + ref.chunk(b"tRNS", bytes(3)) + g["idat"] + g["iend"],
        "tRNS of 2 bytes for truecolour": S + t["ihdr"] + ref.chunk(b"tRNS", bytes(2)) + t["idat"] + t["iend"],
        "tRNS of 257 alphas": S + p["ihdr"] + p["plte"] + ref.chunk(b"tRNS", bytes(257)) + p["idat"] + p["iend"],
        "tRNS twice": S + t["ihdr"] + ref.chunk(b"tRNS", bytes(6)) + ref.chunk(b"tRNS", bytes(6)) + t["idat"] + t["iend"],
        "IDATs apart": S + t["ihdr"] + ref.chunk(b"IDAT", z[:5]) + t["text"] + ref.chunk(b"IDAT", z[5:]) + t["iend"],
        "no IDAT": S + t["ihdr"] + t["iend"],
        "IEND with a body": S + t["ihdr"] + t["idat"] + ref.chunk(b"IEND", b"x"),
        "no IEND": S + t["ihdr"] + t["idat"],
        "ends inside a chunk": (S + t["ihdr"] + t["idat"] + t["iend"])[:-3],
        "a chunk longer than the file": S + t["ihdr"] + struct.pack(">I", 1000) + b"IDAT" + z,
        "a chunk length above 2^31": S + t["ihdr"] + struct.pack(">I", 0x80000000) + b"IDAT" + z,
    }
    return out


def legal_files():
    t, p = _parts(2), _parts(3)
    S = ref.SIG
    z = t["idat"][8:-4]
    return {
        "plain": S + t["ihdr"] + t["idat"] + t["iend"],
        "ancillary chunks everywhere": S + t["ihdr"] + t["text"] + t["idat"] + t["text"] + t["iend"],
        "a suggested palette in a truecolour file": S + t["ihdr"] + t["plte"] + ref.chunk(b"tRNS", bytes(6)) + t["idat"] + t["iend"],
        "IDATs of one byte": S + t["ihdr"] + b"".join(ref.chunk(b"IDAT", z[i:i + 1]) for i in range(len(z))) + t["iend"],
        "an empty IDAT": S + t["ihdr"] + ref.chunk(b"IDAT", b"") + t["idat"] + t["iend"],
        "tRNS longer than PLTE": S + p["ihdr"] + p["plte"] + ref.chunk(b"tRNS", bytes(9)) + p["idat"] + p["iend"],
        "bytes behind IEND": S + t["ihdr"] + t["idat"] + t["iend"] + b"trailing",
    }


@pytest.mark.parametrize("name", sorted(damaged_files()))
def test_damaged_files_are_refused(lib, name):
    data = damaged_files()[name]
    rc, _ = config_rc(lib, data)
    assert rc == FNX_ERR_INVALID, name
    assert b"PNG" in lib.fnx_last_error()
    with pytest.raises(ref.Damaged):
        ref.parse(data)


@pytest.mark.parametrize("name", sorted(legal_files()))
def test_legal_files_pass(lib, name):
    data = legal_files()[name]
    assert config_rc(lib, data) == (FNX_OK, (4, 2)), name
    assert ref.decode(data).shape == (2, 4, 4)
