"""inflate_probe against zlib, without a GPU: on streams zlib made the probe returns the input, the block forms zlib's
settings imply and tokens that expand to the input; every fault a strict inflater refuses is injected into a valid stream
and must raise; the cost helpers are held against small cases worked by hand and against each other."""
from __future__ import annotations

import zlib

import numpy as np
import pytest

import inflate_probe as ip
import png_filter_ref as ref


def image_stream() -> bytes:
    return np.ascontiguousarray(ref.png_stream(ref.smooth_rgba(96, 40, 3, opaque=True), ref.NRGBA)[0]).tobytes()


CONTENTS = {
    "empty": b"",
    "one_byte": b"\x5a",
    "noise": np.random.default_rng(1).integers(0, 256, size=70001, dtype=np.uint8).tobytes(),
    "constant": b"\x33" * 70001,
    "text": b"the quick brown fox jumps over the lazy dog; " * 300,
    "image": image_stream(),
}
SETTINGS = {
    "level0": (0, zlib.Z_DEFAULT_STRATEGY), "level1": (1, zlib.Z_DEFAULT_STRATEGY), "level6": (6, zlib.Z_DEFAULT_STRATEGY),
    "level9": (9, zlib.Z_DEFAULT_STRATEGY), "fixed": (6, zlib.Z_FIXED), "huffman_only": (6, zlib.Z_HUFFMAN_ONLY),
}


def compress(data: bytes, level: int, strategy: int, flush_every: int = 0) -> bytes:
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    if not flush_every:
        return co.compress(data) + co.flush()
    parts = []
    for i in range(0, len(data), flush_every):
        parts += [co.compress(data[i:i + flush_every]), co.flush(zlib.Z_FULL_FLUSH)]
    return b"".join(parts) + co.flush()


def check_blocks(p: ip.Probe, data: bytes):
    assert p.out == data
    assert [b.bfinal for b in p.blocks] == [0] * (len(p.blocks) - 1) + [1]
    at = 0
    for b in p.blocks:
        assert b.out_start == at and b.bit_start < b.bit_end
        if b.btype == ip.STORED:
            assert b.tokens == [] and b.bit_end % 8 == 0
        else:
            assert ip.expand(b.tokens, data[:at]) == b.out, "the tokens re-expand to the block's bytes"
        if b.btype == ip.DYNAMIC:
            assert len(b.ll_lengths) == b.hlit and len(b.d_lengths) == b.hdist and len(b.cl_lengths) == 19
            assert sum(1 if e is None else {16: 3, 17: 3, 18: 11}[s] + e for s, e in b.cl_seq) == b.hlit + b.hdist
        at += len(b.out)
    assert at == len(data)
    assert p.adler == zlib.adler32(data)


@pytest.mark.parametrize("content", sorted(CONTENTS))
@pytest.mark.parametrize("setting", sorted(SETTINGS))
def test_reads_what_zlib_wrote(content, setting):
    data = CONTENTS[content]
    level, strategy = SETTINGS[setting]
    stream = compress(data, level, strategy)
    assert zlib.decompress(stream) == data
    p = ip.probe(stream)
    check_blocks(p, data)
    assert p.cmf == 0x78 and (p.cmf * 256 + p.flg) % 31 == 0
    types = {b.btype for b in p.blocks}
    if setting == "level0":
        assert types == {ip.STORED}
        assert sum(len(b.out) for b in p.blocks) == len(data)
    elif setting == "fixed":
        # Z_FIXED rules the dynamic codes out, not the stored form, which zlib still takes for what does not compress
        assert types == ({ip.STORED} if content == "noise" else {ip.FIXED})
    elif setting == "huffman_only":
        assert all(not isinstance(t, tuple) for b in p.blocks for t in b.tokens), "Z_HUFFMAN_ONLY writes no match"
    if content == "constant" and setting in ("level1", "level6", "level9", "fixed"):
        assert any(isinstance(t, tuple) and t[1] == 1 and t[0] == 258 for b in p.blocks for t in b.tokens)
    if content == "noise":
        assert types == {ip.STORED}


def test_full_flush_every_32k():
    data = CONTENTS["image"] * 9 + CONTENTS["text"]
    assert len(data) > 3 * 32768
    stream = compress(data, 6, zlib.Z_DEFAULT_STRATEGY, 32768)
    p = ip.probe(stream)
    check_blocks(p, data)
    # a full flush ends in an empty stored block and the next block's matches stay behind it
    empties = [i for i, b in enumerate(p.blocks) if b.btype == ip.STORED and not b.out]
    assert len(empties) == -(-len(data) // 32768)
    for i in empties:
        assert p.blocks[i].bit_end % 8 == 0 and p.blocks[i].pad == 0
        flushed_at = p.blocks[i].out_start
        assert flushed_at % 32768 == 0 or flushed_at == len(data)
        for b in p.blocks[i + 1:]:
            for t in b.tokens:
                if isinstance(t, tuple) and t[2] >= flushed_at:
                    assert t[2] - t[1] >= flushed_at
            break


# ---- damaged streams --------------------------------------------------------------------------------------------------------
class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v: int, n: int):                                    # least significant bit first
        self.bits += [(v >> i) & 1 for i in range(n)]
        return self

    def code(self, v: int, n: int):                                   # a Huffman code: most significant bit first
        self.bits += [(v >> (n - 1 - i)) & 1 for i in range(n)]
        return self

    def align(self):
        self.bits += [0] * (-len(self.bits) % 8)
        return self

    def bytes(self) -> bytes:
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(sum(b[i + k] << k for k in range(8)) for i in range(0, len(b), 8))


def zstream(w: BitWriter, out: bytes) -> bytes:
    return b"\x78\x01" + w.bytes() + zlib.adler32(out).to_bytes(4, "big")


def fixed_literal(w: BitWriter, b: int):
    return w.code(0x30 + b, 8) if b < 144 else w.code(0x190 + b - 144, 9)


def fixed_symbol(w: BitWriter, s: int):                               # 256..287
    return w.code(s - 256, 7) if s < 280 else w.code(0xc0 + s - 280, 8)


def dynamic_header(w: BitWriter, cl: dict, nll: int, nd: int):
    """BFINAL = 1, BTYPE = 2, and the code-length code's lengths given as {symbol: length}"""
    last = max(i for i, s in enumerate(ip.CLORD) if cl.get(s, 0)) + 1
    hclen = max(4, last)
    w.put(1, 1).put(2, 2).put(nll - 257, 5).put(nd - 1, 5).put(hclen - 4, 4)
    for i in range(hclen):
        w.put(cl.get(ip.CLORD[i], 0), 3)
    return w


def both(stream: bytes):
    """(the probe's verdict, zlib's) on a stream"""
    try:
        ip.probe(stream)
        mine = True
    except ip.InflateError:
        mine = False
    try:
        d = zlib.decompressobj()
        d.decompress(stream)
        theirs = d.eof and not d.unused_data
    except zlib.error:
        theirs = False
    return mine, theirs


def test_hand_made_streams_are_read():
    """the writer of the damaged streams below is itself right: zlib and the probe read what it writes"""
    w = BitWriter().put(1, 1).put(1, 2)
    for b in b"abc":
        fixed_literal(w, b)
    fixed_symbol(w, 257).code(2, 5)                                   # length 3, distance 3
    fixed_literal(w, 200)
    fixed_symbol(w, 256)
    s = zstream(w, b"abcabc\xc8")
    assert zlib.decompress(s) == b"abcabc\xc8"
    p = ip.probe(s)
    assert p.out == b"abcabc\xc8" and p.blocks[0].tokens == [97, 98, 99, (3, 3, 3), 200] and p.blocks[0].btype == ip.FIXED
    # dynamic: code-length code {1: 1 bit, 18: 1 bit}; literals 'a' and 256 of one bit, one distance code of one bit (incomplete: allowed)
    w = dynamic_header(BitWriter(), {1: 1, 18: 1}, 257, 1)
    w.code(1, 1).put(97 - 11, 7).code(0, 1).code(1, 1).put(138 - 11, 7).code(1, 1).put(256 - 98 - 138 - 11, 7).code(0, 1).code(0, 1)
    w.code(0, 1).code(0, 1).code(1, 1)                                # a a end
    s = zstream(w, b"aa")
    assert zlib.decompress(s) == b"aa"
    p = ip.probe(s)
    b = p.blocks[0]
    assert p.out == b"aa" and b.btype == ip.DYNAMIC and (b.hlit, b.hdist, b.hclen) == (257, 1, 18)
    assert b.cl_seq == [(18, 86), (1, None), (18, 127), (18, 9), (1, None), (1, None)]
    assert b.ll_lengths[97] == 1 and b.ll_lengths[256] == 1 and sum(b.ll_lengths) == 2 and b.d_lengths == (1,)
    assert b.cl_lengths[1] == 1 and b.cl_lengths[18] == 1 and sum(b.cl_lengths) == 2


def damaged():
    good = compress(CONTENTS["text"], 6, zlib.Z_DEFAULT_STRATEGY)
    stored = compress(b"hello, stored block", 0, zlib.Z_DEFAULT_STRATEGY)
    cases = {}
    cases["reserved_btype"] = zstream(BitWriter().put(1, 1).put(3, 2), b"")
    s = bytearray(stored)
    s[5] ^= 0x10                                                      # 78 01 | 01 | LEN LEN | NLEN NLEN
    cases["len_nlen"] = bytes(s)
    cases["oversubscribed_code_length_code"] = zstream(dynamic_header(BitWriter(), {0: 1, 1: 1, 2: 1}, 257, 1).put(0, 64), b"")
    cases["incomplete_code_length_code"] = zstream(dynamic_header(BitWriter(), {1: 1}, 257, 1).put(0, 64), b"")
    # literal/length lengths through the code {0: 1 bit (code 0), 1: 2 bits (10), 2: 3 bits (110), 18: 3 bits (111)}
    def ll_block(l97, l98, l256):
        w = dynamic_header(BitWriter(), {0: 1, 1: 2, 2: 3, 18: 3}, 257, 1)
        sym = {0: (0, 1), 1: (2, 2), 2: (6, 3)}
        w.code(7, 3).put(97 - 11, 7).code(*sym[l97]).code(*sym[l98])
        w.code(7, 3).put(138 - 11, 7).code(7, 3).put(256 - 99 - 138 - 11, 7).code(*sym[l256]).code(*sym[1])
        return w
    cases["oversubscribed_literal_code"] = zstream(ll_block(1, 1, 1).put(0, 32), b"")
    cases["incomplete_literal_code"] = zstream(ll_block(2, 0, 2).code(1, 2), b"")
    cases["no_end_of_block_code"] = zstream(ll_block(1, 1, 0).code(0, 1), b"a")
    cases["repeat_at_the_start"] = zstream(dynamic_header(BitWriter(), {16: 1, 1: 1}, 257, 1).code(0, 1).put(0, 2).put(0, 64), b"")
    cases["run_past_the_lengths"] = zstream(dynamic_header(BitWriter(), {18: 1, 1: 1}, 257, 1).code(0, 1).put(127, 7).code(0, 1).put(127, 7).put(0, 64), b"")
    for s in (286, 287):
        w = fixed_literal(BitWriter().put(1, 1).put(1, 2), 97)
        fixed_symbol(fixed_symbol(w, s).code(0, 5), 256)
        cases[f"length_symbol_{s}"] = zstream(w, b"aaaa")
    for s in (30, 31):
        w = fixed_literal(BitWriter().put(1, 1).put(1, 2), 97)
        fixed_symbol(fixed_symbol(w, 257).code(s, 5), 256)
        cases[f"distance_symbol_{s}"] = zstream(w, b"aaaa")
    w = fixed_literal(BitWriter().put(1, 1).put(1, 2), 97)
    fixed_symbol(fixed_symbol(w, 257).code(1, 5), 256)                # distance 2 behind one byte
    cases["distance_too_far"] = zstream(w, b"aaaa")
    w = fixed_literal(BitWriter().put(1, 1).put(1, 2), 97)
    cases["missing_end_of_block"] = b"\x78\x01" + w.bytes()
    cases["no_final_block"] = b"\x78\x01" + fixed_symbol(BitWriter().put(0, 1).put(1, 2), 256).bytes() + zlib.adler32(b"").to_bytes(4, "big")
    cases["truncated"] = good[:len(good) // 2]
    cases["check_cut_short"] = good[:-1]
    s = bytearray(good)
    s[-1] ^= 1
    cases["wrong_adler"] = bytes(s)
    cases["trailing_byte"] = good + b"\x00"
    cases["header_check"] = b"\x78\x02" + good[2:]
    cases["preset_dictionary"] = b"\x78\x20" + good[2:]
    cases["not_deflate"] = b"\x79\x00"[:1] + bytes([(31 - (0x79 * 256) % 31) % 31]) + good[2:]
    return cases


DAMAGED = damaged()


@pytest.mark.parametrize("fault", sorted(DAMAGED))
def test_damaged_streams_are_refused(fault):
    mine, theirs = both(DAMAGED[fault])
    assert not theirs, "zlib accepts this stream: the test's own construction is wrong"
    assert not mine
    with pytest.raises(ip.InflateError):
        ip.probe(DAMAGED[fault])


def test_every_bit_flip_agrees_with_zlib():
    """each single-bit flip of a small dynamic-block stream: refused by both or read the same by both"""
    rng = np.random.default_rng(8)
    data = rng.choice(np.arange(7, dtype=np.uint8), size=260, p=[.4, .25, .15, .1, .05, .03, .02]).tobytes() + b"abracadabra " * 3
    good = compress(data, 9, zlib.Z_DEFAULT_STRATEGY)
    assert ip.probe(good).blocks[0].btype == ip.DYNAMIC
    refused = 0
    for bit in range(8 * len(good)):
        s = bytearray(good)
        s[bit >> 3] ^= 1 << (bit & 7)
        mine, theirs = both(bytes(s))
        assert mine == theirs, f"bit {bit}: probe {mine}, zlib {theirs}"
        refused += not mine
    assert refused > 8 * len(good) - 16


# ---- the cost helpers -------------------------------------------------------------------------------------------------------
def test_huffman_depth_and_cost():
    assert ip.huffman([]) == (0, 0) and ip.huffman([0, 7, 0]) == (1, 7)
    assert ip.huffman([1, 1]) == (1, 2)
    assert ip.huffman([1, 1, 2, 4]) == (3, 1 * 3 + 1 * 3 + 2 * 2 + 4 * 1)
    assert ip.huffman([1, 1, 1, 1]) == (2, 8), "ties go to the shallower tree"
    fib = [1, 1]
    while len(fib) < 21:
        fib.append(fib[-1] + fib[-2])
    depth, cost = ip.huffman(fib)
    assert depth == 20 and cost == sum(c * min(21 - i, 20) for i, c in enumerate(fib))
    # zlib's own dynamic blocks are Huffman-optimal whenever the depth fits
    p = ip.probe(compress(CONTENTS["image"], 6, zlib.Z_DEFAULT_STRATEGY))
    seen = 0
    for b in p.blocks:
        if b.btype != ip.DYNAMIC:
            continue
        ll, d = ip.histograms(b.tokens)
        for hist, lens, limit in ((ll, b.ll_lengths, 15), (d, b.d_lengths, 15)):
            depth, cost = ip.huffman(hist)
            if depth <= limit and sum(1 for c in hist if c) > 1:
                assert ip.code_cost(hist, lens + (0,) * 300) == cost
                seen += 1
    assert seen >= 2


def test_limited_cost():
    rng = np.random.default_rng(4)
    for _ in range(60):
        hist = [int(v) for v in rng.integers(0, 50, size=int(rng.integers(2, 40)))] + [1, 1]
        depth, cost = ip.huffman(hist)
        assert ip.limited_cost(hist, max(depth, 6)) == cost, "a limit the Huffman code meets costs nothing"
        n = sum(1 for c in hist if c)
        low = max(1, (n - 1).bit_length())
        costs = [ip.limited_cost(hist, L) for L in range(low, depth + 1)]
        assert all(a >= b for a, b in zip(costs, costs[1:])) and costs[-1] == cost
        if n == 1 << low:
            assert costs[0] == low * sum(hist), "a full tree: every code has the limit's length"
    fib = [1, 1, 2, 3, 5, 8, 13, 21]                                  # depth 7
    assert ip.huffman(fib) == (7, sum(c * min(8 - i, 7) for i, c in enumerate(fib)))
    assert ip.limited_cost(fib, 3) == 3 * sum(fib)
    # limit 4 by hand: the optimum is lengths 4 4 4 4 3 3 2 1?  Kraft 4/16 + 2/8 + 1/4 + 1/2 > 1; brute force instead
    best = None
    import itertools
    for lens in itertools.product(range(1, 5), repeat=8):
        if sum(2 ** -l for l in lens) <= 1:
            c = sum(a * b for a, b in zip(sorted(fib, reverse=True), sorted(lens)))
            best = c if best is None or c < best else best
    assert ip.limited_cost(fib, 4) == best


def test_fixed_cost_and_symbols():
    assert [ip.length_symbol(l) for l in (3, 10, 11, 12, 13, 257, 258)] == [257, 264, 265, 265, 266, 284, 285]
    assert [ip.distance_symbol(d) for d in (1, 4, 5, 6, 7, 4096, 4097, 8192, 8193, 12289, 16385, 24577, 32768)] == \
        [0, 3, 4, 4, 5, 23, 24, 25, 26, 27, 28, 29, 29]
    for content in ("text", "image", "constant"):
        stream = compress(CONTENTS[content], 6, zlib.Z_FIXED)
        for b in ip.probe(stream).blocks:
            assert ip.fixed_cost(b.tokens) == b.bit_end - b.bit_start
