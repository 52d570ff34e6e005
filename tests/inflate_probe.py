"""A plain reader of zlib streams (RFC 1950) of deflate blocks (RFC 1951) that keeps what an inflater throws away: where
every block starts and ends, which form it took, the code lengths it sent and how it sent them, and its tokens.  Written
from the two RFCs; it shares nothing with the encoder it judges and uses zlib for adler32 alone.

probe(stream) -> Probe: header bytes, the Adler-32 check, the blocks, the output.  It raises InflateError on everything a
strict inflater refuses (the list is in probe's docstring).  Beside it: the cost helpers the tests hold a block's size
against -- the Huffman optimum and depth of a histogram, the optimum under a length limit (package-merge), the cost of a
token list in the fixed codes."""
from __future__ import annotations

import heapq
import zlib
from dataclasses import dataclass, field

CLORD = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)          # RFC 1951, 3.2.7
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
             8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)
FIXED_LL = (8,) * 144 + (9,) * 112 + (7,) * 24 + (8,) * 8                           # 3.2.6: 288 lengths
FIXED_D = (5,) * 32
STORED, FIXED, DYNAMIC = 0, 1, 2


class InflateError(ValueError):
    pass


@dataclass
class Block:
    bfinal: int
    btype: int
    bit_start: int                       # of BFINAL
    bit_end: int = 0                     # one past the block's last bit (a stored block's last byte)
    out_start: int = 0                   # offset of the block's first output byte in the stream's output
    out: bytes = b""
    tokens: list = field(default_factory=list)      # a literal: int; a match: (length, distance, output offset of its first byte)
    pad: int = 0                         # stored: the bits between the header and LEN, as a number
    hlit: int = 0                        # dynamic only, from here on
    hdist: int = 0
    hclen: int = 0
    cl_lengths: tuple = ()               # 19, by symbol
    cl_seq: list = field(default_factory=list)      # (symbol, extra value or None)
    ll_lengths: tuple = ()               # hlit
    d_lengths: tuple = ()                # hdist


@dataclass
class Probe:
    cmf: int
    flg: int
    adler: int
    blocks: list
    out: bytes
    tail_pad: int                        # the bits between the last block and the check, as a number
    tail_pad_bits: int


class _Bits:
    def __init__(self, data: bytes, pos: int):
        self.d, self.pos, self.end = data, pos, 8 * len(data)

    def bit(self) -> int:
        p = self.pos
        if p >= self.end:
            raise InflateError("the stream ends inside a block")
        self.pos = p + 1
        return (self.d[p >> 3] >> (p & 7)) & 1

    def bits(self, n: int) -> int:
        p = self.pos
        if p + n > self.end:
            raise InflateError("the stream ends inside a block")
        v = 0
        for i in range(n):                                            # least significant bit first
            v |= ((self.d[(p + i) >> 3] >> ((p + i) & 7)) & 1) << i
        self.pos = p + n
        return v


class _Code:
    """a canonical Huffman code from its lengths (3.2.2): count per length and the symbols in code order"""

    def __init__(self, lengths, what: str, may_be_single: bool):
        self.what = what
        self.count = [0] * 16
        for l in lengths:
            self.count[l] += 1
        self.count[0] = 0
        left = 1
        for l in range(1, 16):
            left = 2 * left - self.count[l]
            if left < 0:
                raise InflateError(f"over-subscribed {what} code")
        used = sum(self.count)
        if left > 0:
            # zlib's exceptions: no code at all (using it is the error), or a single code of one bit -- never for the code-length code
            if not (may_be_single and (used == 0 or (used == 1 and self.count[1] == 1))):
                raise InflateError(f"incomplete {what} code")
        offs = [0] * 17
        for l in range(1, 16):
            offs[l + 1] = offs[l] + self.count[l]
        self.symbol = [0] * used
        for s, l in enumerate(lengths):
            if l:
                self.symbol[offs[l]] = s
                offs[l] += 1

    def read(self, br: _Bits) -> int:
        code = first = index = 0
        count = self.count
        for l in range(1, 16):
            code |= br.bit()                                          # Huffman codes arrive most significant bit first
            c = count[l]
            if code - c < first:
                return self.symbol[index + (code - first)]
            index += c
            first = (first + c) << 1
            code <<= 1
        raise InflateError(f"a bit pattern that is no {self.what} code")


_FIXED_LL_CODE = _Code(FIXED_LL, "fixed literal/length", False)
_FIXED_D_CODE = _Code(FIXED_D, "fixed distance", False)


def _read_dynamic(br: _Bits, b: Block):
    b.hlit, b.hdist, b.hclen = br.bits(5) + 257, br.bits(5) + 1, br.bits(4) + 4
    if b.hlit > 286 or b.hdist > 30:
        raise InflateError(f"HLIT {b.hlit} / HDIST {b.hdist}: too many symbols")
    cl = [0] * 19
    for i in range(b.hclen):
        cl[CLORD[i]] = br.bits(3)
    b.cl_lengths = tuple(cl)
    clc = _Code(cl, "code-length", False)
    lens: list = []
    total = b.hlit + b.hdist
    while len(lens) < total:
        s = clc.read(br)
        if s < 16:
            b.cl_seq.append((s, None))
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise InflateError("a repeat with no length before it")
            e = br.bits(2)
            run, v = 3 + e, lens[-1]
        elif s == 17:
            e = br.bits(3)
            run, v = 3 + e, 0
        else:
            e = br.bits(7)
            run, v = 11 + e, 0
        b.cl_seq.append((s, e))
        if len(lens) + run > total:
            raise InflateError("a run of code lengths past HLIT + HDIST")
        lens.extend([v] * run)
    b.ll_lengths, b.d_lengths = tuple(lens[:b.hlit]), tuple(lens[b.hlit:])
    if b.ll_lengths[256] == 0:
        raise InflateError("no end-of-block code")
    return _Code(b.ll_lengths, "literal/length", True), _Code(b.d_lengths, "distance", True)


def probe(stream: bytes) -> Probe:
    """Raises InflateError on: a header that is not deflate with a window of at most 32 KiB, a wrong header check or a preset
    dictionary; BTYPE 3; LEN != ~NLEN; an over-subscribed code; an incomplete code other than a literal/length or distance
    code with no code or a single one-bit code; a repeat with nothing before it or a run past the lengths; no code for the
    end-of-block; a bit pattern outside a code; literal/length symbols 286, 287 or distance symbols 30, 31; a distance beyond
    the output so far; a stream that ends before its last block or check does; a wrong Adler-32; bytes behind the check."""
    stream = bytes(stream)
    if len(stream) < 2:
        raise InflateError("no zlib header")
    cmf, flg = stream[0], stream[1]
    if cmf & 15 != 8 or cmf >> 4 > 7:
        raise InflateError(f"CMF {cmf:#x}: not deflate with a window of at most 32 KiB")
    if (cmf * 256 + flg) % 31:
        raise InflateError("the header check fails")
    if flg & 0x20:
        raise InflateError("a preset dictionary")
    br = _Bits(stream, 16)
    out = bytearray()
    blocks = []
    while True:
        b = Block(bfinal=0, btype=0, bit_start=br.pos, out_start=len(out))
        b.bfinal, b.btype = br.bit(), br.bits(2)
        if b.btype == 3:
            raise InflateError("reserved BTYPE 3")
        if b.btype == STORED:
            npad = -br.pos % 8
            b.pad = br.bits(npad)
            n, nn = br.bits(16), br.bits(16)
            if n != nn ^ 0xffff:
                raise InflateError(f"LEN {n:#x} is not the complement of NLEN {nn:#x}")
            at = br.pos >> 3
            if at + n > len(stream):
                raise InflateError("the stream ends inside a stored block")
            out += stream[at:at + n]
            br.pos += 8 * n
        else:
            llc, dc = (_FIXED_LL_CODE, _FIXED_D_CODE) if b.btype == FIXED else _read_dynamic(br, b)
            tokens = b.tokens
            while True:
                s = llc.read(br)
                if s < 256:
                    tokens.append(s)
                    out.append(s)
                    continue
                if s == 256:
                    break
                if s > 285:
                    raise InflateError(f"literal/length symbol {s}")
                length = LEN_BASE[s - 257] + br.bits(LEN_EXTRA[s - 257])
                ds = dc.read(br)
                if ds > 29:
                    raise InflateError(f"distance symbol {ds}")
                dist = DIST_BASE[ds] + br.bits(DIST_EXTRA[ds])
                at = len(out)
                if dist > at:
                    raise InflateError(f"distance {dist} with {at} bytes of output")
                tokens.append((length, dist, at))
                if dist >= length:
                    out += out[at - dist:at - dist + length]
                else:
                    for i in range(length):
                        out.append(out[at - dist + i])
        b.bit_end = br.pos
        b.out = bytes(out[b.out_start:])
        blocks.append(b)
        if b.bfinal:
            break
    npad = -br.pos % 8
    tail_pad = br.bits(npad)
    at = br.pos >> 3
    if at + 4 > len(stream):
        raise InflateError("the stream ends before its check does")
    adler = int.from_bytes(stream[at:at + 4], "big")
    if adler != zlib.adler32(bytes(out)):
        raise InflateError(f"Adler-32 {adler:#010x}, the output's is {zlib.adler32(bytes(out)):#010x}")
    if at + 4 != len(stream):
        raise InflateError(f"{len(stream) - at - 4} bytes behind the check")
    return Probe(cmf, flg, adler, blocks, bytes(out), tail_pad, npad)


def expand(tokens, before: bytes = b"") -> bytes:
    """the bytes a token list stands for, behind `before` (match offsets count from the start of `before`)"""
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, tuple):
            length, dist, at = t
            assert at == len(out) and dist <= at
            for i in range(length):
                out.append(out[at - dist + i])
        else:
            out.append(t)
    return bytes(out[len(before):])


# ---- symbols and costs ------------------------------------------------------------------------------------------------------
def length_symbol(length: int) -> int:
    s = 28
    while LEN_BASE[s] > length:
        s -= 1
    return 257 + s


def distance_symbol(dist: int) -> int:
    s = 29
    while DIST_BASE[s] > dist:
        s -= 1
    return s


def histograms(tokens):
    """(literal/length counts[286] with the end-of-block, distance counts[30]) of a block's tokens"""
    ll, d = [0] * 286, [0] * 30
    ll[256] = 1
    for t in tokens:
        if isinstance(t, tuple):
            ll[length_symbol(t[0])] += 1
            d[distance_symbol(t[1])] += 1
        else:
            ll[t] += 1
    return ll, d


def extra_bits(tokens) -> int:
    return sum(LEN_EXTRA[length_symbol(t[0]) - 257] + DIST_EXTRA[distance_symbol(t[1])] for t in tokens if isinstance(t, tuple))


def fixed_cost(tokens) -> int:
    """bits of a fixed-code block of these tokens: header, tokens, end-of-block"""
    ll, d = histograms(tokens)
    return 3 + sum(c * FIXED_LL[s] for s, c in enumerate(ll)) + 5 * sum(d) + extra_bits(tokens)


def huffman(hist):
    """(depth, cost) of an unconstrained Huffman code of the non-zero counts: cost = sum count * length, the optimum of any
    prefix code; depth = the longest code when ties go to the shallower subtree, the least depth an optimal code can have.
    One symbol takes one bit; none: (0, 0)."""
    w = [c for c in hist if c]
    if len(w) < 2:
        return len(w), sum(w)
    heap = [(c, 0) for c in w]
    heapq.heapify(heap)
    cost = 0
    while len(heap) > 1:
        a, ha = heapq.heappop(heap)
        b, hb = heapq.heappop(heap)
        cost += a + b
        heapq.heappush(heap, (a + b, max(ha, hb) + 1))
    return heap[0][1], cost


def limited_cost(hist, limit: int) -> int:
    """the least sum count * length of a prefix code whose lengths are at most `limit` (package-merge, Larmore and Hirschberg)"""
    w = sorted(c for c in hist if c)
    n = len(w)
    if n < 2:
        return sum(w)
    if n > 1 << limit:
        raise ValueError(f"{n} symbols do not fit {limit} bits")
    merged = list(w)
    for _ in range(limit - 1):
        packages = [merged[i] + merged[i + 1] for i in range(0, len(merged) - 1, 2)]
        merged = sorted(w + packages)
    return sum(merged[:2 * n - 2])


def code_cost(hist, lengths) -> int:
    return sum(c * lengths[s] for s, c in enumerate(hist) if c)


def kraft(lengths) -> tuple:
    """(sum of 2^(15 - length) over the codes, 2^15): equal when the code is complete"""
    return sum(1 << (15 - l) for l in lengths if l), 1 << 15
