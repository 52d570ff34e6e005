"""A coefficient-level baseline JPEG writer for the tests of the device Huffman decoder (jpeg_dec.hip), and a plain state
walker over the strings it writes.  No DCT, no Pillow, no scipy: the caller chooses the quantised coefficients, the Huffman
tables (as a DHT segment states them: sixteen counts and the values, codes assigned canonically), the sampling, the
quantisation tables and the restart interval, and gets back the file together with a map of every symbol it coded -- where it
starts in the string WITHOUT stuffing, how long its code and its value are, and the decoder state (z, slot) in front of it --
so that a test can prove which bit a symbol landed on instead of hoping for it.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

ZIG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
       57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

SPAN = 1024                      # bits of the string per lane (jpeg_dec_span.inc: DEC_SPAN)
OWN, WARM = 240, 16              # spans a workgroup of the first sync launch owns / decodes ahead of them (DEC_OWN, DEC_WARM)

SYM = np.dtype([("start", np.int64), ("clen", np.uint8), ("size", np.uint8), ("z", np.uint8), ("slot", np.uint8), ("sym", np.uint8),
                ("tab", np.uint8), ("blk", np.int32)])


class Table:
    """One Huffman table as a DHT segment holds it: bits[L - 1] codes of length L, the values in code order."""

    def __init__(self, bits, values):
        bits, values = [int(b) for b in bits], [int(v) for v in values]
        assert len(bits) == 16 and sum(bits) == len(values) <= 256 and len(set(values)) == len(values)
        self.bits, self.values, self.codes = bits, values, {}
        code, k = 0, 0
        for ln in range(1, 17):
            for _ in range(bits[ln - 1]):
                if code + 1 >= (1 << ln):
                    raise ValueError(f"the all-ones code of length {ln} would be assigned (such a table goes to the host route)")
                self.codes[values[k]] = (code, ln)
                code += 1
                k += 1
            code <<= 1
        self._lut = None

    def segment(self, tc, th):
        return bytes([(tc << 4) | th] + self.bits + self.values)

    def lut(self):
        """by the next 16 bits of the string: code length << 8 | symbol; 0: no code of this table starts so"""
        if self._lut is None:
            lut = np.zeros(1 << 16, np.int32)
            for sym, (code, ln) in self.codes.items():
                lut[code << (16 - ln):(code + 1) << (16 - ln)] = (ln << 8) | sym
            self._lut = lut.tolist()
        return self._lut


def _amp(v):
    n = int(abs(v)).bit_length()
    return n, (v if v >= 0 else v + (1 << n) - 1)


def _pack(vals, lens, nbytes):
    """fields of <= 32 bits each, laid end to end from bit 0 (the most significant bit of byte 0)"""
    vals, lens = np.asarray(vals, np.uint64), np.asarray(lens, np.int64)
    assert (lens <= 32).all()
    start = np.concatenate([[0], np.cumsum(lens)[:-1]]) if len(lens) else np.zeros(0, np.int64)
    w, off = start >> 5, start & 31
    v64 = vals << (64 - off - lens).astype(np.uint64)
    words = np.zeros(int(nbytes + 3) // 4 + 2, np.uint64)
    np.add.at(words, w, v64 >> np.uint64(32))                # (fields never overlap: adding is or-ing)
    np.add.at(words, w + 1, v64 & np.uint64(0xffffffff))
    return words.astype(">u4").tobytes()[:nbytes]


class Crafted:
    """data: the file.  coef: (blocks, 64) int16 as coded, zig-zag order, blocks in scan order, the DC absolute (what the
    oracle's decoder returns); dcdiff: the DC differences that were coded.  sym: the symbol map (SYM), start bits in the string
    without stuffing.  string: that string's bytes (padding included); rst: the byte offsets in it at which intervals 1, 2, ...
    start; nslots, dc_of_slot, ac_of_slot: the MCU's layout and the Table of every slot."""


def encode(coef, w, h, dc_tabs, ac_tabs, sampling=None, qtabs=None, restart=0, comp_tabs=None, tile=1, extra=None, cut=None, header_tabs=None,
           max_ac_size=10):
    """coef: (blocks, 64) quantised coefficients, zig-zag order, blocks in scan order, DC absolute.  dc_tabs / ac_tabs: one or two
    Tables (ids 0, 1).  sampling: None for one component, or the luminance factors (hy, vy) of a three-component file.
    qtabs: one or two lists of 64 (zig-zag order, as a DQT segment holds them); default: all ones.  restart: MCUs per interval.
    comp_tabs: per component (dc id, ac id); default: table 0 for Y, the last table given for Cb and Cr.
    tile: the blocks given are one period of a scan that repeats it `tile` times -- the period must be whole bytes, none of
    them 0xff, and end with every DC at 0, so that the bytes simply repeat (for scans too long to write symbol by symbol);
    sym then maps the first period, coef and string are the whole scan's.
    extra: {interval: bytes} put behind that interval's padding, in front of its marker (a DAMAGED file: data the image does
    not have); cut: {interval: n} instead removes the last n bytes in front of the marker.
    header_tabs: (dc_tabs, ac_tabs) the DHT segments state where they are NOT the tables the scan was coded with (damaged too).
    max_ac_size: the largest AC size coded, up to 15 (baseline files of 8-bit images stay within 10; image/jpeg reads them all)."""
    coef = np.asarray(coef)
    assert coef.ndim == 2 and coef.shape[1] == 64
    ncomp = 1 if sampling is None else 3
    hy, vy = (1, 1) if sampling is None else sampling
    assert hy in (1, 2, 4) and vy in (1, 2)
    mx, my = (w + 8 * hy - 1) // (8 * hy), (h + 8 * vy - 1) // (8 * vy)
    ny = hy * vy
    nslots = ny + ncomp - 1
    assert coef.shape[0] * tile == mx * my * nslots, (coef.shape, tile, mx, my, nslots)
    assert tile == 1 or (restart == 0 and coef.shape[0] % nslots == 0)
    dc_tabs, ac_tabs = list(dc_tabs), list(ac_tabs)
    if comp_tabs is None:
        comp_tabs = [(0, 0)] + [(len(dc_tabs) - 1, len(ac_tabs) - 1)] * (ncomp - 1)
    qtabs = [list(q) for q in (qtabs or [[1] * 64])]
    comp_of_slot = [0 if s < ny else s - ny + 1 for s in range(nslots)]
    dc_of_slot = [dc_tabs[comp_tabs[c][0]] for c in comp_of_slot]
    ac_of_slot = [ac_tabs[comp_tabs[c][1]] for c in comp_of_slot]
    tab_of_slot = [(comp_tabs[c][0], 2 + comp_tabs[c][1]) for c in comp_of_slot]

    vals, lens, syms = [], [], []
    intervals = [0]                   # index into vals/lens at which every interval starts
    pos = 0
    pred = [0] * ncomp
    dcdiff = np.zeros(coef.shape[0], np.int32)
    ri_blocks = restart * nslots
    for b in range(coef.shape[0]):
        if ri_blocks and b and b % ri_blocks == 0:
            pad = -pos % 8
            if pad:
                vals.append((1 << pad) - 1); lens.append(pad)
                pos += pad
            intervals.append(len(vals))
            pred = [0] * ncomp
        slot = b % nslots
        c = comp_of_slot[slot]
        zz = coef[b]
        d = int(zz[0]) - pred[c]
        pred[c] = int(zz[0])
        dcdiff[b] = d
        n, bits = _amp(d)
        assert n <= 11, "a DC difference beyond category 11"
        code, ln = dc_of_slot[slot].codes[n]
        syms.append((pos, ln, n, 0, slot, n, tab_of_slot[slot][0], b))
        vals.append((code << n) | bits); lens.append(ln + n)
        pos += ln + n
        ac = ac_of_slot[slot].codes
        nz = np.flatnonzero(zz[1:]) + 1
        z = 1
        for k in nz.tolist():
            run = k - z
            while run > 15:
                code, ln = ac[0xF0]
                syms.append((pos, ln, 0, z, slot, 0xF0, tab_of_slot[slot][1], b))
                vals.append(code); lens.append(ln)
                pos += ln
                z += 16
                run -= 16
            n, bits = _amp(int(zz[k]))
            assert 1 <= n <= max_ac_size <= 15, f"an AC value beyond size {max_ac_size}"
            s = (run << 4) | n
            code, ln = ac[s]
            syms.append((pos, ln, n, z, slot, s, tab_of_slot[slot][1], b))
            vals.append((code << n) | bits); lens.append(ln + n)
            pos += ln + n
            z = k + 1
        if z < 64:
            code, ln = ac[0]
            syms.append((pos, ln, 0, z, slot, 0, tab_of_slot[slot][1], b))
            vals.append(code); lens.append(ln)
            pos += ln
    nbits = pos
    pad = -pos % 8
    if pad:
        vals.append((1 << pad) - 1); lens.append(pad)
        pos += pad
    string = _pack(vals, lens, pos // 8)

    out = Crafted()
    out.sym = np.array(syms, SYM)
    out.nbits, out.nslots, out.restart, out.ri_blocks = nbits, nslots, restart, ri_blocks
    out.dc_of_slot, out.ac_of_slot = dc_of_slot, ac_of_slot
    out.w, out.h, out.mx, out.my = w, h, mx, my
    # the intervals' byte ranges in the string
    starts = np.concatenate([[0], np.cumsum(np.asarray(lens, np.int64))])
    ibytes = [int(starts[i]) // 8 for i in intervals] + [len(string)]
    assert all(int(starts[i]) % 8 == 0 for i in intervals)
    body = bytearray()
    pieces, rst = [], []
    for k in range(len(intervals)):
        piece = string[ibytes[k]:ibytes[k + 1]]
        if extra and k in extra:
            piece += bytes(extra[k])
        if cut and k in cut:
            piece = piece[:len(piece) - cut[k]]
        pieces.append(piece)
    if extra or cut:                                          # a damaged file: the string as the device's host side will see it
        string = b"".join(pieces)
    at = 0
    for k, piece in enumerate(pieces):
        if k:
            rst.append(at)
            body += bytes([0xFF, 0xD0 + ((k - 1) & 7)])
        body += piece.replace(b"\xff", b"\xff\x00")
        at += len(piece)
    out.rst = rst
    if tile > 1:
        assert nbits % 8 == 0 and b"\xff" not in string and all(p == 0 for p in pred), "the period does not repeat as bytes"
        string = string * tile
        body = bytearray(string)
        out.period_bits = nbits
        out.nbits = nbits * tile
        out.coef = np.tile(coef.astype(np.int16), (tile, 1))
        out.dcdiff = np.tile(dcdiff, tile)
    else:
        out.coef = coef.astype(np.int16)
        out.dcdiff = dcdiff
    out.string = string

    head = bytearray(b"\xff\xd8")
    for i, q in enumerate(qtabs):
        assert len(q) == 64 and all(1 <= v <= 255 for v in q)
        head += bytes([0xFF, 0xDB, 0, 67, i] + q)
    comps = [(1, (hy << 4) | vy if ncomp == 3 else 0x11, 0)] + [(2 + i, 0x11, len(qtabs) - 1) for i in range(ncomp - 1)]
    head += bytes([0xFF, 0xC0, 0, 8 + 3 * ncomp, 8, h >> 8, h & 255, w >> 8, w & 255, ncomp])
    for cid, hv, tq in comps:
        head += bytes([cid, hv, tq])
    hdc, hac = header_tabs or (dc_tabs, ac_tabs)
    for tc, tabs in ((0, hdc), (1, hac)):
        for th, t in enumerate(tabs):
            seg = t.segment(tc, th)
            head += bytes([0xFF, 0xC4, (len(seg) + 2) >> 8, (len(seg) + 2) & 255]) + seg
    if restart:
        head += bytes([0xFF, 0xDD, 0, 4, restart >> 8, restart & 255])
    head += bytes([0xFF, 0xDA, 0, 6 + 2 * ncomp, ncomp])
    for c in range(ncomp):
        head += bytes([comps[c][0], (comp_tabs[c][0] << 4) | comp_tabs[c][1]])
    head += bytes([0, 63, 0])
    out.scan_offset = len(head)
    out.data = bytes(head) + bytes(body) + b"\xff\xd9"
    return out


def natural(cr):
    """the coded coefficients as the device's write pass leaves them: natural order, the DC still as the difference"""
    nat = np.zeros_like(cr.coef)
    nat[:, ZIG] = cr.coef
    nat[:, 0] = cr.dcdiff.astype(np.int16)
    return nat


def walk(cr, string, start_bit, z, slot, stop_bit, rst=None):
    """A decoder's state walk over `string` (bytes without stuffing) by code lengths and value sizes only: from (start_bit, z,
    slot) to the first symbol that starts at or after stop_bit.  Returns (bit, z, slot, blocks finished).  cr: anything with
    nslots, dc_of_slot, ac_of_slot (a Crafted).  rst: the byte offsets at which restart intervals start -- standing on one, the
    state starts over; a symbol that would reach across the next one is padding.  Bits past the string read as zeros; where no
    code of the table matches, sixteen bits are taken as symbol 0 (the device's convention for a decoder that is out of step)."""
    luts_dc = [t.lut() for t in cr.dc_of_slot]
    luts_ac = [t.lut() for t in cr.ac_of_slot]
    nslots = cr.nslots
    buf = bytes(string) + b"\0" * 8
    nbytes = len(string)
    bounds = [8 * r for r in (rst or [])]
    rk = 0
    while rk < len(bounds) and bounds[rk] < start_bit:
        rk += 1
    bnext = bounds[rk] if rk < len(bounds) else 1 << 62
    pos, blocks = start_bit, 0
    while pos < stop_bit:
        if pos >= bnext:
            z, slot = 0, 0
            rk += 1
            bnext = bounds[rk] if rk < len(bounds) else 1 << 62
        i, o = pos >> 3, pos & 7
        c16 = 0
        if i < nbytes:
            c16 = (((buf[i] << 16) | (buf[i + 1] << 8) | buf[i + 2]) >> (8 - o)) & 0xffff
        e = (luts_dc if z == 0 else luts_ac)[slot][c16]
        ln, s = (e >> 8, e & 255) if e else (16, 0)
        size, run = s & 15, s >> 4
        if pos + ln + size > bnext:
            pos = bnext
            continue
        pos += ln + size
        z = 1 if z == 0 else (64 if (size == 0 and run != 15) else z + run + 1)
        if z >= 64:
            z, slot, blocks = 0, (slot + 1) % nslots, blocks + 1
    return pos, z, slot, blocks


def state_word(bit, z, slot):
    """dec_state's packing"""
    return bit | (z << 40) | (slot << 48)
