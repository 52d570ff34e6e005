"""The crafted files of the device Huffman decoder's suite (tests/jpeg_craft.py writes them): one place for the three test modules
(test_jpeg_craft.py: the checker and the symbol map; test_jpeg_dec_hostsim.py: the lane body on the CPU; test_jpeg_craft_gpu.py:
the device).  Every case is a dict name -> Crafted; the Huffman lengths and values typed in here are data.  Groups:
  a  code lengths 1..16, gaps in limit[], no code below 12 bits, 255 symbols; all four table selectors (4:2:0)
  b  one probe block sequence behind filler that shifts it by 0..63 bits; eight more files carry it across the 240- and 256-span borders
  c  second symbols of the sync tables' entries, with and without a restart interval
  d  two-bit blocks
  e  restart boundaries: padding of 0 and 7 bits, a padded 0xff, a boundary every byte
  f  a stream in which two decoders out of step never meet
  g  damaged by construction"""
from __future__ import annotations

import functools

import numpy as np

import jpeg_craft as jc
from jpeg_craft import SPAN, Table

# T.81 Annex K.3, luminance: the tables every encoder's default is (bits per length, values)
K_DC = Table([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
K_AC = Table([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d],
             [0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
              0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
              0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
              0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
              0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
              0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
              0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
              0xfa])
# ... and chrominance
K_DC_C = Table([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
# Table K.6: the chrominance AC table (the encoder's crafted-image cases, tests/jpeg_enc_cases.py, need all four)
K_AC_C = Table([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77],
               [0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14,
                0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17,
                0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a,
                0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78,
                0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3,
                0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7,
                0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2,
                0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa])


def _bits(**at):
    """bits[16] from length = count pairs (L3=2: two codes of three bits)"""
    b = [0] * 16
    for k, v in at.items():
        b[int(k[1:]) - 1] = v
    return b


# (a) a code at every length 1..16 (canonically 0, 10, 110, ...: the all-ones code stays free); DC categories 7..11 sit on lengths 12..16
A_DC_ALL = Table([1] * 16, [0, 1, 2, 12, 3, 13, 4, 14, 5, 15, 6, 7, 8, 9, 10, 11])
A_AC_ALL = Table([1] * 16, [0x01, 0x00, 0x11, 0x02, 0xf0, 0x21, 0x03, 0x12, 0x31, 0x04, 0x41, 0x05, 0x22, 0x06, 0x13, 0x0a])
# lengths 2, 13 and 16 only: limit[] stands still across the gaps
A_DC_GAP = Table(_bits(L2=3, L13=4, L16=5), list(range(12)))
A_AC_GAP = Table(_bits(L2=3, L13=4, L16=5), [0x00, 0x01, 0x11, 0x02, 0x21, 0xf0, 0x03, 0x04, 0x12, 0x05, 0x31, 0x0a])
# no code below 12 bits: the fast tables are all zero, every look-up counts its length
A_DC_LONG = Table(_bits(L12=6, L14=6), list(range(12)))
A_AC_LONG = Table(_bits(L12=8, L16=8), [0x00, 0x01, 0x02, 0x11, 0xf0, 0x03, 0x21, 0x12, 0x04, 0x05, 0x31, 0x06, 0x13, 0x22, 0x0a, 0x41])
# 255 symbols: fifteen codes of 4 bits, 240 of 12 bits behind the prefix 1111 (sixteen of its 256 stay free, the all-ones code among them)
A_AC_255 = Table(_bits(L4=15, L12=240), [(7 * i + 3) % 255 for i in range(255)])
A_DC_255 = Table(_bits(L3=6, L12=6), [0, 2, 4, 6, 8, 10, 1, 3, 5, 7, 9, 11])

# (c) an AC table of short codes and small sizes: 0 -> (0, 1), 10 -> EOB, 110 -> ZRL, 1110 -> (0, 2), 11110 -> (1, 2)
C_AC = Table([1, 1, 1, 1, 1] + [0] * 11, [0x01, 0x00, 0xf0, 0x02, 0x12])
C_DC = Table(_bits(L2=3, L3=1), [0, 1, 2, 3])

# (d) one code each: 0 -> category 0, 0 -> EOB
D_DC = Table(_bits(L1=1), [0])
D_AC = Table(_bits(L1=1), [0x00])

# (f) 0 -> category 7; 0 -> (run 6, size 7)
F_DC = Table(_bits(L1=1), [7])
F_AC = Table(_bits(L1=1), [0x67])


def grey_dims(n):
    """a one-component image of n blocks"""
    if n <= 8000:
        return 8 * n, 8
    for rows in range(2, 8000):
        if n % rows == 0 and n // rows <= 8000:
            return 8 * (n // rows), 8 * rows
    raise ValueError(n)


def from_diffs(blocks, nslots=1, comp_of_slot=(0,), ri_blocks=0):
    """blocks: a list of (DC difference, {zig-zag position: value}) -> the (n, 64) array with absolute DCs"""
    coef = np.zeros((len(blocks), 64), np.int32)
    pred = {}
    for b, (d, ac) in enumerate(blocks):
        if ri_blocks and b % ri_blocks == 0:
            pred = {}
        c = comp_of_slot[b % nslots]
        pred[c] = pred.get(c, 0) + d
        coef[b, 0] = pred[c]
        for k, v in ac.items():
            coef[b, k] = v
    assert np.abs(coef).max() < 32768
    return coef


def _value(rng, size):
    m = int(rng.integers(1 << (size - 1), 1 << size))
    return m if rng.integers(2) else -m


def random_blocks(rng, n, dc_of_slot, ac_of_slot, stop=0.15):
    """n blocks that use whatever symbols their slot's tables hold: DC categories and (run, size) pairs drawn evenly from the
    table (the DC categories and every block's first pair in turn), ZRL where the table has it, values of either sign; the DC
    difference's sign pulls the prediction back to 0"""
    nslots = len(dc_of_slot)
    blocks = []
    drift = [0] * nslots
    for b in range(n):
        s = b % nslots
        cats = [c for c in dc_of_slot[s].codes if c <= 11]
        cat = cats[(b // nslots + s) % len(cats)]                   # in turn: every category the table holds is used
        d = 0
        if cat:
            m = int(rng.integers(1 << (cat - 1), 1 << cat))
            d = -m if drift[s] > 0 else m
        drift[s] += d
        syms = [v for v in ac_of_slot[s].codes if 1 <= (v & 15) <= 10]
        zrl = 0xf0 in ac_of_slot[s].codes
        ac, z = {}, 1
        first = syms[(b // nslots + 5 * s) % len(syms)]              # ... and every (run, size) pair, where there are blocks enough
        while z < 64 and (z == 1 or rng.random() > stop):
            v = first if z == 1 else int(rng.choice(syms))
            run, size = v >> 4, v & 15
            if zrl and rng.random() < 0.1:
                run += 16
            if z + run > 63:
                if 0 in ac_of_slot[s].codes:
                    break
                continue
            ac[z + run] = _value(rng, size)
            z += run + 1
        blocks.append((d, ac))
    return blocks


def state_at(cr, bit):
    """from the symbol map: the state of a decoder in step when it reaches the first symbol at or after `bit`"""
    period = getattr(cr, "period_bits", 0)
    base = 0
    if period:
        base, bit = bit // period * period, bit % period
    i = int(np.searchsorted(cr.sym["start"], bit))
    if i == len(cr.sym):
        assert period, "past the last symbol"
        return base + period, 0, 0
    s = cr.sym[i]
    return base + int(s["start"]), int(s["z"]), int(s["slot"])


# ---------------------------------------------------------------------------------------------------------------- (a)
@functools.lru_cache(None)
def group_a():
    out = {}
    for name, dcs, acs in (("a_all_and_gaps", (A_DC_ALL, A_DC_GAP), (A_AC_ALL, A_AC_GAP)), ("a_long_and_255", (A_DC_LONG, A_DC_255), (A_AC_LONG, A_AC_255))):
        # 4:2:0: slots 0..3 are Y (table 0 of each class), 4 and 5 Cb and Cr (table 1)
        dc_of_slot = [dcs[0]] * 4 + [dcs[1]] * 2
        ac_of_slot = [acs[0]] * 4 + [acs[1]] * 2
        rng = np.random.default_rng(len(name))
        blocks = random_blocks(rng, 96, dc_of_slot, ac_of_slot)
        coef = from_diffs(blocks, 6, (0, 0, 0, 0, 1, 2))
        out[name] = jc.encode(coef, 64, 64, dcs, acs, sampling=(2, 2))
    # the same tables the other way round: what was table 1 is the luminance's
    dcs, acs = (A_DC_GAP, A_DC_ALL), (A_AC_255, A_AC_LONG)
    rng = np.random.default_rng(3)
    blocks = random_blocks(rng, 96, [dcs[0]] * 4 + [dcs[1]] * 2, [acs[0]] * 4 + [acs[1]] * 2)
    out["a_swapped"] = jc.encode(from_diffs(blocks, 6, (0, 0, 0, 0, 1, 2)), 64, 64, dcs, acs, sampling=(2, 2))
    return out


# ---------------------------------------------------------------------------------------------------------------- (b)
def _ends(size):
    return [-(1 << size) + 1, -(1 << (size - 1)), 1 << (size - 1), (1 << size) - 1]


def probe_blocks():
    """the fixed probe: see the module's header"""
    blocks = [(0, {})]                                               # DC category 0, EOB at z = 1
    acv = [v for size in range(1, 11) for v in _ends(size)]          # forty AC values: sizes 1..10 at both ends, both signs
    k = 0
    for cat in range(1, 12):
        for d in _ends(cat):                                         # (the four add up to 0: the prediction returns there)
            blocks.append((d, {1: acv[k % 40], 3: acv[(k + 7) % 40]}))
            k += 1
    blocks.append((0, {63: 300}))                                    # ZRL x 3, then (14, 9) lands on 63
    blocks.append((0, {47: -5, 63: 1023}))                           # ... a run of 15 landing exactly on 63
    blocks.append((3, {k: (1023 if k % 2 else -1023) for k in range(1, 64)}))      # 63 values, no EOB
    blocks.append((-3, {k: (1 if k % 3 else -2) for k in range(1, 64)}))           # ... of short symbols
    blocks.append((0, {}))
    return blocks


def _adjust(k):
    """64 blocks of a DC and an EOB, 8 bits each (category 1) but for k of 9 bits (category 2): 512 + k bits"""
    return [((2 if i % 2 == 0 else -2), {}) for i in range(k)] + [((1 if i % 2 == 0 else -1), {}) for i in range(64 - k)]


_FILL = (0, {k: (1000 if k % 2 else -1000) for k in range(1, 64)})      # 2 + 63 x 26 = 1640 bits
_HALF = (0, {k: (1000 if k % 2 else -1000) for k in range(1, 32)})      # 2 + 31 x 26 + 4 = 812 bits


def _fill_to(target_bits):
    """filler of 1640- and 812-bit blocks: the longest that stays 50 bits or more short of target_bits (by less than 878)"""
    n, rem = divmod(target_bits - 50, 1640)
    return [_FILL] * n + ([_HALF] if rem >= 812 else [])


def _grey(blocks):
    w, h = grey_dims(len(blocks))
    return jc.encode(from_diffs(blocks), w, h, [K_DC], [K_AC])


BIG_SHIFTS = (0, 8, 16, 24, 32, 40, 48, 56)


@functools.lru_cache(None)
def group_b():
    out = {}
    probe = probe_blocks()
    full = next(i for i, b in enumerate(probe) if len(b[1]) == 63)    # the probe's block of 63 long symbols
    for k in range(64):
        out[f"b_shift_{k:02d}"] = _grey(_adjust(k) + probe)
    for k in BIG_SHIFTS:
        # filler in front so that the 240-span border falls inside the probe's long block, more filler so that the 256-span border
        # falls inside a second probe's
        head = _adjust(k) + probe[:full]
        head_bits = jc.encode(from_diffs(head), *grey_dims(len(head)), [K_DC], [K_AC]).nbits
        seq = _fill_to(240 * SPAN - head_bits) + _adjust(k) + probe
        tail_bits = jc.encode(from_diffs(seq + probe[:full]), *grey_dims(len(seq) + full), [K_DC], [K_AC]).nbits
        out[f"b_big_{k:02d}"] = _grey(seq + _fill_to(256 * SPAN - tail_bits) + probe)
    return out


# ---------------------------------------------------------------------------------------------------------------- (c)
def _c_blocks(shift):
    ones = {k: (1 if k % 2 else -1) for k in range(1, 64)}           # 63 x (0, 1): two bits a symbol, no EOB -- the last one ends the block
    blocks = []
    blocks += [(1 if i % 2 == 0 else -1, {}) for i in range(shift)]  # category 1: 2 + 1 + 2 bits, shifts what follows by 5 bits each
    for i in range(14):
        blocks.append((0, ones))                                     # a value at 63 and the next block's DC code 00 behind it
        blocks.append((0, {1: 1, 2: -1}))                            # (0, 1) (0, 1) EOB: a pair whose second symbol is the EOB
        blocks.append((2 if i % 2 == 0 else -2, {1: -1, 18: 3, 19: 1, 36: -2, 38: 3}))       # (0, 1) ZRL ...: a pair whose second is ZRL; (0, 2), (1, 2)
        blocks.append((0, {k: (1 if k % 3 else -1) for k in range(1, 40)}))
    return blocks


@functools.lru_cache(None)
def group_c():
    out = {}
    for shift in (0, 1, 2, 3):
        blocks = _c_blocks(shift)
        w, h = grey_dims(len(blocks))
        out[f"c_shift_{shift}"] = jc.encode(from_diffs(blocks), w, h, [C_DC], [C_AC])
        out[f"c_shift_{shift}_rst"] = jc.encode(from_diffs(blocks, ri_blocks=5), w, h, [C_DC], [C_AC], restart=5)
    return out


# ---------------------------------------------------------------------------------------------------------------- (d)
@functools.lru_cache(None)
def group_d():
    out = {"d_4096_blocks": jc.encode(np.zeros((4096, 64), np.int32), 512, 512, [D_DC], [D_AC])}
    n = 4096 - 3                                                     # one block in the last byte: six bits of padding
    w, h = 8 * n, 8
    out["d_last_byte_padded"] = jc.encode(np.zeros((n, 64), np.int32), w, h, [D_DC], [D_AC])
    return out


def d_cut():
    """(d)'s file with its scan's last byte taken out: the blocks run out"""
    data = group_d()["d_4096_blocks"].data
    return data[:-3] + data[-2:]


# ---------------------------------------------------------------------------------------------------------------- (e)
def _interval_grey(rng, want_pad, ff):
    """the blocks of one interval (12 of them) whose coded length leaves want_pad bits of padding; ff: the last block ends in the
    ten 1-bits of a +1023 at position 63, so that the interval's last byte -- padded or not -- is 0xff"""
    body = random_blocks(rng, 9, [K_DC], [K_AC], stop=0.3)
    last = (0, {63: 1023}) if ff else (0, {5: 2})
    for c1 in range(8):                                              # two DC-and-EOB blocks: 6, 8, 9, 10, 11, 13, 15, 17 bits by category
        for c2 in range(8):
            blocks = body + [((1 << c1) - 1 if c1 else 0, {}), (-((1 << c2) - 1) if c2 else 0, {}), last]
            cr = jc.encode(from_diffs(blocks), 8 * len(blocks), 8, [K_DC], [K_AC])
            if -cr.nbits % 8 == want_pad:
                return blocks
    raise AssertionError("no tuning found")


@functools.lru_cache(None)
def group_e():
    out = {}
    rng = np.random.default_rng(5)
    # grey: intervals of 12 blocks, tuned in turn to 0 bits of padding, 7 bits, a padded 0xff, an unpadded 0xff
    blocks = []
    for want, ff in ((0, False), (7, False), (3, True), (0, True), (5, False), (7, True), (0, False), (1, False)):
        blocks += _interval_grey(rng, want, ff)
    out["e_grey"] = jc.encode(from_diffs(blocks, ri_blocks=12), 8 * 12, 8 * 8, [K_DC], [K_AC], restart=12)
    # 4:1:0, ten slots: an interval is one MCU; Y from the luminance tables, Cb and Cr from table 1 (the chroma DC, the same AC);
    # the Cr block is the tuner
    dcs, acs = (K_DC, K_DC_C), (K_AC, K_AC)
    dc_of_slot, ac_of_slot = [K_DC] * 8 + [K_DC_C] * 2, [K_AC] * 10
    comp = (0,) * 8 + (1, 2)
    mcus = []
    wants = [(0, False), (7, False), (2, True), (0, True), (4, False), (7, False)]
    for want, ff in wants:
        body = random_blocks(rng, 9, dc_of_slot, ac_of_slot, stop=0.3)
        found = None
        for cat in range(12):
            for extra_ac in ({}, {1: 1}, {1: 2}, {2: 1}, {1: 5}, {1: 9}, {1: 17}, {1: 33}):
                ac = dict(extra_ac)
                if ff:
                    ac[63] = 1023
                cand = body + [((1 << cat) - 1 if cat else 0, ac)]
                cr = jc.encode(from_diffs(cand, 10, comp), 32, 16, dcs, acs, sampling=(4, 2))
                if -cr.nbits % 8 == want:
                    found = cand
                    break
            if found:
                break
        assert found, (want, ff)
        mcus += found
    out["e_410"] = jc.encode(from_diffs(mcus, 10, comp, ri_blocks=10), 32 * 3, 16 * 2, dcs, acs, sampling=(4, 2), restart=1)
    # a boundary every byte: (d)'s two-bit blocks, one per interval
    out["e_every_byte"] = jc.encode(np.zeros((300, 64), np.int32), 2400, 8, [D_DC], [D_AC], restart=1)
    return out


# ---------------------------------------------------------------------------------------------------------------- (f)
def _f_period():
    blocks = []
    for d in (100, -100):
        blocks.append((d, {7 * k: (64 + 5 * k if k % 2 else -(70 + 3 * k)) for k in range(1, 10)}))
    return from_diffs(blocks)


@functools.lru_cache(None)
def f_big():
    """3648 x 3648: 207 936 blocks of 10 bytes, 16 245 spans, 68 workgroups"""
    return jc.encode(_f_period(), 3648, 3648, [F_DC], [F_AC], tile=207936 // 2)


@functools.lru_cache(None)
def group_f_small():
    """1024 x 640: 10 240 blocks, 800 spans, 4 workgroups; the same with a restart interval of 50 MCUs"""
    per = _f_period()
    coef = np.tile(per, (5120, 1))
    return {"f_4wg": jc.encode(coef, 1024, 640, [F_DC], [F_AC]),
            "f_4wg_rst": jc.encode(coef, 1024, 640, [F_DC], [F_AC], restart=50)}


# ---------------------------------------------------------------------------------------------------------------- (g)
@functools.lru_cache(None)
def group_g():
    """name -> (Crafted, the sound twin or None).  A twin: the same coefficients in a sound file."""
    out = {}
    # a run past position 63: the scan codes (1, 1) at z = 60, the file's DHT says that code is (15, 1)
    ac_coded = Table([1, 1, 1] + [0] * 13, [0x01, 0x00, 0x11])
    ac_stated = Table([1, 1, 1] + [0] * 13, [0x01, 0x00, 0xf1])
    blocks = [(0, {1: 1}), (1, {k: 1 for k in range(1, 60)} | {61: -1}), (-1, {1: 1}), (0, {})]
    out["g_run_past_63"] = (jc.encode(from_diffs(blocks), 32, 8, [C_DC], [ac_coded], header_tabs=([C_DC], [ac_stated])), None)
    # a code outside its table: the scan uses the table's last 16-bit code, the file's DHT ends one code earlier
    ac_stated = Table(_bits(L2=3, L13=4, L16=4), A_AC_GAP.values[:-1])
    blocks = [(0, {1: 1}), (1, {1: -1, 2: 600}), (-1, {2: 1}), (0, {})]
    assert A_AC_GAP.values[-1] == 0x0a
    out["g_code_outside_table"] = (jc.encode(from_diffs(blocks), 32, 8, [A_DC_GAP], [A_AC_GAP], header_tabs=([A_DC_GAP], [ac_stated])), None)
    # an interval whose blocks end 16 (3) bytes before its marker, both inside one span: bytes the image does not have
    rng = np.random.default_rng(9)
    blocks = random_blocks(rng, 8 * 6, [K_DC], [K_AC], stop=0.45)
    coef = from_diffs(blocks, ri_blocks=6)
    twin = jc.encode(coef, 64, 48, [K_DC], [K_AC], restart=6)
    junk = bytes((37 * i + 11) % 251 for i in range(16))
    out["g_ends_16_early"] = (jc.encode(coef, 64, 48, [K_DC], [K_AC], restart=6, extra={0: junk, 3: junk[::-1]}), twin)
    out["g_ends_3_early"] = (jc.encode(coef, 64, 48, [K_DC], [K_AC], restart=6, extra={0: junk[:3], 3: junk[5:8]}), twin)
    return out


def sound_groups():
    """every sound small case, name -> Crafted"""
    out = {}
    for g in (group_a, group_b, group_c, group_d, group_e, group_f_small):
        out.update(g())
    return out
