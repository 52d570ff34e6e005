"""Crafted PIXEL images for the device JPEG encoder's entropy coder (jpeg.hip: jpeg_code_kernel, the scans, jpeg_pack_kernel, the
0xff count and the stuffing, and their batch forms), and a count of what they reach.  The encoder takes pixels, not coefficients,
so every case is built backwards -- an 8 x 8 block clip(rint(F * basis + 128 + dither)) whose quantised DCT has F's value on one
zig-zag position -- and proved forwards: tests/test_jpeg_enc_cases.py counts, from the ORACLE's coefficients, which Huffman
symbols every case reaches.  The seeds typed in here were found by a search on the CPU; the search is not kept, its result is
checked.  No files, no Pillow.  Test infrastructure only.

Three colour axes carry a plane t of 0..255 into the encoder's three components exactly (color.RGBToYCbCr's fixed point):
  gray  (t, t, t)              Y = t, Cb = Cr = 128
  cb    (255 - t, 255 - t, t)  Cb = min(t + 1, 255)  (blue .. yellow; Y and Cr move a little with it)
  cr    (t, 255 - t, 255 - t)  Cr = min(t + 1, 255)  (red .. cyan)
A chroma sample is (sum of 2 x 2 + 2) >> 2, so a chroma block is laid out as a 16 x 16 tile of doubled pixels."""
from __future__ import annotations

import collections
import functools

import numpy as np

import jpeg_craft as jc
from jpeg_craft_cases import K_AC, K_AC_C, K_DC, K_DC_C
from oracle import oracle as orc

Case = collections.namedtuple("Case", "img qualities")

SCAN_PER_WG = 2048               # jpeg.hip: elements a workgroup of the scan kernels owns


def _bases():
    b = np.zeros((64, 8, 8))
    x = np.arange(8)
    for k, nat in enumerate(jc.ZIG):
        v, u = divmod(nat, 8)
        cu, cv = (np.sqrt(0.5) if u == 0 else 1.0), (np.sqrt(0.5) if v == 0 else 1.0)
        b[k] = 0.25 * cu * cv * np.outer(np.cos((2 * x + 1) * v * np.pi / 16), np.cos((2 * x + 1) * u * np.pi / 16))
    return b


BASIS = _bases()                 # BASIS[k]: the 8 x 8 pattern (row, column) whose orthonormal DCT is 1 at zig-zag position k


@functools.lru_cache(None)
def quantisers(quality, chroma):
    """the 64 quantisers of one table in zig-zag order"""
    return orc.jpeg_quant_tables(quality)[1 if chroma else 0].reshape(64)[jc.ZIG].astype(int).tolist()


def ac_block(chroma, run, size, quality, seed):
    """An 8 x 8 plane whose first AC symbol at `quality` is (run, size): one basis function at zig-zag position run + 1, its
    quantised value drawn from the size's range by the seed, uniform dither of +-0.5 under the rounding."""
    rng = np.random.default_rng([int(chroma), run, size, quality, seed])
    v = int(rng.integers(1 << (size - 1), 1 << size)) * (1 if rng.integers(2) else -1)
    f = v * quantisers(quality, chroma)[run + 1]
    plane = np.rint(f * BASIS[run + 1] + 128 + rng.uniform(-0.5, 0.5, (8, 8)))
    return np.clip(plane, 1 if chroma else 0, 255).astype(np.uint8)


def lone_block(chroma, pos, quality, seed):
    """An 8 x 8 plane whose ONLY non-zero AC coefficient at `quality` sits on zig-zag position pos (a value of size 2)"""
    rng = np.random.default_rng([int(chroma), pos, quality, seed, 7])
    v = int(rng.integers(2, 4)) * (1 if rng.integers(2) else -1)
    plane = np.rint(v * quantisers(quality, chroma)[pos] * BASIS[pos] + 128 + rng.uniform(-0.5, 0.5, (8, 8)))
    return np.clip(plane, 1, 255).astype(np.uint8)


def dc_block(chroma, dc):
    """An 8 x 8 plane whose DC coefficient at quality 100 is exactly dc: the sum of (sample - 128) is 8 * dc"""
    base, r = divmod(8 * dc, 64)
    plane = 128 + base + (np.arange(64) < r).reshape(8, 8)
    assert 0 <= plane.min() and plane.max() <= 255 and not (chroma and plane.min() < 1), dc
    return plane.astype(np.uint8)


def flat_block(v=128):
    return np.full((8, 8), v, np.uint8)


def on_axis(t, axis):
    """a plane t of 0..255 -> the opaque NRGBA image on one of the three axes (for cb and cr, t is the wanted sample - 1)"""
    t = np.asarray(t).astype(np.int16)
    img = np.empty(t.shape + (4,), np.uint8)
    r, g, b = {"gray": (t, t, t), "cb": (255 - t, 255 - t, t), "cr": (t, 255 - t, 255 - t)}[axis]
    img[..., 0], img[..., 1], img[..., 2], img[..., 3] = r, g, b, 255
    return img


def sheet(blocks, axis, mcus_per_row=8):
    """Blocks in SCAN order -> one image.  gray: four blocks fill an MCU (Y0 Y1 / Y2 Y3), so consecutive blocks are consecutive in
    the luminance's DC prediction; cb, cr: one block an MCU, every sample doubled.  Short rows are filled with flat 128."""
    blocks = list(blocks)
    if axis == "gray":
        blocks += [flat_block()] * (-len(blocks) % 4)
        cells = [np.block([[blocks[i], blocks[i + 1]], [blocks[i + 2], blocks[i + 3]]]) for i in range(0, len(blocks), 4)]
    else:
        cells = [np.kron(b, np.ones((2, 2), np.uint8)) for b in blocks]
        cells = [c.astype(np.int16) - 1 for c in cells]
    fill = np.full((16, 16), 128 if axis == "gray" else 127, np.int16)
    cells += [fill] * (-len(cells) % mcus_per_row)
    rows = [np.hstack(cells[i:i + mcus_per_row]) for i in range(0, len(cells), mcus_per_row)]
    return on_axis(np.vstack(rows), axis)


# ----------------------------------------------------------------------------------------------------- the found seeds
# (quality, seed) of ac_block for every (run, size): row = run 0..15, column = size 1..10
LUMA_AC = [
    [(100, 0), (100, 0), (100, 0), (100, 0), (100, 0), (100, 0), (100, 0), (100, 0), (100, 0), (100, 0)],
    [(100, 0), (100, 0), (100, 0), (100, 1), (100, 0), (100, 1), (100, 1), (100, 0), (100, 0), (100, 0)],
    [(100, 0), (100, 0), (100, 5), (100, 1), (100, 1), (100, 1), (100, 0), (100, 1), (100, 1), (100, 0)],
    [(100, 0), (100, 5), (100, 6), (100, 3), (100, 0), (100, 3), (100, 0), (100, 0), (100, 4), (100, 14)],
    [(100, 2), (100, 5), (100, 5), (100, 1), (100, 0), (100, 11), (100, 4), (100, 6), (100, 2), (100, 2)],
    [(100, 1), (100, 2), (100, 0), (100, 4), (100, 3), (100, 0), (100, 11), (100, 2), (100, 12), (100, 5)],
    [(100, 1), (100, 25), (100, 7), (100, 3), (100, 2), (100, 6), (100, 1), (100, 5), (100, 1), (100, 26)],
    [(100, 2), (100, 29), (100, 10), (100, 0), (100, 15), (100, 5), (100, 6), (100, 4), (100, 4), (100, 24)],
    [(100, 1), (100, 37), (100, 4), (100, 12), (100, 3), (100, 17), (100, 15), (100, 57), (100, 2), (100, 32)],
    [(100, 9), (100, 64), (100, 56), (100, 4), (100, 5), (100, 2), (100, 19), (100, 1), (100, 4), (100, 2)],
    [(100, 1), (100, 112), (100, 2), (100, 8), (100, 17), (100, 6), (100, 8), (100, 25), (100, 29), (97, 30)],
    [(100, 6), (100, 67), (100, 151), (100, 27), (100, 96), (100, 26), (100, 3), (100, 22), (100, 54), (100, 93)],
    [(100, 12), (100, 69), (100, 104), (100, 16), (100, 5), (100, 90), (100, 46), (100, 22), (100, 42), (100, -1)],
    [(100, 3), (100, 158), (100, 4), (100, 2), (100, 2), (100, 7), (100, 9), (100, 0), (100, 1), (100, 8)],
    [(100, 29), (100, 3), (97, 78), (100, 80), (100, 33), (100, 16), (100, 18), (100, 37), (100, 44), (100, 25)],
    [(100, 6), (97, 19), (100, 0), (100, 62), (100, 58), (100, 130), (100, 132), (100, 25), (100, 19), (100, 140)],
]
CHROMA_AC = [
    [(100, 1), (100, 0), (100, 0), (100, 0), (100, 0), (100, 0), (100, 0), (100, 0), (100, 0), (100, 0)],
    [(100, 0), (100, 0), (100, 2), (100, 0), (100, 2), (100, 1), (100, 1), (100, 0), (100, 1), (100, 0)],
    [(100, 0), (100, 11), (100, 0), (100, 1), (100, 1), (100, 1), (100, 0), (100, 0), (100, 0), (100, 0)],
    [(100, 0), (100, 2), (100, 0), (100, 0), (100, 7), (100, 3), (100, 0), (100, 1), (100, 0), (100, 0)],
    [(100, 0), (100, 0), (100, 4), (100, 0), (100, 1), (100, 1), (100, 1), (100, 1), (100, 1), (100, 1)],
    [(100, 4), (100, 26), (100, 4), (100, 19), (100, 8), (100, 0), (100, 13), (100, 7), (100, 14), (100, 17)],
    [(100, 0), (100, 6), (100, 1), (100, 0), (100, 11), (100, 1), (100, 1), (100, 1), (100, 6), (100, 0)],
    [(100, 3), (100, 6), (100, 4), (100, 1), (100, 19), (100, 7), (100, 5), (100, 3), (100, 13), (100, 3)],
    [(100, 5), (100, 21), (100, 24), (100, 8), (100, 7), (100, 2), (100, 0), (100, 19), (100, 3), (100, 29)],
    [(100, 6), (100, 6), (100, 8), (100, 0), (100, 0), (100, 1), (100, 4), (100, 1), (100, 6), (100, 7)],
    [(100, 4), (100, 32), (100, 18), (100, 7), (100, 12), (100, 42), (100, 10), (100, 13), (100, 2), (100, 20)],
    [(100, 8), (100, 27), (100, 88), (100, 8), (100, 7), (100, 8), (100, 5), (100, 11), (100, 12), (100, 4)],
    [(100, 4), (100, 56), (100, 35), (100, 9), (100, 24), (100, 18), (100, 8), (100, 22), (100, 131), (100, -1)],
    [(100, 3), (100, 153), (100, 85), (100, 11), (100, 8), (100, 5), (100, 16), (100, 2), (100, 1), (100, 9)],
    [(100, 9), (100, 1), (97, 14), (100, 64), (100, 54), (100, 163), (100, 68), (100, 127), (100, 11), (100, 9)],
    [(100, 4), (97, 3), (100, 105), (100, 36), (100, 53), (100, 88), (100, 46), (100, 61), (100, 22), (100, 7)],
]

# Seed -1: no single basis function gave (12, 10) in 300 seeds at quality 100 or 100 to 150 at seven lower ones -- clipped to 0..255, a wave on position 13 large
# enough for size 10 leaks into the twelve positions in front of it.  This block was solved for instead (a linear programme:
# the largest coefficient on position 13 with positions 1..12 at zero and every sample in 1..255; +-0.5 of dither; rounded):
# position 13 comes out at 788.  It serves both tables.
SOLVED = {(12, 10): [[255, 1, 1, 1, 255, 255, 255, 1], [255, 250, 1, 1, 255, 255, 6, 1], [255, 59, 1, 1, 255, 255, 198, 1], [255, 1, 1, 1, 255, 255, 255, 1],
                     [1, 216, 255, 255, 1, 1, 41, 255], [1, 255, 255, 255, 1, 1, 1, 255], [1, 1, 255, 255, 1, 1, 255, 255], [1, 242, 255, 255, 1, 1, 14, 255]]}

# Chroma pairs of size 9 or 10 that no case reaches.  None: on the cb and cr axes a chroma sample takes every value 1..255, so the
# chroma blocks reach what the luminance's do.  (The CPU test proves of any pair listed here that no case reaches it.)
UNREACHED_CHROMA = []

# the only non-zero AC after 15, 16, 17, 31, 32, 47, 48 and 62 zeros: 0, 1, 1, 1, 2, 2, 3 and 3 ZRLs; position 63 leaves no EOB
RUN_ZEROS = (15, 16, 17, 31, 32, 47, 48, 62)
RUN_ZRLS = (0, 1, 1, 1, 2, 2, 3, 3)
RUN_QUALITY = 75
RUN_SEEDS = {False: (0,) * 8, True: (0,) * 8}

# small_image seeds: a padded last byte of 0xff; unstuffed string lengths of 0..3 mod 4 bytes; of 0..7 mod 8 bits
SMALL_FF_TAIL = 170
SMALL_BYTES_MOD4 = (3, 2, 8, 0)
SMALL_BITS_MOD8 = (2, 12, 7, 37, 1, 8, 4, 0)


# ------------------------------------------------------------------------------------------------------------ DC steps
def dc_steps(chroma):
    """Absolute DC values whose differences, from 0, take every category 0..11 with either sign where the range allows it
    (luminance: -1024..1016; chrominance, whose sample 0 the cb / cr axes cannot give: -1016..1016)."""
    lo, hi = (-1016, 1016) if chroma else (-1024, 1016)
    mid = lo // 2
    diffs = [0, mid]                                                 # category 0; down to the middle of the lower half (category 10)
    for cat in range(1, 11):
        a, b = 1 << (cat - 1), (1 << cat) - 1
        diffs += [a, -a, b, -b]
    diffs += [lo - mid, hi - lo, lo - hi, hi - lo, -hi, 0]           # category 11 three times, back to 0, category 0 again
    out = np.cumsum(diffs).tolist()
    assert min(out) >= lo and max(out) <= hi
    return out


# -------------------------------------------------------------------------------------------------------- string shapes
def binary_noise(w, h, seed):
    """every sample 0 or 255, opaque"""
    img = (np.random.default_rng(seed).integers(0, 2, (h, w, 4), dtype=np.uint8) * 255).astype(np.uint8)
    img[..., 3] = 255
    return img


def solid(w, h, rgb):
    img = np.empty((h, w, 4), np.uint8)
    img[...] = tuple(rgb) + (255,)
    return img


def small_image(seed):
    """(image, quality) drawn by the seed: 1..16 pixels a side, noise or one colour"""
    rng = np.random.default_rng([seed, 11])
    w, h = (int(v) for v in rng.integers(1, 17, 2))
    q = int(rng.choice([100, 92, 75, 30]))
    if rng.integers(2):
        return solid(w, h, tuple(int(v) for v in rng.integers(0, 256, 3))), q
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img, q


# ------------------------------------------------------------------------------------------------------------ the cases
def _ac_sheets(out, table, chroma, axes):
    by_q = collections.defaultdict(list)
    for run in range(16):
        for size in range(1, 11):
            if (run, size) in UNREACHED_CHROMA and chroma:
                continue
            q, seed = table[run][size - 1]
            by_q[q].append(np.array(SOLVED[run, size], np.uint8) if seed < 0 else ac_block(chroma, run, size, q, seed))
    for q, blocks in sorted(by_q.items()):
        for axis in axes:
            out[f"ac_{axis}_q{q}"] = Case(sheet(blocks, axis), (q,))


@functools.lru_cache(None)
def cases():
    """name -> Case(img, qualities): every crafted image and the qualities it is meant for"""
    out = {}
    _ac_sheets(out, LUMA_AC, False, ("gray",))
    _ac_sheets(out, CHROMA_AC, True, ("cb", "cr"))
    out["dc_gray"] = Case(sheet([dc_block(False, d) for d in dc_steps(False)], "gray"), (100,))
    for axis in ("cb", "cr"):
        out[f"dc_{axis}"] = Case(sheet([dc_block(True, d) for d in dc_steps(True)], axis), (100,))
    out["dc_halves_gray"] = Case(on_axis(np.repeat([[0, 255]], 16, 0).repeat(16, 1), "gray"), (100,))
    out["dc_halves_cb"] = Case(np.hstack([solid(16, 16, (255, 255, 0)), solid(16, 16, (0, 0, 255))]), (100,))
    out["dc_halves_cr"] = Case(np.hstack([solid(16, 16, (0, 255, 255)), solid(16, 16, (255, 0, 0))]), (100,))
    for chroma, axes in ((False, ("gray",)), (True, ("cb", "cr"))):
        blocks = [lone_block(chroma, z + 1, RUN_QUALITY, s) for z, s in zip(RUN_ZEROS, RUN_SEEDS[chroma])] + [flat_block()]
        for axis in axes:
            out[f"runs_{axis}"] = Case(sheet(blocks, axis, mcus_per_row=3), (RUN_QUALITY,))
    out["shape_a_flat_gray"] = Case(solid(64, 48, (128, 128, 128)), (100, 50, 1))
    out["shape_b_flat_colour"] = Case(solid(64, 48, (200, 40, 120)), (100, 50))
    out["shape_c_binary_noise"] = Case(binary_noise(48, 32, 1), (100,))
    out["shape_d_one_scan_wg_plus_four"] = Case(binary_noise(304, 288, 2), (100,))
    seeds = [SMALL_FF_TAIL] + list(SMALL_BYTES_MOD4) + list(SMALL_BITS_MOD8)
    for seed in sorted(set(seeds)):
        img, q = small_image(seed)
        out[f"shape_e_small_{seed}"] = Case(img, (q,))
    return out


# ------------------------------------------------------------------------------------------------------------- coverage
TABLES = ((K_DC, K_AC), (K_DC_C, K_AC_C))


def coverage(coef):
    """coef: (blocks, 64) quantised coefficients in zig-zag order, blocks in scan order of a 4:2:0 file (Y0 Y1 Y2 Y3 Cb Cr; the DC
    absolute) -- the oracle's layout.  Returns a dict: dc[t], ac[t]: the DC categories and the (run, size) pairs table t codes
    (0 luminance, 1 chrominance); zrl_blocks[t], eob_blocks[t], full_blocks[t]: how many of its blocks code a ZRL, an EOB, none;
    and per block: table, zrl (count), eob (bool), nz (non-zero AC coefficients), last (position of the last one, 0: none),
    bits (the block's length in the string)."""
    coef = np.asarray(coef).astype(np.int64)
    n = coef.shape[0]
    assert coef.shape == (n, 64) and n % 6 == 0
    out = {"dc": (set(), set()), "ac": (set(), set()), "zrl_blocks": [0, 0], "eob_blocks": [0, 0], "full_blocks": [0, 0],
           "table": np.zeros(n, np.int8), "zrl": np.zeros(n, np.int32), "eob": np.zeros(n, bool), "nz": np.zeros(n, np.int32),
           "last": np.zeros(n, np.int32), "bits": np.zeros(n, np.int64)}
    pred = [0, 0, 0]
    for b in range(n):
        slot = b % 6
        comp = 0 if slot < 4 else slot - 3
        t = 1 if comp else 0
        dct, act = TABLES[t]
        d = int(coef[b, 0]) - pred[comp]
        pred[comp] = int(coef[b, 0])
        cat = abs(d).bit_length()
        out["dc"][t].add(cat)
        bits = dct.codes[cat][1] + cat
        z, zrl = 1, 0
        nzs = (np.flatnonzero(coef[b, 1:]) + 1).tolist()
        for k in nzs:
            run = k - z
            zrl += run >> 4
            bits += (run >> 4) * act.codes[0xf0][1]
            size = abs(int(coef[b, k])).bit_length()
            out["ac"][t].add((run & 15, size))
            bits += act.codes[((run & 15) << 4) | size][1] + size
            z = k + 1
        eob = z < 64
        if eob:
            bits += act.codes[0][1]
        out["table"][b], out["zrl"][b], out["eob"][b], out["nz"][b], out["bits"][b] = t, zrl, eob, len(nzs), bits
        out["last"][b] = nzs[-1] if nzs else 0
        out["zrl_blocks"][t] += zrl > 0
        out["eob_blocks"][t] += eob
        out["full_blocks"][t] += not eob
    return out


ALL_PAIRS = frozenset((run, size) for run in range(16) for size in range(1, 11))


# -------------------------------------------------------------------------------------------------- the batched coder's lists
BLUE, YELLOW, RED, CYAN = (0, 0, 255), (255, 255, 0), (255, 0, 0), (0, 255, 255)


def extremes(w, h, seed):
    """MCUs of one saturated colour each, in an order that swings every component's DC from end to end (categories 11 at quality
    100), binary noise in every fourth MCU row, and a last MCU of pure blue: Y, Cb and Cr all end far from 0."""
    cycle = [(0, 0, 0), (255, 255, 255), YELLOW, BLUE, CYAN, RED, (128, 128, 128), BLUE]
    img = binary_noise(w, h, seed)
    mx, my = w // 16, h // 16
    for m in range(mx * my):
        x, y = m % mx, m // mx
        if y % 4 != 1:
            img[16 * y:16 * y + 16, 16 * x:16 * x + 16, :3] = cycle[m % 8]
    img[h - 16:, w - 16:, :3] = BLUE
    return img


@functools.lru_cache(None)
def batches():
    """name -> [(image, target SSIM)]: lists of one geometry for fnx_jpeg_compress_batch, ordered so that an image whose last MCU
    leaves large DC values in all three components is followed by flat gray 128 (a predictor that leaked across the images'
    border would show in the gray's first MCU) and that neighbours' string lengths differ mod 32 bits.  The targets of the
    crafted sheets are out of reach, so the search ends at quality 100, where the sheets reach what they were made for."""
    c = cases()
    luma, cb, cr = c["ac_gray_q100"].img, c["ac_cb_q100"].img, c["ac_cr_q100"].img
    (h0, w0), (h1, w1) = luma.shape[:2], cb.shape[:2]
    far = 0.99999
    return {
        "luma": [(extremes(w0, h0, 3), far), (solid(w0, h0, (128, 128, 128)), 0.94), (luma, far), (binary_noise(w0, h0, 4), 0.97),
                 (solid(w0, h0, (200, 40, 120)), 0.94), (extremes(w0, h0, 5), 0.90), (solid(w0, h0, (128, 128, 128)), 0.99)],
        "chroma": [(cb, far), (extremes(w1, h1, 6), far), (solid(w1, h1, (128, 128, 128)), 0.94), (cr, far),
                   (binary_noise(w1, h1, 7), 0.97)],
    }


# ------------------------------------------------------------------------------------------------------ reading a file's scan
def scan_of(data):
    """(offset, bytes) of the entropy-coded segment of a baseline file: behind the SOS header, in front of EOI"""
    i = 2
    while True:
        assert data[i] == 0xff
        length = int.from_bytes(data[i + 2:i + 4], "big")
        if data[i + 1] == 0xda:
            return i + 2 + length, data[i + 2 + length:-2]
        i += 2 + length


def crafted(coef, w, h):
    """the plain-Python writer's file of these coefficients with the typical tables, 4:2:0 (its symbol map comes with it)"""
    return jc.encode(coef, w, h, [K_DC, K_DC_C], [K_AC, K_AC_C], sampling=(2, 2))


def first_difference(got, want, coef, w, h):
    """A sentence for a failed comparison of two files: the first differing byte, and -- from the Python writer's symbol map of the
    oracle's coefficients -- the block and the symbol that hold its first differing bit.  want: the oracle's file."""
    n = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
    text = f"lengths {len(got)} / {len(want)}, first difference at byte {n}"
    off, scan = scan_of(want)
    if n < off or n >= off + len(scan):
        return text + " (outside the scan)"
    k = n - off
    unstuffed = k - scan[:k].count(b"\xff\x00")                      # every stuffed 0x00 in front of it is no byte of the string
    cr = crafted(coef, w, h)
    bit = 8 * unstuffed + (8 - (got[n] ^ want[n]).bit_length() if n < min(len(got), len(want)) else 0)      # the first bit that differs
    i = max(int(np.searchsorted(cr.sym["start"], bit, side="right")) - 1, 0)
    s = cr.sym[i]
    tab = ("luminance DC", "chrominance DC", "luminance AC", "chrominance AC")[int(s["tab"])]
    return text + (f": byte {unstuffed} of the string, in block {int(s['blk'])} (MCU {int(s['blk']) // 6}, slot {int(s['slot'])}), {tab} symbol "
                   f"0x{int(s['sym']):02x} of {int(s['clen'])} + {int(s['size'])} bits at bit {int(s['start'])}, z = {int(s['z'])}")
