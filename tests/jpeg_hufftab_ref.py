"""The optimised Huffman tables of FNX_JPEG_HUFFMAN_OPTIMIZED in plain Python (include/fennec_hip.h states the rule): the symbol
histogram of a scan from its coefficients, the table build of ITU T.81 Annex K.2 under the stated tie order, and the file the
library has to write -- jpeg_craft.encode with those tables behind the standard file's header.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

import jpeg_craft

MAX_CLEN = 32
TCTH = (0x00, 0x10, 0x01, 0x11)          # luminance DC, luminance AC, chrominance DC, chrominance AC


def _category(v):
    return int(abs(int(v))).bit_length()


def symbol_histogram(coef):
    """coef: (blocks, 64) int16, zig-zag order, blocks in scan order (4:2:0: Y0 Y1 Y2 Y3 Cb Cr per MCU), the DC absolute.
    -> (4, 256) int64: what the scan codes with table 0 luminance DC, 1 luminance AC, 2 chrominance DC, 3 chrominance AC."""
    coef = np.asarray(coef)
    assert coef.ndim == 2 and coef.shape[1] == 64 and coef.shape[0] % 6 == 0
    hist = np.zeros((4, 256), np.int64)
    pred = [0, 0, 0]
    for b in range(coef.shape[0]):
        slot = b % 6
        comp = 0 if slot < 4 else slot - 3
        dc_t = 0 if comp == 0 else 2
        zz = coef[b]
        d = int(zz[0]) - pred[comp]
        pred[comp] = int(zz[0])
        hist[dc_t, _category(d)] += 1
        z = 1
        for k in (np.flatnonzero(zz[1:]) + 1).tolist():
            run = k - z
            while run > 15:
                hist[dc_t + 1, 0xF0] += 1
                run -= 16
            hist[dc_t + 1, (run << 4) | _category(zz[k])] += 1
            z = k + 1
        if z < 64:
            hist[dc_t + 1, 0x00] += 1
    return hist


class TooLong(Exception):
    """an unlimited code size above 32: the table is the standard table of its class"""


def code_sizes(hist):
    """figures K.1 and K.2 over slots 0..255 and the reserved slot 256 of frequency 1 -> the 257 unlimited code sizes"""
    freq = [int(v) for v in hist] + [1]
    assert len(freq) == 257 and any(freq[:256])
    size = [0] * 257
    others = [-1] * 257
    while True:
        c1, v = -1, None
        for i in range(257):                      # the least frequency, the LARGEST index among equals
            if freq[i] and (v is None or freq[i] <= v):
                v, c1 = freq[i], i
        c2, v = -1, None
        for i in range(257):
            if freq[i] and i != c1 and (v is None or freq[i] <= v):
                v, c2 = freq[i], i
        if c2 < 0:
            break
        freq[c1] += freq[c2]
        freq[c2] = 0
        size[c1] += 1
        while others[c1] >= 0:
            c1 = others[c1]
            size[c1] += 1
        others[c1] = c2
        size[c2] += 1
        while others[c2] >= 0:
            c2 = others[c2]
            size[c2] += 1
    return size


def build_table(hist):
    """-> (bits[16], vals) of the optimised table; raises TooLong where a code size exceeds 32 (never indexes past bits[])"""
    size = code_sizes(hist)
    if max(size) > MAX_CLEN:
        raise TooLong(max(size))
    bits = [0] * (MAX_CLEN + 1)
    for s in size:
        if s:
            bits[s] += 1
    for i in range(MAX_CLEN, 16, -1):             # figure K.3
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
    i = 16
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                  # the reserved symbol
    vals = [j for s in range(1, MAX_CLEN + 1) for j in range(256) if size[j] == s]
    assert sum(bits[1:17]) == len(vals)
    return bits[1:17], vals


def standard_tables():
    """the four typical tables of Annex K.3.3 as (bits, vals), out of the DHT segment of a standard file"""
    from oracle import oracle
    data = oracle.jpeg_encode(np.zeros((8, 8, 4), np.uint8), 50)
    return dht_tables(data)


def dht_tables(data):
    """every table of a file's DHT segments: {Tc << 4 | Th: (bits, vals)} -> the list in TCTH's order"""
    found = {}
    i = 2
    while i < len(data):
        assert data[i] == 0xFF
        m = data[i + 1]
        ln = (data[i + 2] << 8) | data[i + 3]
        if m == 0xC4:
            p, end = i + 4, i + 2 + ln
            while p < end:
                bits = list(data[p + 1:p + 17])
                n = sum(bits)
                found[data[p]] = (bits, list(data[p + 17:p + 17 + n]))
                p += 17 + n
        if m == 0xDA:
            break
        i += 2 + ln
    return [found[t] for t in TCTH]


def tables(hist4):
    """the four tables of a file -> [(bits, vals, standard)]"""
    out = []
    std = None
    for t in range(4):
        try:
            bits, vals = build_table(hist4[t])
            out.append((bits, vals, 0))
        except TooLong:
            std = std or standard_tables()
            out.append((std[t][0], std[t][1], 1))
    return out


def lut_words(bits, vals):
    """the coder's look-up words of a table: length << 24 | code by symbol, 0 where the symbol has no code"""
    lut = [0] * 256
    for sym, (code, ln) in jpeg_craft.Table(bits, vals).codes.items():
        lut[sym] = (ln << 24) | code
    return lut


def dht_segment(tabs):
    """ONE segment, the four tables in TCTH's order"""
    body = b"".join(bytes([TCTH[t]] + list(tabs[t][0]) + list(tabs[t][1])) for t in range(4))
    return bytes([0xFF, 0xC4, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + body


def _segment_at(data, marker):
    i = 2
    while i < len(data):
        assert data[i] == 0xFF
        ln = (data[i + 2] << 8) | data[i + 3]
        if data[i + 1] == marker:
            return i, i + 2 + ln
        i += 2 + ln
    raise AssertionError(f"no segment {marker:#x}")


def optimized_file(std_file, coef, w, h):
    """std_file: the standard file of the image (oracle.jpeg_encode), coef its coefficients.  -> (the file under
    FNX_JPEG_HUFFMAN_OPTIMIZED, the crafted scan with its symbol map, the four tables)"""
    tabs = tables(symbol_histogram(coef))
    t = [jpeg_craft.Table(b, v) for b, v, _ in tabs]
    crafted = jpeg_craft.encode(coef, w, h, [t[0], t[2]], [t[1], t[3]], sampling=(2, 2))
    d0, d1 = _segment_at(std_file, 0xC4)
    s0, s1 = _segment_at(std_file, 0xDA)
    assert d1 == s0
    data = std_file[:d0] + dht_segment(tabs) + std_file[s0:s1] + crafted.data[crafted.scan_offset:]
    return data, crafted, tabs


def first_difference(got, want, crafted):
    """where two files part: the segment's name, and inside the scan the block (from the writer's symbol map)"""
    n = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
    if n == len(got) == len(want):
        return None
    i, name = 2, "SOI"
    names = {0xDB: "DQT", 0xC0: "SOF0", 0xC4: "DHT", 0xDA: "SOS"}
    scan = None
    while i < len(want) and want[i] == 0xFF and want[i + 1] in names:
        ln = (want[i + 2] << 8) | want[i + 3]
        if n < i:
            break
        name = names[want[i + 1]]
        if want[i + 1] == 0xDA:
            scan = i + 2 + ln
            break
        i += 2 + ln
    if scan is None or n < scan:
        return f"byte {n} (lengths {len(got)} / {len(want)}): segment {name}"
    # the byte's place in the string without stuffing
    body = want[scan:n]
    at = 8 * (len(body) - body.count(b"\xff\x00"))
    k = int(np.searchsorted(crafted.sym["start"], at, side="right")) - 1
    blk = int(crafted.sym["blk"][max(k, 0)])
    return f"byte {n} (lengths {len(got)} / {len(want)}): scan, bit {at}, block {blk}"


def size_bisect(size_of, w, h, target):
    """jpegQualitySearchOpt's bisection (targetsize.go:129-165) over size_of(quality) -> (quality, size, steps)"""
    bpp = target * 8 / (w * h)
    lo, hi = 1, 100
    if bpp < 0.5:
        hi = 40
    elif bpp < 1.0:
        lo, hi = 10, 70
    elif bpp < 2.0:
        lo, hi = 30, 90
    elif bpp > 4.0:
        lo = 60
    q, sz, n = 0, 0, 0
    while lo <= hi:
        mid = (lo + hi) // 2
        ln = size_of(mid)
        n += 1
        if ln <= target:
            q, sz = mid, ln
            lo = mid + 1
        else:
            hi = mid - 1
    return q, sz, n


def geometric_histogram(n):
    """counts ceil(1.7^(i + 1)), i = 0..n-1: the unlimited code size reaches exactly n"""
    import math
    h = [0] * 256
    for i in range(n):
        h[i] = math.ceil(1.7 ** (i + 1))
    return h


def hostsim_histograms():
    """the synthetic part of the list both the hostsim test and the GPU test run: [(name, class, [256 counts])]"""
    out = []
    one = [0] * 256
    one[0x21] = 7
    out.append(("single_symbol", 1, one))
    out.append(("all_equal", 3, [5] * 256))
    for n in (16, 17, 32, 33):
        out.append((f"geometric_{n}", n % 4, geometric_histogram(n)))
    rng = np.random.default_rng(20261020)
    for k in range(200):
        nsym = int(rng.integers(1, 257))
        top = int(2 ** rng.integers(1, 32))                      # counts up to 2^31
        h = np.zeros(256, np.int64)
        h[rng.choice(256, nsym, replace=False)] = rng.integers(1, top + 1, nsym)
        out.append((f"random_{k}", k % 4, h.tolist()))
    return out


# ------------------------------------------------------------------------------------------------ the images of the tests
def _noise(w, h, seed, alpha=False):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if not alpha:
        img[..., 3] = 255
    return img


def _photo_like(w, h, seed):
    """smooth gradients with a little texture: what a photograph's blocks look like to the coder"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.empty((h, w, 4), np.uint8)
    for c, (fx, fy) in enumerate(((0.11, 0.07), (0.05, 0.13), (0.09, 0.03))):
        v = 128 + 70 * np.sin(fx * x + c) * np.cos(fy * y - c) + 25 * np.sin(0.9 * x + 0.7 * y) + rng.normal(0, 6, (h, w))
        img[..., c] = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    img[..., 3] = 255
    return img


def plain_images():
    """name -> image: flat, padded edge MCUs, more than one workgroup of the histogram kernel (288 blocks), translucent"""
    flat = np.full((16, 16, 4), 255, np.uint8)
    flat[..., :3] = 128                           # every DC difference 0, every block an EOB: one symbol per table
    return {"flat_16x16": flat, "edge_17x9": _photo_like(17, 9, 3), "noise_128x96": _noise(128, 96, 5),
            "translucent_40x24": _noise(40, 24, 7, alpha=True)}


def crafted_images():
    """tests/jpeg_enc_cases.py's sheets that reach the AC symbols, the DC categories and the zero runs: name -> (image, quality)"""
    import jpeg_enc_cases
    return {name: (c.img, c.qualities[0]) for name, c in jpeg_enc_cases.cases().items() if name.startswith(("ac_", "dc_", "runs_"))}


def real_histograms():
    """[(name, (4, 256) histogram)] of real coefficients: one symbol per table, noise at quality 90, the crafted sheets"""
    from oracle import oracle
    out = []
    jobs = [("flat_16x16", plain_images()["flat_16x16"], 75), ("noise_48x64_q90", _noise(48, 64, 11), 90)]
    jobs += [(name, img, q) for name, (img, q) in crafted_images().items()]
    for name, img, q in jobs:
        _, coef = oracle.jpeg_encode(img, q, with_coefficients=True)
        out.append((name, symbol_histogram(coef)))
    return out


def all_histograms():
    """the list the hostsim test and the GPU test both run: [(name, class, [256 counts])]"""
    out = []
    for name, h4 in real_histograms():
        for t in range(4):
            out.append((f"{name}_t{t}", t, [int(v) for v in h4[t]]))
    return out + hostsim_histograms()
