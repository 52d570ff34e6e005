"""FNX_JPEG_SUBSAMPLING_444 in plain numpy (include/fennec_hip.h states the rule above fnx_ctx_set_jpeg_subsampling): writer.go's
file with every component at sampling 1 x 1, restated from the oracle's per-block primitives -- rgb_to_ycbcr, jpeg_fdct, jpeg_idct,
jpeg_quant_tables, ycbcr_to_nrgba(ratio 0) -- and written by tests/jpeg_craft.py's coefficient-level writer.  The cases of
tests/test_jpeg444_ref.py (CPU) and tests/test_jpeg444_gpu.py live here too.  Test infrastructure only."""
from __future__ import annotations

import functools

import numpy as np

import jpeg_craft as jc
import jpeg_hufftab_ref as href
from oracle import oracle as orc

QUALITIES = (1, 50, 75, 100)
TCTH = href.TCTH


# ----------------------------------------------------------------------------------------------------------- the definition
def dims(w, h):
    """mx, my: the padding is to 8, not to 16"""
    return (w + 7) // 8, (h + 7) // 8


def ycc_planes(img):
    """(3, 8 my, 8 mx) uint8: Y, Cb, Cr of every pixel min(x, w - 1), min(y, h - 1) (toYCbCr's clamp), each through
    color.RGBToYCbCr of its premultiplied RGB (color.NRGBA.RGBA(): c * 0x101 * a / 0xff, the high byte kept); no averaging"""
    h, w = img.shape[:2]
    mx, my = dims(w, h)
    ys, xs = np.minimum(np.arange(8 * my), h - 1), np.minimum(np.arange(8 * mx), w - 1)
    px = img[ys][:, xs].astype(np.uint32)
    rgb = ((px[..., :3] * 0x101 * px[..., 3:4] // 0xff) >> 8).astype(np.uint8)
    colours, inverse = np.unique(rgb.reshape(-1, 3), axis=0, return_inverse=True)
    ycc = np.array([orc.rgb_to_ycbcr(int(r), int(g), int(b)) for r, g, b in colours], np.uint8)
    return np.ascontiguousarray(ycc[inverse.reshape(-1)].reshape(8 * my, 8 * mx, 3).transpose(2, 0, 1))


def fdct_blocks(planes):
    """(3, my, mx, 64) int32, natural order: fdct.go of every block (level shift included, scaled up by 8)"""
    _, ph, pw = planes.shape
    my, mx = ph // 8, pw // 8
    out = np.empty((3, my, mx, 64), np.int32)
    for c in range(3):
        for by in range(my):
            for bx in range(mx):
                out[c, by, bx] = orc.jpeg_fdct(planes[c, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8]).reshape(64)
    return out


def quantisers(quality):
    """(2, 64) int64, natural order: table 0 for Y, table 1 for Cb and Cr"""
    lum, chr_ = orc.jpeg_quant_tables(quality)
    return np.stack([lum.reshape(64), chr_.reshape(64)]).astype(np.int64)


def quantise(fd, quality):
    """writer.go div(b, 8 q): nearest, halves away from zero, in exact integers -> (3, my, mx, 64) int64, natural order"""
    q = quantisers(quality)[[0, 1, 1]][:, None, None, :]
    b = fd.astype(np.int64)
    return np.sign(b) * ((np.abs(b) + 4 * q) // (8 * q))


def scan_coefficients(quant):
    """(3 mx my, 64) int16, zig-zag order, blocks in scan order: raster order, the MCU is Y Cb Cr; the DC absolute"""
    _, my, mx, _ = quant.shape
    return np.ascontiguousarray(quant.transpose(1, 2, 0, 3).reshape(my * mx * 3, 64)[:, jc.ZIG]).astype(np.int16)


def decoded_planes(quant, quality):
    """reader.go: multiplication by q, idct.go, level shift and clip -> (3, 8 my, 8 mx) uint8"""
    _, my, mx, _ = quant.shape
    deq = quant * quantisers(quality)[[0, 1, 1]][:, None, None, :]
    out = np.empty((3, 8 * my, 8 * mx), np.uint8)
    for c in range(3):
        for by in range(my):
            for bx in range(mx):
                s = orc.jpeg_idct(deq[c, by, bx].astype(np.int32))
                out[c, 8 * by:8 * by + 8, 8 * bx:8 * bx + 8] = np.clip(s, -128, 127) + 128
    return out


def to_nrgba(planes, w, h):
    """toNRGBARef of the image.YCbCr (ratio 4:4:4) the file decodes to"""
    return np.ascontiguousarray(orc.ycbcr_to_nrgba(planes[0], planes[1], planes[2], 0)[:h, :w])


def symbol_histogram(coef):
    """jpeg_hufftab_ref.symbol_histogram for the 4:4:4 scan: (4, 256) int64, luminance DC / AC for Y, chrominance DC / AC for Cb
    and Cr, the DC predictions per component (three scan positions back, 0 at the first MCU)"""
    coef = np.asarray(coef)
    assert coef.ndim == 2 and coef.shape[1] == 64 and coef.shape[0] % 3 == 0
    hist = np.zeros((4, 256), np.int64)
    pred = [0, 0, 0]
    for b in range(coef.shape[0]):
        comp = b % 3
        dc_t = 0 if comp == 0 else 2
        zz = coef[b]
        d = int(zz[0]) - pred[comp]
        pred[comp] = int(zz[0])
        hist[dc_t, abs(d).bit_length()] += 1
        z = 1
        for k in (np.flatnonzero(zz[1:]) + 1).tolist():
            run = k - z
            hist[dc_t + 1, 0xF0] += run >> 4
            hist[dc_t + 1, ((run & 15) << 4) | abs(int(zz[k])).bit_length()] += 1
            z = k + 1
        if z < 64:
            hist[dc_t + 1, 0x00] += 1
    return hist


@functools.lru_cache(None)
def standard_tables():
    return tuple((tuple(b), tuple(v)) for b, v in href.standard_tables())


def craft(coef, w, h, quality, tabs=None):
    """jpeg_craft's file of these coefficients at sampling 1 x 1 with the quality's tables; tabs: four (bits, vals, ...) in TCTH's
    order (default: the typical tables)"""
    t = [jc.Table(x[0], x[1]) for x in (tabs or standard_tables())]
    q = quantisers(quality)[:, jc.ZIG].tolist()
    return jc.encode(coef, w, h, [t[0], t[2]], [t[1], t[3]], sampling=(1, 1), qtabs=q)


def _sof0_y_sampling(data):
    i, _ = href._segment_at(data, 0xC0)
    assert data[i + 9] == 3 and data[i + 10] == 1                    # three components, the first is Y
    return i + 11


def header_444(file_420):
    """the header the library writes at 4:4:4 out of its 4:2:0 file of the same w, h, quality and Huffman mode: one byte of SOF0"""
    _, end = href._segment_at(file_420, 0xDA)
    at = _sof0_y_sampling(file_420)
    assert file_420[at] == 0x22
    return file_420[:at] + b"\x11" + file_420[at + 1:end]


class Ref:
    """One image at one quality, computed once: coef (scan order, zig-zag), planes (the decoded file's), image (toNRGBARef of
    them), crafted (the writer's file with its symbol map), scan (the entropy-coded segment), file (what fnx_jpeg_encode writes:
    header_444 of the oracle's 4:2:0 file, the segment, EOI), hist; and under FNX_JPEG_HUFFMAN_OPTIMIZED: opt_tabs, opt_crafted,
    opt_file."""

    def __init__(self, img, quality, fd=None):
        self.h, self.w = img.shape[:2]
        self.quality = quality
        fd = fdct_blocks(ycc_planes(img)) if fd is None else fd
        self.quant = quantise(fd, quality)
        self.coef = scan_coefficients(self.quant)
        self.std_420 = orc.jpeg_encode(img, quality)
        self.header = header_444(self.std_420)
        self.crafted = craft(self.coef, self.w, self.h, quality)
        self.scan = self.crafted.data[self.crafted.scan_offset:-2]
        self.file = self.header + self.scan + b"\xff\xd9"

    @functools.cached_property
    def planes(self):
        return decoded_planes(self.quant, self.quality)

    @functools.cached_property
    def image(self):
        return to_nrgba(self.planes, self.w, self.h)

    @functools.cached_property
    def hist(self):
        return symbol_histogram(self.coef)

    @functools.cached_property
    def opt_tabs(self):
        return href.tables(self.hist)

    @functools.cached_property
    def opt_crafted(self):
        return craft(self.coef, self.w, self.h, self.quality, self.opt_tabs)

    @functools.cached_property
    def opt_file(self):
        d0, d1 = href._segment_at(self.header, 0xC4)
        assert d1 == href._segment_at(self.header, 0xDA)[0]
        return self.header[:d0] + href.dht_segment(self.opt_tabs) + self.header[d1:] + self.opt_crafted.data[self.opt_crafted.scan_offset:]


def first_difference(got_scan, want_scan, crafted):
    """A sentence for two entropy-coded segments that differ: the first differing bit's block and symbol, from the writer's map"""
    n = next((i for i, (a, b) in enumerate(zip(got_scan, want_scan)) if a != b), min(len(got_scan), len(want_scan)))
    if n == len(got_scan) == len(want_scan):
        return None
    text = f"lengths {len(got_scan)} / {len(want_scan)}, first difference at byte {n} of the segment"
    unstuffed = n - want_scan[:n].count(b"\xff\x00")
    bit = 8 * unstuffed + (8 - (got_scan[n] ^ want_scan[n]).bit_length() if n < min(len(got_scan), len(want_scan)) else 0)
    s = crafted.sym[max(int(np.searchsorted(crafted.sym["start"], bit, side="right")) - 1, 0)]
    tab = ("luminance DC", "chrominance DC", "luminance AC", "chrominance AC")[int(s["tab"])]
    blk = int(s["blk"])
    return text + (f": bit {bit} of the string, block {blk} (MCU {blk // 3}, {'Y Cb Cr'.split()[blk % 3]}), {tab} symbol 0x{int(s['sym']):02x} of "
                   f"{int(s['clen'])} + {int(s['size'])} bits at bit {int(s['start'])}, z = {int(s['z'])}")


# ---------------------------------------------------------------------------------------------------------------- the searches
def quality_search(score_of, target):
    """compressJPEGOptimal's bisection (compress.go:24-74) over score_of(quality) -> (quality, ssim, steps, found, scores tried)"""
    target = 0.999 if target >= 1.0 else target
    lo, hi = 1, 100
    if target >= 0.99:
        lo = 75
    elif target >= 0.97:
        lo = 50
    elif target >= 0.94:
        lo = 30
    elif target >= 0.90:
        lo = 15
    best_q, best_s, steps, found, tried = 100, 1.0, 0, False, {}
    while lo <= hi:
        mid = (lo + hi) // 2
        s = score_of(mid)
        tried[mid] = s
        steps += 1
        if s >= target:
            best_q, best_s, found = mid, s, True
            hi = mid - 1
        else:
            lo = mid + 1
    return best_q, best_s, steps, found, tried


# ------------------------------------------------------------------------------------------------------------------ the cases
def noise(w, h, seed):
    img = np.random.default_rng(seed).integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = 255
    return img


def ramp(w, h):
    """a smooth ramp: red along x, green along y, blue along the diagonal"""
    y, x = np.mgrid[0:h, 0:w]
    img = np.full((h, w, 4), 255, np.uint8)
    img[..., 0] = x * 255 // max(w - 1, 1)
    img[..., 1] = y * 255 // max(h - 1, 1)
    img[..., 2] = (x + y) * 255 // max(w + h - 2, 1)
    return img


def translucent(w, h, seed):
    """noise whose alpha mixes 0, 1, 128, 254 and 255: the premultiplied branch and the opaque one, pixel by pixel"""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    img[..., 3] = np.array([0, 1, 128, 254, 255], np.uint8)[rng.integers(0, 5, (h, w))]
    return img


def photo_like(w, h, seed):
    return href._photo_like(w, h, seed)


SMALL = ((1, 1), (7, 9), (8, 8), (16, 16), (17, 23))       # clamping; padding to 8, not 16
LARGE = ((264, 24), (24, 520), (528, 40))                  # 297 scan blocks and a 256-px colour workgroup inside the row; grid y; SSIMFast's downsampled branch


@functools.lru_cache(None)
def cases():
    """name -> (image, qualities)"""
    import jpeg_enc_cases
    out = {}
    for k, (w, h) in enumerate(SMALL):
        out[f"noise_{w}x{h}"] = (noise(w, h, 100 + k), QUALITIES)
    for k, (w, h) in enumerate(LARGE):
        out[f"noise_{w}x{h}"] = (noise(w, h, 200 + k), (75,))
    out["ramp_17x23"] = (ramp(17, 23), QUALITIES)
    out["ramp_264x24"] = (ramp(264, 24), (75,))
    out["translucent_17x23"] = (translucent(17, 23, 300), QUALITIES)
    out["translucent_264x24"] = (translucent(264, 24, 301), (75,))
    enc = jpeg_enc_cases.cases()
    for name in ("runs_gray", "ac_gray_q100", "shape_c_binary_noise"):      # ZRLs; every (run, size) up to size 10; saturated samples
        out[name] = (np.ascontiguousarray(enc[name].img), enc[name].qualities[:1])
    for v in out.values():
        v[0].setflags(write=False)
    return out


@functools.lru_cache(None)
def _fdct_of(name):
    return fdct_blocks(ycc_planes(image(name)))


def image(name):
    return cases()[name][0] if name in cases() else extra_images()[name]


@functools.lru_cache(None)
def extra_images():
    """the searches' images (not among the byte-for-byte cases)"""
    out = {"photo_48x40": photo_like(48, 40, 21), "photo_528x40": photo_like(528, 40, 23)}
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(None)
def ref(name, quality):
    """the restatement of one case at one quality: computed once, shared, never changed"""
    return Ref(image(name), quality, _fdct_of(name))
