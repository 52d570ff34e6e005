"""The PNG encoder's row stage restated in numpy, straight from the rule above fnx_png_filter in include/fennec_hip.h, and a
minimal chunk writer -- the reference of tests/test_png_filter_*.py.  Nothing here shares code with the library.

raw_rows: the packing (alpha dropped for opaque images, indices packed MSB first).  filter_rows: the five filters against
the raw row above, the sum of abs8 over each, the first smallest in the order Up, Paeth, None, Sub, Average."""
from __future__ import annotations

import struct
import zlib

import numpy as np

PALETTED, GRAY, NRGBA = 1, 2, 3            # fennec_amd.FNX_PNG_*
ORDER = (2, 4, 0, 1, 3)                    # Up, Paeth, None, Sub, Average


def visible_opaque(img) -> bool:
    """image.NRGBA.Opaque(): the w visible pixels of the h rows"""
    return bool(np.all(img[..., 3] == 255))


def depth_of(ncolors: int) -> int:
    return 1 if ncolors <= 2 else 2 if ncolors <= 4 else 4 if ncolors <= 16 else 8


def raw_rows(src, kind, ncolors=0, opaque=-1):
    """-> (raw (h, n) uint8, bpp or 0 for paletted, color_type, bit_depth)"""
    src = np.asarray(src)
    if kind == NRGBA:
        h, w = src.shape[:2]
        if opaque < 0:
            opaque = 1 if visible_opaque(src) else 0
        if opaque:
            return np.ascontiguousarray(src[..., :3]).reshape(h, 3 * w), 3, 2, 8
        return np.ascontiguousarray(src).reshape(h, 4 * w), 4, 6, 8
    h, w = src.shape
    if kind == GRAY:
        return np.ascontiguousarray(src), 1, 0, 8
    depth = depth_of(ncolors)
    if depth == 8:
        return np.ascontiguousarray(src), 0, 3, 8
    per = 8 // depth
    n = (w * depth + 7) // 8
    padded = np.zeros((h, n * per), dtype=np.uint16)
    padded[:, :w] = src
    raw = np.zeros((h, n), dtype=np.uint16)
    for e in range(per):                   # the first pixel of a byte in its top bits; a partial last byte filled with zeros
        raw |= padded[:, e::per] << (depth * (per - 1 - e))
    return (raw & 255).astype(np.uint8), 0, 3, depth


def _shift(a, bpp):
    out = np.zeros_like(a)
    out[bpp:] = a[:-bpp] if bpp < len(a) else a[:0]
    return out


def residuals(cur, prev, bpp):
    """the five filtered rows (uint8, mod 256) of one raw row, indexed by PNG filter type"""
    c, p = cur.astype(np.int32), prev.astype(np.int32)
    left, ul = _shift(c, bpp), _shift(p, bpp)
    pa, pb, pc = np.abs(p - ul), np.abs(left - ul), np.abs(left + p - 2 * ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, p, ul))
    return [((c - pred) & 255).astype(np.uint8) for pred in (0 * c, left, p, (left + p) >> 1, paeth)]


def abs8_sum(row) -> int:
    d = row.astype(np.int64)
    return int(np.where(d < 128, d, 256 - d).sum())


def filter_rows(raw, bpp):
    """-> (stream (h, 1 + n) uint8, the chosen types (h,))"""
    h, n = raw.shape
    out = np.zeros((h, 1 + n), dtype=np.uint8)
    prev = np.zeros(n, dtype=np.uint8)
    for y in range(h):
        if bpp == 0:                       # paletted rows are never filtered
            out[y, 1:] = raw[y]
        else:
            rows = residuals(raw[y], prev, bpp)
            best, cost = ORDER[0], abs8_sum(rows[ORDER[0]])
            for f in ORDER[1:]:
                s = abs8_sum(rows[f])
                if s < cost:
                    best, cost = f, s
            out[y, 0] = best
            out[y, 1:] = rows[best]
        prev = raw[y]
    return out, out[:, 0].copy()


def png_stream(src, kind, ncolors=0, opaque=-1):
    """-> (stream (h, 1 + n) uint8, color_type, bit_depth)"""
    raw, bpp, color_type, depth = raw_rows(src, kind, ncolors, opaque)
    return filter_rows(raw, bpp)[0], color_type, depth


def _chunk(tag: bytes, body: bytes) -> bytes:
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body))


def write_png(stream, w, h, color_type, depth, palette=None) -> bytes:
    """signature, IHDR, PLTE, tRNS (up to the last alpha != 255), IDAT, IEND"""
    out = [b"\x89PNG\r\n\x1a\n", _chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, 0))]
    if color_type == 3:
        pal = np.asarray(palette, dtype=np.uint8).reshape(-1, 4)
        out.append(_chunk(b"PLTE", pal[:, :3].tobytes()))
        keep = 0
        for i, a in enumerate(pal[:, 3]):
            if a != 255:
                keep = i + 1
        if keep:
            out.append(_chunk(b"tRNS", pal[:keep, 3].tobytes()))
    out += [_chunk(b"IDAT", zlib.compress(np.ascontiguousarray(stream).tobytes(), 9)), _chunk(b"IEND", b"")]
    return b"".join(out)


def decode_png(data: bytes):
    """Pillow's reading of a file as (h, w, 4) NRGBA"""
    import io

    from PIL import Image
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGBA"))


def chunks(data: bytes):
    """[(tag, body)] of a PNG file, CRCs checked"""
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    out, i = [], 8
    while i < len(data):
        n, = struct.unpack(">I", data[i:i + 4])
        tag, body = data[i + 4:i + 8], data[i + 8:i + 8 + n]
        assert struct.unpack(">I", data[i + 8 + n:i + 12 + n])[0] == zlib.crc32(tag + body), tag
        out.append((tag, body))
        i += 12 + n
    return out


# ---- content shared by the CPU and GPU tests --------------------------------------------------------------------------
def noise_rgba(w, h, seed, opaque=True):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(h, w, 4), dtype=np.uint8)
    if opaque:
        img[..., 3] = 255
    return img


def smooth_rgba(w, h, seed, opaque=True):
    """gradients with a little noise: Sub, Average and Paeth territory"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([x * 3 + y, x + y * 2, (x * y) // 7 + 40, 255 - x // 2], axis=-1)
    img = ((base + rng.integers(0, 3, size=base.shape)) & 255).astype(np.uint8)
    if opaque:
        img[..., 3] = 255
    return np.ascontiguousarray(img)


def tie_cases():
    """[(name, NRGBA image (opaque), expected types per row)] with the answers the rule gives on paper"""
    zero = np.zeros((4, 9, 4), np.uint8)
    zero[..., 3] = 255
    const = np.full((4, 9, 4), 77, np.uint8)
    const[..., 3] = 255
    return [
        # every residual of every filter is 0: the first one tried stays
        ("all_zero", zero, [2, 2, 2, 2]),
        # row 0: Up = None = 27 x 77, Paeth = Sub = 3 x 77 (left neighbours only), Average = 3 x 77 + 24 x 39: Paeth is tried
        # before Sub and stays; below, Up is all zeros
        ("constant", const, [4, 2, 2, 2]),
    ]


def abs8_cases():
    """[(name, gray plane of one row, the five sums by type number, the expected type)], worked out on paper.  The row above
    is zeros, so Up = None and Paeth = Sub (left is the only non-zero neighbour), and only the order of trial separates them.
      [0, 1, 129]    None 0+1+127, Sub 0+1+128 (129 - 1 = 128), Average 0+1+127 (129 - (1 >> 1)): Up stays, 128 < 129.
                     Without the fold (129 costs 129, as a byte SAD of the operands gives) None would cost 130 and Paeth win.
      [0, 1, 128]    None 0+1+128, Sub 0+1+127, Average 0+1+128: Paeth, 128 < 129.  With abs8(128) = 127 all five tie
                     at 128 and Up would stay; with abs8(128) = -128 Up would win outright.
      [0, 129, 127]  None 0+127+127, Sub 0+127+2 (127 - 129 = 254), Average 0+127+63 (127 - 64): Paeth, 129.  Without
                     the fold Sub costs 0+129+254 and Average (0+129+63) would win."""
    return [
        ("fold_129", np.array([[0, 1, 129]], np.uint8), [128, 129, 128, 128, 129], 2),
        ("keep_128", np.array([[0, 1, 128]], np.uint8), [129, 128, 129, 129, 128], 4),
        ("both_sides", np.array([[0, 129, 127]], np.uint8), [254, 129, 254, 190, 129], 4),
    ]
