"""fnx_png_decode restated in numpy and plain Python integers, straight from the rule above it in include/fennec_hip.h -- the
reference of tests/test_png_decode_*.py -- and a PNG WRITER that makes every case those tests need without Pillow.  Nothing
here shares code with the library: the chunk walk uses zlib.crc32, the stream comes from zlib.decompress, the rows are
reconstructed one by one and the pixel rule is spelt out per pixel kind.

decode(data) -> (h, w, 4) uint8, or raises Damaged / Unsupported.
write_png(samples, color_type, depth, ...) -> bytes; samples: (h, w, channels) integers in the file's own sample range."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SIG = b"\x89PNG\r\n\x1a\n"
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
PAIRS = [(0, 1), (0, 2), (0, 4), (0, 8), (0, 16), (2, 8), (2, 16), (3, 1), (3, 2), (3, 4), (3, 8), (4, 8), (4, 16), (6, 8), (6, 16)]


class Damaged(ValueError):
    pass


class Unsupported(ValueError):
    pass


# ---- the writer -------------------------------------------------------------------------------------------------------------
def chunk(tag: bytes, body: bytes, crc: int | None = None) -> bytes:
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body) if crc is None else crc)


def ihdr(w, h, depth, color_type, compression=0, filt=0, interlace=0) -> bytes:
    return chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, compression, filt, interlace))


def pack_rows(samples, color_type, depth):
    """(h, w, channels) samples -> (h, rowbytes) uint8: depth 1/2/4 packed MSB first (a partial last byte filled with zeros),
    depth 16 big-endian"""
    s = np.asarray(samples)
    if s.ndim == 2:
        s = s[..., None]
    h, w, ch = s.shape
    assert ch == CHANNELS[color_type]
    if depth == 8:
        return np.ascontiguousarray(s.astype(np.uint8)).reshape(h, w * ch)
    if depth == 16:
        v = s.astype(np.uint16).reshape(h, w * ch)
        out = np.empty((h, w * ch * 2), np.uint8)
        out[:, 0::2] = v >> 8
        out[:, 1::2] = v & 255
        return out
    per = 8 // depth
    n = (w * depth + 7) // 8
    padded = np.zeros((h, n * per), np.uint16)
    padded[:, :w] = s[..., 0]
    raw = np.zeros((h, n), np.uint16)
    for e in range(per):
        raw |= padded[:, e::per] << (depth * (per - 1 - e))
    return raw.astype(np.uint8)


def bpp_of(color_type, depth) -> int:
    return max(1, CHANNELS[color_type] * depth // 8)


def paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
    return a if pa <= pb and pa <= pc else b if pb <= pc else c


def filter_stream(raw, bpp, filters):
    """raw (h, n) -> the stream (h, 1 + n): row y filtered with type filters[y] against the RAW row above.  A type above 4 is
    written as it is, the row unfiltered (a damaged file on purpose)."""
    h, n = raw.shape
    out = np.zeros((h, 1 + n), np.uint8)
    prev = np.zeros(n, np.int32)
    for y in range(h):
        t = int(filters[y])
        cur = raw[y].astype(np.int32)
        left = np.zeros(n, np.int32)
        left[bpp:] = cur[:-bpp] if bpp < n else cur[:0]
        ul = np.zeros(n, np.int32)
        ul[bpp:] = prev[:-bpp] if bpp < n else prev[:0]
        if t == 1:
            pred = left
        elif t == 2:
            pred = prev
        elif t == 3:
            pred = (left + prev) >> 1
        elif t == 4:
            pa, pb, pc = np.abs(prev - ul), np.abs(left - ul), np.abs(left + prev - 2 * ul)
            pred = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, prev, ul))
        else:
            pred = np.zeros(n, np.int32)
        out[y, 0] = t
        out[y, 1:] = (cur - pred) & 255
        prev = cur
    return out


def split(body: bytes, sizes):
    """body cut into pieces of the given sizes, the last size repeating"""
    if not sizes:
        return [body]
    out, i, k = [], 0, 0
    while i < len(body):
        n = sizes[min(k, len(sizes) - 1)]
        out.append(body[i:i + n])
        i += n
        k += 1
    return out or [b""]


def write_png(samples, color_type, depth, filters=None, palette=None, trns=None, idat_sizes=None, level=6, interlace=0, extra=()):
    """samples: (h, w, channels) in the file's sample range.  filters: a type per row (default 0).  palette: (n, 3) for PLTE.
    trns: the tRNS chunk's BODY (bytes).  idat_sizes: split sizes of the zlib stream over IDAT chunks.  extra: chunks (bytes)
    placed in front of the first IDAT."""
    s = np.asarray(samples)
    h, w = s.shape[:2]
    raw = pack_rows(s, color_type, depth)
    filters = [0] * h if filters is None else list(filters)
    stream = filter_stream(raw, bpp_of(color_type, depth), filters)
    out = [SIG, ihdr(w, h, depth, color_type, interlace=interlace)]
    if palette is not None:
        out.append(chunk(b"PLTE", np.asarray(palette, np.uint8).reshape(-1, 3).tobytes()))
    if trns is not None:
        out.append(chunk(b"tRNS", bytes(trns)))
    out += list(extra)
    out += [chunk(b"IDAT", piece) for piece in split(zlib.compress(stream.tobytes(), level), idat_sizes)]
    out.append(chunk(b"IEND", b""))
    return b"".join(out)


# ---- the reader -------------------------------------------------------------------------------------------------------------
def parse(data: bytes):
    """the chunk walk -> dict(w, h, color_type, depth, plte (n, 3) or None, trns bytes or None, z)"""
    if data[:8] != SIG:
        raise Damaged("signature")
    pos, first = 8, True
    f = dict(plte=None, trns=None)
    z, stage = [], "hdr"            # hdr -> plte -> trns -> idat -> after
    while True:
        if len(data) - pos < 12:
            raise Damaged("the file ends inside a chunk")
        n, = struct.unpack(">I", data[pos:pos + 4])
        if n > 0x7fffffff or len(data) - pos - 12 < n:
            raise Damaged("chunk length")
        tag, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        if struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] != zlib.crc32(tag + body):
            raise Damaged("CRC")
        pos += 12 + n
        if first:
            if tag != b"IHDR" or n != 13:
                raise Damaged("IHDR is not first")
            w, h, depth, ct, comp, filt, il = struct.unpack(">IIBBBBB", body)
            if not (1 <= w <= 0x7fffffff and 1 <= h <= 0x7fffffff) or (ct, depth) not in PAIRS or comp or filt or il > 1:
                raise Damaged("IHDR")
            if il == 1:
                raise Unsupported("Adam7")
            if w > 65535 or h > 65535:
                raise Unsupported("dimensions")
            f.update(w=w, h=h, depth=depth, color_type=ct)
            first = False
            continue
        ct, depth = f["color_type"], f["depth"]
        if tag == b"IHDR":
            raise Damaged("second IHDR")
        if tag == b"PLTE":
            if stage != "hdr" or ct in (0, 4) or n == 0 or n % 3 or n > 768 or (ct == 3 and n // 3 > 1 << depth):
                raise Damaged("PLTE")
            f["plte"] = np.frombuffer(body, np.uint8).reshape(-1, 3)
            stage = "plte"
        elif tag == b"tRNS":
            if stage in ("trns", "idat", "after") or ct in (4, 6):
                raise Damaged("tRNS")
            if ct == 3 and (stage != "plte" or n > 256):
                raise Damaged("tRNS of a paletted file")
            if ct in (0, 2) and n != (2 if ct == 0 else 6):
                raise Damaged("tRNS length")
            f["trns"] = body
            stage = "trns"
        elif tag == b"IDAT":
            if stage == "after" or (ct == 3 and f["plte"] is None):
                raise Damaged("IDAT")
            z.append(body)
            stage = "idat"
        elif tag == b"IEND":
            if n or stage not in ("idat", "after"):
                raise Damaged("IEND")
            f["z"] = b"".join(z)
            return f
        elif stage == "idat":
            stage = "after"


def unfilter(stream, bpp):
    """(h, 1 + n) -> the reconstructed rows (h, n), row by row, byte by byte where the filter is serial"""
    h, n = stream.shape[0], stream.shape[1] - 1
    out = np.zeros((h, n), np.uint8)
    prev = [0] * n
    for y in range(h):
        t = int(stream[y, 0])
        if t > 4:
            raise Damaged("filter type")
        fr = stream[y, 1:].tolist()
        cur = [0] * n
        if t == 0:
            cur = fr
        elif t == 2:
            cur = [(fr[i] + prev[i]) & 255 for i in range(n)]
        else:
            for i in range(n):
                a = cur[i - bpp] if i >= bpp else 0
                b = prev[i]
                c = prev[i - bpp] if i >= bpp else 0
                pred = a if t == 1 else (a + b) >> 1 if t == 3 else paeth(a, b, c)
                cur[i] = (fr[i] + pred) & 255
        out[y] = cur
        prev = cur
    return out


def nrgba64_pixel(R, G, B, A):
    """convertToNRGBA of a color.NRGBA64, in Python integers"""
    if A == 0:
        return (0, 0, 0, 0)
    if A == 0xffff:
        return (R >> 8, G >> 8, B >> 8, 255)
    return tuple(((v * A // 0xffff) * 0xffff // A) >> 8 for v in (R, G, B)) + (A >> 8,)


def palette_pixel(r, g, b, t):
    """a Paletted entry (r, g, b, t) as color.NRGBA through convertToNRGBA"""
    if t == 255:
        return (r, g, b, 255)
    if t == 0:
        return (0, 0, 0, 0)
    a16 = t * 0x101
    return tuple((((v * 0x101) * t // 0xff) * 0xffff // a16) >> 8 for v in (r, g, b)) + (t,)


def palette_table(plte, trns):
    tab = np.zeros((256, 4), np.uint8)
    for i in range(256):
        r, g, b = (int(v) for v in plte[i]) if i < len(plte) else (0, 0, 0)
        t = trns[i] if trns is not None and i < len(trns) else 255
        tab[i] = palette_pixel(r, g, b, t)
    return tab


def samples_of(rows, w, color_type, depth):
    """reconstructed rows -> (h, w, channels) integer samples"""
    ch = CHANNELS[color_type]
    h = rows.shape[0]
    if depth == 8:
        return rows[:, :w * ch].astype(np.int64).reshape(h, w, ch)
    if depth == 16:
        v = rows[:, :w * ch * 2].astype(np.int64)
        return ((v[:, 0::2] << 8) | v[:, 1::2]).reshape(h, w, ch)
    per = 8 // depth
    out = np.zeros((h, rows.shape[1] * per), np.int64)
    for e in range(per):
        out[:, e::per] = (rows >> (depth * (per - 1 - e))) & ((1 << depth) - 1)
    return out[:, :w].reshape(h, w, 1)


def expand(rows, w, color_type, depth, plte=None, trns=None):
    """image.Decode's pixel model + toNRGBA, per the table above fnx_png_decode"""
    s = samples_of(rows, w, color_type, depth)
    h = s.shape[0]
    out = np.zeros((h, w, 4), np.uint8)
    if color_type == 3:
        return palette_table(plte, trns)[s[..., 0]]
    key = None if trns is None else [int.from_bytes(trns[2 * k:2 * k + 2], "big") for k in range(len(trns) // 2)]
    if depth <= 8:
        if color_type == 0:
            y = s[..., 0] * {1: 0xff, 2: 0x55, 4: 0x11, 8: 1}[depth]
            out[..., 0] = out[..., 1] = out[..., 2] = y
            out[..., 3] = 255
            if key is not None:
                out[..., 3] = np.where(s[..., 0] == (key[0] & 0xff), 0, 255)
        elif color_type == 2:
            out[..., :3] = s
            out[..., 3] = 255
            if key is not None:
                hit = (s[..., 0] == (key[0] & 0xff)) & (s[..., 1] == (key[1] & 0xff)) & (s[..., 2] == (key[2] & 0xff))
                out[..., 3] = np.where(hit, 0, 255)
        elif color_type == 4:
            out[..., 0] = out[..., 1] = out[..., 2] = s[..., 0]
            out[..., 3] = s[..., 1]
        else:
            out[...] = s
        return out
    # 16 bits
    if color_type in (0, 2) and key is None:
        out[..., :3] = (s >> 8) if color_type == 2 else (s[..., :1] >> 8)
        out[..., 3] = 255
        return out
    for yy in range(h):
        for xx in range(w):
            v = [int(t) for t in s[yy, xx]]
            if color_type == 0:
                px = (v[0], v[0], v[0], 0 if v[0] == key[0] else 0xffff)
            elif color_type == 2:
                px = (v[0], v[1], v[2], 0 if v == key else 0xffff)
            elif color_type == 4:
                px = (v[0], v[0], v[0], v[1])
            else:
                px = tuple(v)
            out[yy, xx] = nrgba64_pixel(*px)
    return out


def decode(data: bytes):
    f = parse(data)
    ch = CHANNELS[f["color_type"]]
    rowbytes = (f["w"] * ch * f["depth"] + 7) // 8
    try:
        d = zlib.decompressobj()
        raw = d.decompress(f["z"])
        if not d.eof:
            raise Damaged("the zlib stream ends early")
    except zlib.error as e:
        raise Damaged(str(e))
    if len(raw) != f["h"] * (1 + rowbytes):
        raise Damaged("not enough / too much pixel data")
    stream = np.frombuffer(raw, np.uint8).reshape(f["h"], 1 + rowbytes)
    rows = unfilter(stream, bpp_of(f["color_type"], f["depth"]))
    return expand(rows, f["w"], f["color_type"], f["depth"], f["plte"], f["trns"])


def filter_types(data: bytes):
    """the filter type of every row of a file"""
    f = parse(data)
    rowbytes = (f["w"] * CHANNELS[f["color_type"]] * f["depth"] + 7) // 8
    return list(zlib.decompress(f["z"])[::1 + rowbytes])


# ---- content shared by the CPU and GPU tests --------------------------------------------------------------------------------
def random_samples(w, h, color_type, depth, seed, palette_len=None):
    """samples over the whole range; alpha channels get 0, full and partial values in every image"""
    rng = np.random.default_rng(seed)
    ch = CHANNELS[color_type]
    top = (palette_len if color_type == 3 and palette_len else 1 << depth)
    s = rng.integers(0, top, size=(h, w, ch), dtype=np.int64)
    if color_type in (4, 6):
        full = (1 << depth) - 1
        pick = rng.integers(0, 3, size=(h, w))
        s[..., -1] = np.where(pick == 0, 0, np.where(pick == 1, full, s[..., -1]))
    return s


def random_palette(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(n, 3), dtype=np.uint8)
