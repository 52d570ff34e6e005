"""Adam7-interlaced PNG files for the tests, built from png_decode_ref's functions alone: the rule above fnx_png_decode in
include/fennec_hip.h says that the inflated stream is the present passes back to back, each an image of its own with its own
packed rows and filter bytes -- so a writer is pack_rows + filter_stream per pass, and a reader unfilter + expand per pass.

write_adam7(samples, color_type, depth, ...) -> bytes      decode_adam7(data) -> (h, w, 4) uint8, or raises ref.Damaged
passes(w, h, color_type, depth) -> (pw[7], ph[7], rowbytes[7], stream_bytes), absent passes as zeros"""
from __future__ import annotations

import struct
import zlib

import numpy as np

import png_decode_ref as ref

PASSES = [(0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)]   # x0, y0, dx, dy


def passes(w, h, color_type, depth):
    bits = ref.CHANNELS[color_type] * depth
    pw, ph, rb, total = [], [], [], 0
    for x0, y0, dx, dy in PASSES:
        cw, ch = len(range(x0, w, dx)), len(range(y0, h, dy))
        if cw == 0 or ch == 0:
            cw = ch = 0
        pw.append(cw)
        ph.append(ch)
        rb.append((cw * bits + 7) // 8 if cw else 0)
        total += ch * (1 + rb[-1]) if cw else 0
    return pw, ph, rb, total


def pass_filters(filters, h, w):
    """filters: None (all 0), an int seed (random types 0..4 per pass row), or a list of seven lists -> seven lists"""
    counts = [len(range(y0, h, dy)) if len(range(x0, w, dx)) else 0 for x0, y0, dx, dy in PASSES]
    if filters is None:
        return [[0] * n for n in counts]
    if isinstance(filters, (int, np.integer)):
        rng = np.random.default_rng(int(filters))
        return [rng.integers(0, 5, size=n).tolist() for n in counts]
    assert len(filters) == 7 and all(len(f) == n for f, n in zip(filters, counts)), "a filter type per row of every pass"
    return [list(f) for f in filters]


def adam7_stream(samples, color_type, depth, filters=None) -> bytes:
    """the bytes zlib compresses: the present passes' filtered rows back to back"""
    s = np.asarray(samples)
    if s.ndim == 2:
        s = s[..., None]
    h, w = s.shape[:2]
    fl = pass_filters(filters, h, w)
    out = []
    for p, (x0, y0, dx, dy) in enumerate(PASSES):
        sub = s[y0::dy, x0::dx]
        if sub.shape[0] == 0 or sub.shape[1] == 0:
            continue
        out.append(ref.filter_stream(ref.pack_rows(sub, color_type, depth), ref.bpp_of(color_type, depth), fl[p]).tobytes())
    return b"".join(out)


def file_around(stream: bytes, w, h, color_type, depth, palette=None, trns=None, idat_sizes=None, level=6, z=None) -> bytes:
    """an Adam7 file whose inflated stream is `stream` (z: the IDAT bytes as they are, instead of zlib.compress(stream))"""
    out = [ref.SIG, ref.ihdr(w, h, depth, color_type, interlace=1)]
    if palette is not None:
        out.append(ref.chunk(b"PLTE", np.asarray(palette, np.uint8).reshape(-1, 3).tobytes()))
    if trns is not None:
        out.append(ref.chunk(b"tRNS", bytes(trns)))
    body = zlib.compress(stream, level) if z is None else z
    out += [ref.chunk(b"IDAT", piece) for piece in ref.split(body, idat_sizes)]
    out.append(ref.chunk(b"IEND", b""))
    return b"".join(out)


def write_adam7(samples, color_type, depth, filters=None, palette=None, trns=None, idat_sizes=None, level=6) -> bytes:
    s = np.asarray(samples)
    h, w = s.shape[:2]
    return file_around(adam7_stream(s, color_type, depth, filters), w, h, color_type, depth, palette, trns, idat_sizes, level)


def deinterlaced_header(data: bytes) -> bytes:
    """the file with interlace 0 in its IHDR and a fresh CRC, so that ref.parse walks its chunks; Damaged where there is no
    Adam7 IHDR to rewrite"""
    if data[:8] != ref.SIG or len(data) < 33 or data[12:16] != b"IHDR" or data[8:12] != struct.pack(">I", 13):
        raise ref.Damaged("signature / IHDR")
    if struct.unpack(">I", data[29:33])[0] != zlib.crc32(data[12:29]):
        raise ref.Damaged("CRC")
    if data[28] != 1:
        raise ref.Damaged("not an Adam7 file")
    return data[:8] + ref.chunk(b"IHDR", data[16:28] + b"\0") + data[33:]


def inflate(z: bytes) -> bytes:
    try:
        d = zlib.decompressobj()
        raw = d.decompress(z)
        if not d.eof:
            raise ref.Damaged("the zlib stream ends early")
    except zlib.error as e:
        raise ref.Damaged(str(e))
    return raw


def pass_filter_types(data: bytes):
    """the filter bytes of every pass of a file, seven lists"""
    f = ref.parse(deinterlaced_header(data))
    raw = inflate(f["z"])
    _, ph, rb, total = passes(f["w"], f["h"], f["color_type"], f["depth"])
    if len(raw) != total:
        raise ref.Damaged("not enough / too much pixel data")
    out, at = [], 0
    for p in range(7):
        out.append(list(raw[at:at + ph[p] * (1 + rb[p]):1 + rb[p]]) if ph[p] else [])
        at += ph[p] * (1 + rb[p])
    return out


def decode_adam7(data: bytes):
    f = ref.parse(deinterlaced_header(data))
    w, h, ct, depth = f["w"], f["h"], f["color_type"], f["depth"]
    raw = inflate(f["z"])
    pw, ph, rb, total = passes(w, h, ct, depth)
    if len(raw) != total:
        raise ref.Damaged("not enough / too much pixel data")
    out = np.zeros((h, w, 4), np.uint8)
    at = 0
    for p, (x0, y0, dx, dy) in enumerate(PASSES):
        if ph[p] == 0:
            continue
        n = ph[p] * (1 + rb[p])
        stream = np.frombuffer(raw[at:at + n], np.uint8).reshape(ph[p], 1 + rb[p])
        at += n
        rows = ref.unfilter(stream, ref.bpp_of(ct, depth))
        out[y0::dy, x0::dx] = ref.expand(rows, pw[p], ct, depth, f["plte"], f["trns"])
    return out
