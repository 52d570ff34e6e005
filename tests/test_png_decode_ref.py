"""tests/png_decode_ref.py -- the GPU tests' reference -- held against Pillow, against the encoder-side restatement
(png_filter_ref) and against cases worked out by hand for every arithmetic branch of the rule above fnx_png_decode."""
from __future__ import annotations

import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_decode_ref as ref  # noqa: E402
import png_filter_ref as enc  # noqa: E402


def _pillow_file(im, **kw) -> bytes:
    b = io.BytesIO()
    im.save(b, "PNG", **kw)
    return b.getvalue()


def _smooth(w, h, ch, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = np.stack([(x * (3 + k) + y * (k + 1)) for k in range(ch)], -1)
    return ((base + rng.integers(0, 4, size=base.shape)) & 255).astype(np.uint8)


@pytest.mark.parametrize("mode,ch", [("L", 1), ("LA", 2), ("RGB", 3), ("RGBA", 4)])
def test_against_pillow_8bit(mode, ch):
    Image = pytest.importorskip("PIL.Image")
    a = _smooth(37, 29, ch, 3)                     # smooth content: Pillow's encoder picks all five filters
    data = _pillow_file(Image.fromarray(a[..., 0] if ch == 1 else a, mode))
    assert ref.parse(data)["color_type"] == {1: 0, 2: 4, 3: 2, 4: 6}[ch]
    assert len(set(ref.filter_types(data))) >= 2
    want = np.asarray(Image.open(io.BytesIO(data)).convert("RGBA"))
    assert np.array_equal(ref.decode(data), want)


def test_against_pillow_1bit_and_16bit_grey():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2, size=(13, 21)).astype(bool)
    data = _pillow_file(Image.fromarray(bits))
    f = ref.parse(data)
    assert (f["color_type"], f["depth"]) == (0, 1)
    got = ref.decode(data)
    assert np.array_equal(got[..., 0], np.where(bits, 255, 0)) and np.all(got[..., 3] == 255)
    g16 = rng.integers(0, 65536, size=(11, 17)).astype(np.uint16)
    data = _pillow_file(Image.fromarray(g16))
    f = ref.parse(data)
    assert (f["color_type"], f["depth"]) == (0, 16)
    back = np.asarray(Image.open(io.BytesIO(data))).astype(np.int64)
    assert np.array_equal(back, g16)
    got = ref.decode(data)
    assert np.array_equal(got[..., 1], g16 >> 8) and np.all(got[..., 3] == 255)


@pytest.mark.parametrize("with_trns", [False, True])
def test_against_pillow_paletted(with_trns):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(7)
    idx = rng.integers(0, 40, size=(19, 23), dtype=np.uint8)
    pal = rng.integers(0, 256, size=(40, 3), dtype=np.uint8)
    im = Image.fromarray(idx, "P")
    im.putpalette(pal.tobytes())
    alphas = bytes([0, 255, 128, 7] + [255] * 36)
    data = _pillow_file(im, transparency=alphas) if with_trns else _pillow_file(im)
    f = ref.parse(data)
    assert f["color_type"] == 3 and (f["trns"] is not None) == with_trns
    back = Image.open(io.BytesIO(data))
    assert np.array_equal(np.asarray(back), idx)                # the indices: chunk walk, inflate, unfilter, unpack
    want = np.asarray(back.convert("RGBA"))
    got = ref.decode(data)
    assert np.array_equal(got[..., 3], want[..., 3])
    opaque = want[..., 3] == 255
    assert np.array_equal(got[opaque], want[opaque])            # Pillow keeps (r, g, b) under alpha; toNRGBA's round trip does not


@pytest.mark.parametrize("kind", ["rgb", "rgba", "gray", "pal8", "pal4", "pal2", "pal1"])
def test_round_trip_through_the_encoder_restatement(kind):
    rng = np.random.default_rng(11)
    w, h = 31, 17
    if kind in ("rgb", "rgba"):
        img = enc.smooth_rgba(w, h, 2, opaque=kind == "rgb")
        stream, ct, depth = enc.png_stream(img, enc.NRGBA)
        data = enc.write_png(stream, w, h, ct, depth)
        assert np.array_equal(ref.decode(data), img)
        return
    if kind == "gray":
        plane = _smooth(w, h, 1, 4)[..., 0]
        stream, ct, depth = enc.png_stream(plane, enc.GRAY)
        data = enc.write_png(stream, w, h, ct, depth)
        want = np.stack([plane, plane, plane, np.full_like(plane, 255)], -1)
        assert np.array_equal(ref.decode(data), want)
        return
    n = {"pal8": 200, "pal4": 16, "pal2": 4, "pal1": 2}[kind]
    plane = rng.integers(0, n, size=(h, w), dtype=np.uint8)
    pal = np.concatenate([rng.integers(0, 256, size=(n, 3), dtype=np.uint8), np.full((n, 1), 255, np.uint8)], 1)
    stream, ct, depth = enc.png_stream(plane, enc.PALETTED, ncolors=n)
    data = enc.write_png(stream, w, h, ct, depth, palette=pal)
    assert np.array_equal(ref.decode(data), pal[plane])


def test_writer_and_reader_agree_on_every_pair_and_filter():
    for ct, depth in ref.PAIRS:
        s = ref.random_samples(9, 7, ct, depth, 1)
        data = ref.write_png(s, ct, depth, filters=[0, 1, 2, 3, 4, 4, 3], palette=ref.random_palette(1 << min(depth, 8), 2) if ct == 3 else None,
                             idat_sizes=[1, 5])
        f = ref.parse(data)
        raw = ref.pack_rows(s, ct, depth)
        import zlib
        stream = np.frombuffer(zlib.decompress(f["z"]), np.uint8).reshape(7, -1)
        assert np.array_equal(ref.unfilter(stream, ref.bpp_of(ct, depth)), raw)
        assert np.array_equal(ref.samples_of(raw, 9, ct, depth), s)


# ---- the arithmetic branches, by hand ---------------------------------------------------------------------------------------
def test_palette_trns_round_trip_is_lossy_as_the_reference_s():
    # (200, 100, 50) under t = 128: A16 = 0x8080 = 32896; r: 200 * 257 = 51400, * 128 / 255 = 25800, * 65535 / 32896 = 51398,
    # >> 8 = 200; g: 25700 -> 12900 -> 25699 >> 8 = 100; b: 12850 -> 6450 -> 12849 >> 8 = 50 -- and one that moves:
    # (255, 1, 3) under t = 3: A16 = 771; 65535 * 3 / 255 = 771 -> 771 * 65535 / 771 = 65535 >> 8 = 255;
    # 257 * 3 / 255 = 3 -> 3 * 65535 / 771 = 255 >> 8 = 0 (1 became 0); 771 * 3 / 255 = 9 -> 9 * 65535 / 771 = 765 >> 8 = 2 (3 became 2)
    assert ref.palette_pixel(200, 100, 50, 128) == (200, 100, 50, 128)
    assert ref.palette_pixel(255, 1, 3, 3) == (255, 0, 2, 3)
    assert ref.palette_pixel(9, 8, 7, 0) == (0, 0, 0, 0)
    assert ref.palette_pixel(9, 8, 7, 255) == (9, 8, 7, 255)
    data = ref.write_png(np.array([[[0], [1], [2], [3]]]), 3, 8, palette=[[255, 1, 3], [9, 8, 7]], trns=bytes([3, 0, 77]))
    # index 2 lies behind PLTE but inside tRNS: black under alpha 77; index 3 behind both: opaque black
    assert ref.decode(data).tolist() == [[[255, 0, 2, 3], [0, 0, 0, 0], [0, 0, 0, 77], [0, 0, 0, 255]]]


def test_sixteen_bit_partial_alpha():
    # R = 0x1234 = 4660, A = 0x8000 = 32768: r' = 4660 * 32768 / 65535 = 2330; 2330 * 65535 / 32768 = 4659 = 0x1233 -> 0x12
    # R = 0x0100 = 256, A = 0x0101 = 257: r' = 256 * 257 / 65535 = 1; 1 * 65535 / 257 = 255 -> 0x00 (the high byte 1 is lost)
    assert ref.nrgba64_pixel(0x1234, 0xffff, 0, 0x8000) == (0x12, 0xff, 0, 0x80)
    assert ref.nrgba64_pixel(0x0100, 0x0100, 0x0100, 0x0101) == (0, 0, 0, 1)
    s = np.array([[[0x1234, 0xffff, 0, 0x8000], [0x4000, 0x5000, 0x6000, 0xffff], [0x4000, 0x5000, 0x6000, 0]]])
    assert ref.decode(ref.write_png(s, 6, 16)).tolist() == [[[0x12, 0xff, 0, 0x80], [0x40, 0x50, 0x60, 255], [0, 0, 0, 0]]]
    ga = np.array([[[0x0100, 0x0101], [0xabcd, 0xffff]]])
    assert ref.decode(ref.write_png(ga, 4, 16)).tolist() == [[[0, 0, 0, 1], [0xab, 0xab, 0xab, 255]]]


def test_transparent_colour_kept_at_8_bits_and_zeroed_at_16():
    # 8 bits: Go decodes to *image.NRGBA, toNRGBA copies: the colour stays under alpha 0.  The match is on the LOW byte of tRNS.
    rgb = np.array([[[10, 20, 30], [10, 20, 31]]])
    assert ref.decode(ref.write_png(rgb, 2, 8, trns=bytes([0xaa, 10, 0xbb, 20, 0xcc, 30]))).tolist() == [[[10, 20, 30, 0], [10, 20, 31, 255]]]
    g4 = np.array([[[5], [6]]])
    assert ref.decode(ref.write_png(g4, 0, 4, trns=bytes([0x77, 5]))).tolist() == [[[0x55, 0x55, 0x55, 0], [0x66, 0x66, 0x66, 255]]]
    g8 = np.array([[[200], [201]]])
    assert ref.decode(ref.write_png(g8, 0, 8, trns=bytes([0, 200]))).tolist() == [[[200, 200, 200, 0], [201, 201, 201, 255]]]
    # 16 bits: NRGBA64 through convertToNRGBA: A = 0 zeroes the colour; the match is on the full sample
    rgb16 = np.array([[[0x0a0b, 0x1415, 0x1e1f], [0x0a0b, 0x1415, 0x1e20]]])
    assert ref.decode(ref.write_png(rgb16, 2, 16, trns=bytes([0x0a, 0x0b, 0x14, 0x15, 0x1e, 0x1f]))).tolist() == [[[0, 0, 0, 0], [0x0a, 0x14, 0x1e, 255]]]
    g16 = np.array([[[0x1234], [0x1235]]])
    assert ref.decode(ref.write_png(g16, 0, 16, trns=bytes([0x12, 0x34]))).tolist() == [[[0, 0, 0, 0], [0x12, 0x12, 0x12, 255]]]
    # without tRNS: Gray16 / RGBA64, the high bytes
    assert ref.decode(ref.write_png(g16, 0, 16)).tolist() == [[[0x12, 0x12, 0x12, 255], [0x12, 0x12, 0x12, 255]]]


def test_filters_by_hand():
    # one grey row over a row of 10s: Average of a = 250, b = 10 is 130 (9-bit sum); Paeth: p = 15 is nearest c; ties go a, b, c
    assert ref.paeth(5, 5, 5) == 5 and ref.paeth(10, 20, 15) == 15 and ref.paeth(1, 9, 3) == 9 and ref.paeth(0, 0, 200) == 0
    stream = np.array([[0, 10, 10, 10], [3, 245, 1, 2]], np.uint8)
    # row 1 Average: x0 = 245 + (0 + 10 >> 1) = 250; x1 = 1 + (250 + 10 >> 1) = 131; x2 = 2 + (131 + 10 >> 1) = 72
    assert ref.unfilter(stream, 1).tolist() == [[10, 10, 10], [250, 131, 72]]
    with pytest.raises(ref.Damaged):
        ref.unfilter(np.array([[5, 1, 2]], np.uint8), 1)
