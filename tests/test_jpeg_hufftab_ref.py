"""The plain-Python statement of the optimised Huffman tables (tests/jpeg_hufftab_ref.py) on its own, without the library: its
tables are libjpeg's (Pillow's optimize=True files), its files decode back to the coefficients they were made from, and they
are no longer than the standard files."""
from __future__ import annotations

import io

import numpy as np
import pytest

import jpeg_hufftab_ref as ref
from oracle import oracle


def _pillow_images():
    rng = np.random.default_rng(42)
    y, x = np.mgrid[0:64, 0:128].astype(np.float64)
    smooth = np.stack([128 + 100 * np.sin(x / 17) * np.cos(y / 11), 128 + 90 * np.cos(x / 23 + y / 9), 40 + 1.5 * x], -1)
    smooth = np.clip(np.rint(smooth), 0, 255).astype(np.uint8)
    return [("noise_33x17_q5", rng.integers(0, 256, (17, 33, 3), dtype=np.uint8), 5),
            ("noise_64x48_q50", rng.integers(0, 256, (48, 64, 3), dtype=np.uint8), 50),
            ("smooth_128x64_q75", smooth, 75),
            ("smooth_47x31_q100", smooth[:31, :47], 100),
            ("noise_128x64_q95", rng.integers(0, 256, (64, 128, 3), dtype=np.uint8), 95)]


@pytest.mark.parametrize("name,rgb,quality", _pillow_images(), ids=[c[0] for c in _pillow_images()])
def test_tables_are_pillows(name, rgb, quality):
    """all four DHT tables of Pillow's optimize=True file equal the helper's, built from that file's own coefficients"""
    Image = pytest.importorskip("PIL.Image")
    buf = io.BytesIO()
    Image.fromarray(rgb, "RGB").save(buf, "JPEG", quality=quality, subsampling=2, optimize=True)
    data = buf.getvalue()
    coef = oracle.jpeg_decode_planes(data, with_coefficients=True)[-1]
    want = ref.dht_tables(data)
    got = ref.tables(ref.symbol_histogram(coef))
    for t in range(4):
        assert got[t][2] == 0
        assert (list(got[t][0]), list(got[t][1])) == (list(want[t][0]), list(want[t][1])), (name, t)


def _images():
    out = [(name, img, q) for name, img in ref.plain_images().items() for q in (1, 50, 75, 100)]
    out += [(name, img, q) for name, (img, q) in ref.crafted_images().items()]
    out += [("photo_64x48", ref._photo_like(64, 48, 9), q) for q in (30, 75)]
    out += [("sizes_48x40", ref._photo_like(48, 40, 21), q) for q in (1, 10, 25, 50, 75, 90, 100)]
    return out


def test_files_decode_back_and_are_no_longer():
    for name, img, q in _images():
        std, coef = oracle.jpeg_encode(img, q, with_coefficients=True)
        h, w = img.shape[:2]
        data, crafted, tabs = ref.optimized_file(std, coef, w, h)
        back = oracle.jpeg_decode_planes(data, with_coefficients=True)
        assert (back[0], back[1], back[2]) == (w, h, 2), name
        assert np.array_equal(back[-1], coef), (name, q)
        assert np.array_equal(crafted.coef, coef)
        assert len(data) <= len(std), (name, q, len(data), len(std))
        assert data.count(b"\xff\xc4") >= 1 and ref.dht_tables(data) == [(list(b), list(v)) for b, v, _ in tabs]


def test_a_code_size_above_32_is_flagged_not_indexed():
    for n in (16, 17, 32):
        bits, vals = ref.build_table(ref.geometric_histogram(n))
        assert sum(bits) == n == len(vals)
    with pytest.raises(ref.TooLong):
        ref.build_table(ref.geometric_histogram(33))
    h4 = [ref.geometric_histogram(33)] * 4
    assert [(list(b), list(v), s) for b, v, s in ref.tables(h4)] == [(list(b), list(v), 1) for b, v in ref.standard_tables()]


def test_a_single_symbol_gets_the_one_bit_code_zero():
    h = [0] * 256
    h[5] = 3
    bits, vals = ref.build_table(h)
    assert (bits, vals) == ([1] + [0] * 15, [5]) and ref.lut_words(bits, vals)[5] == 1 << 24
