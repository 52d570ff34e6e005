"""The numpy restatement of the PNG encoder's row stage (tests/png_filter_ref.py) anchored without a GPU and without our reading
of Go: what it writes, wrapped by its own chunk writer, is a PNG that Pillow decodes back to the source -- for every row form,
with and without tRNS -- and the tie and abs8 cases have the answers worked out on paper."""
from __future__ import annotations

import numpy as np
import pytest

import png_filter_ref as ref
from png_filter_ref import GRAY, NRGBA, PALETTED


def paletted(w, h, ncolors, seed, translucent=False):
    """-> (palette (ncolors, 4), index plane (h, w)) with every index in use where the image has room"""
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, size=(ncolors, 4), dtype=np.uint8)
    pal[:, 3] = 255
    if translucent:
        pal[:: 3, 3] = rng.integers(0, 255, size=len(pal[:: 3]), dtype=np.uint8)
        pal[-1, 3] = 255                                             # tRNS stops at the last alpha != 255
    idx = rng.integers(0, ncolors, size=(h, w), dtype=np.uint8)
    idx.ravel()[:min(ncolors, w * h)] = np.arange(min(ncolors, w * h), dtype=np.uint8)
    return pal, idx


CONTENT = {
    "rgb_noise": lambda: ref.noise_rgba(64, 67, 1),
    "rgb_smooth": lambda: ref.smooth_rgba(67, 31, 2),
    "rgba_noise": lambda: ref.noise_rgba(33, 17, 3, opaque=False),
    "rgba_smooth": lambda: ref.smooth_rgba(67, 31, 4, opaque=False),
    "rgb_1x1": lambda: ref.noise_rgba(1, 1, 5),
    "rgb_one_column": lambda: ref.noise_rgba(1, 9, 6),
}


@pytest.mark.parametrize("name", sorted(CONTENT))
def test_nrgba_streams_decode_with_pillow(name):
    img = CONTENT[name]()
    h, w = img.shape[:2]
    stream, ct, depth = ref.png_stream(img, NRGBA)
    assert (ct, depth) == ((2, 8) if ref.visible_opaque(img) else (6, 8))
    assert stream.shape == (h, 1 + (3 if ct == 2 else 4) * w)
    assert np.array_equal(ref.decode_png(ref.write_png(stream, w, h, ct, depth)), img)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (67, 31)])
def test_gray_streams_decode_with_pillow(w, h):
    g = ref.smooth_rgba(w, h, 7)[..., 0].copy()
    stream, ct, depth = ref.png_stream(g, GRAY)
    assert (ct, depth) == (0, 8) and stream.shape == (h, 1 + w)
    want = np.stack([g, g, g, np.full_like(g, 255)], axis=-1)
    assert np.array_equal(ref.decode_png(ref.write_png(stream, w, h, ct, depth)), want)


@pytest.mark.parametrize("translucent", [False, True])
@pytest.mark.parametrize("ncolors,depth", [(256, 8), (17, 8), (16, 4), (5, 4), (4, 2), (3, 2), (2, 1), (1, 1)])
def test_paletted_streams_decode_with_pillow(ncolors, depth, translucent):
    for w in (1, 7, 13, 64):                                          # partial last bytes at every depth
        pal, idx = paletted(w, 5, ncolors, 10 * ncolors + w, translucent)
        stream, ct, d = ref.png_stream(idx, PALETTED, ncolors)
        assert (ct, d) == (3, depth) and stream.shape == (5, 1 + (w * depth + 7) // 8)
        assert not stream[:, 0].any(), "paletted rows are never filtered"
        data = ref.write_png(stream, w, 5, ct, d, pal)
        assert np.array_equal(ref.decode_png(data), pal[idx])
        tags = [t for t, _ in ref.chunks(data)]
        assert tags == ([b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND"] if (pal[:, 3] != 255).any() else [b"IHDR", b"PLTE", b"IDAT", b"IEND"])


def test_every_filter_type_is_chosen_somewhere():
    """the content of these tests reaches all five types; content that stops doing so fails here"""
    seen = set()
    for name in sorted(CONTENT):
        raw, bpp, _, _ = ref.raw_rows(CONTENT[name](), NRGBA)
        seen |= set(int(t) for t in ref.filter_rows(raw, bpp)[1])
    assert seen == {0, 1, 2, 3, 4}, seen
    raw, bpp, _, _ = ref.raw_rows(ref.noise_rgba(64, 67, 1), NRGBA)
    assert set(int(t) for t in ref.filter_rows(raw, bpp)[1]) == {0, 1, 2, 3, 4}, "uniform RGB noise at 64 x 67 alone reaches all five"


@pytest.mark.parametrize("case", ref.tie_cases(), ids=lambda c: c[0])
def test_ties_go_to_the_filter_tried_first(case):
    _, img, want = case
    raw, bpp, ct, _ = ref.raw_rows(img, NRGBA)
    assert ct == 2 and [int(t) for t in ref.filter_rows(raw, bpp)[1]] == want


@pytest.mark.parametrize("case", ref.abs8_cases(), ids=lambda c: c[0])
def test_abs8_at_127_128_129(case):
    _, g, sums, want = case
    rows = ref.residuals(g[0], np.zeros_like(g[0]), 1)
    assert [ref.abs8_sum(r) for r in rows] == sums
    stream, types = ref.filter_rows(g, 1)
    assert [int(t) for t in types] == [want]
    assert np.array_equal(stream[0, 1:], rows[want])


def test_abs8_itself():
    assert ref.abs8_sum(np.array([127], np.uint8)) == 127
    assert ref.abs8_sum(np.array([128], np.uint8)) == 128
    assert ref.abs8_sum(np.array([129], np.uint8)) == 127
    assert ref.abs8_sum(np.array([0, 1, 255], np.uint8)) == 2


def test_the_row_above_is_raw_not_filtered():
    """Up of two equal rows is all zeros whatever filter the first one got"""
    row = ref.noise_rgba(40, 1, 11)
    img = np.concatenate([row, row], axis=0)
    stream, _, _ = ref.png_stream(img, NRGBA)
    assert stream[1, 0] == 2 and not stream[1, 1:].any()
