"""Adam7 without a GPU: the tests' own writer and reader (png_adam7_ref.py) against the non-interlaced reference on the same
samples and against Pillow's reader, fnx_png_adam7_passes against the helper's geometry, and the two new entries' argument
checks."""
from __future__ import annotations

import ctypes as C
import io

import numpy as np
import pytest

import fennec_amd
import png_adam7_ref as a7
import png_decode_ref as ref
from fennec_amd import FNX_ERR_INVALID, FNX_ERR_UNSUPPORTED, FNX_HOST, FNX_OK

SIZES = [(1, 1), (2, 3), (5, 3), (3, 5), (8, 8), (9, 17), (33, 10)]


def case(ct, depth, w, h, seed):
    """samples, palette, tRNS body"""
    s = ref.random_samples(w, h, ct, depth, seed)
    pal = ref.random_palette(1 << depth, seed) if ct == 3 else None
    return s, pal


@pytest.mark.parametrize("ct,depth", ref.PAIRS)
def test_interlaced_and_non_interlaced_files_decode_alike(ct, depth):
    for k, (w, h) in enumerate(SIZES):
        s, pal = case(ct, depth, w, h, 10 * k + depth)
        plain = ref.write_png(s, ct, depth, filters=np.random.default_rng(k).integers(0, 5, size=h).tolist(), palette=pal)
        il = a7.write_adam7(s, ct, depth, filters=k, palette=pal, idat_sizes=[1, 9] if k % 2 else None)
        assert fennec_amd.png_info(il) == (w, h, ct, depth, 1)
        assert np.array_equal(a7.decode_adam7(il), ref.decode(plain)), (w, h)
        if w * h > 40:
            assert len({t for p in a7.pass_filter_types(il) for t in p}) == 5      # the random plans use every filter type


@pytest.mark.parametrize("ct,depth", [p for p in ref.PAIRS if p[1] <= 8 and p[0] != 4])
def test_against_pillow(ct, depth):
    Image = pytest.importorskip("PIL.Image")
    for k, (w, h) in enumerate(SIZES):
        s, pal = case(ct, depth, w, h, 50 + k)
        il = a7.write_adam7(s, ct, depth, filters=100 + k, palette=pal)
        im = Image.open(io.BytesIO(il))
        assert np.array_equal(np.asarray(im.convert("RGBA")), a7.decode_adam7(il)), (w, h)


def test_wrong_stream_sizes_are_damaged():
    s = ref.random_samples(9, 5, 2, 8, 1)
    assert a7.passes(9, 5, 2, 8)[3] == 146
    mislabelled = ref.write_png(s, 2, 8, interlace=1)              # a non-interlaced stream (140 bytes) under an Adam7 header
    with pytest.raises(ref.Damaged):
        a7.decode_adam7(mislabelled)
    stream = a7.adam7_stream(s, 2, 8, 3)
    assert len(stream) == 146
    for bad in (stream[:-1], stream + b"\0"):
        with pytest.raises(ref.Damaged):
            a7.decode_adam7(a7.file_around(bad, 9, 5, 2, 8))
    with pytest.raises(ref.Damaged):
        a7.decode_adam7(ref.write_png(s, 2, 8))                     # not an Adam7 file at all


# ---- fnx_png_adam7_passes ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ct,depth", ref.PAIRS)
def test_pass_geometry(ct, depth):
    dims = [(w, h) for w in range(1, 18) for h in range(1, 18)] + [(65535, 1), (1, 65535)]
    absent = 0
    for w, h in dims:
        pw, ph, rb, total = a7.passes(w, h, ct, depth)
        assert fennec_amd.png_adam7_passes(w, h, ct, depth) == (pw, ph, rb, total), (w, h)
        assert sum(a * b for a, b in zip(pw, ph)) == w * h                       # every pixel is in exactly one pass
        assert all((pw[p] == 0) == (ph[p] == 0) == (rb[p] == 0) for p in range(7))
        absent += sum(1 for p in range(7) if ph[p] == 0)
        if w < 5:
            assert ph[1] == 0
        if h < 5:
            assert ph[2] == 0
        if w == 1:
            assert ph[1] == ph[3] == ph[5] == 0
        if h == 1:
            assert ph[2] == ph[4] == ph[6] == 0
    assert absent > 0
    assert fennec_amd.png_adam7_passes(1, 1, ct, depth)[3] == 1 + (ref.CHANNELS[ct] * depth + 7) // 8


def test_pass_geometry_bad_arguments():
    lib = fennec_amd.load_library()
    pw, ph, rb, total = (C.c_int * 7)(), (C.c_int * 7)(), (C.c_size_t * 7)(), C.c_size_t()
    call = lambda w, h, ct, d, a=pw, b=ph, c=rb, t=C.byref(total): lib.fnx_png_adam7_passes(w, h, ct, d, a, b, c, t)   # noqa: E731
    assert call(9, 5, 2, 8) == FNX_OK and total.value == 146
    for w, h, ct, d in ((0, 5, 2, 8), (5, 0, 2, 8), (-1, 5, 2, 8), (65536, 1, 0, 1), (1, 65536, 0, 1), (9, 5, 1, 8), (9, 5, 2, 4), (9, 5, 3, 16),
                        (9, 5, 0, 3), (9, 5, 4, 4), (9, 5, 6, 2), (9, 5, 7, 8), (9, 5, 2, 0)):
        assert call(w, h, ct, d) == FNX_ERR_INVALID, (w, h, ct, d)
    assert call(9, 5, 2, 8, a=None) == FNX_ERR_INVALID
    assert call(9, 5, 2, 8, b=None) == FNX_ERR_INVALID
    assert call(9, 5, 2, 8, c=None) == FNX_ERR_INVALID
    assert call(9, 5, 2, 8, t=None) == FNX_ERR_INVALID
    with pytest.raises(fennec_amd.FennecError):
        fennec_amd.png_adam7_passes(9, 5, 2, 4)


# ---- fnx_ctx_set_png_adam7 ---------------------------------------------------------------------------------------------------
def test_the_setter_refuses_a_null_ctx_and_the_probe_without_a_ctx_keeps_its_answer():
    lib = fennec_amd.load_library()
    names = fennec_amd.exported_symbols()
    assert "fnx_ctx_set_png_adam7" in names and "fnx_png_adam7_passes" in names
    assert hasattr(fennec_amd.Context, "set_png_adam7")
    assert lib.fnx_ctx_set_png_adam7(None, 1) == FNX_ERR_INVALID
    assert lib.fnx_ctx_set_png_adam7(None, 0) == FNX_ERR_INVALID
    il = a7.write_adam7(ref.random_samples(9, 5, 2, 8, 1), 2, 8, filters=1)
    src = np.frombuffer(il, np.uint8)
    w, h = C.c_int(-1), C.c_int(-1)
    assert lib.fnx_png_decode(None, src.ctypes.data, len(il), FNX_HOST, None, 0, C.byref(w), C.byref(h)) == FNX_ERR_UNSUPPORTED
    assert b"Adam7" in lib.fnx_last_error()
