"""fnx_png_encoded_size, fnx_png_target_size, fnx_hit_target_size and fennec_CompressFileHitTargetSize in the C ABI (no GPU
needed): declared by the header with their parameter counts, exported by the built library, known to the binding; the new
strategy bits and the format constants have the header's values; every refusal the header lists is answered before the ctx is
looked at (the calls below pass no ctx: a refusal that names an argument came first, good arguments are refused for the ctx);
and the entries that were there before still refuse the new bits."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import fennec_amd
from fennec_amd import (FNX_FORMAT_AUTO, FNX_FORMAT_JPEG, FNX_FORMAT_PNG, FNX_TS_ALL, FNX_TS_FALLBACK_PNG, FNX_TS_PNG_ALL, FNX_TS_QUANTIZE,
                        FNX_TS_SCALE_PNG, FileOptions, SizeCandidate, TargetOptions)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = fennec_amd.FNX_ERR_INVALID
ENTRIES = {"fnx_png_encoded_size": 11, "fnx_png_target_size": 17, "fnx_hit_target_size": 17, "fennec_CompressFileHitTargetSize": 13}


def _header():
    return open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


@pytest.fixture(scope="module")
def lib():
    return fennec_amd.load_library()


def _err(lib):
    return lib.fnx_last_error().decode()


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_declared_exported_and_bound(lib, name):
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    m = re.search(rf"\bint\s+{name}\s*\(([^;]*)\)\s*;", code)
    assert m, f"{name} is not declared"
    assert len(m.group(1).split(",")) == ENTRIES[name]
    assert name in fennec_amd.exported_symbols()
    assert hasattr(lib, name), f"libfennec_hip.so does not export {name}"
    assert len(getattr(lib, name).argtypes) == ENTRIES[name]


def test_constants_agree_with_the_header():
    defs = dict(re.findall(r"^#define\s+(FNX_(?:TS|FORMAT)_\w+)\s+(\d+)", _header(), flags=re.M))
    assert (int(defs["FNX_TS_QUANTIZE"]), int(defs["FNX_TS_SCALE_PNG"]), int(defs["FNX_TS_FALLBACK_PNG"])) == (16, 32, 64)
    assert (FNX_TS_QUANTIZE, FNX_TS_SCALE_PNG, FNX_TS_FALLBACK_PNG, FNX_TS_PNG_ALL) == (16, 32, 64, 112)
    assert (int(defs["FNX_FORMAT_AUTO"]), int(defs["FNX_FORMAT_JPEG"]), int(defs["FNX_FORMAT_PNG"])) == (0, 1, 2)
    assert (FNX_FORMAT_AUTO, FNX_FORMAT_JPEG, FNX_FORMAT_PNG) == (0, 1, 2)
    assert FNX_TS_ALL == 15 and not FNX_TS_ALL & FNX_TS_PNG_ALL
    for name in ("png_encoded_size", "png_target_size", "hit_target_size", "compress_file_hit_target_size"):
        assert callable(getattr(fennec_amd.Context, name)), name


class Call:
    """a complete argument list of fnx_png_target_size / fnx_hit_target_size on a 8 x 6 host image, every pointer valid"""

    def __init__(self, ncand):
        self.img = np.zeros((6, 8, 4), dtype=np.uint8)
        self.win_arr, self.window = fennec_amd._f64(np.full(64, 1.0 / 64))
        self.cand = (SizeCandidate * ncand)()
        self.win, self.n = C.c_int(7), C.c_size_t(7)
        self.out = np.zeros(4096, dtype=np.uint8)
        self.back = np.zeros((6, 8, 4), dtype=np.uint8)

    def args(self, which, **change):
        a = dict(ctx=None, space=fennec_amd.FNX_HOST, src=self.img.ctypes.data, sstride=32, w=8, h=6, target_bytes=1000, which=which,
                 window=self.window, cancel=None, cand=self.cand, winner=C.byref(self.win), out=self.out.ctypes.data, cap=4096,
                 nbytes=C.byref(self.n), img=self.back.ctypes.data, istride=32)
        a.update(change)
        return list(a.values())


ENTRY = {"fnx_png_target_size": (3, FNX_TS_PNG_ALL), "fnx_hit_target_size": (5, FNX_FORMAT_AUTO)}
REFUSALS = [(dict(src=None), "src"), (dict(window=None), "window"), (dict(cand=None), "cand"), (dict(winner=None), "winner"),
            (dict(nbytes=None), "nbytes"), (dict(out=None), "out"), (dict(target_bytes=0), "target_bytes"), (dict(target_bytes=-5), "target_bytes"),
            (dict(sstride=48), "tight"), (dict(space=9), "space"), (dict(w=0), "dimensions"), (dict(istride=16), "img")]


@pytest.mark.parametrize("name", sorted(ENTRY))
@pytest.mark.parametrize("change,word", REFUSALS, ids=[f"{next(iter(c))}={next(iter(c.values()))}" for c, _ in REFUSALS])
def test_refusals_come_before_the_ctx(lib, name, change, word):
    ncand, which = ENTRY[name]
    c = Call(ncand)
    assert getattr(lib, name)(*c.args(which, **change)) == INVALID
    assert word in _err(lib) and "null ctx" not in _err(lib), _err(lib)
    assert (c.win.value, c.n.value) == (7, 7)                         # nothing was touched


@pytest.mark.parametrize("mask", [0, -1, 1, 8, FNX_TS_ALL, FNX_TS_PNG_ALL | 1, FNX_TS_PNG_ALL | 128, 128])
def test_png_entry_refuses_a_mask_outside_its_three_bits(lib, mask):
    c = Call(3)
    assert lib.fnx_png_target_size(*c.args(mask)) == INVALID
    assert "strategies" in _err(lib) and "null ctx" not in _err(lib)


@pytest.mark.parametrize("fmt", [-1, 3, 16])
def test_hit_entry_refuses_a_format_outside_0_to_2(lib, fmt):
    c = Call(5)
    assert lib.fnx_hit_target_size(*c.args(fmt)) == INVALID
    assert "format" in _err(lib) and "null ctx" not in _err(lib)


def test_a_padded_source_is_refused_only_where_quantize_runs(lib):
    c = Call(3)
    wide = np.zeros((6, 12, 4), dtype=np.uint8)
    padded = dict(src=wide.ctypes.data, sstride=48)
    assert lib.fnx_png_target_size(*c.args(FNX_TS_QUANTIZE, **padded)) == INVALID and "tight" in _err(lib)
    assert lib.fnx_png_target_size(*c.args(FNX_TS_SCALE_PNG | FNX_TS_FALLBACK_PNG, **padded)) == INVALID and "null ctx" in _err(lib)
    c5 = Call(5)
    assert lib.fnx_hit_target_size(*c5.args(FNX_FORMAT_PNG, **padded)) == INVALID and "tight" in _err(lib)
    assert lib.fnx_hit_target_size(*c5.args(FNX_FORMAT_JPEG, **padded)) == INVALID and "null ctx" in _err(lib)


@pytest.mark.parametrize("name", sorted(ENTRY))
def test_good_arguments_are_refused_for_the_ctx(lib, name):
    ncand, which = ENTRY[name]
    c = Call(ncand)
    assert getattr(lib, name)(*c.args(which)) == INVALID and "null ctx" in _err(lib)
    assert getattr(lib, name)(*c.args(which, out=None, cap=0)) == INVALID and "null ctx" in _err(lib)      # the size-only form
    assert getattr(lib, name)(*c.args(which, img=None, istride=0)) == INVALID and "null ctx" in _err(lib)


def test_encoded_size_refusals(lib):
    idx = np.zeros((9, 67), np.uint8)
    pal = np.zeros((4, 4), np.uint8)
    n = C.c_size_t(7)
    good = [None, fennec_amd.FNX_HOST, fennec_amd.FNX_PNG_PALETTED, idx.ctypes.data, 67, 67, 9, 4, -1, pal.ctypes.data, C.byref(n)]
    assert lib.fnx_png_encoded_size(*good) == INVALID and "null ctx" in _err(lib)
    for at, value, word in ((9, None, "palette"), (3, None, "src"), (10, None, "nbytes"), (7, 0, "ncolors"), (7, 257, "ncolors"), (4, 66, "stride"),
                            (2, 7, "kind"), (1, 9, "space"), (8, 2, "opaque"), (5, 0, "dims")):
        a = list(good)
        a[at] = value
        assert lib.fnx_png_encoded_size(*a) == INVALID
        assert word in _err(lib) and "null ctx" not in _err(lib), (at, _err(lib))
    assert n.value == 7


class FileCall:
    def __init__(self):
        self.data = np.zeros(64, dtype=np.uint8)
        self.o = FileOptions(1, 0, 0, 0, 0.0)
        self.cand = (SizeCandidate * 5)()
        self.win, self.n = C.c_int(7), C.c_size_t(7)
        self.out = np.zeros(4096, dtype=np.uint8)
        self.dims = (C.c_int * 4)()

    def args(self, **change):
        a = dict(ctx=None, data=self.data.ctypes.data, n=64, file=C.byref(self.o), target_bytes=1000, format=FNX_FORMAT_AUTO, cancel=None,
                 cand=self.cand, winner=C.byref(self.win), out=self.out.ctypes.data, cap=4096, nbytes=C.byref(self.n), dims=self.dims)
        a.update(change)
        return list(a.values())


@pytest.mark.parametrize("change,word", [(dict(data=None), "NULL"), (dict(file=None), "NULL"), (dict(cand=None), "NULL"), (dict(winner=None), "NULL"),
                                         (dict(nbytes=None), "NULL"), (dict(dims=None), "NULL"), (dict(out=None), "NULL"),
                                         (dict(target_bytes=0), "target_bytes"), (dict(target_bytes=-1), "target_bytes"),
                                         (dict(format=3), "format"), (dict(format=-1), "format")])
def test_file_entry_refusals_come_before_the_ctx(lib, change, word):
    c = FileCall()
    assert lib.fennec_CompressFileHitTargetSize(*c.args(**change)) == INVALID
    assert word in _err(lib) and "null ctx" not in _err(lib)
    assert (c.win.value, c.n.value) == (7, 7)


def test_file_entry_with_good_arguments_is_refused_for_the_ctx(lib):
    c = FileCall()
    for fmt in (FNX_FORMAT_AUTO, FNX_FORMAT_JPEG, FNX_FORMAT_PNG):
        assert lib.fennec_CompressFileHitTargetSize(*c.args(format=fmt)) == INVALID and "null ctx" in _err(lib)
    assert lib.fennec_CompressFileHitTargetSize(*c.args(out=None, cap=0)) == INVALID and "null ctx" in _err(lib)


@pytest.mark.parametrize("bits", [FNX_TS_QUANTIZE, FNX_TS_SCALE_PNG, FNX_TS_FALLBACK_PNG, FNX_TS_ALL | FNX_TS_QUANTIZE, FNX_TS_PNG_ALL])
def test_the_old_entries_still_refuse_the_new_bits(lib, bits):
    """the file entry checks its options before its ctx, so the refusal can be read here; fnx_jpeg_target_size's own refusal
    (behind its ctx) is read on the GPU, in test_hit_target_size_gpu.py"""
    data = np.zeros(64, dtype=np.uint8)
    o = TargetOptions.make(1000, strategies=bits)
    cand = (SizeCandidate * 4)()
    win, n = C.c_int(7), C.c_size_t(7)
    out = np.zeros(4096, dtype=np.uint8)
    dims = (C.c_int * 4)()
    assert lib.fennec_CompressFileTargetSize(None, data.ctypes.data, 64, C.byref(o), None, cand, C.byref(win), out.ctypes.data, 4096, C.byref(n),
                                             dims) == INVALID
    assert "strategies" in _err(lib) and "ctx" not in _err(lib)
    c = Call(4)
    assert lib.fnx_jpeg_target_size(*c.args(bits)) == INVALID
