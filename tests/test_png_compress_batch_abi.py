"""fnx_png_file_bound, fnx_png_compress_batch and fnx_png_recompress_batch without a GPU: the header's declarations, the
library's exports, the Python bindings, the bound's arithmetic, and the refusal of bad arguments before the context is looked
at."""
from __future__ import annotations

import ctypes as C
import os
import re

import pytest

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FNX_BATCH_MAX = 65535            # include/fennec_hip.h
NAMES = ("fnx_png_file_bound", "fnx_png_compress_batch", "fnx_png_recompress_batch")


@pytest.fixture(scope="module")
def lib():
    return fennec_amd.load_library()


def test_header_python_and_library_agree(lib):
    text = open(os.path.join(ROOT, "include", "fennec_hip.h")).read()
    raw = C.CDLL(fennec_amd.LIB_PATH)
    for name in NAMES:
        assert name in fennec_amd.exported_symbols() and hasattr(raw, name), name
    nparams = {}
    for name in NAMES[1:]:
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        nparams[name] = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(nparams["fnx_png_compress_batch"]) == 11 and len(lib.fnx_png_compress_batch.argtypes) == 11
    assert len(nparams["fnx_png_recompress_batch"]) == 12 and len(lib.fnx_png_recompress_batch.argtypes) == 12
    assert nparams["fnx_png_recompress_batch"][4] == "int workers"
    assert re.search(r"\bsize_t\s+fnx_png_file_bound\s*\(\s*int w,\s*int h\s*\)\s*;", text)
    assert lib.fnx_png_file_bound.restype is C.c_size_t
    assert re.search(r"^#define FNX_PNG_COMPRESS_CHUNK 32\b", text, re.M) and fennec_amd.FNX_PNG_COMPRESS_CHUNK == 32
    assert re.search(r"^#define FNX_PNG_COMPRESS_CHUNK_BYTES \(\(size_t\)1 << 30\)", text, re.M)
    for name in ("png_compress_batch", "png_recompress_batch"):
        assert callable(getattr(fennec_amd.Context, name))
    assert callable(fennec_amd.png_file_bound)


def test_the_bound_is_pure_and_monotonic(lib):
    dims = [1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 1031, 4096, 32767, 32768, 65535]
    table = {(w, h): fennec_amd.png_file_bound(w, h) for w in dims for h in dims}
    for (w, h), v in table.items():
        assert fennec_amd.png_file_bound(w, h) == v                              # the same answer again: no state
        rgba = 8 + 25 + 12 + fennec_amd.deflate_bound(h * (4 * w + 1)) + 12
        paletted = 8 + 25 + (12 + 768) + (12 + 256) + 12 + fennec_amd.deflate_bound(h * (w + 1)) + 12
        assert v >= rgba and v >= paletted, (w, h)
    for a, b in zip(dims, dims[1:]):
        for o in dims:
            assert table[(a, o)] < table[(b, o)] and table[(o, a)] < table[(o, b)]
    # a one-pixel image: the paletted layout is the larger one
    assert fennec_amd.png_file_bound(1, 1) == 8 + 25 + 780 + 268 + 12 + fennec_amd.deflate_bound(2) + 12
    for w, h in ((0, 5), (5, 0), (-1, 5), (65536, 1), (1, 65536)):
        assert fennec_amd.png_file_bound(w, h) == 0


def compress_args(n=1):
    return [(C.c_void_p * 1)(None), (C.c_int * 1)(16), (C.c_int * 1)(4), (C.c_int * 1)(4), (C.c_void_p * 1)(None), (C.c_size_t * 1)(0),
            (C.c_size_t * 1)(99), (C.c_int * 1)(-7), (C.c_int * 1)(77)]


def recompress_args():
    return [(C.c_void_p * 1)(None), (C.c_size_t * 1)(0), (C.c_void_p * 1)(None), (C.c_size_t * 1)(0), (C.c_size_t * 1)(99), (C.c_int * 1)(-7),
            (C.c_int * 1)(-7), (C.c_int * 1)(-7), (C.c_int * 1)(77)]


@pytest.mark.parametrize("n", [0, -1, FNX_BATCH_MAX + 1])
def test_n_is_refused_before_the_ctx(lib, n):
    a = compress_args()
    assert lib.fnx_png_compress_batch(None, n, *a) == fennec_amd.FNX_ERR_INVALID
    assert b"FNX_BATCH_MAX" in lib.fnx_last_error() and b"ctx" not in lib.fnx_last_error()
    assert (a[6][0], a[7][0], a[8][0]) == (99, -7, 77)
    r = recompress_args()
    assert lib.fnx_png_recompress_batch(None, n, r[0], r[1], 0, *r[2:]) == fennec_amd.FNX_ERR_INVALID
    assert b"FNX_BATCH_MAX" in lib.fnx_last_error() and b"ctx" not in lib.fnx_last_error()
    assert (r[4][0], r[8][0]) == (99, 77)


def test_null_arrays_are_refused_before_the_ctx(lib):
    for k in range(9):
        a = compress_args()
        a[k] = None
        assert lib.fnx_png_compress_batch(None, 1, *a) == fennec_amd.FNX_ERR_INVALID, k
        assert b"NULL array" in lib.fnx_last_error(), k
    for k in range(9):
        r = recompress_args()
        r[k] = None
        assert lib.fnx_png_recompress_batch(None, 1, r[0], r[1], 0, *r[2:]) == fennec_amd.FNX_ERR_INVALID, k
        assert b"NULL array" in lib.fnx_last_error(), k


@pytest.mark.parametrize("workers", [-1, 65, 1 << 20])
def test_workers_are_refused_before_the_ctx(lib, workers):
    r = recompress_args()
    assert lib.fnx_png_recompress_batch(None, 1, r[0], r[1], workers, *r[2:]) == fennec_amd.FNX_ERR_INVALID
    assert b"workers" in lib.fnx_last_error()
    assert r[8][0] == 77


def test_good_arguments_without_a_ctx_are_refused_for_the_ctx(lib):
    a = compress_args()
    assert lib.fnx_png_compress_batch(None, 1, *a) == fennec_amd.FNX_ERR_INVALID and b"ctx" in lib.fnx_last_error()
    assert (a[6][0], a[7][0], a[8][0]) == (99, -7, 77)
    r = recompress_args()
    assert lib.fnx_png_recompress_batch(None, 1, r[0], r[1], 64, *r[2:]) == fennec_amd.FNX_ERR_INVALID and b"ctx" in lib.fnx_last_error()
    assert r[8][0] == 77
