"""fnx_png_decode_batch without a GPU: the header's declaration, the library's export, the Python binding, a C99 client, and
the refusal of a call without a context."""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fennec_amd
import png_decode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return fennec_amd.load_library()


def test_header_python_and_library_agree(lib):
    text = open(os.path.join(ROOT, "include", "fennec_hip.h")).read()
    m = re.search(r"\bint\s+fnx_png_decode_batch\s*\(([^;]*)\)\s*;", text)
    assert m, "the header declares fnx_png_decode_batch"
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]
    assert len(params) == 10, params
    assert params[0] == "fnx_ctx *ctx" and params[6] == "int workers" and params[9] == "int *status"
    assert re.search(r"^#define FNX_PNG_DECODE_CHUNK 32\b", text, re.M)
    assert fennec_amd.FNX_PNG_DECODE_CHUNK == 32
    assert re.search(r"^#define FNX_PNG_DECODE_CHUNK_BYTES ", text, re.M), "the chunk's byte budget is a constant beside it"
    assert "fnx_png_decode_batch" in fennec_amd.exported_symbols() and hasattr(C.CDLL(fennec_amd.LIB_PATH), "fnx_png_decode_batch")
    assert callable(getattr(fennec_amd.Context, "png_decode_batch"))
    assert len(lib.fnx_png_decode_batch.argtypes) == 10


def test_header_is_plain_c_and_links_from_c(lib, tmp_path):
    png = ref.write_png(np.zeros((2, 3, 1), np.int64), 0, 8)
    src = tmp_path / "png_batch_abi.c"
    src.write_text(r'''
#include "fennec_hip.h"
static const uint8_t png[] = {%s};
int main(void) {
    const uint8_t *files[1] = {png};
    const size_t sizes[1] = {sizeof png};
    uint8_t *dsts[1] = {0};
    const int strides[1] = {12};
    int w[1] = {-1}, h[1] = {-1}, status[1] = {7};
    /* no context: refused, not crashed, nothing written */
    if (fnx_png_decode_batch(0, 1, files, sizes, dsts, strides, 1, w, h, status) >= 0) return 1;
    if (w[0] != -1 || h[0] != -1 || status[0] != 7) return 2;
    if (FNX_PNG_DECODE_CHUNK_BYTES < ((size_t)1 << 20)) return 3;
    return FNX_PNG_DECODE_CHUNK == 32 ? 0 : 4;
}
''' % ", ".join(str(v) for v in png))
    exe = tmp_path / "png_batch_abi"
    libdir = os.path.dirname(fennec_amd.LIB_PATH)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe),
                           "-L", libdir, "-lfennec_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"])
    assert subprocess.call([str(exe)]) == 0


def test_a_null_ctx_is_refused(lib):
    png = np.frombuffer(ref.write_png(np.zeros((2, 3, 1), np.int64), 0, 8), np.uint8)
    files = (C.c_void_p * 1)(png.ctypes.data)
    sizes = (C.c_size_t * 1)(png.size)
    dsts = (C.c_void_p * 1)(None)
    strides = (C.c_int * 1)(12)
    ws, hs, status = (C.c_int * 1)(-1), (C.c_int * 1)(-1), (C.c_int * 1)(7)
    rc = lib.fnx_png_decode_batch(None, 1, files, sizes, dsts, strides, 0, ws, hs, status)
    assert rc == fennec_amd.FNX_ERR_INVALID and b"ctx" in lib.fnx_last_error()
    assert (ws[0], hs[0], status[0]) == (-1, -1, 7)
