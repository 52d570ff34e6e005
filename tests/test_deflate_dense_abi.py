"""The deflate level exists at every layer (no GPU needed): the header declares fnx_ctx_set_deflate_level and its constants, the
built library exports it, the binding knows its signature, the Python constants equal the header's, bad arguments are refused
without a device, the stream's bound is what it was, and the dense kernels are part of the build."""
from __future__ import annotations

import ctypes as C
import os
import re

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header() -> str:
    return open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


def test_header_declares_the_entry():
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    assert re.search(r"\bint\s+fnx_ctx_set_deflate_level\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*int\s+level\s*\)\s*;", code)
    assert "fnx_ctx_set_deflate_level" in fennec_amd.exported_symbols()


def test_library_exports_the_entry():
    lib = fennec_amd.load_library()
    assert hasattr(lib, "fnx_ctx_set_deflate_level"), "libfennec_hip.so does not export fnx_ctx_set_deflate_level"
    f = lib.fnx_ctx_set_deflate_level
    assert f.restype is C.c_int and len(f.argtypes) == 2 and f.argtypes[1] is C.c_int


def test_constants_agree_with_the_header():
    defs = dict(re.findall(r"^#define\s+(FNX_DEFLATE_\w+)\s+(\d+)", _header(), flags=re.M))
    assert int(defs["FNX_DEFLATE_LEVEL_FAST"]) == fennec_amd.FNX_DEFLATE_LEVEL_FAST == 0
    assert int(defs["FNX_DEFLATE_LEVEL_DENSE"]) == fennec_amd.FNX_DEFLATE_LEVEL_DENSE == 1
    assert int(defs["FNX_DEFLATE_DENSE_DEPTH"]) == fennec_amd.FNX_DEFLATE_DENSE_DEPTH >= 1
    assert callable(fennec_amd.Context.set_deflate_level)


def test_bad_arguments_are_refused_without_a_device():
    """no ctx: refused whatever the level, good ones included; fnx_last_error says which entry"""
    lib = fennec_amd.load_library()
    for level in (0, 1, -1, 2):
        assert lib.fnx_ctx_set_deflate_level(None, level) == fennec_amd.FNX_ERR_INVALID, level
        assert b"fnx_ctx_set_deflate_level" in lib.fnx_last_error()


def test_the_bound_is_unchanged():
    lib = fennec_amd.load_library()
    ch = fennec_amd.FNX_DEFLATE_CHUNK
    for n in (1, 100, ch - 1, ch, ch + 1, 2 * ch + 3, 10 * ch + 7, 1 << 25):
        assert lib.fnx_deflate_bound(n) == n + 10 * max(1, -(-n // ch)) + 6, n


def test_the_dense_kernels_are_part_of_the_build():
    csrc = os.path.join(ROOT, "fennec_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert {"deflate_chunk.inc", "deflate_codes.inc", "deflate_dense_chunk.inc"} <= set(hdrs)
    src = open(os.path.join(csrc, "deflate.hip")).read()
    for kernel in ("deflate_dense_chunk_kernel", "deflate_dense_chunk_batch_kernel"):
        assert re.search(rf"__global__[^\n]*\b{kernel}\(", src), kernel
    assert src.count('#include "deflate_dense_chunk.inc"') == 2, "the twins share one body"
