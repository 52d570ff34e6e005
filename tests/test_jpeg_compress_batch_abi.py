"""fnx_jpeg_compress_batch in the C ABI (no GPU needed): declared by the header with its 15 parameters, exported by the
built library, and wrapped by fennec_amd.Context.jpeg_compress_batch."""
from __future__ import annotations

import os
import re

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _decl(name):
    text = open(os.path.join(ROOT, "include", "fennec_hip.h")).read()
    m = re.search(rf"\bint {name}\((.*?)\);", text, flags=re.S)
    assert m, name
    return re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)


def test_header_declares_fnx_jpeg_compress_batch():
    params = [p.strip() for p in _decl("fnx_jpeg_compress_batch").split(",")]
    assert len(params) == 15, params
    assert params[0] == "fnx_ctx *ctx" and params[1] == "int n"
    assert params[2].replace(" ", "") == "constuint8_t*const*srcs"
    assert params[8].replace(" ", "") == "uint8_t*const*outs"
    assert params[-2].replace(" ", "") == "int*steps" and params[-1].replace(" ", "") == "int*status"
    assert "fnx_jpeg_compress_batch" in fennec_amd.exported_symbols()


def test_library_exports_it():
    lib = fennec_amd.load_library()
    assert hasattr(lib, "fnx_jpeg_compress_batch")
    assert len(lib.fnx_jpeg_compress_batch.argtypes) == 15


def test_context_has_jpeg_compress_batch():
    assert callable(getattr(fennec_amd.Context, "jpeg_compress_batch", None))
