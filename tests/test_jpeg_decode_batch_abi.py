"""fnx_jpeg_decode_batch and fnx_jpeg_recompress_batch in the C ABI (no GPU needed): declared by the header with their
parameters and the chunk constant, exported by the built library, wrapped by fennec_amd.Context."""
from __future__ import annotations

import os
import re

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


def _decl(name):
    m = re.search(rf"\bint {name}\((.*?)\);", HEADER, flags=re.S)
    assert m, name
    return [p.strip().replace(" ", "") for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")]


def test_header_declares_fnx_jpeg_decode_batch_and_its_chunk():
    params = _decl("fnx_jpeg_decode_batch")
    assert params == ["fnx_ctx*ctx", "intn", "constuint8_t*const*files", "constsize_t*sizes", "uint8_t*const*dsts", "constint*dstrides",
                      "int*ws", "int*hs", "int*status"], params
    m = re.search(r"^#define FNX_JPEG_DECODE_CHUNK\s+(\d+)", HEADER, flags=re.M)
    assert m and int(m.group(1)) == 32
    assert "fnx_jpeg_decode_batch" in fennec_amd.exported_symbols()


def test_header_declares_fnx_jpeg_recompress_batch():
    params = _decl("fnx_jpeg_recompress_batch")
    assert len(params) == 15, params
    assert params[:4] == ["fnx_ctx*ctx", "intn", "constuint8_t*const*files", "constsize_t*sizes"]
    assert params[4:8] == ["constdouble*target_ssim", "constdouble*window", "uint8_t*const*outs", "constsize_t*caps"]
    assert params[8:] == ["size_t*nbytes", "int*quality", "double*ssim", "int*steps", "int*ws", "int*hs", "int*status"]
    assert "fnx_jpeg_recompress_batch" in fennec_amd.exported_symbols()


def test_library_exports_both():
    lib = fennec_amd.load_library()
    assert hasattr(lib, "fnx_jpeg_decode_batch") and len(lib.fnx_jpeg_decode_batch.argtypes) == 9
    assert hasattr(lib, "fnx_jpeg_recompress_batch") and len(lib.fnx_jpeg_recompress_batch.argtypes) == 15


def test_context_has_both_methods():
    assert callable(getattr(fennec_amd.Context, "jpeg_decode_batch", None))
    assert callable(getattr(fennec_amd.Context, "jpeg_recompress_batch", None))
