"""The JPEG subsampling mode exists at every layer (no GPU needed): the header declares fnx_ctx_set_jpeg_subsampling and the mode's
two constants, the built library exports it, the binding knows its signature, the default mode is 4:2:0, bad arguments are refused
without a device, and the 4:4:4 colour kernel and the shared layout are part of the build."""
from __future__ import annotations

import ctypes as C
import os
import re

import pytest

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "fnx_ctx_set_jpeg_subsampling"
FOLLOW = ("fnx_jpeg_roundtrip", "fnx_jpeg_quality_search", "fnx_jpeg_encode", "fnx_jpeg_compress", "fnx_jpeg_size_search",
          "fnx_jpeg_symbol_histogram")
REFUSE = ("fnx_jpeg_encode_scaled", "fnx_jpeg_target_size", "fnx_hit_target_size", "fnx_jpeg_recompress", "fnx_jpeg_compress_batch",
          "fnx_jpeg_recompress_batch", "fennec_CompressFileJPEG", "fennec_CompressFileTargetSize", "fennec_CompressFileHitTargetSize")


def _header() -> str:
    return open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


def test_header_declares_the_setter_and_states_the_rule_above_it():
    text = _header()
    code = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    assert re.search(r"\bint\s+fnx_ctx_set_jpeg_subsampling\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*int\s+mode\s*\)\s*;", code)
    assert NAME in fennec_amd.exported_symbols()
    # the comment in front of the constants names every entry that follows the mode and every entry that refuses it
    comment = text[:text.index("#define FNX_JPEG_SUBSAMPLING_420")].rsplit("/*", 1)[1]
    for entry in FOLLOW + REFUSE:
        assert re.search(rf"\b{entry}\b", comment), entry
    assert "0x11 instead of 0x22" in comment and "(w + 7) / 8" in comment


def test_library_exports_the_setter_and_the_binding_has_it():
    lib = fennec_amd.load_library()
    assert hasattr(lib, NAME), f"libfennec_hip.so does not export {NAME}"
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 2
    assert callable(fennec_amd.Context.set_jpeg_subsampling)


def test_constants_and_the_default():
    defs = dict(re.findall(r"^#define\s+(FNX_JPEG_SUBSAMPLING_\w+)\s+(\d+)", _header(), flags=re.M))
    assert set(defs) == {"FNX_JPEG_SUBSAMPLING_420", "FNX_JPEG_SUBSAMPLING_444"}
    assert int(defs["FNX_JPEG_SUBSAMPLING_420"]) == fennec_amd.FNX_JPEG_SUBSAMPLING_420 == 0
    assert int(defs["FNX_JPEG_SUBSAMPLING_444"]) == fennec_amd.FNX_JPEG_SUBSAMPLING_444 == 1
    # a fresh ctx writes 4:2:0: the member's initialiser is that mode's value
    common = open(os.path.join(ROOT, "fennec_amd", "csrc", "common.hpp")).read()
    assert re.search(r"^\s*int\s+jpeg_subsampling\s*=\s*0\s*;", common, flags=re.M)


def test_bad_arguments_are_refused_without_a_device():
    lib = fennec_amd.load_library()
    for mode in (0, 1, -1, 2, 444):
        assert getattr(lib, NAME)(None, mode) == fennec_amd.FNX_ERR_INVALID, mode
        assert NAME.encode() in lib.fnx_last_error()


def test_the_binding_refuses_a_mode_it_does_not_know():
    class NoCtx(fennec_amd.Context):
        def __init__(self):                      # no device: the name check comes before the library is called
            pass

        def __del__(self):
            pass

    with pytest.raises(fennec_amd.FennecError, match="'420' or '444'"):
        NoCtx().set_jpeg_subsampling("422")


def test_the_kernel_and_the_layout_are_part_of_the_build():
    csrc = os.path.join(ROOT, "fennec_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    hdrs = re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "jpeg_layout.hpp" in hdrs
    src = open(os.path.join(csrc, "jpeg.hip")).read()
    assert re.search(r"__global__[^\n]*\bjpeg_ycc444_kernel\(", src)
    assert src.count('#include "jpeg_layout.hpp"') == 1
    # the layout's facts stand in one place: the coder's kernels take them from it, for the mode they are instantiated with
    layout = open(os.path.join(csrc, "jpeg_layout.hpp")).read()
    for fn in ("jpeg_layout_dims", "jpeg_mcu_blocks", "jpeg_scan_index", "jpeg_slot_class", "jpeg_slot_prev"):
        assert re.search(rf"\b{fn}\s*\(", layout), fn
        assert re.search(rf"\b{fn}\s*\(", src), fn
    assert not re.search(r"%\s*6\b", src) and not re.search(r"blk\s*-\s*6\b", src)
