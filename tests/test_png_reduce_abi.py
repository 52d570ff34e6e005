"""compressPNG's pixel stages exist at every layer (no GPU needed): the header declares fnx_png_reduce,
fennec_CompressFilePNGReduce and the three kinds, the built library exports them, the binding knows their signatures, the
Python wrappers are there, the cgo shim routes tryPalettize and the PNG branch of a JPEG source through them, and the kernels'
file is part of the build."""
from __future__ import annotations

import os
import re

import pytest

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["fnx_png_reduce", "fennec_CompressFilePNGReduce"]


def _header() -> str:
    return open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


def _code(text: str) -> str:
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_header_declares_both_entries():
    code = _code(_header())
    assert re.search(r"\bint\s+fnx_png_reduce\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*int\s+space\s*,\s*const\s+uint8_t\s*\*src\s*,\s*int\s+sstride\s*,"
                     r"\s*int\s+w\s*,\s*int\s+h\s*,\s*int\s+max_colors\s*,\s*int\s*\*kind\s*,\s*uint8_t\s*\*palette\s*,\s*int\s*\*ncolors\s*,"
                     r"\s*uint8_t\s*\*plane\s*,\s*int\s+pstride\s*\)\s*;", code)
    assert re.search(r"\bint\s+fennec_CompressFilePNGReduce\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*const\s+uint8_t\s*\*data\s*,\s*size_t\s+n\s*,"
                     r"\s*const\s+fennec_FileOptions\s*\*opts\s*,\s*int\s*\*kind\s*,\s*uint8_t\s*\*palette\s*,\s*int\s*\*ncolors\s*,"
                     r"\s*uint8_t\s*\*out\s*,\s*size_t\s+cap\s*,\s*size_t\s*\*nbytes\s*,\s*int\s+dims\[4\]\s*\)\s*;", code)
    for name in ENTRIES:
        assert name in fennec_amd.exported_symbols()


def test_header_defines_the_three_kinds():
    text = _header()
    for name, value in (("FNX_PNG_PALETTED", 1), ("FNX_PNG_GRAY", 2), ("FNX_PNG_NRGBA", 3)):
        assert re.search(rf"^#define\s+{name}\s+{value}\b", text, flags=re.M), name
        assert getattr(fennec_amd, name) == value


@pytest.mark.parametrize("name", ENTRIES)
def test_every_entry_cites_the_go_it_replaces(name):
    text = _header()
    decl = text.index(f"int {name}(")
    comment = text[text.rindex("/*", 0, text.rindex("*/", 0, decl)):decl] if name == "fennec_CompressFilePNGReduce" else \
        text[text.index("/* ---- compressPNG's pixel stages"):decl]
    for cite in ("compress.go:90-153", "convert.go:76-100"):
        assert cite in comment, f"{name}: the comment above it does not cite {cite}"


def test_header_states_the_palette_order_rule():
    text = _header()
    block = text[text.index("/* ---- compressPNG's pixel stages"):text.index("int fnx_png_reduce(")]
    assert "first occurrence" in block and "Go map" in block and "ANY order is a reference answer" in block


@pytest.mark.parametrize("name", ENTRIES)
def test_library_exports_the_entry(name):
    lib = fennec_amd.load_library()
    assert hasattr(lib, name), f"libfennec_hip.so does not export {name}"
    assert getattr(lib, name).argtypes, f"{name} has no declared signature in the binding"
    assert len(getattr(lib, name).argtypes) == {"fnx_png_reduce": 12, "fennec_CompressFilePNGReduce": 11}[name]


def test_python_wrappers_exist():
    for name in ("png_reduce", "tryPalettize", "compress_file_png_reduce"):
        assert callable(getattr(fennec_amd.Context, name)), name
    for name in ("png_reduce", "tryPalettize"):
        assert callable(getattr(fennec_amd, name)), name


def test_bad_arguments_are_refused_without_a_device():
    """the checks in front of the first device call: no ctx, no GPU needed"""
    lib = fennec_amd.load_library()
    assert lib.fnx_png_reduce(None, 0, None, 0, 4, 4, 256, None, None, None, None, 0) == fennec_amd.FNX_ERR_INVALID
    assert lib.fennec_CompressFilePNGReduce(None, None, 0, None, None, None, None, None, 0, None, None) == fennec_amd.FNX_ERR_INVALID


def test_shim_routes_tryPalettize_and_the_png_branch():
    shim = open(os.path.join(ROOT, "go", "fennec_hip.go")).read()
    for call in ("C.fnx_png_reduce(", "C.fennec_CompressFilePNGReduce("):
        assert call in shim, call
    m = re.search(r"^func tryPalettize\(img \*image\.NRGBA, maxColors int\) \*image\.Paletted \{.*?^\}", shim, flags=re.S | re.M)
    assert m, "the shim has no tryPalettize with the reference's signature (compress.go:112)"
    body = m.group(0)
    assert "tryPalettizeGo(" in body and "fellBack(" in body and "C.fnx_png_reduce(" in body
    # the PNG branch of a JPEG source hands the reference's png.Encoder one of its three image types
    for wrapped in ("image.Paletted", "image.Gray", "image.NRGBA"):
        assert wrapped in shim[shim.index("C.fennec_CompressFilePNGReduce("):], wrapped


def test_kernels_are_part_of_the_build():
    mk = open(os.path.join(ROOT, "fennec_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "png_reduce.hip" in srcs
    src = open(os.path.join(ROOT, "fennec_amd", "csrc", "png_reduce.hip")).read()
    for kernel in ("png_colors_kernel", "png_finish_kernel", "png_plane_kernel"):
        assert re.search(rf"__global__[^\n]*\b{kernel}\(", src), kernel
