"""The device deflate exists at every layer (no GPU needed): the header declares fnx_deflate_bound, fnx_deflate, fnx_png_encode
and fennec_CompressFilePNG, the built library exports them, the binding knows their signatures and constants, the Python names
are there, the kernels' file is part of the build, the bound is the stored bound, and bad arguments are refused without a device."""
from __future__ import annotations

import inspect
import os
import re

import pytest

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"fnx_deflate_bound": 1, "fnx_deflate": 8, "fnx_png_encode": 13, "fennec_CompressFilePNG": 9}


def _header() -> str:
    return open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


def _code(text: str) -> str:
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_header_declares_the_entries():
    code = _code(_header())
    assert re.search(r"\bsize_t\s+fnx_deflate_bound\s*\(\s*size_t\s+n\s*\)\s*;", code)
    assert re.search(r"\bint\s+fnx_deflate\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*int\s+space\s*,\s*const\s+uint8_t\s*\*src\s*,\s*size_t\s+n\s*,"
                     r"\s*int\s+row\s*,\s*uint8_t\s*\*out\s*,\s*size_t\s+cap\s*,\s*size_t\s*\*nbytes\s*\)\s*;", code)
    assert re.search(r"\bint\s+fnx_png_encode\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*int\s+space\s*,\s*int\s+kind\s*,\s*const\s+uint8_t\s*\*src\s*,"
                     r"\s*int\s+sstride\s*,\s*int\s+w\s*,\s*int\s+h\s*,\s*int\s+ncolors\s*,\s*int\s+opaque\s*,\s*const\s+uint8_t\s*\*palette\s*,"
                     r"\s*uint8_t\s*\*out\s*,\s*size_t\s+cap\s*,\s*size_t\s*\*nbytes\s*\)\s*;", code)
    assert re.search(r"\bint\s+fennec_CompressFilePNG\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*const\s+uint8_t\s*\*data\s*,\s*size_t\s+n\s*,"
                     r"\s*const\s+fennec_FileOptions\s*\*opts\s*,\s*uint8_t\s*\*out\s*,\s*size_t\s+cap\s*,\s*size_t\s*\*nbytes\s*,"
                     r"\s*int\s+dims\[4\]\s*,\s*int\s*\*kind\s*\)\s*;", code)
    for name in ENTRIES:
        assert name in fennec_amd.exported_symbols()


def test_constants_agree_with_the_header():
    defs = dict(re.findall(r"^#define\s+(FNX_DEFLATE_\w+)\s+(\d+)", _header(), flags=re.M))
    assert int(defs["FNX_DEFLATE_CHUNK"]) == fennec_amd.FNX_DEFLATE_CHUNK
    assert int(defs["FNX_DEFLATE_SUB"]) == fennec_amd.FNX_DEFLATE_SUB
    assert fennec_amd.FNX_DEFLATE_SUB >= 64 and fennec_amd.FNX_DEFLATE_CHUNK % fennec_amd.FNX_DEFLATE_SUB == 0
    assert fennec_amd.FNX_DEFLATE_CHUNK <= 32768                     # a distance is at most 32768 (RFC 1951)


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_library_exports_the_entry(name):
    lib = fennec_amd.load_library()
    assert hasattr(lib, name), f"libfennec_hip.so does not export {name}"
    assert getattr(lib, name).argtypes, f"{name} has no declared signature in the binding"
    assert len(getattr(lib, name).argtypes) == ENTRIES[name]


def test_python_names_exist():
    for name in ("deflate", "png_encode", "compress_file_png", "compress_png"):
        assert callable(getattr(fennec_amd.Context, name)), name
    for name in ("deflate", "png_encode", "deflate_bound"):
        assert callable(getattr(fennec_amd, name)), name
    sig = inspect.signature(fennec_amd.Context.compress_png)
    assert sig.parameters["device_deflate"].default is False and sig.parameters["level"].default == 9
    assert inspect.signature(fennec_amd.Context.deflate).parameters["row"].default == 0


def test_bound_is_the_stored_bound():
    """every chunk stored (5 bytes) and closed by the empty stored block (5), 2 bytes of header, 4 of Adler-32"""
    lib = fennec_amd.load_library()
    C = fennec_amd.FNX_DEFLATE_CHUNK
    sizes = [0, 1, 2, 100, C - 1, C, C + 1, 2 * C, 2 * C + 3, 10 * C + 7, 1 << 25, (1 << 32) + 5]
    bounds = [lib.fnx_deflate_bound(n) for n in sizes]
    for n, b in zip(sizes, bounds):
        assert b >= n + 6, (n, b)
        assert b == n + 10 * max(1, -(-n // C)) + 6, (n, b)
    assert bounds == sorted(bounds)
    assert all(lib.fnx_deflate_bound(n + 1) >= lib.fnx_deflate_bound(n) for n in range(C - 3, C + 3))
    assert fennec_amd.deflate_bound(1) == lib.fnx_deflate_bound(1)


def test_bad_arguments_are_refused_without_a_device():
    """the checks in front of the first device call: no ctx, no GPU needed"""
    lib = fennec_amd.load_library()
    bad = fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_deflate(None, 0, None, 0, 0, None, 0, None) == bad            # n = 0, null pointers
    assert lib.fnx_deflate(None, 0, None, 16, 0, None, 0, None) == bad
    assert lib.fnx_deflate(None, 7, None, 16, 0, None, 0, None) == bad           # a bad space
    assert lib.fnx_png_encode(None, 0, fennec_amd.FNX_PNG_NRGBA, None, 0, 4, 4, 0, -1, None, None, 0, None) == bad
    assert lib.fnx_png_encode(None, 0, fennec_amd.FNX_PNG_PALETTED, None, 4, 4, 4, 4, -1, None, None, 0, None) == bad
    assert lib.fnx_png_encode(None, 9, fennec_amd.FNX_PNG_GRAY, None, 4, 4, 4, 0, -1, None, None, 0, None) == bad
    assert lib.fennec_CompressFilePNG(None, None, 0, None, None, 0, None, None, None) == bad
    assert lib.fnx_last_error()


def test_kernels_are_part_of_the_build():
    mk = open(os.path.join(ROOT, "fennec_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "deflate.hip" in srcs and "png_api.cpp" in srcs
    src = open(os.path.join(ROOT, "fennec_amd", "csrc", "deflate.hip")).read()
    for kernel in ("deflate_chunk_kernel", "deflate_gather_kernel"):
        assert re.search(rf"__global__[^\n]*\b{kernel}\(", src), kernel
    head = src[:src.index("#include")]
    for words in ("RFC 1950", "RFC 1951", "no scratch", "VGPRs"):
        assert words in head, words
    assert "asm" not in _code(re.sub(r"//[^\n]*", " ", src)), "no inline assembly is needed"
