"""The PNG encoder's row stage exists at every layer (no GPU needed): the header declares fnx_png_filter and
fennec_CompressFilePNGStream with the rule in the comment, the built library exports them, the binding knows their signatures,
the Python names are there, the cgo shim's encodePNG goes through the entry, the kernels' file is part of the build, bad
arguments are refused without a device, and fennec_amd.png_file writes files Pillow reads."""
from __future__ import annotations

import os
import re

import numpy as np
import pytest

import fennec_amd
import png_filter_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"fnx_png_filter": 14, "fennec_CompressFilePNGStream": 13}


def _header() -> str:
    return open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


def _code(text: str) -> str:
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def _comment_above(name: str) -> str:
    text = _header()
    decl = text.index(f"int {name}(")
    return text[text.rindex("/*", 0, text.rindex("*/", 0, decl)):decl]


def test_header_declares_both_entries():
    code = _code(_header())
    assert re.search(r"\bint\s+fnx_png_filter\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*int\s+space\s*,\s*int\s+kind\s*,\s*const\s+uint8_t\s*\*src\s*,"
                     r"\s*int\s+sstride\s*,\s*int\s+w\s*,\s*int\s+h\s*,\s*int\s+ncolors\s*,\s*int\s+opaque\s*,\s*uint8_t\s*\*out\s*,"
                     r"\s*size_t\s+cap\s*,\s*size_t\s*\*nbytes\s*,\s*int\s*\*color_type\s*,\s*int\s*\*bit_depth\s*\)\s*;", code)
    assert re.search(r"\bint\s+fennec_CompressFilePNGStream\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*const\s+uint8_t\s*\*data\s*,\s*size_t\s+n\s*,"
                     r"\s*const\s+fennec_FileOptions\s*\*opts\s*,\s*int\s*\*kind\s*,\s*uint8_t\s*\*palette\s*,\s*int\s*\*ncolors\s*,"
                     r"\s*int\s*\*color_type\s*,\s*int\s*\*bit_depth\s*,\s*uint8_t\s*\*out\s*,\s*size_t\s+cap\s*,\s*size_t\s*\*nbytes\s*,"
                     r"\s*int\s+dims\[4\]\s*\)\s*;", code)
    for name in ENTRIES:
        assert name in fennec_amd.exported_symbols()


def test_header_states_the_rule():
    block = _comment_above("fnx_png_filter")
    for cite in ("compress.go:94-107", "targetsize.go:189", "targetsize.go:342"):
        assert cite in block, cite
    for words in ("Up, Paeth, None, Sub, Average", "strictly smaller", "abs8(d) = d < 128 ? d : 256 - d", "abs8(128) = 128",
                  "(left[i] + prev[i]) >> 1", "pa <= pb && pa <= pc", "packed MSB first", "image.NRGBA.Opaque()",
                  "row padding is not looked at", "always get type 0", "FNX_DEVICE_SRC", "independent of launch geometry"):
        assert words in block, words
    assert "compress.go:94-107" in _comment_above("fennec_CompressFilePNGStream")


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_library_exports_the_entry(name):
    lib = fennec_amd.load_library()
    assert hasattr(lib, name), f"libfennec_hip.so does not export {name}"
    assert getattr(lib, name).argtypes, f"{name} has no declared signature in the binding"
    assert len(getattr(lib, name).argtypes) == ENTRIES[name]


def test_python_names_exist():
    for name in ("png_filter", "compress_png", "compress_file_png_stream"):
        assert callable(getattr(fennec_amd.Context, name)), name
    for name in ("png_filter", "compress_png", "png_file"):
        assert callable(getattr(fennec_amd, name)), name


def test_bad_arguments_are_refused_without_a_device():
    """the checks in front of the first device call: no ctx, no GPU needed"""
    lib = fennec_amd.load_library()
    assert lib.fnx_png_filter(None, 0, fennec_amd.FNX_PNG_NRGBA, None, 0, 4, 4, 0, -1, None, 0, None, None, None) == fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_png_filter(None, 0, fennec_amd.FNX_PNG_PALETTED, None, 4, 4, 4, 0, -1, None, 0, None, None, None) == fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_png_filter(None, 0, fennec_amd.FNX_PNG_PALETTED, None, 4, 4, 4, 257, -1, None, 0, None, None, None) == fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_png_filter(None, 0, fennec_amd.FNX_PNG_GRAY, None, 3, 4, 4, 0, -1, None, 0, None, None, None) == fennec_amd.FNX_ERR_INVALID
    assert lib.fennec_CompressFilePNGStream(None, None, 0, None, None, None, None, None, None, None, 0, None, None) == fennec_amd.FNX_ERR_INVALID


def test_shim_encodes_through_the_entry():
    shim = open(os.path.join(ROOT, "go", "fennec_hip.go")).read()
    assert "C.fnx_png_filter(" in shim
    m = re.search(r"^func encodePNG\(w io\.Writer, m image\.Image\) error \{.*?^\}", shim, flags=re.S | re.M)
    assert m, "the shim has no encodePNG(w io.Writer, m image.Image) error"
    body = m.group(0)
    for helper in set(re.findall(r"\b(\w+HIP)\(", body)):
        h = re.search(rf"^func {helper}\(.*?^}}", shim, flags=re.S | re.M)
        body += h.group(0) if h else ""
    assert "C.fnx_png_filter(" in body and "fellBack(" in body
    assert re.search(r"png\.Encoder\{CompressionLevel: png\.BestCompression\}\)?\.Encode\(", body), "no Go twin to fall back to"
    assert "zlib.BestCompression" in body
    for wrapped in ("*image.NRGBA", "*image.Gray", "*image.Paletted"):
        assert wrapped in body, wrapped


def test_kernels_are_part_of_the_build():
    mk = open(os.path.join(ROOT, "fennec_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "png_filter.hip" in srcs
    src = open(os.path.join(ROOT, "fennec_amd", "csrc", "png_filter.hip")).read()
    for kernel in ("png_filter_kernel", "png_pack_kernel", "png_alpha_kernel"):
        assert re.search(rf"__global__[^\n]*\b{kernel}\(", src), kernel
    assert re.search(r"VGPRs?:", src[:src.index("#include")]), "the file header states the VGPR count"


def _palette(n, translucent_upto):
    rng = np.random.default_rng(n)
    pal = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    pal[:, 3] = 255
    pal[:translucent_upto, 3] = rng.integers(0, 255, size=translucent_upto, dtype=np.uint8)
    return pal


@pytest.mark.parametrize("ncolors,upto", [(2, 0), (4, 1), (16, 16), (200, 57)])
def test_png_file_paletted_decodes_with_pillow(ncolors, upto):
    pal = _palette(ncolors, upto)
    idx = np.random.default_rng(1).integers(0, ncolors, size=(9, 13), dtype=np.uint8)
    stream, ct, depth = ref.png_stream(idx, ref.PALETTED, ncolors)
    data = fennec_amd.png_file(stream, 13, 9, ct, depth, pal)
    assert np.array_equal(ref.decode_png(data), pal[idx])
    got = ref.chunks(data)
    assert [t for t, _ in got] == ([b"IHDR", b"PLTE", b"tRNS", b"IDAT", b"IEND"] if upto else [b"IHDR", b"PLTE", b"IDAT", b"IEND"])
    assert len(dict(got)[b"PLTE"]) == 3 * ncolors
    if upto:
        assert dict(got)[b"tRNS"] == pal[:upto, 3].tobytes()       # up to and including the last alpha != 255


@pytest.mark.parametrize("opaque", [True, False])
def test_png_file_truecolour_and_gray_decode_with_pillow(opaque):
    img = ref.smooth_rgba(31, 12, 3, opaque)
    stream, ct, depth = ref.png_stream(img, ref.NRGBA)
    data = fennec_amd.png_file(stream, 31, 12, ct, depth)
    assert np.array_equal(ref.decode_png(data), img)
    assert data == ref.write_png(stream, 31, 12, ct, depth), "the library's writer and the tests' agree byte for byte"
    g = np.ascontiguousarray(img[..., 1])
    stream, ct, depth = ref.png_stream(g, ref.GRAY)
    assert np.array_equal(ref.decode_png(fennec_amd.png_file(stream, 31, 12, ct, depth))[..., 0], g)
