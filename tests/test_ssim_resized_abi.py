"""The resize-then-score entry points exist at every layer (no GPU needed): the header declares them and the "resize_box"
form, the built library exports them, the Python wrappers are there, and the cgo shim routes SSIM / MSSSIM with differing
dims through them."""
from __future__ import annotations

import os
import re

import pytest

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["fnx_lanczos_box_downsample", "fnx_ssim_fast_resized", "fnx_ssim_resized", "fnx_msssim_resized", "fennec_computeSSIMNRGBA"]


def _header() -> str:
    return open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


@pytest.mark.parametrize("name", ENTRIES)
def test_header_declares_the_entry(name):
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    assert re.search(rf"\bint\s+{name}\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*int\s+space\b", code), f"{name} is not declared"
    assert name in fennec_amd.exported_symbols()


def test_every_entry_cites_the_go_it_replaces():
    text = _header()
    for name, cite in [("fnx_lanczos_box_downsample", "ssim.go:244-309"), ("fnx_ssim_fast_resized", "targetsize.go:563-568"),
                       ("fnx_ssim_resized", "ssim.go:24-43"), ("fnx_msssim_resized", "ssim.go:313-365"),
                       ("fennec_computeSSIMNRGBA", "targetsize.go:563-568")]:
        decl = text.index(f"int {name}(")
        comment = text[text.rindex("/*", 0, decl):decl]
        assert cite in comment, f"{name}: the comment above it does not cite {cite}"


def test_header_lists_the_form_and_the_fused_domain():
    text = _header()
    assert '"resize_box" "1"' in text
    block = text[text.index("boxDownsample(lanczosResize(src, midW, midH), dstW, dstH)"):text.index("int fnx_lanczos_box_downsample(")]
    assert "Fused domain" in block and "resize_box_kernel" in block and "composed" in block


@pytest.mark.parametrize("name", ENTRIES)
def test_library_exports_the_entry(name):
    lib = fennec_amd.load_library()
    assert hasattr(lib, name), f"libfennec_hip.so does not export {name}"
    assert getattr(lib, name).argtypes, f"{name} has no declared signature in the binding"


def test_python_wrappers_exist():
    for name in ("computeSSIMNRGBA", "lanczosBoxDownsample", "ssim_fast_resized", "ssim_resized", "msssim_resized", "SSIM", "MSSSIM"):
        assert callable(getattr(fennec_amd.Context, name)), name
    for name in ("computeSSIMNRGBA", "lanczosBoxDownsample"):
        assert callable(getattr(fennec_amd, name)), name


def test_the_form_name_is_a_form_of_the_library():
    src = open(os.path.join(ROOT, "fennec_amd", "csrc", "runtime.cpp")).read()
    names = src[src.index("FORM_NAMES[FORM_COUNT]"):]
    names = names[:names.index("};")]
    assert '"resize_box"' in names
    common = open(os.path.join(ROOT, "fennec_amd", "csrc", "common.hpp")).read()
    assert "FORM_RESIZE_BOX" in common[common.index("enum Form"):common.index("FORM_COUNT")]


def test_shim_scores_differing_dims_in_one_call():
    shim = open(os.path.join(ROOT, "go", "fennec_hip.go")).read()
    for call in ("C.fnx_ssim_resized(", "C.fnx_msssim_resized(", "C.fnx_ssim_fast_resized("):
        assert call in shim, call
    m = re.search(r"^func computeSSIMNRGBA\(a, b \*image\.NRGBA\) float64 \{.*?^\}", shim, flags=re.S | re.M)
    assert m, "the shim has no computeSSIMNRGBA with the reference's signature (targetsize.go:563)"
    body = m.group(0)
    # refused or not made: the reference's body on the shadowed functions, which count their own fallbacks
    assert "resizedHIP(resizedFast" in body and "lanczosResize(b, w, h)" in body and "return SSIMFast(a, b)" in body
    for fn in ("SSIM", "MSSSIM"):
        body = re.search(rf"^func {fn}\(.*?^\}}", shim, flags=re.S | re.M).group(0)
        assert "resizedHIP(" in body and "fellBack(" in body and re.search(r"\b\w+Go\(", body)


def _ssim_fast_dims(w, h):
    import ctypes as C
    nw, nh = C.c_int(), C.c_int()
    fennec_amd.load_library().fennec_ssimFastDims(w, h, C.byref(nw), C.byref(nh))
    return nw.value, nh.value


@pytest.mark.parametrize("aw,ah", [(513, 300), (520, 513), (1000, 600), (1280, 720), (1920, 1080), (3840, 2160), (4000, 3000),
                                   (8192, 4320), (8192, 8192), (600, 9000), (1001, 603)])
def test_every_target_size_pair_is_in_the_fused_domain(aw, ah):
    """fnx_lanczos_box_fused (host arithmetic): b = int(aw s) x int(ah s) for 0.05 <= s < 1 with both dims >= 8, a's long side
    from 513 to beyond 8192 px -- what jpegQualityScaleSearch / scaleSearch hand computeSSIMNRGBA"""
    pw, ph = _ssim_fast_dims(aw, ah)
    scales = [0.05 + (0.999 - 0.05) * k / 40 for k in range(41)] + [0.75, 0.5, 0.375, 0.25]
    seen = 0
    for s in scales:
        bw, bh = int(aw * s), int(ah * s)
        if bw < 8 or bh < 8:
            continue
        seen += 1
        assert fennec_amd.lanczos_box_fused(bw, bh, aw, ah, pw, ph), (aw, ah, bw, bh)
    assert seen >= 30


def test_what_lies_outside_the_fused_domain():
    assert not fennec_amd.lanczos_box_fused(2000, 1200, 1000, 600, 512, 307)        # a downscale
    assert not fennec_amd.lanczos_box_fused(500, 1200, 1000, 600, 512, 307)         # ... on one axis
    assert not fennec_amd.lanczos_box_fused(500, 300, 1000, 600, 1200, 720)         # dst above mid
    (oh, ih, wh), tv = fennec_amd.precomputeWeights(1000, 500), fennec_amd.precomputeWeights(600, 300)
    ih = ih.copy()
    ih[int(oh[400]) + 2] += 1 if ih[int(oh[400]) + 2] + 1 < 500 else -1             # a gap in one output's tap indices
    assert not fennec_amd.lanczos_box_fused(500, 300, 1000, 600, 512, 307, ((oh, ih, wh), tv))
    ih[:] = 10 ** 6                                                                   # indices outside the source
    assert not fennec_amd.lanczos_box_fused(500, 300, 1000, 600, 512, 307, ((oh, ih, wh), tv))
