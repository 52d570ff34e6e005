"""fnx_median_cut and fnx_quantize exist at every layer (no GPU needed): the header declares them with the rule and its line
citations above them, the built library exports them, the binding knows their signatures, the Python wrappers are there, the
kernel's file is part of the build, and every refusal the header lists is answered before any device work -- with no ctx at
all here, where the refusal is told apart from the missing ctx by its message."""
from __future__ import annotations

import ctypes as C
import os
import re

import numpy as np
import pytest

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = fennec_amd.FNX_ERR_INVALID


def _header() -> str:
    return open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


def test_header_declares_both_entries():
    code = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    assert re.search(r"\bint\s+fnx_median_cut\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*int\s+space\s*,\s*const\s+uint8_t\s*\*src\s*,\s*int\s+sstride\s*,"
                     r"\s*int\s+w\s*,\s*int\s+h\s*,\s*int\s+nlevels\s*,\s*const\s+int\s*\*max_colors\s*,\s*uint8_t\s*\*palettes\s*,"
                     r"\s*int\s*\*ncolors\s*\)\s*;", code)
    assert re.search(r"\bint\s+fnx_quantize\s*\(\s*fnx_ctx\s*\*ctx\s*,\s*int\s+space\s*,\s*const\s+uint8_t\s*\*src\s*,\s*int\s+sstride\s*,"
                     r"\s*int\s+w\s*,\s*int\s+h\s*,\s*int\s+max_colors\s*,\s*uint8_t\s*\*palette\s*,\s*int\s*\*ncolors\s*,"
                     r"\s*uint8_t\s*\*indices\s*,\s*int\s+istride\s*,\s*uint8_t\s*\*quantized\s*,\s*int\s+qstride\s*,"
                     r"\s*const\s+double\s*\*window\s*,\s*double\s*\*ssim\s*\)\s*;", code)
    for name in ("fnx_median_cut", "fnx_quantize"):
        assert name in fennec_amd.exported_symbols()


def test_header_states_the_rule_with_its_citations():
    text = _header()
    block = text[text.index("/* ---- medianCut (targetsize.go:352-486)"):text.index("int fnx_median_cut(")]
    for cite in ("targetsize.go:426-441", "targetsize.go:449-479", "targetsize.go:400-414", "targetsize.go:443-445", ":469-471", ":473"):
        assert cite in block, cite
    for phrase in ("THE LIBRARY'S TIE RULE", "ANY tie order is a reference answer", "sample number j", "sstride != 4*w", "64 bits",
                   "strictly ascending", "FIRST"):
        assert phrase in block, phrase
    for stale in ("medianCut itself stays with the\n * caller",):
        assert stale not in text


@pytest.mark.parametrize("name,nargs", [("fnx_median_cut", 10), ("fnx_quantize", 15)])
def test_library_exports_the_entry(name, nargs):
    lib = fennec_amd.load_library()
    assert hasattr(C.CDLL(fennec_amd.LIB_PATH), name), f"libfennec_hip.so does not export {name}"
    assert len(getattr(lib, name).argtypes) == nargs


def test_python_wrappers_exist():
    for name in ("median_cut", "quantize"):
        assert callable(getattr(fennec_amd.Context, name)) and callable(getattr(fennec_amd, name)), name


def test_kernel_is_part_of_the_build():
    mk = open(os.path.join(ROOT, "fennec_amd", "csrc", "Makefile")).read()
    assert "median_cut.hip" in re.search(r"^SRCS\s*=(.*)$", mk, flags=re.M).group(1).split()
    assert "median_cut_split.inc" in re.search(r"^HDRS\s*=(.*)$", mk, flags=re.M).group(1).split()
    src = open(os.path.join(ROOT, "fennec_amd", "csrc", "median_cut.hip")).read()
    assert re.search(r"__global__[^\n]*\bmedian_cut_kernel\(", src)


def _call(levels=(16, 256), w=4, h=4, src=True, sstride=None, space=0, pal=True, ncol=True, lv=True):
    """fnx_median_cut without a ctx -> (status, message)"""
    lib = fennec_amd.load_library()
    img = np.zeros((max(h, 1), max(w, 1), 4), np.uint8)
    arr = (C.c_int * max(len(levels), 1))(*levels)
    out = np.zeros((max(len(levels), 1), 256, 4), np.uint8)
    n = (C.c_int * max(len(levels), 1))()
    rc = lib.fnx_median_cut(None, space, img.ctypes.data if src else None, 4 * w if sstride is None else sstride, w, h, len(levels),
                            arr if lv else None, out.ctypes.data if pal else None, n if ncol else None)
    return rc, (lib.fnx_last_error() or b"").decode()


@pytest.mark.parametrize("kw,msg", [
    (dict(src=False), "src pixel pointer is null"),
    (dict(lv=False), "max_colors"),
    (dict(pal=False), "palettes/ncolors is null"),
    (dict(ncol=False), "palettes/ncolors is null"),
    (dict(levels=()), "at least one level"),
    (dict(levels=(0,)), "outside 1..256"),
    (dict(levels=(16, 257)), "outside 1..256"),
    (dict(levels=(16, 16)), "strictly ascending"),
    (dict(levels=(32, 16)), "strictly ascending"),
    (dict(sstride=20), "tight images only"),
    (dict(sstride=12), "tight images only"),
    (dict(w=-1), "negative dims"),
    (dict(h=-1), "negative dims"),
    (dict(space=7), "space must be"),
    (dict(), "null ctx"),                                    # everything else in order: only the ctx is missing
    (dict(w=0, src=False), "null ctx"),                      # an empty image needs no pixels
])
def test_refusals_come_before_any_device_work(kw, msg):
    rc, err = _call(**kw)
    assert rc == INVALID and msg in err, (kw, rc, err)


def test_quantize_refusals():
    lib = fennec_amd.load_library()
    img = np.zeros((4, 4, 4), np.uint8)
    pal = np.zeros((256, 4), np.uint8)
    idx = np.zeros((4, 4), np.uint8)
    n, s = C.c_int(0), C.c_double(0)
    win = (C.c_double * 64)()

    def call(src=img.ctypes.data, sstride=16, w=4, h=4, mc=16, p=pal.ctypes.data, nc=C.byref(n), ip=idx.ctypes.data, istride=4, window=win,
             ssim=C.byref(s)):
        rc = lib.fnx_quantize(None, 0, src, sstride, w, h, mc, p, nc, ip, istride, None, 0, window, ssim)
        return rc, (lib.fnx_last_error() or b"").decode()

    for kw, msg in ((dict(src=None), "src pixel pointer is null"), (dict(sstride=32), "tight images only"), (dict(mc=0), "outside 1..256"),
                    (dict(mc=257), "outside 1..256"), (dict(p=None), "palette/ncolors is null"), (dict(nc=None), "palette/ncolors is null"),
                    (dict(w=0, src=None), "an empty image"), (dict(w=-2), "negative dims"), (dict(ip=None, ssim=None), "no output requested"),
                    (dict(istride=3), "index stride"), (dict(window=None), "window is null"), (dict(), "null ctx")):
        rc, err = call(**kw)
        assert rc == INVALID and msg in err, (kw, rc, err)


def test_empty_image_answer():
    """w*h == 0: one entry (0, 0, 0, 255) at every level and no device work (targetsize.go:443-445) -- on a GPU box through a
    ctx; without a GPU the call is refused for its missing ctx alone (the test above)"""
    lib = fennec_amd.load_library()
    if lib.fnx_device_count() <= 0:
        rc, err = _call(w=0, h=5, src=False)
        assert rc == INVALID and "null ctx" in err
        return
    ctx = fennec_amd.Context(0)
    for shape in ((0, 5, 4), (5, 0, 4), (0, 0, 4)):
        pals = ctx.median_cut(np.zeros(shape, np.uint8), (2, 16, 256))
        assert [p.tolist() for p in pals] == [[[0, 0, 0, 255]]] * 3
