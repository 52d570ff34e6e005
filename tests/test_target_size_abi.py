"""Target-size mode's entry points in the C ABI (no GPU needed): declared by the header, exported by the built library,
and laid out in ctypes as the header lays out fnx_size_candidate."""
from __future__ import annotations

import ctypes as C
import os
import re

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "fennec_hip.h")).read()


def test_header_declares_the_target_size_entry_points():
    text = _header()
    for name in ("fnx_jpeg_encode_scaled", "fnx_jpeg_target_size"):
        assert re.search(rf"\bint {name}\(", text), name
    defines = dict(re.findall(r"^#define (FNX_TS_\w+) (\d+)", text, flags=re.M))
    assert defines == {"FNX_TS_QUALITY": "1", "FNX_TS_QUALITY_SCALE": "2", "FNX_TS_SCALE": "4", "FNX_TS_FALLBACK": "8"}
    assert (fennec_amd.FNX_TS_QUALITY, fennec_amd.FNX_TS_QUALITY_SCALE, fennec_amd.FNX_TS_SCALE, fennec_amd.FNX_TS_FALLBACK) == (1, 2, 4, 8)
    assert "Target-size mode stays the caller's" not in text


def test_library_exports_them():
    lib = fennec_amd.load_library()
    assert hasattr(lib, "fnx_jpeg_encode_scaled") and hasattr(lib, "fnx_jpeg_target_size")


def test_size_candidate_layout():
    s = fennec_amd.SizeCandidate
    assert C.sizeof(s) == 40
    assert [(n, getattr(s, n).offset) for n, _ in s._fields_] == [
        ("strategy", 0), ("quality", 4), ("final_w", 8), ("final_h", 12), ("steps", 16), ("reserved", 20), ("nbytes", 24), ("ssim", 32)]
    body = re.search(r"typedef struct fnx_size_candidate \{(.*?)\} fnx_size_candidate;", _header(), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(int32_t|int64_t|double)\s+([\w ,]+);", body)
    names = [n.strip() for _, group in fields for n in group.split(",")]
    assert names == [n for n, _ in s._fields_]
