"""The device CRC-32's C ABI without a GPU: fnx_crc32 and fnx_ctx_set_png_crc exist in the header and the library with their
constants, the setter refuses a NULL ctx and an unknown mode, and png_frame.cpp's tail with the IDAT chunk's CRC handed in
(tools/png_frame_crc_host.cpp, under AddressSanitizer + UndefinedBehaviorSanitizer as a stand-alone program) writes png_file's
bytes."""
from __future__ import annotations

import ctypes
import os
import re
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import fennec_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fennec_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(fennec_amd.LIB_PATH):
        subprocess.check_call(["make", "-s", "-j8", "-C", CSRC])
    return fennec_amd.load_library()


def test_the_symbols_and_constants_are_in_header_library_and_binding(lib):
    header = open(os.path.join(ROOT, "include", "fennec_hip.h")).read()
    raw = ctypes.CDLL(fennec_amd.LIB_PATH)
    for name in ("fnx_crc32", "fnx_ctx_set_png_crc"):
        assert name in fennec_amd.exported_symbols()
        assert hasattr(raw, name) and hasattr(lib, name)
    for name, value in (("FNX_PNG_CRC_HOST", 0), ("FNX_PNG_CRC_DEVICE", 1), ("FNX_CRC_RUN", 64), ("FNX_CRC_PIECE", 16384)):
        assert int(re.search(rf"#define {name}\s+(\d+)", header).group(1)) == value == getattr(fennec_amd, name)
    assert fennec_amd.FNX_CRC_PIECE == 256 * fennec_amd.FNX_CRC_RUN
    assert callable(fennec_amd.Context.crc32) and callable(fennec_amd.Context.set_png_crc)


def test_the_setter_refuses_a_null_ctx_and_an_unknown_mode(lib):
    for mode in (fennec_amd.FNX_PNG_CRC_HOST, fennec_amd.FNX_PNG_CRC_DEVICE, 2, -1):
        assert lib.fnx_ctx_set_png_crc(None, mode) == fennec_amd.FNX_ERR_INVALID
        assert b"fnx_ctx_set_png_crc" in lib.fnx_last_error()


def test_crc32_refuses_bad_arguments_without_a_ctx(lib):
    out = ctypes.c_uint32(7)
    data = np.zeros(4, np.uint8)
    assert lib.fnx_crc32(None, fennec_amd.FNX_HOST, data.ctypes.data, 4, 0, ctypes.byref(out)) == fennec_amd.FNX_ERR_INVALID
    assert out.value == 7


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tools/png_frame_crc_host.cpp")
    out = tmp_path_factory.mktemp("png_frame_crc_host") / "png_frame_crc_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, os.path.join(ROOT, "tools", "png_frame_crc_host.cpp")] +
                          [os.path.join(CSRC, name) for name in ("png_frame.cpp", "png_parse.cpp", "png_compress_plan.cpp")] + ["-o", str(out)])
    return out


def test_the_tail_with_a_given_crc_writes_png_files_bytes(exe, tmp_path):
    rng = np.random.default_rng(5)
    pal = np.concatenate([rng.integers(0, 256, (16, 3), dtype=np.uint8), np.full((16, 1), 255, np.uint8)], axis=1)
    pal[3, 3], pal[9, 3] = 0, 128
    # (w, h, colour type, depth, palette, the bytes deflate reads): a stream of 1 byte and two of 70 000, stored (level 0), so that
    # the IDAT body is longer than one stored block holds
    cases = [(1, 1, 0, 8, None, b"\x00"),
             (6999, 10, 0, 8, None, rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()),
             (13998, 10, 3, 4, pal, rng.integers(0, 256, 70000, dtype=np.uint8).tobytes())]
    records, want = [], []
    for w, h, ct, depth, p, raw in cases:
        z = zlib.compress(raw, 0)
        records.append(struct.pack("<7I", w, h, ct, depth, 0 if p is None else len(p), len(z), zlib.crc32(b"IDAT" + z)) +
                       (b"" if p is None else p.tobytes()) + z)
        want.append(fennec_amd.png_file(np.frombuffer(raw, np.uint8), w, h, ct, depth, p, 0))
    assert len(zlib.compress(cases[1][5], 0)) > 70000
    (tmp_path / "cases.bin").write_bytes(b"".join(records))
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert int(lines[0], 16) == (~zlib.crc32(b"IDAT")) & 0xffffffff          # the register, not the finished CRC
    assert lines[1] == f"png_frame_crc_host: {len(cases)} frames; no sanitizer report"
    out = (tmp_path / "out.bin").read_bytes()
    at = 0
    for k, file in enumerate(want):
        for form in ("given", "computed"):
            (n,) = struct.unpack_from("<I", out, at)
            assert out[at + 4:at + 4 + n] == file, (k, form)
            at += 4 + n
    assert at == len(out)


def test_a_wrong_crc_is_written_as_given(exe, tmp_path):
    """the given-CRC form reads no byte of the body: what it is handed is what the chunk ends with"""
    z = zlib.compress(b"\x00", 0)
    (tmp_path / "cases.bin").write_bytes(struct.pack("<7I", 1, 1, 0, 8, 0, len(z), 0xdeadbeef) + z)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert r.returncode == 0 and r.stderr == ""
    out = (tmp_path / "out.bin").read_bytes()
    (n,) = struct.unpack_from("<I", out, 0)
    given, computed = out[4:4 + n], out[8 + n:8 + 2 * n]
    assert given[-16:-12] == b"\xde\xad\xbe\xef" and given[:-16] == computed[:-16] and given[-12:] == computed[-12:]
    assert computed == fennec_amd.png_file(np.zeros(1, np.uint8), 1, 1, 0, 8, None, 0)
