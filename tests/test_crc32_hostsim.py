"""crc32.hip's kernels on the CPU: tools/crc32_hostsim compiles crc32_piece.inc's own text -- a piece's remainder as a loop over
a workgroup's lanes, the fold of the pieces' words and the seed -- under AddressSanitizer + UndefinedBehaviorSanitizer as a
stand-alone program, and every CRC it prints is zlib.crc32's.  CPU only; the Python module is not involved."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

import crc32_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler for the host"
    build = tmp_path_factory.mktemp("crc32_hostsim")
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tools", "crc32_hostsim"), f"BUILD={build}", f"CXX={cxx}"])
    return build / "crc32_hostsim"


def test_constants_are_the_headers():
    import re
    header = open(os.path.join(ROOT, "include", "fennec_hip.h")).read()
    assert int(re.search(r"#define FNX_CRC_RUN\s+(\d+)", header).group(1)) == cc.RUN
    assert int(re.search(r"#define FNX_CRC_PIECE\s+(\d+)", header).group(1)) == cc.PIECE == 256 * cc.RUN


def test_every_case_is_zlibs_crc32(exe, tmp_path):
    for key, data in cc.blobs().items():
        (tmp_path / key).write_bytes(data)
    cases = cc.cases()
    lines = [f"{name} {offset} {length} {seed:x} {tmp_path / key}" for name, offset, length, seed, key, _ in cases]
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stderr == ""
    got = dict(line.split() for line in r.stdout.splitlines())
    assert len(got) == len(cases)
    wrong = [(name, got[name], f"{want:08x}") for name, _, _, _, _, want in cases if got[name] != f"{want:08x}"]
    assert not wrong, wrong[:10]


def test_a_short_file_and_a_bad_line_are_refused(exe, tmp_path):
    (tmp_path / "three").write_bytes(b"abc")
    for text in (f"short 0 4 0 {tmp_path / 'three'}\n", "no numbers here\n", f"far 16 3 0 {tmp_path / 'three'}\n"):
        (tmp_path / "cases.txt").write_text(text)
        r = subprocess.run([str(exe), str(tmp_path / "cases.txt")], capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and r.stderr
