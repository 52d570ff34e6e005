"""fennec_amd/csrc/jpeg_layout.hpp on the CPU (tools/jpeg_layout_hostsim, built with the address and undefined-behaviour
sanitizers): the functions the JPEG coder's kernels and host code take their layout from, against a plain walk of writer.go's
loops in both subsampling modes, and against the block counts tests/jpeg444_ref.py and the oracle work with.  No GPU."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

import jpeg444_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    build = str(tmp_path_factory.mktemp("jpeg_layout_hostsim") / "build")
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler for the host"
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "jpeg_layout_hostsim"), f"BUILD={build}", f"CXX={cxx}"], check=True)
    return os.path.join(build, "jpeg_layout_hostsim")


def _run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, f"jpeg_layout_hostsim: exit {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-4000:]}"
    return [tuple(int(v) for v in line.split()) for line in r.stdout.splitlines()]


def test_the_layout_is_writer_gos_walk_in_both_modes(exe):
    rows = _run(exe)
    assert len(rows) == 2 * (40 * 40 + 7)
    assert {mode for _, _, mode, _, _, _ in rows} == {0, 1}


def test_the_block_counts_are_the_restatements(exe):
    sizes = ref.SMALL + ref.LARGE
    rows = _run(exe, *[v for wh in sizes for v in wh])
    got = {(w, h, mode): (mx, my, n) for w, h, mode, mx, my, n in rows}
    for w, h in sizes:
        mx, my = ref.dims(w, h)
        assert got[w, h, 1] == (mx, my, 3 * mx * my)
        assert got[w, h, 0] == ((w + 15) // 16, (h + 15) // 16, 6 * ((w + 15) // 16) * ((h + 15) // 16))
    assert got[264, 24, 1][2] == 297


def test_a_size_that_is_no_jpeg_size_is_refused(exe):
    r = subprocess.run([exe, "0", "5"], capture_output=True, text=True)
    assert r.returncode == 1 and "not a JPEG size" in r.stdout
