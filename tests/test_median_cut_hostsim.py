"""median_cut.hip's single-workgroup run on the CPU (tools/median_cut_hostsim: fennec_amd/csrc/median_cut_split.inc, the text the
kernel includes, inside a host program that runs the workgroup as a loop over its lanes, phase by phase), built with
AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program and run in a child process; nothing is loaded into
Python.  Its palettes equal the numpy restatement's (tests/median_cut_ref.py) byte for byte on every shared case."""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np
import pytest

import median_cut_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def hostsim(tmp_path_factory):
    build = str(tmp_path_factory.mktemp("median_cut_hostsim") / "build")
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler for the host"
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "median_cut_hostsim"), f"BUILD={build}", f"CXX={cxx}"], check=True)
    return os.path.join(build, "median_cut_hostsim")


def run(exe, img, levels):
    h, w = img.shape[:2]
    r = subprocess.run([exe, str(w), str(h)] + [str(c) for c in levels], input=np.ascontiguousarray(img).tobytes(), capture_output=True)
    assert r.returncode == 0, f"median_cut_hostsim: exit {r.returncode}\n{r.stderr.decode()[-4000:]}"
    out = []
    lines = r.stdout.decode().splitlines()
    assert len(lines) == len(levels)
    for line, level in zip(lines, levels):
        f = line.split()
        assert int(f[0]) == level and len(f) == 2 + int(f[1])
        out.append(np.array([list(bytes.fromhex(e)) for e in f[2:]], dtype=np.uint8).reshape(-1, 4))
    return out


@pytest.mark.parametrize("name", sorted(ref.CASES))
def test_hostsim_equals_the_restatement(hostsim, name):
    img, levels = ref.CASES[name]
    want, _ = ref.want(name)
    got = run(hostsim, img, levels)
    for level, g, w in zip(levels, got, want):
        assert g.shape == w.shape, (name, level, g.shape, w.shape)
        assert np.array_equal(g, w), (name, level, np.argwhere(g != w)[:4])


def test_the_text_is_the_kernels(hostsim):
    """the program and the kernel include one file, and neither holds a copy of its phases"""
    inc = "median_cut_split.inc"
    main = open(os.path.join(ROOT, "tools", "median_cut_hostsim", "main.cpp")).read()
    hip = open(os.path.join(ROOT, "fennec_amd", "csrc", "median_cut.hip")).read()
    assert f'#include "{inc}"' in main and f'#include "{inc}"' in hip
    assert "mc_ph_" not in main and "mc_ph_" not in hip


def test_bad_arguments_exit_2(hostsim):
    for argv in (["4", "4"], ["0", "4", "16"], ["4", "4", "16", "16"], ["4", "4", "257"]):
        assert subprocess.run([hostsim] + argv, input=b"", capture_output=True).returncode == 2
    assert subprocess.run([hostsim, "4", "4", "16"], input=b"\0" * 63, capture_output=True).returncode == 2
