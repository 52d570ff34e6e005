"""jpeg_ffcount_strips_kernel's lane body on the CPU (tools/jpeg_ffcount_hostsim: fennec_amd/csrc/jpeg_ffcount_strips.inc, the text
the kernel includes, inside a host program), built with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program
and run in a child process; nothing is loaded into Python.  The program builds block sequences as strips, bit counts and
positions, runs the body for every block and compares the sum with a pack-then-count of its own; this file checks that the
cases the ownership rule can go wrong on were really among them."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    build = str(tmp_path_factory.mktemp("jpeg_ffcount_hostsim") / "build")
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler for the host"
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "jpeg_ffcount_hostsim"), f"BUILD={build}", f"CXX={cxx}"], check=True)
    r = subprocess.run([os.path.join(build, "jpeg_ffcount_hostsim")], capture_output=True, text=True)
    assert r.returncode == 0, f"jpeg_ffcount_hostsim: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}"
    out = {}
    for line in r.stdout.splitlines():
        m = re.fullmatch(r"(\w+) nblk=(\d+) bits=(\d+) ff=(\d+) want=(\d+) last_ff=([01])", line)
        assert m, line
        out[m.group(1)] = dict(nblk=int(m.group(2)), bits=int(m.group(3)), ff=int(m.group(4)), want=int(m.group(5)), last_ff=int(m.group(6)))
    return out


def test_every_case_agrees_with_the_packed_string(cases):
    assert len(cases) >= 50
    for name, c in cases.items():
        assert c["ff"] == c["want"], (name, c)


def test_lengths_cover_the_strip(cases):
    """4 .. 1600 bits a block (52 words), several workgroups' worth of blocks"""
    rnd = [c for n, c in cases.items() if n.startswith("random_")]
    assert len(rnd) >= 6 and max(c["nblk"] for c in rnd) > 1024
    assert all(c["bits"] > 100 * c["nblk"] for c in rnd)                       # long blocks are among them
    assert cases["single_block_1600_1024"]["ff"] == 200 and cases["single_block_4_1024"]["ff"] == 1


def test_runs_of_minimal_blocks(cases):
    """a byte of 4-bit blocks spans two of them, of 4- and 5-bit blocks three and more"""
    c = cases["run_of_4_bit_blocks_1024"]
    assert c["bits"] == 4 * c["nblk"] and c["ff"] == (c["bits"] + 7) // 8
    c = cases["short_blocks_1024"]
    assert c["ff"] == (c["bits"] + 7) // 8 and c["bits"] % 8
    assert cases["run_of_4_bit_blocks_1000"]["ff"] > 0 and cases["short_blocks_1000"]["ff"] > 0


def test_single_blocks(cases):
    for length in (4, 7, 8, 9, 31, 32, 33, 64, 1599, 1600):
        c = cases[f"single_block_{length}_1024"]
        assert (c["nblk"], c["bits"], c["ff"]) == (1, length, (length + 7) // 8)
        assert f"single_block_{length}_512" in cases


def test_all_ones_and_the_padded_last_byte(cases):
    for rem in range(8):
        c = cases[f"all_ones_rem_{rem}"]
        assert c["bits"] % 8 == rem and c["ff"] == (c["bits"] + 7) // 8 > 0 and c["last_ff"] == 1
        e, z = cases[f"ones_at_the_end_rem_{rem}"], cases[f"zero_in_the_last_byte_rem_{rem}"]
        assert e["bits"] % 8 == rem and e["last_ff"] == 1 and z["last_ff"] == 0 and z["ff"] == e["ff"] - 1
    assert cases["all_ones_rem_0"]["bits"] % 8 == 0                             # a total that is a multiple of 8: no padding
