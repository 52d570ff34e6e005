"""jpeg_hufftab_kernel's body on the CPU (tools/jpeg_hufftab_hostsim: fennec_amd/csrc/jpeg_hufftab.inc, the text the kernel
includes, inside a host program with the wave's lanes as a loop), built with AddressSanitizer and UndefinedBehaviorSanitizer as a
stand-alone program and run in a child process; nothing is loaded into Python.  Its tables -- counts, values, the coder's
look-up words, the "standard table taken" flag -- against the plain-Python statement of the rule (tests/jpeg_hufftab_ref.py) on
histograms of real coefficients and on the shapes the rule can go wrong on."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

import jpeg_hufftab_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse(stdout):
    """the program's output -> {name: (standard, bits, vals, lut)}"""
    out = {}
    lines = stdout.splitlines()
    assert len(lines) % 4 == 0
    for k in range(0, len(lines), 4):
        name, std, nvals = lines[k].split()
        bits, vals, lut = (lines[k + j].split() for j in (1, 2, 3))
        assert (bits[0], vals[0], lut[0]) == ("bits", "vals", "lut") and std.startswith("standard=") and nvals.startswith("nvals=")
        v = [int(x) for x in vals[1:]]
        assert len(v) == int(nvals[6:])
        out[name] = (int(std[9:]), [int(x) for x in bits[1:]], v, [int(x, 16) for x in lut[1:]])
    return out


def expected(cls, hist):
    """the helper's side of one histogram: (standard, bits, vals, lut)"""
    try:
        bits, vals = ref.build_table(hist)
        std = 0
    except ref.TooLong:
        bits, vals = ref.standard_tables()[cls]
        std = 1
    return std, list(bits), list(vals), ref.lut_words(bits, vals)


@pytest.fixture(scope="module")
def histograms():
    return ref.all_histograms()


@pytest.fixture(scope="module")
def sim(tmp_path_factory, histograms):
    tmp = tmp_path_factory.mktemp("jpeg_hufftab_hostsim")
    build = str(tmp / "build")
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler for the host"
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "jpeg_hufftab_hostsim"), f"BUILD={build}", f"CXX={cxx}"], check=True)
    path = str(tmp / "histograms.txt")
    with open(path, "w") as f:
        for name, cls, h in histograms:
            f.write(f"{name} {cls} " + " ".join(str(int(v)) for v in h) + "\n")
    r = subprocess.run([os.path.join(build, "jpeg_hufftab_hostsim"), path], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr, f"jpeg_hufftab_hostsim: exit {r.returncode}\n{r.stdout[-1000:]}\n{r.stderr[-4000:]}"
    return parse(r.stdout)


def test_every_table_is_the_helpers(sim, histograms):
    assert len(sim) == len(histograms) >= 200 + 6 + 8
    for name, cls, h in histograms:
        got, want = sim[name], expected(cls, h)
        for part, g, w in zip(("standard", "bits", "vals", "lut"), got, want):
            assert g == w, (name, part, g, w)


def test_the_list_holds_what_it_should(sim, histograms):
    by_name = {name: (cls, h) for name, cls, h in histograms}
    # one symbol per table: a single one-bit code, never the all-ones one
    for t in range(4):
        std, bits, vals, lut = sim[f"flat_16x16_t{t}"]
        assert (std, bits, len(vals)) == (0, [1] + [0] * 15, 1) and lut[vals[0]] == 1 << 24
    assert sim["single_symbol"][1:3] == ([1] + [0] * 15, [0x21])
    # all 256 symbols alike: every choice a tie; 255 codes of eight bits would leave no room for the reserved one
    std, bits, vals, _ = sim["all_equal"]
    assert std == 0 and len(vals) == 256 and sorted(vals) == list(range(256)) and sum(bits) == 256
    # the crafted sheets reach all 162 AC symbols of both classes
    for t in (1, 3):
        seen = set()
        for name, (cls, h) in by_name.items():
            if name.startswith(("ac_", "runs_")) and name.endswith(f"_t{t}"):
                seen |= {s for s in range(256) if h[s]}
        assert len(seen & {(r << 4) | s for r in range(16) for s in range(1, 11)}) == 160 and {0x00, 0xF0} <= seen, t
    # the length limiter: 16 untouched, 17 and 32 limited, 33 flagged with the standard table of its class
    for n in (16, 17, 32, 33):
        assert max(ref.code_sizes(ref.geometric_histogram(n))) == n
        std, bits, vals, _ = sim[f"geometric_{n}"]
        assert std == (1 if n == 33 else 0)
        if n == 33:
            assert (bits, vals) == tuple(ref.standard_tables()[33 % 4])
        else:
            assert len(vals) == n and sum(bits) == n
    rnd = [h for name, _, h in histograms if name.startswith("random_")]
    nsym = [sum(1 for v in h if v) for h in rnd]
    assert len(rnd) == 200 and max(max(h) for h in rnd) > 2 ** 30 and min(nsym) < 16 and max(nsym) > 240
