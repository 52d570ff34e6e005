"""jpeg_dec.hip's span decoder on the CPU (tools/jpeg_dec_hostsim: fennec_amd/csrc/jpeg_dec_span.inc, the text the kernels include,
behind the real jpeg_parse.cpp), built with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program and run in
child processes; nothing is loaded into Python.  Over the crafted files of tests/jpeg_craft_cases.py: the coefficients its write
pass leaves equal the ones the writer coded -- coefficient by coefficient, no pixels between -- every lane's start state equals
the plain walker's (tests/jpeg_craft.py), and the device's pass structure replayed sequentially reaches the same states."""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_craft as jc
import jpeg_craft_cases as cs
from jpeg_craft import SPAN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Sim:
    def __init__(self, tmp):
        self.dir = str(tmp)
        build = os.path.join(self.dir, "build")
        cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
        assert cxx, "no C++ compiler for the host"
        subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "jpeg_dec_hostsim"), f"BUILD={build}", f"CXX={cxx}"], check=True)
        self.exe = os.path.join(build, "jpeg_dec_hostsim")
        self.done = {}

    def run(self, name, data, replay=True):
        """-> dict: exit (the status), stderr, the header's fields as ints (route as text), states (uint64 per lane), coef ((blocks, 64) int16)"""
        if name in self.done:
            return self.done[name]
        path = os.path.join(self.dir, name + ".jpg")
        with open(path, "wb") as f:
            f.write(data)
        r = subprocess.run([self.exe, path] + (["replay"] if replay else []), capture_output=True)
        os.remove(path)
        head, _, rest = r.stdout.partition(b"\n")
        out = {"exit": r.returncode, "stderr": r.stderr.decode(errors="replace")[-3000:]}
        for kv in head.decode().split():
            k, v = kv.split("=")
            out[k] = v if k == "route" else int(v)
        if out.get("route") == "device":
            nl, nb = out["nlanes"], out["nblk"]
            assert len(rest) == 8 * nl + 128 * nb, (name, len(rest))
            out["states"] = np.frombuffer(rest[:8 * nl], np.uint64)
            out["coef"] = np.frombuffer(rest[8 * nl:], np.int16).reshape(nb, 64)
        self.done[name] = out
        return out


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    return Sim(tmp_path_factory.mktemp("jpeg_dec_hostsim"))


def walker_states(cr):
    """every span's start state by the plain walker, chained from the string's first bit"""
    nl = (8 * len(cr.string) + SPAN - 1) // SPAN
    out, st = [], (0, 0, 0)
    for i in range(nl):
        out.append(jc.state_word(*st))
        st = jc.walk(cr, cr.string, *st, (i + 1) * SPAN, cr.rst)[:3]
    return np.array(out, np.uint64)


def _check_sound(sim, name, cr):
    r = sim.run(name, cr.data)
    assert r["exit"] == 0 and r["route"] == "device", (name, r["exit"], r["stderr"])
    assert (r["err"], r["nblk"], r["nbits"], r["rst"]) == (0, len(cr.coef), 8 * len(cr.string), len(cr.rst)), (name, r)
    assert r["blocks"] >= r["nblk"], name                           # (the zeros behind the string can read as blocks too)
    bad = np.flatnonzero((r["coef"] != jc.natural(cr)).any(axis=1))
    assert len(bad) == 0, (name, "first block that differs", int(bad[0]), r["coef"][bad[0]].tolist(), jc.natural(cr)[bad[0]].tolist())
    assert r["replay_ok"] == 1, (name, r["stderr"])
    return r


@pytest.mark.parametrize("group", ["a", "b", "c", "d", "e", "f_small"])
def test_hostsim_coefficients_and_states(sim, group):
    files = getattr(cs, "group_" + group)()
    for name, cr in files.items():
        r = _check_sound(sim, name, cr)
        want = walker_states(cr)
        diff = np.flatnonzero(r["states"] != want)
        assert len(diff) == 0, (name, "lane", int(diff[0]), hex(int(r["states"][diff[0]])), hex(int(want[diff[0]])))
        # ... and where the walker's chain stands on a symbol of a sound file, that is the map's state
        for lane in range(1, len(want), max(1, len(want) // 16)):
            bit = int(want[lane]) & 0xffffffffff
            if np.searchsorted(cr.sym["start"], bit) < len(cr.sym) and bit in cr.sym["start"]:
                assert jc.state_word(*cs.state_at(cr, lane * SPAN)) == int(want[lane]), (name, lane)


def test_hostsim_the_stream_that_never_falls_into_step(sim):
    """(f): a workgroup's chain of corrections takes all 256 passes, and every round across workgroups rights exactly one -- 67
    rounds that change something and the quiet one, beyond the 64 round flags"""
    big = cs.f_big()
    r = _check_sound(sim, "f_big", big)
    assert (r["nlanes"], r["passes"], r["rounds"]) == (16245, 256, 68), r
    # by the map: every fifth span starts a block, the others start 2, 4, 6, 8 bytes into one (z = 1 + 7 k after the DC and k values)
    want = np.array([jc.state_word(*cs.state_at(big, k * SPAN)) for k in range(40)], np.uint64)
    assert np.array_equal(r["states"][:40], want)
    period = r["states"][5:10] - r["states"][0:5]
    assert np.array_equal(r["states"][5:] - r["states"][:-5], np.tile(period, r["nlanes"] // 5)[:r["nlanes"] - 5])
    small = sim.run("f_4wg", cs.group_f_small()["f_4wg"].data)
    assert (small["passes"], small["rounds"]) == (256, 4)
    rst = sim.run("f_4wg_rst", cs.group_f_small()["f_4wg_rst"].data)
    assert rst["rounds"] == 1 and rst["passes"] <= 6                 # a boundary every 500 bytes puts every decoder right


def test_hostsim_minimal_blocks_cut_short(sim):
    r = sim.run("d_cut", cs.d_cut())
    assert r["exit"] == 0 and r["route"] == "refused" and r["stderr"] == ""         # fewer than two bits a block: refused before anything is sized


def test_hostsim_damaged_by_construction(sim):
    g = cs.group_g()
    r = sim.run("g_run_past_63", g["g_run_past_63"][0].data)
    assert r["exit"] == 0 and r["err"] & 4, r
    r = sim.run("g_code_outside_table", g["g_code_outside_table"][0].data)
    assert r["exit"] == 0 and r["err"] & 1, r
    # an interval whose blocks end bytes before its marker: clean under UBSan (the write pass's jump to the boundary used to leave
    # its three words behind: a shift by 64 and more, the next interval's first symbols from stale words), and the blocks of
    # every interval -- the next one's too -- are what the writer put there
    for name in ("g_ends_16_early", "g_ends_3_early"):
        cr, twin = g[name]
        r = sim.run(name, cr.data)
        assert r["exit"] == 0 and r["stderr"] == "", (name, r["stderr"])
        assert r["err"] == 0 and r["replay_ok"] == 1 and np.array_equal(r["coef"], jc.natural(twin)), (name, r["err"])
        assert np.array_equal(r["states"], walker_states(cr)), name
        assert r["blocks"] > r["nblk"]                                # going by position, the appended bytes read as blocks
