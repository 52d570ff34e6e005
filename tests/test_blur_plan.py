"""GaussianBlur's host plan (fennec_amd/csrc/blur_plan.cpp) as a stand-alone program (tools/blur_plan_host.cpp), built from those
two files alone under AddressSanitizer and UndefinedBehaviorSanitizer and fed a sweep of calls on stdin.  What is asserted:
the mirror rule (a call's one-pass blur + SSIMFast form is its plain kernel's SCORE form or none), that the sweep reaches every
family and form, and each documented boundary of the route as a pair of neighbouring cases.  CPU only; no Python module is
loaded into the program."""
from __future__ import annotations

import math
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256                                   # MI355X
MATRIX = ("mfma", "mfma_wide")
RF = {2: 14, 3: 22, 4: 24, 5: 38, 6: 46, 7: 54, 8: 62}     # frame radius of blur_mfma_wide_kernel<NKH> (blur_plan.hpp: mf_wide_rf)


# ---- tables ----
def gaussian(radius):
    """effects.go:153-165 with sigma = radius / 3"""
    sigma = radius / 3.0
    k = [math.exp(-(x * x) / (2 * sigma * sigma)) for x in range(-radius, radius + 1)]
    s = sum(k)
    return [v / s for v in k]


def binomial(radius):
    return [math.comb(2 * radius, i) / 4.0 ** radius for i in range(2 * radius + 1)]


def peaked(radius, centre):
    """non-negative, sums to 1, the centre weight given"""
    k = [(1.0 - centre) / (2 * radius)] * (2 * radius + 1)
    k[radius] = centre
    return k


def negative(radius):
    """sums to 1 with negative lobes (an unsharp mask): outside what the guarded kernels' bound covers"""
    k = [-0.2 / (2 * radius)] * (2 * radius + 1)
    k[radius] = 1.2
    return k


def ssim_fast_dims(w, h):
    """ssim.go:52-56"""
    if max(w, h) <= 512:
        return w, h
    scale = 512.0 / max(w, h)
    return int(max(8, math.floor(w * scale + 0.5))), int(max(8, math.floor(h * scale + 0.5)))


def case(w, h, kernel, exact=False, n=1, cus=CUS, dst=None):
    dw, dh = dst or ssim_fast_dims(w, h)
    return (cus, n, w, h, int(exact), dw, dh, (len(kernel) - 1) // 2, tuple(kernel))


def sweep_cases():
    small = [(w, h) for w in (63, 64, 65, 128) for h in (31, 32, 33, 48)]                                       # 64 px, 32 rows
    segs = [(w, h) for w in (640, 1920) for h in (271, 272, 273, 543, 544, 545, 1087, 1088, 1089)]              # segment caps
    odd = [(s, s * 3 // 4) for s in range(1843, 2048, 17)] + [(s * 9 // 16, s) for s in range(1849, 2048, 17)]  # boxes under 4 px
    odd += [(s, t) for s in range(1840, 1848) for t in (s, s * 3 // 4)]                                         # ratio 3.6: 1843.2 / 512
    odd += [(2047, 1151), (2048, 1152), (1600, 1200), (2200, 1467), (2560, 1440)]
    full = [(1920, 1080), (3840, 2160)]
    some = (1, 3, 6, 7, 8, 9, 14, 15, 16, 17, 22, 23, 24, 25, 26, 27, 38, 39, 62, 63)
    gauss = {r: gaussian(r) for r in range(1, 64)}
    out = []
    for exact in (False, True):
        out += [case(w, h, gauss[r], exact) for (w, h) in small + odd for r in some]
        for n in (1, 32):
            out += [case(w, h, gauss[r], exact, n) for (w, h) in segs for r in some]
            out += [case(w, h, gauss[r], exact, n) for (w, h) in full for r in range(1, 64)]
        for (w, h) in small + segs[::3] + odd[::2] + full:
            out += [case(w, h, binomial(r), exact) for r in (1, 2, 4, 6, 7, 8, 12, 20)]
            out += [case(w, h, negative(r), exact) for r in (1, 8, 9, 16, 17)]
            out += [case(w, h, peaked(3, c), exact) for c in (0.48, 0.49)]
        out += [case(3840, 2160, gauss[6], exact, 70000), case(7680, 4320, gauss[6], exact, 4), case(7680, 4320, gauss[12], exact, 4)]
        out += [case(3840, 2160, gauss[6], exact, n, cus) for n in (1, 8) for cus in (64, 304)]
    return out


# ---- the program ----
SANITIZE = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


def build_program(directory, flags):
    """tools/blur_plan_host.cpp + blur_plan.cpp by g++ alone, with `flags` on top of -O1"""
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tools/blur_plan_host.cpp")
    exe = os.path.join(str(directory), "blur_plan_host")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off"] + flags + ["-I" + os.path.join(ROOT, "fennec_amd", "csrc"),
                           os.path.join(ROOT, "tools", "blur_plan_host.cpp"), os.path.join(ROOT, "fennec_amd", "csrc", "blur_plan.cpp"), "-o", exe])
    return exe


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    return build_program(tmp_path_factory.mktemp("blur_plan"), SANITIZE)


def case_line(c):
    return " ".join(str(v) for v in c[:8]) + " " + " ".join(float(v).hex() for v in c[8])


PLAIN = re.compile(r"^plain (\w+) nkh=(\d+) R=(\d+) tall=(\d) guard=(\d) wdp=(\d) seg=(\d+) gq=(\d+) route=(.+)$")
SCORED = re.compile(r"^scored (\w+) seg=(\d+) nbx=(\d+) nby=(\d+) tall=(\d) route=(.+)$")


def parse(line):
    plain, scored, crcs = line.split(" | ")
    m = PLAIN.match(plain)
    assert m, line
    r = dict(family=m.group(1), nkh=int(m.group(2)), radius=int(m.group(3)), tall=int(m.group(4)), guard=int(m.group(5)), wdp=int(m.group(6)),
             seg=int(m.group(7)), gq=int(m.group(8)), route=m.group(9), scored=None, line=line)
    if scored != "none":
        s = SCORED.match(scored)
        assert s, line
        r["scored"] = dict(tile=s.group(1), seg=int(s.group(2)), nbx=int(s.group(3)), nby=int(s.group(4)), tall=int(s.group(5)), route=s.group(6))
    return r


def run(program, cases):
    r = subprocess.run([program], input="\n".join(case_line(c) for c in cases) + "\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.splitlines()
    assert len(lines) == len(cases)
    return [parse(l) for l in lines]


@pytest.fixture(scope="module")
def sweep(program):
    cases = sweep_cases()
    return cases, run(program, cases)


def plan(program, *a, **kw):
    return run(program, [case(*a, **kw)])[0]


# ---- the mirror rule ----
def test_the_one_pass_form_is_the_plain_kernels_or_none(sweep):
    cases, plans = sweep
    assert len(cases) > 5000
    for c, p in zip(cases, plans):
        s = p["scored"]
        if s is None:
            continue
        # the geometry is cut for the plain family's tile, and only the families with a SCORE form have one
        assert p["family"] in MATRIX + ("direct",) and (s["tile"] == "matrix") == (p["family"] in MATRIX), p["line"]
        assert p["radius"] <= (8 if p["family"] == "direct" else 24), p["line"]
        assert ("GUARD" in s["route"]) == ("GUARD" in p["route"]) == bool(c[4]), p["line"]
        assert s["route"].split("<")[0] == p["route"].split("<")[0] and "<SCORE" in s["route"], p["line"]
        assert s["seg"] <= {"mfma": 272, "mfma_wide": 544, "direct": 104}[p["family"]] and (s["nbx"] + 1) * (s["nby"] + 1) <= 1024, p["line"]


def test_the_sweep_reaches_every_family_and_form(sweep):
    _, plans = sweep
    plain = {p["family"] for p in plans}
    assert plain == {"mfma", "mfma_wide", "direct", "exact", "generic_f32", "generic_f64"}
    assert {p["family"] for p in plans if p["scored"]} == {"mfma", "mfma_wide", "direct"}
    assert {p["nkh"] for p in plans if p["family"] == "mfma_wide"} == set(range(2, 9))
    assert {(p["tall"], p["guard"]) for p in plans if p["family"] == "direct"} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # the class tools/fuzz_blur.py once found: GaussianBlur alone runs on the matrix pipe, its one-pass geometry does not fit
    # (boxes under 4 px: long side 1843 .. 2047) -- and no other kernel may take the step
    lost = [p for c, p in zip(_, plans) if p["family"] in MATRIX and p["scored"] is None and p["radius"] <= 6 and 1844 <= max(c[2], c[3]) <= 2047
            and min(c[2] / c[5], c[3] / c[6]) >= 3.6]
    assert len(lost) >= 10, len(lost)


def test_segments_keep_their_caps(sweep):
    cases, plans = sweep
    for c, p in zip(cases, plans):
        if p["family"] in MATRIX:
            assert 16 <= p["seg"] <= 544 and p["seg"] % 16 == 0, p["line"]
    assert any(p["seg"] > 272 for p in plans if p["family"] == "mfma") and any(p["scored"]["seg"] > 272 for p in plans if p["scored"] and p["family"] == "mfma_wide")


# ---- the documented boundaries, each as a pair of neighbouring cases ----
def test_64_by_32_is_the_smallest_matrix_image(program):
    for exact in (False, True):
        assert plan(program, 64, 32, gaussian(6), exact)["family"] == "mfma"
        assert plan(program, 63, 32, gaussian(6), exact)["family"] == "direct"
        assert plan(program, 64, 31, gaussian(6), exact)["family"] == "direct"
        assert plan(program, 64, 32, gaussian(7), exact)["family"] == "mfma_wide"
        assert plan(program, 63, 32, gaussian(7), exact)["family"] == "direct"


def test_radius_6_is_narrow_and_7_wide(program):
    a, b = plan(program, 640, 480, gaussian(6)), plan(program, 640, 480, gaussian(7))
    assert (a["family"], a["nkh"], a["route"]) == ("mfma", 0, "blur_mfma_kernel")
    assert (b["family"], b["nkh"], b["route"]) == ("mfma_wide", 2, "blur_mfma_wide_kernel")


def test_nkh_steps_at_the_frame_radii(program):
    plans = run(program, [case(640, 480, gaussian(r), exact) for r in range(7, 64) for exact in (False, True)])
    for p in plans:
        r = p["radius"]
        if r == 63:
            assert (p["family"], p["route"]) == ("generic_f64", "blur_pass_kernel<double> x 2"), p["line"]
        else:
            assert (p["family"], p["nkh"]) == ("mfma_wide", min(k for k in RF if r <= RF[k])), p["line"]


def test_a_weight_of_049_takes_the_direct_kernel(program):
    for exact in (False, True):
        assert plan(program, 640, 480, peaked(3, 0.4899), exact)["family"] == "mfma"
        p = plan(program, 640, 480, peaked(3, 0.49), exact)
        assert (p["family"], p["guard"]) == ("direct", int(exact)), p["line"]
        assert plan(program, 640, 480, peaked(3, 0.75), exact)["family"] == "direct"


def test_a_negative_weight_under_exact(program):
    for r in range(1, 18):
        p = plan(program, 640, 480, negative(r), True)
        assert p["family"] == ("exact" if r <= 8 else "generic_f64"), p["line"]
        assert p["route"] == ("blur_exact_kernel" if r <= 8 else "blur_pass_kernel<double> x 2")
        assert p["scored"] is None
        assert plan(program, 640, 480, negative(r), False)["family"] == ("direct" if r <= 16 else "generic_f32")


def test_fast_generic_is_float_up_to_radius_26(program):
    # an image the matrix kernels do not take, past the direct kernel's 16
    for r, want in ((16, "direct"), (17, "generic_f32"), (26, "generic_f32"), (27, "generic_f64"), (40, "generic_f64")):
        assert plan(program, 63, 40, gaussian(r))["family"] == want
        assert plan(program, 63, 40, gaussian(r), True)["family"] == ("direct" if r <= 16 else "generic_f64")
    assert plan(program, 63, 40, gaussian(17))["route"] == "blur_pass_kernel<float> x 2"


def test_direct_exact_uploads_its_weights_past_radius_8(program):
    assert [plan(program, 63, 40, gaussian(r), True)["wdp"] for r in (8, 9)] == [0, 1]
    assert [plan(program, 63, 40, gaussian(r), False)["wdp"] for r in (8, 9)] == [0, 0]


def test_a_box_ratio_under_36_has_no_one_pass_form(program):
    # dst 512: 1843 / 512 = 3.5996, 1844 / 512 = 3.6016.  The direct kernel (a weight of 0.49), whose geometry takes small boxes
    t = peaked(3, 0.49)
    a, b = plan(program, 1843, 1843, t), plan(program, 1844, 1844, t)
    assert a["family"] == b["family"] == "direct"
    assert a["scored"] is None and b["scored"] is not None and b["scored"]["route"] == "blur_direct_kernel<SCORE>"
    # the short side's ratio counts: 1844 x 1382 -> 512 x 384, 1382 / 384 = 3.599
    assert plan(program, 1844, 1382, t, dst=(512, 384))["scored"] is None
    assert plan(program, 1844, 1383, t, dst=(512, 384))["scored"] is not None
    # and no form where SSIMFast does not downsample at all
    assert plan(program, 512, 512, gaussian(6))["scored"] is None


def test_the_segment_caps(program):
    # one tall image column: the plain launches march up to 544 rows per workgroup, the one-pass narrow form 272, the wide form 544
    for r, fam, cap in ((6, "mfma", 272), (7, "mfma_wide", 544)):
        p = plan(program, 1152, 4352, gaussian(r), n=64)
        assert (p["family"], p["seg"]) == (fam, 544), p["line"]
        assert p["scored"] and p["scored"]["seg"] == cap, p["line"]


def test_more_than_65535_images_take_the_direct_kernel_and_no_one_pass_form(program):
    p = plan(program, 640, 480, gaussian(6), n=65536)
    assert p["family"] == "direct" and p["scored"] is None
    assert plan(program, 640, 480, gaussian(6), n=65535)["family"] == "mfma"
