"""png_parse.cpp -- everything fnx_png_decode does to a file's bytes before its first launch -- as a stand-alone program under
AddressSanitizer and UndefinedBehaviorSanitizer (tools/fuzz_png_host.cpp), over truncations and a few thousand mutations of
files of several colour types.  CPU only; the Python module is not involved.  tools/fuzz_png_host.sh is the long run."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

import png_decode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tools/fuzz_png_host.cpp")
    exe = tmp_path_factory.mktemp("fuzz_png") / "fuzz_png_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "fennec_amd", "csrc"),
                           os.path.join(ROOT, "tools", "fuzz_png_host.cpp"), os.path.join(ROOT, "fennec_amd", "csrc", "png_parse.cpp"),
                           "-o", str(exe)])
    return exe


def test_mutated_files_leave_no_report(fuzz, tmp_path):
    files = []
    for k, (ct, depth, level) in enumerate([(2, 8, 6), (3, 2, 9), (6, 16, 1), (0, 4, 0), (3, 8, 6)]):
        s = ref.random_samples(13, 66, ct, depth, k)
        pal = ref.random_palette(1 << min(depth, 8), k) if ct == 3 else None
        trns = bytes(range(1 << min(depth, 8))) if ct == 3 else bytes(2) if ct == 0 else bytes(6) if ct == 2 else None
        p = tmp_path / f"f{k}.png"
        p.write_bytes(ref.write_png(s, ct, depth, filters=[(y + k) % 5 for y in range(66)], palette=pal, trns=trns,
                                    idat_sizes=[1, 40] if k % 2 else None, level=level))
        files.append(str(p))
    r = subprocess.run([str(fuzz), "900"] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    assert "no sanitizer report" in r.stdout
    counts = [int(w) for w in r.stdout.replace(",", " ").split() if w.isdigit()]
    assert counts[0] > 100 and counts[2] > 1000, r.stdout          # mutations both ways: files that still decode, files refused
