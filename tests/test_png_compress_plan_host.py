"""fnx_png_compress_batch's host plan (fennec_amd/csrc/png_compress_plan.cpp) as a stand-alone program
(tools/png_compress_plan_host.cpp), built from those two files alone under AddressSanitizer and UndefinedBehaviorSanitizer:
about 40 descriptor sets -- every kind and depth; 1 x 1, w = 1, h = 1; streams of exactly 32768 and 32769 bytes; 33 and 70
images; an image whose worst case alone passes the byte cap -- each chunk planned under four classifications.  The program
checks that units tile every image exactly once and in order, that no two regions overlap, that the chunks follow from the
dimensions alone and stay under the cap wherever they hold more than one image.  CPU only; no Python module is loaded into it."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tools/png_compress_plan_host.cpp")
    exe = tmp_path_factory.mktemp("png_compress_plan") / "png_compress_plan_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "fennec_amd", "csrc"), os.path.join(ROOT, "tools", "png_compress_plan_host.cpp"),
                           os.path.join(ROOT, "fennec_amd", "csrc", "png_compress_plan.cpp"), "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def report(program):
    r = subprocess.run([str(program)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout[-4000:] + r.stderr[-4000:]
    return r.stdout


def test_every_set_passes_under_the_sanitizers(report):
    m = re.search(r"^(\d+) sets: ok$", report, re.M)
    assert m and 38 <= int(m.group(1)) <= 44, report[-2000:]
    assert "FAILED" not in report


def chunks_of(report, name):
    m = re.search(r"^%s\s+(\d+) images,\s+(\d+) chunks, largest (\d+) bytes$" % re.escape(name), report, re.M)
    assert m, name
    return int(m.group(1)), int(m.group(2)), int(m.group(3))


def test_chunks_of_at_most_32_images(report):
    assert chunks_of(report, "many 32")[:2] == (32, 1)
    assert chunks_of(report, "many 33")[:2] == (33, 2)
    assert chunks_of(report, "many 64")[:2] == (64, 2)
    assert chunks_of(report, "many 70")[:2] == (70, 3)


def test_photographs_go_a_few_per_chunk(report):
    n, chunks, largest = chunks_of(report, "4K photographs")
    assert n == 9 and 2 <= chunks <= 5 and largest <= 1 << 30            # about 200 MB each: four or five to a chunk


def test_an_image_above_the_cap_is_a_chunk_of_its_own(report):
    # 2 icons | the first large image | an icon | the second | the third | the last icon
    n, chunks, largest = chunks_of(report, "one above the cap")
    assert (n, chunks) == (7, 6) and largest > 1 << 30
    assert chunks_of(report, "the largest image")[:2] == (1, 1)
