"""fnx_png_decode_batch's host side -- png_parse.cpp's png_prepare_many: chunk walk, inflate, row plan and palette table of a
list of files on several threads -- as a stand-alone program (tools/png_batch_host.cpp), built once under AddressSanitizer +
UndefinedBehaviorSanitizer and once under ThreadSanitizer.  About 40 small files, damaged, interlaced, empty and non-PNG ones
among them, with workers = 1, 3 and 8: every item's status, refusal text, stream bytes, unit table and palette table equal
the workers = 1 result, and no sanitizer reports.  CPU only; the Python module is not involved."""
from __future__ import annotations

import os
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import png_decode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path_factory, name, sanitize):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tools/png_batch_host.cpp")
    exe = tmp_path_factory.mktemp(name) / "png_batch_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + sanitize +
                          ["-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "fennec_amd", "csrc"),
                           os.path.join(ROOT, "tools", "png_batch_host.cpp"), os.path.join(ROOT, "fennec_amd", "csrc", "png_parse.cpp"),
                           "-o", str(exe)])
    return exe


@pytest.fixture(scope="module")
def asan(tmp_path_factory):
    return build(tmp_path_factory, "png_batch_asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


@pytest.fixture(scope="module")
def tsan(tmp_path_factory):
    return build(tmp_path_factory, "png_batch_tsan", ["-fsanitize=thread"])


def file_set():
    """name -> bytes: every colour type / depth pair, two more per bpp group with many units, and the refused kinds"""
    out = {}
    for k, (ct, depth) in enumerate(ref.PAIRS):
        w, h = 3 + 2 * k, 5 + 9 * k
        s = ref.random_samples(w, h, ct, depth, k)
        pal = ref.random_palette(max(1, (1 << min(depth, 8)) - 1), k) if ct == 3 else None
        trns = bytes(range(3)) if ct == 3 else bytes(2) if ct == 0 else bytes(6) if ct == 2 else None
        filters = np.random.default_rng(k).integers(0, 5, size=h).tolist()
        out[f"pair_{ct}_{depth}"] = ref.write_png(s, ct, depth, filters=filters, palette=pal, trns=trns, idat_sizes=[1, 50] if k % 2 else None,
                                                  level=(0, 1, 6, 9)[k % 4])
    for k, (ct, depth, h) in enumerate([(2, 8, 400), (6, 8, 333), (0, 8, 257), (3, 8, 200), (6, 16, 130), (4, 16, 70)]):
        s = ref.random_samples(9, h, ct, depth, 50 + k)
        pal = ref.random_palette(256, k) if ct == 3 else None
        out[f"units_{ct}_{depth}"] = ref.write_png(s, ct, depth, filters=[(y // 64) % 2 if y % 64 == 0 else 2 + y % 3 for y in range(h)], palette=pal)
    s = ref.random_samples(9, 5, 2, 8, 1)
    good = ref.write_png(s, 2, 8, filters=[0, 1, 2, 3, 4])
    flipped = bytearray(good)
    flipped[len(good) - 20] ^= 0x40
    out.update({
        "truncated": good[:-30],
        "half": good[:len(good) // 2],
        "bad_crc": bytes(flipped),
        "filter_5": ref.write_png(s, 2, 8, filters=[0, 1, 5, 3, 4]),
        "adam7": ref.write_png(s, 2, 8, interlace=1),
        "adam7_paletted": ref.write_png(ref.random_samples(4, 4, 3, 2, 2), 3, 2, palette=ref.random_palette(4, 1), interlace=1),
        "too_wide": ref.SIG + ref.ihdr(65536, 1, 1, 0) + ref.chunk(b"IDAT", zlib.compress(b"\0")) + ref.chunk(b"IEND", b""),
        "jpeg": b"\xff\xd8\xff\xe0\x00\x10JFIF\x00" + bytes(range(200)),
        "text": b"not a PNG file at all, only some text that is longer than a signature and an IHDR chunk would be\n" * 2,
        "empty": b"",
        "signature_only": ref.SIG,
        "short_stream": ref.SIG + ref.ihdr(9, 5, 8, 2) + ref.chunk(b"IDAT", zlib.compress(b"\0" * (5 * 28 - 1))) + ref.chunk(b"IEND", b""),
        "long_stream": ref.SIG + ref.ihdr(9, 5, 8, 2) + ref.chunk(b"IDAT", zlib.compress(b"\0" * (5 * 28 + 1))) + ref.chunk(b"IEND", b""),
        "promises_14_gb": ref.SIG + ref.ihdr(60000, 60000, 8, 6) + ref.chunk(b"IDAT", zlib.compress(b"\0" * 1000)) + ref.chunk(b"IEND", b""),
        "no_plte": ref.SIG + ref.ihdr(4, 2, 8, 3) + ref.chunk(b"IDAT", zlib.compress(bytes(10))) + ref.chunk(b"IEND", b""),
        "bad_adler": ref.SIG + ref.ihdr(9, 5, 8, 2) + ref.chunk(b"IDAT", zlib.compress(b"\0" * 140)[:-1] + b"\x7f") + ref.chunk(b"IEND", b""),
        "good_again": good,
    })
    return out


def run(exe, tmp_path):
    files = file_set()
    assert 38 <= len(files) <= 44
    paths = []
    for name, data in files.items():
        p = tmp_path / name
        p.write_bytes(data)
        paths.append(str(p))
    r = subprocess.run([str(exe)] + paths, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    assert "no sanitizer report" in r.stdout
    # 15 pairs + 6 with many units + the good file again are prepared; the two Adam7 files and the wide one are unsupported
    assert f"{len(files)} files: 22 prepared, 3 unsupported, {len(files) - 25} invalid" in r.stdout, r.stdout


def test_the_file_set_is_what_it_says():
    files = file_set()
    for name, data in files.items():
        if name.startswith(("pair_", "units_", "good")):
            ref.decode(data)
        elif name in ("adam7", "adam7_paletted", "too_wide"):
            with pytest.raises(ref.Unsupported):
                ref.parse(data)
        else:
            with pytest.raises(ref.Damaged):
                ref.decode(data)


def test_workers_agree_under_asan_and_ubsan(asan, tmp_path):
    run(asan, tmp_path)


def test_workers_agree_under_tsan(tsan, tmp_path):
    run(tsan, tmp_path)
