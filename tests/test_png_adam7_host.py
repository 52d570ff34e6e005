"""The host side of an Adam7 decode -- png_parse.cpp's parse with the accept flag, png_stream_size, png_inflate and the
per-pass row plan -- as a stand-alone program (tools/png_adam7_host.cpp) built under AddressSanitizer +
UndefinedBehaviorSanitizer and run directly.  About 30 small files; per file the program's status, stream size and units per
pass are compared with what png_adam7_ref.py says.  CPU only; the Python module is not involved."""
from __future__ import annotations

import os
import shutil
import subprocess
import zlib

import pytest

import png_adam7_ref as a7
import png_decode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, INVALID, UNSUPPORTED = 0, -1, -5                # include/fennec_hip.h
UNIT_MIN_ROWS = 64                                   # png_row_plan: a unit ends at the first None / Sub row at which it holds this many rows


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tools/png_adam7_host.cpp")
    out = tmp_path_factory.mktemp("png_adam7_asan") / "png_adam7_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + os.path.join(ROOT, "fennec_amd", "csrc"),
                           os.path.join(ROOT, "tools", "png_adam7_host.cpp"), os.path.join(ROOT, "fennec_amd", "csrc", "png_parse.cpp"),
                           "-o", str(out)])
    return out


def units_of(types):
    """png_row_plan of one pass, restated: the number of units of rows with these filter types"""
    if not types:
        return 0
    n, start = 1, 0
    for y, t in enumerate(types):
        if t <= 1 and y - start >= UNIT_MIN_ROWS:
            n += 1
            start = y
    return n


def expected(data):
    """(status, stream bytes, units per pass) of an Adam7 file with the accept flag on, from the helper alone"""
    try:
        types = a7.pass_filter_types(data)
    except ref.Damaged:
        return (INVALID, 0, [0] * 7)
    if any(t > 4 for p in types for t in p):
        return (INVALID, 0, [0] * 7)
    f = ref.parse(a7.deinterlaced_header(data))
    return (OK, a7.passes(f["w"], f["h"], f["color_type"], f["depth"])[3], [units_of(p) for p in types])


def file_set():
    """name -> (bytes, accept): good files of every bpp and of the small sizes, a file with several units per pass, and the
    refused kinds"""
    out = {}
    sizes = [(1, 1), (2, 3), (5, 3), (3, 5), (8, 8), (9, 17), (33, 10), (4, 1), (1, 4), (4, 4), (2, 2), (1, 9), (9, 1), (3, 3), (16, 16)]
    for k, (ct, depth) in enumerate(ref.PAIRS):
        w, h = sizes[k]
        s = ref.random_samples(w, h, ct, depth, k)
        pal = ref.random_palette(1 << depth, k) if ct == 3 else None
        out[f"pair_{ct}_{depth}_{w}x{h}"] = (a7.write_adam7(s, ct, depth, filters=k, palette=pal, idat_sizes=[1, 50] if k % 2 else None,
                                                            level=(0, 1, 6, 9)[k % 4]), True)
    assert {ref.bpp_of(ct, d) for ct, d in ref.PAIRS} == {1, 2, 3, 4, 6, 8}
    # 5 x 600: the passes have 75, 75, 75, 150, 150, 300 and 300 rows: None / Sub rows every 70 rows cut them into several units
    h = 600
    fl = [[(0 if (y // 70) % 2 else 1) if y % 70 == 0 else 2 + y % 3 for y in range(n)] for n in (75, 75, 75, 150, 150, 300, 300)]
    out["units"] = (a7.write_adam7(ref.random_samples(5, h, 6, 8, 77), 6, 8, filters=fl), True)
    s = ref.random_samples(9, 5, 2, 8, 1)
    stream = a7.adam7_stream(s, 2, 8, 5)
    assert len(stream) == 146
    good = a7.file_around(stream, 9, 5, 2, 8)
    p1 = bytearray(stream)
    p1[0] = 5                                            # pass 1 is one row of 1 + 6 bytes
    p7 = bytearray(stream)
    p7[146 - 2 * 28] = 5                                 # pass 7: two rows of 1 + 27 bytes, the stream's last
    z = zlib.compress(stream)
    out.update({
        "good": (good, True),
        "one_byte_short": (a7.file_around(stream[:-1], 9, 5, 2, 8), True),
        "one_byte_long": (a7.file_around(stream + b"\0", 9, 5, 2, 8), True),
        "filter_5_in_pass_1": (a7.file_around(bytes(p1), 9, 5, 2, 8), True),
        "filter_5_in_pass_7": (a7.file_around(bytes(p7), 9, 5, 2, 8), True),
        "mislabelled": (ref.write_png(s, 2, 8, interlace=1), True),
        "truncated_zlib": (a7.file_around(b"", 9, 5, 2, 8, z=z[:len(z) // 2]), True),
        "bad_adler": (a7.file_around(b"", 9, 5, 2, 8, z=z[:-1] + bytes([z[-1] ^ 1])), True),
        "promises_too_much": (a7.file_around(b"\0" * 1000, 60000, 60000, 6, 8), True),
        "no_plte": (a7.file_around(a7.adam7_stream(ref.random_samples(4, 4, 3, 2, 2), 3, 2), 4, 4, 3, 2), True),
        "accept_off": (good, False),
        "accept_off_paletted": (a7.write_adam7(ref.random_samples(4, 4, 3, 2, 2), 3, 2, palette=ref.random_palette(4, 1)), False),
    })
    return out


def test_the_file_set_is_what_it_says():
    files = file_set()
    assert 26 <= len(files) <= 34
    for name, (data, accept) in files.items():
        status, total, units = expected(data)
        if name.startswith(("pair_", "units", "good")):
            assert status == OK and a7.decode_adam7(data).shape[2] == 4, name
        else:
            assert status == (OK if name.startswith("accept_off") else INVALID), name
    assert expected(files["units"][0])[2] == [2, 2, 2, 3, 3, 5, 5]
    assert a7.pass_filter_types(files["filter_5_in_pass_1"][0])[0] == [5]
    assert a7.pass_filter_types(files["filter_5_in_pass_7"][0])[6][0] == 5
    absent = sum(1 for name, (data, _) in files.items() if name.startswith("pair_") for u in expected(data)[2] if u == 0)
    assert absent >= 20                                   # the small sizes leave passes out


def test_host_side_under_asan_and_ubsan(exe, tmp_path):
    files = file_set()
    on = [n for n, (_, accept) in files.items() if accept]
    off = [n for n, (_, accept) in files.items() if not accept]
    for name, (data, _) in files.items():
        (tmp_path / name).write_bytes(data)
    r = subprocess.run([str(exe)] + [str(tmp_path / n) for n in on] + ["--off"] + [str(tmp_path / n) for n in off],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[-1] == f"png_adam7_host: {len(files)} files; no sanitizer report"
    assert len(lines) == len(files) + 1
    for name, line in zip(on + off, lines):
        got = [int(v) for v in line.split()]
        if name in off:
            assert got == [UNSUPPORTED, 0] + [0] * 7, name
        else:
            status, total, units = expected(files[name][0])
            assert got == [status, total] + units, name
