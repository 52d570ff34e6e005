"""The PNG host code that states a step once for several entry points, as a stand-alone program (tools/png_frame_host.cpp)
under AddressSanitizer + UndefinedBehaviorSanitizer: the file frame around a zlib stream (png_frame.cpp: fnx_png_encode's and
the compress batch's files) against png_decode_ref's SIG / ihdr / chunk, byte for byte, in a buffer of exactly file_bytes(zsize)
bytes; and an Adam7 file's pass descriptors (png_parse.cpp: png_adam7_passes, fnx_png_decode's and the decode batch's) against
png_adam7_ref's pass geometry.  CPU only; the Python module is not involved."""
from __future__ import annotations

import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import png_adam7_ref as a7
import png_decode_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fennec_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build tools/png_frame_host.cpp")
    out = tmp_path_factory.mktemp("png_frame_host") / "png_frame_host"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + CSRC, os.path.join(ROOT, "tools", "png_frame_host.cpp")] +
                          [os.path.join(CSRC, name) for name in ("png_frame.cpp", "png_parse.cpp", "png_compress_plan.cpp")] + ["-o", str(out)])
    return out


def depth_of(ncolors):
    return 1 if ncolors <= 2 else 2 if ncolors <= 4 else 4 if ncolors <= 16 else 8


def palette_of(ncolors, seed, last_alpha):
    """(ncolors, 4) r g b a: every alpha 255 but a few below index last_alpha and the one at last_alpha (None: all 255)"""
    rng = np.random.default_rng(seed)
    pal = np.concatenate([ref.random_palette(ncolors, seed), np.full((ncolors, 1), 255, np.uint8)], axis=1)
    if last_alpha is not None:
        pal[:last_alpha, 3] = np.where(rng.integers(0, 2, size=last_alpha) == 0, 255, rng.integers(0, 255, size=last_alpha))
        pal[last_alpha, 3] = rng.integers(0, 255)
    return pal


def frame_cases():
    """(name, w, h, colour type, depth, palette (n, 4) or None): sizes whose rows make a stream of a few hundred bytes"""
    out = []
    for ct, (w, h) in ((0, (17, 17)), (2, (10, 10)), (6, (9, 8))):
        out.append((f"type_{ct}", w, h, ct, 8, None))
    for k, ncolors in enumerate((1, 2, 16, 256)):
        d = depth_of(ncolors)
        w, h = {1: (61, 37), 4: (33, 17), 8: (17, 17)}[d]
        out.append((f"paletted_{ncolors}", w, h, 3, d, palette_of(ncolors, k, ncolors // 2)))
    for name, last in (("no_trns", None), ("trns_first", 0), ("trns_middle", 7), ("trns_last", 15)):
        out.append((name, 33, 17, 3, 4, palette_of(16, 10, last)))
    out.append(("trns_last_of_256", 17, 17, 3, 8, palette_of(256, 11, 255)))
    return out


def expected_file(w, h, ct, depth, pal, z):
    out = [ref.SIG, ref.ihdr(w, h, depth, ct)]
    if ct == 3:
        out.append(ref.chunk(b"PLTE", pal[:, :3].tobytes()))
        translucent = np.nonzero(pal[:, 3] != 255)[0]
        if len(translucent):
            out.append(ref.chunk(b"tRNS", pal[:translucent[-1] + 1, 3].tobytes()))
    return b"".join(out + [ref.chunk(b"IDAT", z), ref.chunk(b"IEND", b"")])


def test_the_frame_is_the_reference_writers_byte_for_byte(exe, tmp_path):
    records, want, real = [], [], []
    for k, (name, w, h, ct, depth, pal) in enumerate(frame_cases()):
        samples = ref.random_samples(w, h, ct, depth, k, palette_len=None if pal is None else len(pal))
        filters = np.random.default_rng(k).integers(0, 5, size=h).tolist()
        stream = ref.filter_stream(ref.pack_rows(samples, ct, depth), ref.bpp_of(ct, depth), filters).tobytes()
        for z in (b"\x5a", zlib.compress(stream, 0)):      # (stored blocks: the size is the rows' own)
            assert len(z) == 1 or 200 <= len(z) <= 999, (name, len(z))
            n = 0 if pal is None else len(pal)
            records.append(struct.pack("<6I", w, h, ct, depth, n, len(z)) + (b"" if pal is None else pal.tobytes()) + z)
            want.append((name, expected_file(w, h, ct, depth, pal, z)))
            real.append(None if len(z) == 1 else ref.write_png(samples, ct, depth, filters=filters, palette=None if pal is None else pal[:, :3],
                                                              trns=pal[:, 3].tobytes() if pal is not None and (pal[:, 3] != 255).any() else None))
    (tmp_path / "cases").write_bytes(b"".join(records))
    r = subprocess.run([str(exe), "frame", str(tmp_path / "cases"), str(tmp_path / "out")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr           # the canary behind every file is intact
    assert f"{len(want)} frames; no sanitizer report" in r.stdout
    got = (tmp_path / "out").read_bytes()
    at = 0
    for (name, file), other in zip(want, real):
        (n,) = struct.unpack_from("<I", got, at)
        assert got[at + 4:at + 4 + n] == file, name
        at += 4 + n
        if other is not None:          # a real stream: the file reads back, as the pixels an independently written file holds
            assert np.array_equal(ref.decode(file), ref.decode(other)), name
    assert at == len(got)


ADAM7 = [(1, 1, 2, 8), (3, 2, 2, 8), (9, 5, 2, 8), (9, 5, 0, 1)]


@pytest.mark.parametrize("w,h,ct,depth", ADAM7)
def test_adam7_pass_descriptors(exe, tmp_path, w, h, ct, depth):
    path = tmp_path / "adam7.png"
    path.write_bytes(a7.write_adam7(ref.random_samples(w, h, ct, depth, 3), ct, depth, filters=5))
    r = subprocess.run([str(exe), "adam7", str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert r.returncode == 0 and not r.stderr, r.stdout + r.stderr           # first index 0 and 5: the same but for the offset
    lines = r.stdout.splitlines()
    head = dict(zip(lines[0].split()[0::2], map(int, lines[0].split()[1::2])))
    got = [dict(zip(ln.split()[0::2], map(int, ln.split()[1::2]))) for ln in lines[1:] if ln.startswith("pass ")]
    pw, ph, rb, total = a7.passes(w, h, ct, depth)
    present = [p for p in range(7) if ph[p]]
    assert [g["pass"] for g in got] == present and head["count"] == len(present) and head["stream_bytes"] == total
    if (w, h) == (1, 1):
        assert present == [0]
    if (w, h) == (3, 2):
        assert len(present) < 7
    off, end = 0, 0
    for k, (g, p) in enumerate(zip(got, present)):
        assert (g["off"], g["spitch"], g["rowbytes"], g["ph"]) == (off, 1 + rb[p], rb[p], ph[p])
        assert g["npix"] == rb[p] // ref.bpp_of(ct, depth)
        off += ph[p] * (1 + rb[p])
        assert (g["slot"], g["slot5"]) == (k, 5 + k)                          # the present passes in order from the first index
        assert g["rows"] % 16 == 0 and g["ppitch"] % 16 == 0 and g["ppitch"] >= rb[p] and g["ppitch"] - rb[p] < 16
        assert g["rows"] >= end                                               # disjoint: a plane starts behind the one before it
        end = g["rows"] + g["ppitch"] * ph[p]
    assert end <= head["planes_bytes"]
