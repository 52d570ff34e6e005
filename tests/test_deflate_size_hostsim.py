"""The size-only form of deflate.hip's chunk kernels (deflate_chunk_size_kernel, deflate_dense_chunk_size_kernel) and
deflate_size_kernel, on the CPU: tools/deflate_hostsim --size-only, the stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer that the other hostsim tests build, run in a child process.  Per chunk the byte count it reports is
the length of that chunk's bytes in the stream the EMITTING run of the same program writes (read off the stream by
inflate_probe, which knows nothing of the encoder), the total is the stream's length, at both levels; a sanitizer report ends
the program with a non-zero exit status, which fails the test."""
from __future__ import annotations

import os
import subprocess

import numpy as np
import pytest

import deflate_contract as dc
import deflate_hostsim as hs
import inflate_probe as ip
from deflate_contract import CH
from test_deflate_gpu import RATIO_CASES


def noise(n, seed):
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


def smooth_rgb():
    stream = RATIO_CASES["smooth_rgb"]()[0]                           # 512 x 256
    return np.ascontiguousarray(stream).reshape(-1), stream.shape[1]


# name -> (the stream's bytes, the row hint)
STREAMS = {
    "limit15": lambda: (dc.limit15(), 0),
    "limit15_second_chunk": lambda: (dc.behind_noise(dc.limit15()), 0),
    "ties": lambda: (dc.ties(), 0),
    "limit7": lambda: (dc.limit7(), 0),
    "three_bytes_4097": lambda: (dc.three_bytes(4097)[0], 0),
    "forms": lambda: (dc.forms(), 0),                                 # stored, dynamic, fixed side by side
    "constant_chunk": lambda: (np.full(CH, 0x5A, np.uint8), 0),
    "two_chunks_and_a_byte": lambda: (np.resize((np.arange(dc.ROW) * 37 + 11).astype(np.uint8), 2 * CH + 1), dc.ROW),
    "noise_3_chunks": lambda: (noise(3 * CH, 7), 0),                  # stored chunks
    "five_bytes": lambda: (np.array([1, 2, 3, 4, 5], np.uint8), 0),   # the fixed form
    "smooth_rgb": smooth_rgb,
}


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    work = tmp_path_factory.mktemp("deflate_size_hostsim")
    exe = hs.build(str(work / "build"))

    def run(x, row, dense):
        name = os.path.join(str(work), "in.bin")
        with open(name, "wb") as f:
            f.write(x.tobytes())
        level = ["--dense"] if dense else []
        r = subprocess.run([exe, "--size-only"] + level + [name, str(row)], capture_output=True, text=True)
        assert r.returncode == 0, f"deflate_hostsim --size-only: exit {r.returncode}\n{r.stderr[-4000:]}"
        assert r.stderr == "", r.stderr[-4000:]
        lines = [l.split() for l in r.stdout.splitlines()]
        assert lines[-1][0] == "total" and all(l[0] == "chunk" and int(l[1]) == c for c, l in enumerate(lines[:-1]))
        r = subprocess.run([exe] + level + [name, os.path.join(str(work), "out.bin"), str(row)], capture_output=True, text=True)
        assert r.returncode == 0, f"deflate_hostsim: exit {r.returncode}\n{r.stderr[-4000:]}"
        with open(os.path.join(str(work), "out.bin"), "rb") as f:
            stream = f.read()
        return [int(l[2]) for l in lines[:-1]], int(lines[-1][1]), stream
    return run


def chunk_lengths(stream: bytes, n: int):
    """the bytes of every chunk in an emitted stream: its block and, behind all but the last, the empty stored block"""
    p = ip.probe(stream)
    nch = -(-n // CH)
    assert len(p.blocks) == 2 * nch - 1
    out = []
    for c in range(nch):
        first = p.blocks[2 * c]
        end = p.blocks[2 * c + 1].bit_end if c < nch - 1 else (first.bit_end + 7) // 8 * 8
        assert first.bit_start % 8 == 0 and end % 8 == 0
        out.append((end - first.bit_start) // 8)
    return out, [b.btype for b in p.blocks[::2]]


@pytest.mark.parametrize("dense", [False, True], ids=["fast", "dense"])
@pytest.mark.parametrize("name", sorted(STREAMS))
def test_size_only_counts_are_the_emitting_runs(sim, name, dense):
    x, row = STREAMS[name]()
    counts, total, stream = sim(x, row, dense)
    want, btypes = chunk_lengths(stream, len(x))
    print(f"{name} {'dense' if dense else 'fast'}: chunks {want} forms {btypes} stream {len(stream)}")
    assert counts == want
    assert total == len(stream) == 2 + sum(want) + 4
    # the inputs reach the forms they are here for
    if name == "forms":
        assert btypes == [ip.STORED, ip.DYNAMIC, ip.FIXED]
    if name == "noise_3_chunks":
        assert btypes == [ip.STORED] * 3
    if name == "five_bytes":
        assert btypes == [ip.FIXED]
