"""deflate.hip's batched kernels on the CPU (tools/deflate_hostsim --batch: deflate_chunk_batch_kernel and
deflate_gather_batch_kernel compiled against the stand-in headers, a workgroup as 256 threads, under AddressSanitizer and
UndefinedBehaviorSanitizer, a stand-alone program in a child process): several inputs in one pair of launches, every stream
equal to the single-input run of the same bytes -- which test_deflate_hostsim.py holds to the stream's contract -- and the
streams back to back at their true sizes.  Inputs of one chunk, of exactly one chunk, of a chunk and a byte and of four chunks
sit side by side, so a unit's stream, its last-of-stream flag and the per-stream prefix are exercised."""
from __future__ import annotations

import os
import subprocess
import zlib

import numpy as np
import pytest

import deflate_hostsim as hs
from deflate_contract import CH
from test_deflate_gpu import CONTENTS


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    work = tmp_path_factory.mktemp("deflate_batch_hostsim")
    return hs.build(str(work / "build")), str(work)


def run_batch(sim, inputs, row):
    exe, work = sim
    names = []
    for i, x in enumerate(inputs):
        names.append(os.path.join(work, f"in{i}.bin"))
        with open(names[-1], "wb") as f:
            f.write(x.tobytes())
    out = os.path.join(work, "batch")
    r = subprocess.run([exe, "--batch", str(row), out] + names, capture_output=True, text=True)
    assert r.returncode == 0, f"deflate_hostsim --batch: exit {r.returncode}\n{r.stderr[-4000:]}"
    return [open(f"{out}.{i}", "rb").read() for i in range(len(inputs))]


def inputs_for(row):
    gen = CONTENTS["pair_and_noise"][0]
    smooth = CONTENTS[sorted(CONTENTS)[0]][0]
    return [gen(1), gen(259), smooth(CH), gen(CH + 1), smooth(3 * CH + 777), gen(row or 5), np.full(CH + 128, 0xFF, np.uint8), smooth(4097)]


@pytest.mark.parametrize("row", [0, 128])
def test_every_stream_equals_the_single_run(sim, row):
    exe, work = sim
    inputs = inputs_for(row)
    streams = run_batch(sim, inputs, row)
    for i, x in enumerate(inputs):
        want = hs.run(exe, work, x, row)[0]
        assert streams[i] == want, f"input {i} of {x.size} bytes"
        assert zlib.decompress(streams[i]) == x.tobytes()


def test_a_stream_does_not_depend_on_its_place(sim):
    inputs = inputs_for(0)
    a = run_batch(sim, inputs, 0)
    b = run_batch(sim, inputs[::-1], 0)
    assert a == b[::-1]
    assert run_batch(sim, inputs[3:4], 0) == a[3:4]                       # a batch of one
