"""Builds and runs tools/deflate_hostsim: deflate.hip's own source compiled for the CPU, a workgroup as 256 threads, under
AddressSanitizer and UndefinedBehaviorSanitizer.  A stand-alone program in a child process, the sanitizers' runtimes linked
into it statically, started in the caller's environment as it is; nothing is loaded into Python."""
from __future__ import annotations

import os
import shutil
import subprocess

import numpy as np

from fennec_amd import FNX_DEFLATE_CHUNK as CH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(build_dir: str) -> str:
    cxx = os.environ.get("CXX") or next((c for c in ("c++", "g++", "clang++", "/opt/rocm/llvm/bin/clang++") if shutil.which(c)), None)
    assert cxx, "no C++ compiler for the host"
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tools", "deflate_hostsim"), f"BUILD={build_dir}", f"CXX={cxx}"], check=True)
    return os.path.join(build_dir, "deflate_hostsim")


def run(exe: str, work: str, x: np.ndarray, row: int = 0, src_offset: int = 0, dst_offset: int = 0):
    """-> (the stream, per chunk the parse's tokens in inflate_probe's form)"""
    names = [os.path.join(work, f) for f in ("in.bin", "out.bin", "tokens.bin")]
    with open(names[0], "wb") as f:
        f.write(x.tobytes())
    r = subprocess.run([exe, names[0], names[1], str(row), str(src_offset), str(dst_offset), names[2]], capture_output=True, text=True)
    assert r.returncode == 0, f"deflate_hostsim: exit {r.returncode}\n{r.stderr[-4000:]}"
    with open(names[1], "rb") as f:
        stream = f.read()
    words = np.fromfile(names[2], dtype="<u4")
    chunks, i, c = [], 0, 0
    while i < len(words):
        k = int(words[i])
        at, tokens = c * CH, []
        for w in words[i + 1:i + 1 + k].tolist():
            if w >> 31:
                tokens.append((((w >> 16) & 0xff) + 3, (w & 0xffff) + 1, at))
                at += tokens[-1][0]
            else:
                tokens.append(w)
                at += 1
        chunks.append(tokens)
        i += 1 + k
        c += 1
    return stream, chunks
