"""Runs tools/deflate_hostsim with the dense level's switches (--dense, --table, --batch --dense); the program is built by
deflate_hostsim.build as for the fast level's tests: a stand-alone program under AddressSanitizer and
UndefinedBehaviorSanitizer in a child process, nothing loaded into Python."""
from __future__ import annotations

import os
import subprocess

import numpy as np

import deflate_hostsim as hs
from fennec_amd import FNX_DEFLATE_CHUNK as CH

build = hs.build


def _tokens(words: np.ndarray) -> list:
    """per chunk the tokens in inflate_probe's form: a literal's byte, (length, distance, stream offset)"""
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
    return chunks


def run(exe: str, work: str, x: np.ndarray, row: int = 0, src_offset: int = 0, dst_offset: int = 0, table: bool = False):
    """-> (the dense stream, per chunk the lazy walk's tokens, per chunk the (L, D) table as a list of (L, D) or None)"""
    names = [os.path.join(work, f) for f in ("dense_in.bin", "dense_out.bin", "dense_tokens.bin", "dense_table.bin")]
    with open(names[0], "wb") as f:
        f.write(x.tobytes())
    cmd = [exe, "--dense"] + (["--table", names[3]] if table else [])
    r = subprocess.run(cmd + [names[0], names[1], str(row), str(src_offset), str(dst_offset), names[2]], capture_output=True, text=True)
    assert r.returncode == 0, f"deflate_hostsim --dense: exit {r.returncode}\n{r.stderr[-4000:]}"
    with open(names[1], "rb") as f:
        stream = f.read()
    tokens = _tokens(np.fromfile(names[2], dtype="<u4"))
    tables = None
    if table:
        words = np.fromfile(names[3], dtype="<u4")
        tables, i = [], 0
        while i < len(words):
            k = int(words[i])
            t = words[i + 1:i + 1 + k]
            tables.append([(int(w) >> 16, (int(w) & 0xffff) + 1 if w else 0) for w in t.tolist()])
            i += 1 + k
    return stream, tokens, tables


def run_fast(exe: str, work: str, x: np.ndarray, row: int = 0) -> bytes:
    return hs.run(exe, work, x, row)[0]


def run_batch(exe: str, work: str, inputs, row: int = 0) -> list:
    names = []
    for i, x in enumerate(inputs):
        names.append(os.path.join(work, f"dense_in{i}.bin"))
        with open(names[-1], "wb") as f:
            f.write(x.tobytes())
    out = os.path.join(work, "dense_batch")
    r = subprocess.run([exe, "--batch", "--dense", str(row), out] + names, capture_output=True, text=True)
    assert r.returncode == 0, f"deflate_hostsim --batch --dense: exit {r.returncode}\n{r.stderr[-4000:]}"
    return [open(f"{out}.{i}", "rb").read() for i in range(len(inputs))]
