"""The byte strings and the case list the CRC-32 tests share (tests/test_crc32_hostsim.py: crc32_piece.inc as a CPU program;
tests/test_crc32_gpu.py: Context.crc32): lengths around a lane's run and a workgroup's piece, every source alignment, three
seeds, three kinds of content, one flipped bit at the first and last byte of a run and of a piece, and splits of one string."""
from __future__ import annotations

import functools
import zlib

import numpy as np

RUN, PIECE = 64, 16384                       # FNX_CRC_RUN, FNX_CRC_PIECE (test_png_crc_abi.py holds them against the header)
LENGTHS = list(range(10)) + [RUN - 1, RUN, RUN + 1, 2 * RUN + 3, PIECE - 1, PIECE, PIECE + 1, PIECE + RUN + 1, 3 * PIECE + 5]
LONGEST = 3 * PIECE + 5
SEEDS = (0, 0xffffffff, 0x9d3c5a17)          # the last one: drawn once, kept
KINDS = ("zero", "ff", "random")
# (position, bit): the first and the last byte of a run inside a piece, of a piece inside the string, and of the string
FLIPS = ((5 * RUN, 0x01), (6 * RUN - 1, 0x80), (PIECE, 0x01), (2 * PIECE - 1, 0x80), (0, 0x01), (PIECE - 1, 0x80))
SPLITS = (1, RUN, PIECE)


@functools.lru_cache(maxsize=None)
def blobs() -> dict:
    """name -> bytes: the three kinds at LONGEST bytes, each with one bit flipped at each of FLIPS, and each one's part behind
    each of SPLITS"""
    out = {"zero": bytes(LONGEST), "ff": b"\xff" * LONGEST,
           "random": np.random.default_rng(20240607).integers(0, 256, LONGEST, dtype=np.uint8).tobytes()}
    for kind in KINDS:
        for pos, bit in FLIPS:
            b = bytearray(out[kind])
            b[pos] ^= bit
            out[f"{kind}_flip{pos}"] = bytes(b)
        for split in SPLITS:
            out[f"{kind}_behind{split}"] = out[kind][split:]
    return out


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    """(name, source offset, length, seed, blob, expected CRC): the CRC of the blob's first `length` bytes continued from `seed`"""
    b = blobs()
    out = []
    for kind in KINDS:
        for length in LENGTHS:
            for offset in range(8):
                for seed in SEEDS:
                    out.append((f"{kind}_n{length}_o{offset}_s{seed:x}", offset, length, seed, kind))
        for pos, _ in FLIPS:
            for length in (PIECE, LONGEST):
                if pos < length:
                    for offset in (0, 3):
                        out.append((f"{kind}_flip{pos}_n{length}_o{offset}", offset, length, 0, f"{kind}_flip{pos}"))
        for split in SPLITS:                 # crc(A B) = crc(B, seed = crc(A))
            for offset in (0, 5):
                out.append((f"{kind}_split{split}_o{offset}", offset, LONGEST - split, zlib.crc32(b[kind][:split]), f"{kind}_behind{split}"))
    full = []
    for name, offset, length, seed, key in out:
        want = zlib.crc32(b[key][:length], seed)
        if "_split" in name:
            assert want == zlib.crc32(b[key.split("_")[0]])
        full.append((name, offset, length, seed, key, want))
    return tuple(full)
