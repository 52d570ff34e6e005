#!/usr/bin/env python3
"""What FNX_JPEG_HUFFMAN_OPTIMIZED saves and costs, against the standard mode of the same build: per size
(512 x 512, 1080p, 4K) and quality (30, 75, 90) of fennec_amd.synth content the file's bytes under both modes, the wall time
of a file and of a size query under both modes and both size routes (the packed string, form "jpeg_size" "1"), and the quality
fnx_jpeg_size_search reaches for a target set to the standard file's size at quality 75.
python tools/time_jpeg_huffman.py [--reps N] [W H ...]   -> a markdown table on stdout"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fennec_amd  # noqa: E402
from fennec_amd import synth  # noqa: E402

MODES = ("standard", "optimized")


def wall_ms(ctx, call, reps):
    """median of three runs of `reps` back-to-back calls (every call waits for its own result)"""
    call()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            call()
        runs.append((time.perf_counter() - t0) / reps * 1e3)
    return sorted(runs)[1]


def main():
    args = sys.argv[1:]
    reps = 30
    if args[:1] == ["--reps"]:
        reps, args = int(args[1]), args[2:]
    sizes = [(int(args[i]), int(args[i + 1])) for i in range(0, len(args) - 1, 2)] or [(512, 512), (1920, 1080), (3840, 2160)]
    ctx = fennec_amd.Context(0)
    print("| size | q | bytes std | bytes opt | saved | file ms std | file ms opt | query ms std | query ms opt | 1-wait query ms std | 1-wait query ms opt |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    reached = []
    for w, h in sizes:
        img = torch.from_numpy(synth.large_photo(w, h, 1)).cuda()
        torch.cuda.synchronize()
        for q in (30, 75, 90):
            row = {}
            for mode in MODES:
                ctx.set_jpeg_huffman(mode)
                row[mode, "bytes"] = len(ctx.jpeg_encode(img, q))
                row[mode, "file"] = wall_ms(ctx, lambda: ctx.jpeg_encode(img, q), reps)
                for form in ("0", "1"):
                    with ctx.forms(jpeg_size=form):
                        assert ctx.jpeg_encoded_size(img, q) == row[mode, "bytes"]
                        row[mode, "query" + form] = wall_ms(ctx, lambda: ctx.jpeg_encoded_size(img, q), reps)
            s, o = row["standard", "bytes"], row["optimized", "bytes"]
            print(f"| {w}x{h} | {q} | {s} | {o} | {100.0 * (s - o) / s:.1f} % | " + " | ".join(
                f"{row[m, k]:.3f}" for k in ("file", "query0", "query1") for m in MODES) + " |", flush=True)
            if q == 75:
                got = {}
                for mode in MODES:
                    ctx.set_jpeg_huffman(mode)
                    r = ctx.jpeg_size_search(img, s, skip_ssim=True)
                    got[mode] = (r[1], len(r[0]), r[3]) if r else None
                reached.append((w, h, s, got))
    ctx.set_jpeg_huffman("standard")
    print()
    print("| size | target (std bytes at q 75) | std: quality, bytes, steps | opt: quality, bytes, steps |")
    print("|---|---|---|---|")
    for w, h, s, got in reached:
        print(f"| {w}x{h} | {s} | {got['standard']} | {got['optimized']} |")


if __name__ == "__main__":
    main()
