#!/usr/bin/env python3
"""What FNX_JPEG_SUBSAMPLING_444 costs and gives, against 4:2:0 on the same ctx: per size (fennec_amd.synth's
photograph-like image at 4K and at 512 x 512) and mode the wall time of fnx_jpeg_encode at quality 75, of a size query on each
route (the packed string, form "jpeg_size" "1") and of fnx_jpeg_compress at target 0.94 -- the median of 7 calls after a warm-up
call, every call waiting for its own result -- with the file's bytes at quality 75, and the quality, bytes, SSIM and steps the
compress call ends at.
python tools/time_jpeg_444.py [--reps N] [W H ...]   -> a markdown table on stdout"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fennec_amd  # noqa: E402
from fennec_amd import synth  # noqa: E402

MODES = ("420", "444")
QUALITY, TARGET = 75, 0.94


def wall_ms(call, reps):
    """median of `reps` calls after one warm-up call (each call ends in its own wait for the result)"""
    call()
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        runs.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(runs)


def main():
    args = sys.argv[1:]
    reps = 7
    if args[:1] == ["--reps"]:
        reps, args = int(args[1]), args[2:]
    sizes = [(int(args[i]), int(args[i + 1])) for i in range(0, len(args) - 1, 2)] or [(3840, 2160), (512, 512)]
    ctx = fennec_amd.Context(0)
    print(f"| size | mode | bytes at q {QUALITY} | encode ms | query ms | 1-wait query ms | compress ms | compress: quality | bytes | SSIM | steps |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for w, h in sizes:
        img = torch.from_numpy(synth.large_photo(w, h, 1)).cuda()
        torch.cuda.synchronize()
        for mode in MODES:
            ctx.set_jpeg_subsampling(mode)
            nbytes = len(ctx.jpeg_encode(img, QUALITY))
            enc = wall_ms(lambda: ctx.jpeg_encode(img, QUALITY), reps)
            query = {}
            for form in ("0", "1"):
                with ctx.forms(jpeg_size=form):
                    assert ctx.jpeg_encoded_size(img, QUALITY) == nbytes
                    query[form] = wall_ms(lambda: ctx.jpeg_encoded_size(img, QUALITY), reps)
            data, q, ssim, steps = ctx.jpeg_compress(img, TARGET)
            comp = wall_ms(lambda: ctx.jpeg_compress(img, TARGET), reps)
            print(f"| {w}x{h} | 4:{mode[1]}:{mode[2]} | {nbytes} | {enc:.3f} | {query['0']:.3f} | {query['1']:.3f} | {comp:.3f} | {q} | {len(data)} | "
                  f"{ssim:.6f} | {steps} |", flush=True)
    ctx.set_jpeg_subsampling("420")


if __name__ == "__main__":
    main()
