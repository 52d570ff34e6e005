"""compressJPEGOptimal (compress.go:21-87) of n device-resident images of one geometry on one ctx, two ways:

  loop    n calls of Context.jpeg_compress (fnx_jpeg_compress): per item, one host wait per search step, two for the file's
          bit and 0xff totals and one for its bytes
  batch   one call of Context.jpeg_compress_batch (fnx_jpeg_compress_batch): per chunk of the batch, one wait per search step
          for all items still searching, two for the totals of all files and one for their bytes

per row: wall ms per image (median of --reps after a warm-up), the speed-up, and the host waits per batch of n.  Every
batch result is checked against the loop's (file bytes, quality, ssim, steps) before it is timed.

    python tools/time_jpeg_compress_batch.py [--reps 3] [--target 0.94]
"""
from __future__ import annotations

import argparse
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fennec_amd  # noqa: E402
from fennec_amd import synth  # noqa: E402

SIZES = [(512, 512), (1920, 1080), (3840, 2160)]
NS = [1, 8, 32]
SCRATCH = 1 << 30          # api.cpp: JPEG_BATCH_SCRATCH


def al256(v):
    return (v + 255) & ~255


def batch_chunk(ctx, w, h):
    """items per chunk of fnx_jpeg_compress_batch (api.cpp's rule restated: per-item scratch against JPEG_BATCH_SCRATCH)"""
    _, pw, ph = ctx.ssimFastDims(w, h)
    ds = (pw, ph) != (w, h)
    mx, my = (w + 15) // 16, (h + 15) // 16
    pb = al256(256 * mx * my + 2 * 64 * mx * my + 16)
    rb = al256(pw * ph * 4 + 16)
    db = al256(w * h * 4 + 16)
    fused = ds and w >= pw and h >= ph
    per_item = 2 * pb + rb + (rb if ds else 0) + (0 if fused else db) + mx * my * 6 * (128 + 208 + 4 + 8) + 256
    return max(1, SCRATCH // per_item)


def contents(kind, w, h, n):
    if kind == "photo":
        base = [synth.large_photo(w, h, k) for k in range(min(n, 4))]
    else:
        ramp = synth.make_test_image(w, h)
        base = [ramp, np.ascontiguousarray(ramp[::-1]), np.ascontiguousarray(ramp[:, ::-1]), np.ascontiguousarray(ramp[::-1, ::-1])][:min(n, 4)]
    return [base[i % len(base)] for i in range(n)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--target", type=float, default=0.94)
    args = ap.parse_args()
    import torch

    ctx = fennec_amd.Context(0)
    print(f"# {torch.cuda.get_device_name(0)}; target SSIM {args.target}; ms per image = median of {args.reps} after one warm-up")
    print(f"{'size':>10} {'content':>7} {'n':>3} {'loop ms':>8} {'batch ms':>9} {'speedup':>8} {'waits loop':>10} {'waits batch':>11} {'chunks':>6}"
          f" {'steps':>7}")
    for w, h in SIZES:
        for kind in ("photo", "ramp"):
            for n in NS:
                imgs = [torch.from_numpy(im).cuda() for im in contents(kind, w, h, n)]
                torch.cuda.synchronize()
                want = [ctx.jpeg_compress(im, args.target) for im in imgs]
                got = ctx.jpeg_compress_batch(imgs, args.target)
                assert got == want, f"{w}x{h} {kind} n={n}: the batch differs from the loop"

                def loop():
                    return [ctx.jpeg_compress(im, args.target) for im in imgs]

                def batch():
                    return ctx.jpeg_compress_batch(imgs, args.target)

                t = {}
                for name, fn in (("loop", loop), ("batch", batch)):
                    fn()
                    ts = []
                    for _ in range(args.reps):
                        t0 = time.perf_counter()
                        fn()
                        ts.append(time.perf_counter() - t0)
                    t[name] = statistics.median(ts) * 1e3 / n
                steps = [r[3] for r in want]
                chunk = batch_chunk(ctx, w, h)
                nch = math.ceil(n / chunk)
                waits_loop = sum(s + 3 for s in steps)
                waits_batch = sum(max(steps[c:c + chunk]) + 3 for c in range(0, n, chunk))
                print(f"{w:>5}x{h:<4} {kind:>7} {n:>3} {t['loop']:>8.2f} {t['batch']:>9.2f} {t['loop'] / t['batch']:>7.2f}x"
                      f" {waits_loop:>10} {waits_batch:>11} {nch:>6} {min(steps):>3}-{max(steps):<3}", flush=True)
                del imgs
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
