"""image.Decode (+ toNRGBA) and CompressBatch's item body for n JPEG files in host memory on one ctx, two ways each:

  loop    n calls of Context.jpeg_decode(device=True) / Context.jpeg_recompress (fnx_jpeg_decode / fnx_jpeg_recompress): per
          file its own chain of launches and at least two host waits in the decoder
  batch   one call of Context.jpeg_decode_batch(device=True) / Context.jpeg_recompress_batch (fnx_jpeg_decode_batch /
          fnx_jpeg_recompress_batch): one set of the decoder's launches per chunk of <= 32 files, a wait per pair of repair
          rounds and one for the chunk's verdicts

over three file sets -- 3840 x 2160 4:2:0 quality-90 photographs, the same at 1920 x 1080, and a mixed set (thumbnails to
4K, every subsampling, grey, restart intervals) -- at n = 1, 2, 4, 8, 16, 32.  Per row: wall ms and HIP-event ms per file,
each the median over --rounds medians of --reps timed calls (after one warm-up), and the spread (max - min) of those
medians.  Every batch result is checked against the loop's before it is timed.  On a build without the batch entries the
batch columns read "-": the loop columns are the baseline.

    python tools/time_jpeg_decode_batch.py [--reps 20] [--rounds 3] [--ns 1,2,4,8,16,32] [--sets 4k,1080p,mixed] [--no-recompress]
                                             [--recompress-rounds R]
"""
from __future__ import annotations

import argparse
import io
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fennec_amd  # noqa: E402
from fennec_amd import synth  # noqa: E402


def pil(img, grey=False, **kw):
    from PIL import Image
    buf = io.BytesIO()
    if grey:
        Image.fromarray(np.ascontiguousarray(img[..., 1]), "L").save(buf, "JPEG", **kw)
    else:
        Image.fromarray(np.ascontiguousarray(img[..., :3]), "RGB").save(buf, "JPEG", **kw)
    return buf.getvalue()


def file_set(name, n):
    if name in ("4k", "1080p"):
        w, h = (3840, 2160) if name == "4k" else (1920, 1080)
        base = [pil(synth.large_photo(w, h, k), quality=90, subsampling=2) for k in range(min(n, 4))]
    else:
        kinds = [((160, 120), dict(quality=85, subsampling=2)), ((1920, 1080), dict(quality=90, subsampling=2)),
                 ((640, 480), dict(quality=92, subsampling=0)), ((203, 117), dict(quality=80, subsampling=1, optimize=True)),
                 ((3840, 2160), dict(quality=90, subsampling=2)), ((320, 200), dict(quality=88, grey=True)),
                 ((1280, 720), dict(quality=88, subsampling=2, restart_marker_rows=1)), ((800, 600), dict(quality=75, subsampling=2))]
        base = [pil(synth.large_photo(w, h, k), **kw) for k, ((w, h), kw) in enumerate(kinds[:min(n, len(kinds))])]
    return [base[i % len(base)] for i in range(n)]


def timed(fn, n, reps, rounds):
    """-> ((wall ms per file, spread), (event ms per file, spread)): medians of `rounds` medians of `reps` calls"""
    import torch
    fn()
    walls, evs = [], []
    for _ in range(rounds):
        tw, te = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            t0 = time.perf_counter()
            fn()
            e1.record()
            torch.cuda.synchronize()
            tw.append((time.perf_counter() - t0) * 1e3 / n)
            te.append(e0.elapsed_time(e1) / n)
        walls.append(statistics.median(tw))
        evs.append(statistics.median(te))
    return (statistics.median(walls), max(walls) - min(walls)), (statistics.median(evs), max(evs) - min(evs))


def cell(r):
    return "         -      -         -      -" if r is None else f"{r[0][0]:>10.3f} {r[0][1]:>6.3f} {r[1][0]:>9.3f} {r[1][1]:>6.3f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--recompress-rounds", type=int, default=0, help="rounds of the recompress rows (default: --rounds)")
    ap.add_argument("--ns", default="1,2,4,8,16,32")
    ap.add_argument("--sets", default="4k,1080p,mixed")
    ap.add_argument("--target", type=float, default=0.94)
    ap.add_argument("--no-recompress", action="store_true")
    args = ap.parse_args()
    import torch

    ctx = fennec_amd.Context(0)
    have = hasattr(ctx, "jpeg_decode_batch") and hasattr(ctx, "jpeg_recompress_batch")
    ns = [int(v) for v in args.ns.split(",")]
    print(f"# {torch.cuda.get_device_name(0)}; ms per file: median of {args.rounds} ({args.recompress_rounds or args.rounds} for recompress) medians of {args.reps} calls after one warm-up, +- = max - min of"
          f" those medians; batch entries {'present' if have else 'absent (loop columns only)'}")
    print(f"{'op':>10} {'set':>6} {'n':>3} | {'loop wall':>10} {'+-':>6} {'loop gpu':>9} {'+-':>6} | {'batch wall':>10} {'+-':>6} {'batch gpu':>9} {'+-':>6} | {'wall x':>6}")
    for name in args.sets.split(","):
        every = file_set(name, max(ns))
        for op in ("decode",) + (() if args.no_recompress else ("recompress",)):
            for n in ns:
                files = every[:n]
                if op == "decode":
                    def loop():
                        return [ctx.jpeg_decode(f, device=True) for f in files]

                    def batch():
                        return ctx.jpeg_decode_batch(files, device=True)[0]
                    if have:
                        assert all(torch.equal(a, b) for a, b in zip(loop(), batch())), f"{name} n={n}: the batch differs from the loop"
                else:
                    ctx.jpeg_decode(files[0], device=True)           # (the ctx launches on torch's stream from here on: the events see it)

                    def loop():
                        return [ctx.jpeg_recompress(f, args.target) for f in files]

                    def batch():
                        return ctx.jpeg_recompress_batch(files, args.target)
                    if have:
                        assert loop() == batch(), f"{name} n={n}: the batch differs from the loop"
                rounds = args.recompress_rounds if op == "recompress" and args.recompress_rounds > 0 else args.rounds
                rl = timed(loop, n, args.reps, rounds)
                rb = timed(batch, n, args.reps, rounds) if have else None
                ratio = f"{rl[0][0] / rb[0][0]:>5.2f}x" if rb else "     -"
                print(f"{op:>10} {name:>6} {n:>3} | {cell(rl)} | {cell(rb)} | {ratio}", flush=True)
        del every
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
