"""fennec_CompressBatchTargetSize over 64 JPEG files of 1920 x 1080 (quality 92 files of synthetic photographs), each at most
--target bytes: items per second of the pool at 1, 4 and 16 workers, median of --reps batches after one warm-up batch per
worker count (the pool keeps its contexts, so the warm-up pays for their scratch).

    python tools/time_batch_target_size.py [--reps 3] [--files 64] [--target 150000]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fennec_amd  # noqa: E402
from fennec_amd import batch, synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--files", type=int, default=64)
    ap.add_argument("--target", type=int, default=150000)
    args = ap.parse_args()
    import torch
    ctx = fennec_amd.Context(0)
    distinct = [ctx.jpeg_encode(synth.large_photo(1920, 1080, k), 92) for k in range(8)]
    files = [distinct[i % len(distinct)] for i in range(args.files)]
    ctx.jpeg_encoded_size(synth.large_photo(64, 64, 0), 50)
    print(f"# {torch.cuda.get_device_name(0)}; {args.files} files of 1920 x 1080 ({sum(map(len, files)) // len(files)} bytes on average), "
          f"target {args.target} bytes, median of {args.reps}; size queries: {ctx.last_kernel(16)}")
    print(f"{'workers':>7} {'s / batch':>10} {'items / s':>10} {'failed':>6} {'queries / item':>14} {'winners':>16}")
    for workers in (1, 4, 16):
        batch.compress_batch_target_size_native(files, args.target, workers=workers)
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            results, out, summ = batch.compress_batch_target_size_native(files, args.target, workers=workers)
            ts.append(time.perf_counter() - t0)
        t = statistics.median(ts)
        wins = sorted({r.winner for r in results if r.Err is None})
        assert all(len(o) <= args.target for r, o in zip(results, out) if r.Err is None and r.winner != 3)
        print(f"{workers:7d} {t:10.3f} {len(files) / t:10.1f} {summ.Failed:6d} {sum(r.steps for r in results) / len(results):14.1f} {wins!s:>16}")
    fennec_amd.load_library().fennec_pool_release()


if __name__ == "__main__":
    main()
