"""compressPNG for n resident images on one ctx, two ways:

  loop    n calls of Context.compress_png(img, device_deflate=True) (fnx_png_reduce + fnx_png_encode): per image its own
          launches and four to six host waits
  batch   one call of Context.png_compress_batch(imgs) (fnx_png_compress_batch): per chunk of up to 32 images one set of
          launches and three host waits

over three image sets made here from seeds -- "icons": 64 x 64, 16 colours (4-bit paletted files); "screens": 512 x 512
screenshots of 40 colours in flat rectangles (8-bit paletted); "photos": 3840 x 2160 photographs (RGB rows) -- at n = 1, 8, 32,
128.  Per row, in ms per image: the wall time of each way around work that ends in a synchronise (the two ways alternate inside
every round; median of --rounds medians of --reps calls after a warm-up of both, and the spread max - min of those medians);
"gpu": the library's own HIP-event time of the launches of each way (fnx_ctx_profile), summed -- the batch's taken chunk by
chunk, as the library keeps the events of its last 32 launches.  Every batch result
is checked against the loop's, byte for byte, before it is timed.  The loop is the existing single route of the same build.

Each row is measured by a child process of its own under --limit seconds; the first row that fails or runs out of time ends
the run, nothing is retried.

    python tools/time_png_compress_batch.py [--reps 5] [--rounds 3] [--ns 1,8,32,128] [--sets icons,screens,photos] [--limit 300]
"""
from __future__ import annotations

import argparse
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def icon(seed):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (16, 4), dtype=np.uint8)
    pal[:, 3] = 255
    idx = np.zeros((64, 64), np.int64)
    for _ in range(24):                                    # overlapping discs and bars: runs of one colour, as icons have
        x, y, r, c = rng.integers(0, 64), rng.integers(0, 64), rng.integers(3, 20), rng.integers(0, 16)
        yy, xx = np.ogrid[:64, :64]
        idx[(xx - x) ** 2 + (yy - y) ** 2 < r * r] = c
    return pal[idx]


def screen(seed):
    rng = np.random.default_rng(seed)
    pal = rng.integers(0, 256, (40, 4), dtype=np.uint8)
    pal[:, 3] = 255
    idx = np.zeros((512, 512), np.int64)
    for _ in range(300):                                   # windows, buttons, lines of text
        x, y = rng.integers(0, 512, 2)
        w, h = rng.integers(2, 200), rng.integers(1, 60)
        idx[y:y + h, x:x + w] = rng.integers(0, 40)
    return pal[idx]


def image_set(name, n):
    from fennec_amd import synth
    if name == "icons":
        return [icon(k) for k in range(n)]
    if name == "screens":
        base = [screen(k) for k in range(min(n, 16))]
    else:
        base = [synth.large_photo(3840, 2160, k) for k in range(min(n, 2))]
    return [base[i % len(base)] for i in range(n)]


def timed_pair(fa, fb, n, reps, rounds):
    """the two ways alternating: -> ((median, spread) of a, (median, spread) of b), ms per image"""
    import torch

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n
    fa()
    fb()
    meds = ([], [])
    for _ in range(rounds):
        ta, tb = [], []
        for _ in range(reps):
            ta.append(once(fa))
            tb.append(once(fb))
        meds[0].append(statistics.median(ta))
        meds[1].append(statistics.median(tb))
    return tuple((statistics.median(m), max(m) - min(m)) for m in meds)


def event_ms(ctx, calls):
    """the HIP-event time of the launches of every call of a list, read call by call (the library keeps the last 32 launches)"""
    import fennec_amd
    ctx.profile(fennec_amd.PROF_MAIN)
    total = 0.0
    for fn in calls:
        fn()
        while True:
            try:
                total += ctx.kernel_ms()
            except fennec_amd.FennecError:
                break
    ctx.profile(0)
    return total


def row(name, n, reps, rounds):
    import torch

    import fennec_amd
    ctx = fennec_amd.Context(0)
    hosts = image_set(name, n)
    devs = {}
    imgs = []
    for a in hosts:                                        # a repeated image is one device tensor
        if id(a) not in devs:
            devs[id(a)] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
        imgs.append(devs[id(a)])
    torch.cuda.synchronize()

    def loop():
        return [ctx.compress_png(t, device_deflate=True) for t in imgs]

    def batch():
        return ctx.png_compress_batch(imgs)[0]
    want = loop()
    assert batch() == want, f"{name} n={n}: the batch differs from the loop"
    (lm, ls), (bm, bs) = timed_pair(loop, batch, n, reps, rounds)
    group = 4 if name == "photos" else 32                # images of one chunk: its launches fit the library's 32 event pairs
    gl = event_ms(ctx, [lambda t=t: ctx.compress_png(t, device_deflate=True) for t in imgs]) / n
    gb = event_ms(ctx, [lambda k=k: ctx.png_compress_batch(imgs[k:k + group]) for k in range(0, n, group)]) / n
    kb = sum(len(f) for f in want) / n / 1024
    print(f"{name:>8} {n:>4} | {lm:>9.3f} {ls:>7.3f} | {bm:>9.3f} {bs:>7.3f} | {gl:>8.3f} {gb:>8.3f} | {kb:>9.1f} | {lm / bm:>5.2f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ns", default="1,8,32,128")
    ap.add_argument("--sets", default="icons,screens,photos")
    ap.add_argument("--limit", type=int, default=300, help="seconds a row's process may take")
    ap.add_argument("--row", nargs=2, metavar=("SET", "N"), help="measure this row in this process (what the parent starts)")
    args = ap.parse_args()
    if args.row:
        row(args.row[0], int(args.row[1]), args.reps, args.rounds)
        return 0
    print(f"# ms per image: median of {args.rounds} medians of {args.reps} calls after a warm-up, the two ways alternating; +- = max - min of those"
          f" medians; gpu: HIP-event ms per image of one call's launches; KiB: mean file size; x: loop / batch (wall)")
    print(f"{'set':>8} {'n':>4} | {'loop':>9} {'+-':>7} | {'batch':>9} {'+-':>7} | {'gpu loop':>8} {'gpu bat.':>8} | {'KiB/file':>9} | {'x':>6}", flush=True)
    for name in args.sets.split(","):
        for n in (int(v) for v in args.ns.split(",")):
            cmd = [sys.executable, os.path.abspath(__file__), "--row", name, str(n), "--reps", str(args.reps), "--rounds", str(args.rounds)]
            try:
                rc = subprocess.run(cmd, timeout=args.limit).returncode
            except subprocess.TimeoutExpired:
                print(f"{name} n={n}: no result within {args.limit} s; the run ends here", flush=True)
                return 1
            if rc != 0:
                print(f"{name} n={n}: exit status {rc}; the run ends here", flush=True)
                return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
