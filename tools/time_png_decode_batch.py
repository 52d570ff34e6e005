"""image.Decode + toNRGBA for n PNG files in host memory on one ctx, two ways:

  loop    n calls of Context.png_decode(space="device") (fnx_png_decode): per file its inflate on the calling thread, its own
          upload and its own two launches -- a single-chain file is ONE workgroup of png_unfilter_kernel
  batch   one call of Context.png_decode_batch(device=True, workers=W) (fnx_png_decode_batch) at W = 1, 4, 8, 16: the inflates
          of a chunk on W host threads, then the chunk's chains in one set of launches

over three file sets written here -- "rgb": 3840 x 2160 truecolour files whose rows are all of type Up, one chain of 2160 rows
each; "pal": 3840 x 2160 8-bit paletted files, rows of type None; "mixed": thumbnails to 4K, grey, truecolour, alpha, 16 bit,
paletted, None / Sub / Up rows -- at n = 1, 2, 4, 8, 16, 32.  Per row, in ms per file: the wall time of each way (median of
--rounds medians of --reps calls after one warm-up, and the spread max - min of those medians); "gpu": the library's own HIP
event time of the batched kernels of one call (fnx_ctx_profile), summed over its launches; "units": the workgroups of
png_unfilter_batch_kernel the files make, i.e. how many compute units the chains can occupy at once.  Every batch result is
checked against the loop's before it is timed.

Each row is measured by a child process of its own under --limit seconds; the first row that fails or runs out of time ends
the run, nothing is retried.

    python tools/time_png_decode_batch.py [--reps 3] [--rounds 2] [--ns 1,2,4,8,16,32] [--sets rgb,pal,mixed] [--limit 240]
"""
from __future__ import annotations

import argparse
import os
import statistics
import struct
import subprocess
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WORKERS = (1, 4, 8, 16)
CHANNELS = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}
UNIT_MIN_ROWS = 64                 # png_row_plan: a unit ends at the first None / Sub row at which it holds this many rows


def chunk(tag, body):
    return struct.pack(">I", len(body)) + tag + body + struct.pack(">I", zlib.crc32(tag + body))


def write_png(raw, w, color_type, depth, filters, palette=None):
    """raw: (h, rowbytes) uint8, the unfiltered rows; filters: one of 0 (None), 1 (Sub), 2 (Up) per row -- in numpy"""
    h, n = raw.shape
    bpp = max(1, CHANNELS[color_type] * depth // 8)
    f = np.asarray(filters)
    left = np.zeros_like(raw)
    left[:, bpp:] = raw[:, :-bpp]
    up = np.zeros_like(raw)
    up[1:] = raw[:-1]
    body = np.where((f == 1)[:, None], raw - left, np.where((f == 2)[:, None], raw - up, raw)).astype(np.uint8)
    stream = np.concatenate([f.astype(np.uint8)[:, None], body], axis=1).tobytes()
    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, 0))
    if palette is not None:
        out += chunk(b"PLTE", palette.tobytes())
    return out + chunk(b"IDAT", zlib.compress(stream, 1)) + chunk(b"IEND", b"")


def units_of(filters):
    count, start = 1, 0
    for y, t in enumerate(filters):
        if t <= 1 and y - start >= UNIT_MIN_ROWS:
            count += 1
            start = y
    return count


def make(kind, w, h, seed):
    """-> (file bytes, units)"""
    from fennec_amd import synth
    photo = synth.large_photo(w, h, seed)
    rng = np.random.default_rng(seed)
    if kind == "rgb":
        raw, ct, depth, filters, pal = photo[..., :3].reshape(h, 3 * w), 2, 8, [2] * h, None
    elif kind == "pal":
        raw, ct, depth, filters = (photo[..., 1] // 2 + photo[..., 0] // 2), 3, 8, [0] * h
        pal = rng.integers(0, 256, size=(256, 3), dtype=np.uint8)
    elif kind == "rgba":
        raw, ct, depth, filters, pal = photo.reshape(h, 4 * w), 6, 8, [1 if y % 97 == 0 else 2 for y in range(h)], None
    elif kind == "grey":
        raw, ct, depth, filters, pal = photo[..., 1], 0, 8, [(0, 1, 2)[y % 3] for y in range(h)], None
    else:                          # "rgb16": the high and the low byte of every sample
        raw = np.repeat(photo[..., :3].reshape(h, 3 * w), 2, axis=1)
        ct, depth, filters, pal = 2, 16, [2] * h, None
    return write_png(np.ascontiguousarray(raw, dtype=np.uint8), w, ct, depth, filters, pal), units_of(filters)


def file_set(name, n):
    if name in ("rgb", "pal"):
        base = [make(name, 3840, 2160, k) for k in range(min(n, 2))]
    else:
        kinds = [("rgb", 160, 120), ("rgba", 1920, 1080), ("grey", 640, 480), ("pal", 203, 117), ("rgb", 3840, 2160), ("rgb16", 320, 200),
                 ("pal", 1280, 720), ("rgba", 800, 600)]
        base = [make(k, w, h, i) for i, (k, w, h) in enumerate(kinds[:min(n, len(kinds))])]
    picked = [base[i % len(base)] for i in range(n)]
    return [p[0] for p in picked], sum(p[1] for p in picked)


def timed(fn, n, reps, rounds):
    import torch
    fn()
    meds = []
    for _ in range(rounds):
        t = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) * 1e3 / n)
        meds.append(statistics.median(t))
    return statistics.median(meds), max(meds) - min(meds)


def row(name, n, reps, rounds):
    import torch

    import fennec_amd
    ctx = fennec_amd.Context(0)
    files, units = file_set(name, n)

    def loop():
        return [ctx.png_decode(f, "device") for f in files]
    cells = [timed(loop, n, reps, rounds)]
    want = loop()
    gpu = None
    for workers in WORKERS:
        def batch():
            return ctx.png_decode_batch(files, device=True, workers=workers)
        images, statuses = batch()
        assert all(s == fennec_amd.FNX_OK for s in statuses) and all(torch.equal(a, b) for a, b in zip(want, images)), \
            f"{name} n={n} workers={workers}: the batch differs from the loop"
        del images
        cells.append(timed(batch, n, reps, rounds))
        if gpu is None:                              # the batched kernels' own time: the same launches whatever `workers`
            ctx.profile(fennec_amd.PROF_MAIN)
            batch()
            gpu = 0.0
            while True:
                try:
                    gpu += ctx.kernel_ms()
                except fennec_amd.FennecError:
                    break
            ctx.profile(0)
    text = " | ".join(f"{m:>9.3f} {s:>7.3f}" for m, s in cells)
    print(f"{name:>6} {n:>3} | {text} | {gpu / n:>8.3f} {units:>6} | {cells[0][0] / cells[1][0]:>5.2f}x {cells[0][0] / cells[3][0]:>5.2f}x", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--ns", default="1,2,4,8,16,32")
    ap.add_argument("--sets", default="rgb,pal,mixed")
    ap.add_argument("--limit", type=int, default=240, help="seconds a row's process may take")
    ap.add_argument("--row", nargs=2, metavar=("SET", "N"), help="measure this row in this process (what the parent starts)")
    args = ap.parse_args()
    if args.row:
        row(args.row[0], int(args.row[1]), args.reps, args.rounds)
        return 0
    print(f"# ms per file: median of {args.rounds} medians of {args.reps} calls after one warm-up, +- = max - min of those medians; gpu: the"
          f" batched kernels' HIP-event ms per file; units: workgroups of png_unfilter_batch_kernel; x: loop / batch at workers 1 and 8")
    head = " | ".join(f"{c:>9} {'+-':>7}" for c in ("loop",) + tuple(f"batch w{w}" for w in WORKERS))
    print(f"{'set':>6} {'n':>3} | {head} | {'gpu':>8} {'units':>6} | {'x w1':>6} {'x w8':>6}", flush=True)
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
