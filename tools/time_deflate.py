"""fnx_png_encode at 4K against the host route, per image and per deflate level (Context.set_deflate_level: a row for "fast", a
row for "dense"): the HIP-event time of each launch (fnx_ctx_profile: the row stage, deflate_chunk_kernel or
deflate_dense_chunk_kernel, deflate_gather_kernel), the call's wall time from a resident image to the PNG file in host memory,
and beside it png_filter to host memory followed by zlib.compress at levels 1, 6 and 9 on one thread -- with every file's size.
    python tools/time_deflate.py [W H [REPS]]"""
import os
import sys
import time
import zlib

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import fennec_amd
from fennec_amd import FNX_PNG_NRGBA, FNX_PNG_PALETTED

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (3840, 2160)
rng = np.random.default_rng(1)
y, x = np.mgrid[0:H, 0:W]
smooth = np.stack([x // 8 + y // 16, x // 16 + y // 8, (x + y) // 24, 0 * x + 255], axis=-1)
smooth = np.ascontiguousarray(((smooth + rng.integers(0, 2, size=smooth.shape)) & 255).astype(np.uint8))
smooth[..., 3] = 255
pal256 = np.ascontiguousarray(((x // 5 + (y // 3) * 7) % 256).astype(np.uint8))
flat2 = np.ascontiguousarray((((x // 64) + (y // 64)) % 2).astype(np.uint8))
noise = rng.integers(0, 256, size=(H, W, 4), dtype=np.uint8)
noise[..., 3] = 255
palette = rng.integers(0, 256, size=(256, 4), dtype=np.uint8)
palette[:, 3] = 255
CASES = [("smooth RGB", smooth, FNX_PNG_NRGBA, 0, 1, None), ("paletted, 256 colours", pal256, FNX_PNG_PALETTED, 256, -1, palette),
         ("flat, 2 colours", flat2, FNX_PNG_PALETTED, 2, -1, palette[:2]), ("noise RGB", noise, FNX_PNG_NRGBA, 0, 1, None)]
ctx = fennec_amd.Context(0)
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 7
print(f"fnx_png_encode against png_filter + host zlib, {W}x{H}, device sources; times in ms (median of {REPS} after warm-up; zlib: one run)")
print(f"{'image':22s} {'level':5s} {'stream MB':>9s} | {'rows':>6s} {'chunk':>8s} {'gather':>7s} {'wall':>8s} {'file KB':>9s} | "
      f"{'filter->host':>12s} | {'zlib 1':>8s} {'file KB':>9s} | {'zlib 6':>8s} {'file KB':>9s} | {'zlib 9':>8s} {'file KB':>9s}")
for name, src, kind, ncolors, opaque, pal in CASES:
    t = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    rows = []
    for level in ("fast", "dense"):
        ctx.set_deflate_level(level)
        for _ in range(2):
            file = ctx.png_encode(t, kind, ncolors, opaque, pal)
        wall = []
        for _ in range(REPS):
            t0 = time.perf_counter()
            ctx.png_encode(t, kind, ncolors, opaque, pal)
            wall.append((time.perf_counter() - t0) * 1e3)
        ctx.profile(True)
        ks = []
        for _ in range(REPS):
            ctx.png_encode(t, kind, ncolors, opaque, pal)
            ks.append([ctx.kernel_ms() for _ in range(3)])
        ctx.profile(False)
        rows.append((level, np.median(np.array(ks), axis=0), np.median(wall), len(file)))
    ctx.set_deflate_level("fast")
    host = np.empty(H * (1 + 4 * W), dtype=np.uint8)
    ctx.png_filter(t, kind, ncolors, opaque, host)
    fw = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        stream, ct, bd = ctx.png_filter(t, kind, ncolors, opaque, host)
        fw.append((time.perf_counter() - t0) * 1e3)
    raw = stream.tobytes()
    cols = []
    for level in (1, 6, 9):
        t0 = time.perf_counter()
        z = zlib.compress(raw, level)
        ms = (time.perf_counter() - t0) * 1e3
        # the file around the stream: signature, IHDR, IDAT's and IEND's frames (57 bytes), PLTE for the paletted kinds
        cols.append(f"{ms:8.1f} {(len(z) + 57 + (0 if pal is None else 12 + 3 * ncolors)) / 1e3:9.1f}")
    for level, k, wall, size in rows:
        print(f"{name:22s} {level:5s} {len(raw) / 1e6:9.1f} | {k[0]:6.3f} {k[1]:8.3f} {k[2]:7.3f} {wall:8.2f} {size / 1e3:9.1f} | "
              f"{np.median(fw):12.2f} | " + " | ".join(cols), flush=True)
