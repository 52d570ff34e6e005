"""fnx_png_reduce at 4K, per call: HIP-event times of its kernels (fnx_ctx_profile brackets every launch of the call: colours,
finish, plane, and the gray plane where there is one), the call's span on the stream (events around it) and its wall time --
beside fnx_scan_flags (isGrayscale) on the same image, the same read-once shape, as the yardstick.
    python tools/time_png_reduce.py [W H]"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import fennec_amd
from fennec_amd import synth

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (3840, 2160)
KIND = {fennec_amd.FNX_PNG_PALETTED: "PALETTED", fennec_amd.FNX_PNG_GRAY: "GRAY", fennec_amd.FNX_PNG_NRGBA: "NRGBA"}
rng = np.random.default_rng(1)


def few(n):
    pal = rng.integers(0, 256, size=(n, 4), dtype=np.uint8)
    pal[:, 0] = np.arange(n)                                   # distinct
    if n == 2:                                                 # flat graphics: long runs
        idx = (np.add.outer(np.arange(H) // 64, np.arange(W) // 64) % 2)
    else:
        idx = rng.integers(0, n, size=(H, W))
    return np.ascontiguousarray(pal[idx])


def translucent_gray():
    v = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
    return np.ascontiguousarray(np.stack([v, v, v, rng.integers(0, 256, size=(H, W), dtype=np.uint8)], axis=-1))


CASES = [("2 colours", few(2), 3), ("256 colours", few(256), 3), ("photograph", synth.large_photo(W, H, 0), 3),
         ("translucent gray", translucent_gray(), 4)]
ctx = fennec_amd.Context(0)
print(f"fnx_png_reduce, {W}x{H} device images, us per call (median of 30 after warm-up)")
print(f"{'image':18s} {'kind':9s} {'colours':>8s} {'finish':>8s} {'plane':>8s} {'gray pl.':>8s} | {'stream':>8s} {'wall':>8s} | {'scan_flags stream':>17s} {'wall':>8s}")
for name, img, launches in CASES:
    t = torch.from_numpy(img).cuda()
    plane = torch.empty((H, W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def span(call, reps=30):
        stream, wall = [], []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            t0 = time.perf_counter()
            call()
            wall.append((time.perf_counter() - t0) * 1e6)
            e1.record()
            e1.synchronize()
            stream.append(e0.elapsed_time(e1) * 1e3)
        return float(np.median(stream)), float(np.median(wall))

    for _ in range(10):
        kind = ctx.png_reduce(t, plane=plane)[0]
        ctx.isGrayscale(t)
    s_us, w_us = span(lambda: ctx.png_reduce(t, plane=plane))
    g_us, gw_us = span(lambda: ctx.isGrayscale(t))
    ctx.profile(True)
    ks = []
    for _ in range(30):
        ctx.png_reduce(t, plane=plane)
        ks.append([ctx.kernel_ms() * 1e3 for _ in range(launches)])
    ctx.profile(False)
    k = np.median(np.array(ks), axis=0)
    gp = f"{k[3]:8.2f}" if launches == 4 else f"{'-':>8s}"
    print(f"{name:18s} {KIND[kind]:9s} {k[0]:8.2f} {k[1]:8.2f} {k[2]:8.2f} {gp} | {s_us:8.1f} {w_us:8.1f} | {g_us:17.1f} {gw_us:8.1f}")
