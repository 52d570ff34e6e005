"""fnx_png_filter at 4K, per call, for the four row forms (RGB, RGBA, gray, paletted): the HIP-event time of its kernel
(fnx_ctx_profile brackets the launch; with opaque = -1 the alpha scan in front of it too), the call's span on the stream
(events around it) and its wall time -- beside fnx_scan_flags (isGrayscale) on the same NRGBA image, the read-once yardstick
of DESIGN.md 5.4.
    python tools/time_png_filter.py [W H]"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import fennec_amd
from fennec_amd import FNX_PNG_GRAY, FNX_PNG_NRGBA, FNX_PNG_PALETTED, synth

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (3840, 2160)
rng = np.random.default_rng(1)
photo = synth.large_photo(W, H, 0)
photo[..., 3] = 255
translucent = photo.copy()
translucent[..., 3] = rng.integers(0, 256, size=(H, W), dtype=np.uint8)
gray = np.ascontiguousarray(photo[..., 1])
CASES = [("RGB (opaque stated)", photo, FNX_PNG_NRGBA, 0, 1, 1), ("RGB (opaque decided)", photo, FNX_PNG_NRGBA, 0, -1, 2),
         ("RGBA", translucent, FNX_PNG_NRGBA, 0, 0, 1), ("gray", gray, FNX_PNG_GRAY, 0, -1, 1),
         ("paletted, 256 colours", gray, FNX_PNG_PALETTED, 256, -1, 1), ("paletted, 16 colours", gray >> 4, FNX_PNG_PALETTED, 16, -1, 1),
         ("paletted, 2 colours", gray >> 7, FNX_PNG_PALETTED, 2, -1, 1)]
ctx = fennec_amd.Context(0)
image = torch.from_numpy(photo).cuda()
print(f"fnx_png_filter, {W}x{H} device sources, device stream, us per call (median of 30 after warm-up)")
print(f"{'rows':24s} {'MB in':>7s} {'MB out':>7s} {'alpha':>8s} {'kernel':>8s} | {'stream':>8s} {'wall':>8s} | {'scan_flags stream':>17s} {'wall':>8s}")


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


for name, src, kind, ncolors, opaque, launches in CASES:
    t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
    out = torch.empty(H * (1 + 4 * W), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for _ in range(10):
        stream = ctx.png_filter(t, kind, ncolors, opaque, out)[0]
        ctx.isGrayscale(image)
    s_us, w_us = span(lambda: ctx.png_filter(t, kind, ncolors, opaque, out))
    g_us, gw_us = span(lambda: ctx.isGrayscale(image))
    ctx.profile(True)
    ks = []
    for _ in range(30):
        ctx.png_filter(t, kind, ncolors, opaque, out)
        ks.append([ctx.kernel_ms() * 1e3 for _ in range(launches)])
    ctx.profile(False)
    k = np.median(np.array(ks), axis=0)
    alpha = f"{k[0]:8.2f}" if launches == 2 else f"{'-':>8s}"
    print(f"{name:24s} {src.nbytes / 1e6:7.1f} {stream.numel() / 1e6:7.1f} {alpha} {k[-1]:8.2f} | {s_us:8.1f} {w_us:8.1f} | {g_us:17.1f} {gw_us:8.1f}")
