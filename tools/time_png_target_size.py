"""The PNG size query and the PNG target-size legs at 4K, per deflate level (Context.set_deflate_level):
 1. per image -- a photograph, a smooth RGB image, a 256-colour paletted image, all resident -- the wall time of
    fnx_png_encoded_size (the row stage, the deflate kernels' size-only forms, 8 bytes back) beside fnx_png_encode's (the file in
    host memory) on the same image, with the HIP-event time of each launch of the size query (fnx_ctx_profile);
 2. the whole fnx_png_target_size per leg on the photograph, with its `steps`: quantize at a target every level fits, at one
    only the 16-colour level fits; the scale leg; the fallback.
Times are host clocks around calls that end in a device wait: the median of REPS after warm-up, with the smallest and largest.
    python tools/time_png_target_size.py [W H [REPS]] [--encode-only]
--encode-only: part 1's fnx_png_encode column alone (what a build without the size query can run, for comparing two builds)."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import numpy as np
import torch

import fennec_amd
from fennec_amd import FNX_PNG_NRGBA, FNX_PNG_PALETTED, synth

args = [a for a in sys.argv[1:] if not a.startswith("--")]
ENCODE_ONLY = "--encode-only" in sys.argv
W, H = (int(args[0]), int(args[1])) if len(args) > 1 else (3840, 2160)
REPS = int(args[2]) if len(args) > 2 else 7
rng = np.random.default_rng(1)
y, x = np.mgrid[0:H, 0:W]
smooth = np.stack([x // 8 + y // 16, x // 16 + y // 8, (x + y) // 24, 0 * x + 255], axis=-1)      # tools/time_deflate.py's images
smooth = np.ascontiguousarray(((smooth + rng.integers(0, 2, size=smooth.shape)) & 255).astype(np.uint8))
smooth[..., 3] = 255
pal256 = np.ascontiguousarray(((x // 5 + (y // 3) * 7) % 256).astype(np.uint8))
palette = rng.integers(0, 256, size=(256, 4), dtype=np.uint8)
palette[:, 3] = 255
photo = synth.large_photo(W, H, 7)
CASES = [("photograph", photo, FNX_PNG_NRGBA, 0, 1, None), ("smooth RGB", smooth, FNX_PNG_NRGBA, 0, 1, None),
         ("paletted, 256 colours", pal256, FNX_PNG_PALETTED, 256, -1, palette)]
ctx = fennec_amd.Context(0)


def timed(call):
    for _ in range(2):
        out = call()
    ms = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, float(np.median(ms)), min(ms), max(ms)


print(f"PNG size query against the file, {W}x{H}, device sources; wall ms: median of {REPS} after warm-up (min .. max)")
print(f"{'image':22s} {'level':5s} | {'size query':>28s} | {'rows':>6s} {'chunk':>8s} {'sum':>6s} | {'fnx_png_encode':>28s} | {'file bytes':>10s}")
for name, src, kind, ncolors, opaque, pal in CASES:
    t = torch.from_numpy(src).cuda()
    torch.cuda.synchronize()
    for level in ("fast", "dense"):
        ctx.set_deflate_level(level)
        file, em, elo, ehi = timed(lambda: ctx.png_encode(t, kind, ncolors, opaque, pal))
        enc = f"{em:9.3f} ({elo:7.3f} .. {ehi:7.3f})"
        if ENCODE_ONLY:
            print(f"{name:22s} {level:5s} | {'':28s} | {'':6s} {'':8s} {'':6s} | {enc:>28s} | {len(file):10d}", flush=True)
            continue
        size, sm, slo, shi = timed(lambda: ctx.png_encoded_size(t, kind, ncolors, opaque, pal))
        assert size == len(file), (size, len(file))
        ctx.profile(True)
        ks = []
        for _ in range(REPS):
            ctx.png_encoded_size(t, kind, ncolors, opaque, pal)
            ks.append([ctx.kernel_ms() for _ in range(3)])
        ctx.profile(False)
        k = np.median(np.array(ks), axis=0)
        print(f"{name:22s} {level:5s} | {sm:9.3f} ({slo:7.3f} .. {shi:7.3f}) | {k[0]:6.3f} {k[1]:8.3f} {k[2]:6.3f} | {enc:>28s} | {size:10d}", flush=True)
if ENCODE_ONLY:
    sys.exit(0)

print()
print(f"fnx_png_target_size on the photograph, {W}x{H}, device source; wall ms as above")
print(f"{'leg':34s} {'level':5s} | {'wall':>28s} | {'steps':>5s} {'winner bytes':>12s} {'final':>11s}")
t = torch.from_numpy(photo).cuda()
torch.cuda.synchronize()
for level in ("fast", "dense"):
    ctx.set_deflate_level(level)
    sizes = []
    for n in (256, 16):
        pal, idx, _, _ = ctx.quantize(t, n, want_quantized=False, want_ssim=False)
        sizes.append(ctx.png_encoded_size(idx, FNX_PNG_PALETTED, len(pal), -1, pal))
    legs = [("quantize, every level fits", 1 << 40, fennec_amd.FNX_TS_QUANTIZE), ("quantize, only 16 colours fit", sizes[1], fennec_amd.FNX_TS_QUANTIZE),
            ("scale, target = s16 / 4", sizes[1] // 4, fennec_amd.FNX_TS_SCALE_PNG), ("fallback", 1, fennec_amd.FNX_TS_FALLBACK_PNG)]
    for leg, target, bits in legs:
        got, m, lo, hi = timed(lambda: ctx.png_target_size(t, target, bits))
        c = got["candidates"][got["winner"]]
        print(f"{leg:34s} {level:5s} | {m:9.3f} ({lo:7.3f} .. {hi:7.3f}) | {c['steps']:5d} {c['nbytes']:12d} {c['final_w']:5d}x{c['final_h']:<5d}", flush=True)
