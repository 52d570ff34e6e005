"""fnx_png_decode of the same pixels stored non-interlaced and Adam7-interlaced (fnx_ctx_set_png_adam7), at 4K: a
photograph-like RGB8 image under two filter plans and a paletted image.  Per file: the whole call from the file's bytes in
host memory to the NRGBA image resident on the device (wall clock), the HIP-event time of its two launches (fnx_ctx_profile:
png_unfilter_kernel + png_expand_kernel, or png_unfilter_batch_kernel over the seven passes + png_expand_adam7_kernel), and
fnx_inflate of its IDAT stream on its own (ms; the launches in us).  Every figure is the median of REPS calls after a warm-up,
with the spread (min .. max) behind it.  No target is set: the question is whether the two Adam7 launches cost about what the
two non-interlaced ones do, and whether inflate dominates both.
    python tools/time_png_adam7.py [W H]"""
import os
import sys
import time
import zlib

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np

import fennec_amd
import png_adam7_ref as a7
import png_decode_ref as ref
import png_filter_ref as enc

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (3840, 2160)
REPS = 25
rgb = enc.smooth_rgba(W, H, 1, opaque=True)[..., :3].astype(np.int64)
yy, xx = np.mgrid[0:H, 0:W]
pal_idx = ((xx // 5 + (yy // 3) * 7) % 256).astype(np.int64)[..., None]
palette = ref.random_palette(256, 1)
ROWS = a7.passes(W, H, 2, 8)[1]


def plan(kind, n):
    return [4] * n if kind == "paeth" else [(1, 2, 3, 4)[y & 3] for y in range(n)] if kind == "mixed" else [0] * n


CASES = [
    ("RGB8, all Paeth", lambda: ref.write_png(rgb, 2, 8, filters=plan("paeth", H)),
     lambda: a7.write_adam7(rgb, 2, 8, filters=[plan("paeth", n) for n in ROWS])),
    ("RGB8, Sub/Up/Average/Paeth", lambda: ref.write_png(rgb, 2, 8, filters=plan("mixed", H)),
     lambda: a7.write_adam7(rgb, 2, 8, filters=[plan("mixed", n) for n in ROWS])),
    ("paletted 8 bit, None", lambda: ref.write_png(pal_idx, 3, 8, palette=palette),
     lambda: a7.write_adam7(pal_idx, 3, 8, palette=palette)),
]


def stats(v, digits=2):
    v = np.asarray(v, dtype=np.float64)
    return f"{np.median(v):8.{digits}f} ({v.min():.{digits}f} .. {v.max():.{digits}f})"


def wall(f):
    out = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


plain_ctx = fennec_amd.Context(0)
adam7_ctx = fennec_amd.Context(0)
adam7_ctx.set_png_adam7(True)
print(f"fnx_png_decode, {W}x{H}, the file in host memory -> NRGBA on the device; ms (the two launches: us), median of {REPS} calls (min .. max)")
print(f"{'file':28s} {'stored':>9s} {'file MB':>8s} {'stream MB':>9s} | {'whole call':>26s} | {'inflate':>26s} | {'unfilter us':>26s} | {'expand us':>26s}")
for name, make_plain, make_adam7 in CASES:
    images = []
    for stored, make, ctx, route in (("plain", make_plain, plain_ctx, "png_unfilter_kernel, png_expand_kernel"),
                                     ("Adam7", make_adam7, adam7_ctx, "png_unfilter_batch_kernel, png_expand_adam7_kernel")):
        data = make()
        z = ref.parse(a7.deinterlaced_header(data) if stored == "Adam7" else data)["z"]
        raw_len = len(zlib.decompress(z))
        for _ in range(3):
            img = ctx.png_decode(data, "device")
        ctx.sync()
        assert ctx.last_kernel() == route
        images.append(img.cpu().numpy())

        def whole():
            ctx.png_decode(data, "device")
            ctx.sync()
        w = wall(whole)
        ctx.profile(True)
        ks = []
        for _ in range(REPS):
            ctx.png_decode(data, "device")
            ks.append([ctx.kernel_ms(), ctx.kernel_ms()])
        ctx.profile(False)
        ks = np.array(ks) * 1e3
        infl = wall(lambda: fennec_amd.inflate(z, cap=raw_len))
        print(f"{name:28s} {stored:>9s} {len(data) / 1e6:8.1f} {raw_len / 1e6:9.1f} | {stats(w):>26s} | {stats(infl):>26s} | {stats(ks[:, 0], 0):>26s} | "
              f"{stats(ks[:, 1], 1):>26s}", flush=True)
    assert np.array_equal(images[0], images[1]), "the two files hold the same pixels"
