"""fnx_png_decode at 4K, stage by stage, per kind of file: the host's share (the chunk walk, and fnx_inflate of the IDAT stream,
each timed on its own), the upload (a pinned copy of the inflated stream's size, timed on its own with HIP events), the HIP-
event time of png_unfilter_kernel and png_expand_kernel (fnx_ctx_profile), and the whole call from the file's bytes in host
memory to the NRGBA image resident on the device.  Beside them, as context and measured on the same box: a bare zlib.decompress
of the same IDAT stream, and -- where Pillow is importable -- Image.open(...).load() (libpng's decode to the file's own pixel
format, no conversion to RGBA).
    python tools/time_png_decode.py [W H]"""
import io
import os
import sys
import time
import zlib

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch

import fennec_amd
import png_decode_ref as ref
import png_filter_ref as enc

W, H = (int(sys.argv[1]), int(sys.argv[2])) if len(sys.argv) > 2 else (3840, 2160)
REPS = 7
rgb = enc.smooth_rgba(W, H, 1, opaque=True)
rgba = enc.smooth_rgba(W, H, 2, opaque=False)
yy, xx = np.mgrid[0:H, 0:W]
pal_idx = ((xx // 5 + (yy // 3) * 7) % 256).astype(np.int64)[..., None]
rgba16 = (rgba.astype(np.int64) * 257 + np.random.default_rng(3).integers(0, 64, size=rgba.shape)) & 0xffff


def with_picked_filters(img, opaque):
    """the file png.Encoder's row stage would write: the filters tests/png_filter_ref.py picks, zlib level 6"""
    stream, ct, depth = enc.png_stream(img, enc.NRGBA, opaque=1 if opaque else 0)
    return b"".join([ref.SIG, ref.ihdr(W, H, depth, ct), ref.chunk(b"IDAT", zlib.compress(stream.tobytes(), 6)), ref.chunk(b"IEND", b"")])


CASES = [
    ("RGB, all Paeth (one chain)", lambda: ref.write_png(rgb[..., :3].astype(np.int64), 2, 8, filters=[4] * H)),
    ("RGB, the encoder's filters", lambda: with_picked_filters(rgb, True)),
    ("RGBA, the encoder's filters", lambda: with_picked_filters(rgba, False)),
    ("paletted, 8 bit", lambda: ref.write_png(pal_idx, 3, 8, palette=ref.random_palette(256, 1), trns=bytes(range(0, 256, 2)))),
    ("RGBA, 16 bit", lambda: ref.write_png(rgba16, 6, 16, filters=[(1, 2, 3, 4)[y & 3] for y in range(H)])),
]


def med(f, reps=REPS):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


try:
    from PIL import Image
    Image.MAX_IMAGE_PIXELS = None
except ImportError:
    Image = None

ctx = fennec_amd.Context(0)
print(f"fnx_png_decode, {W}x{H}, the file in host memory -> NRGBA on the device; ms unless stated (median of {REPS} after warm-up)")
print(f"{'file':30s} {'file MB':>8s} {'stream MB':>9s} {'chains':>7s} | {'walk':>6s} {'inflate':>8s} {'upload':>7s} {'unfilter us':>11s} {'expand us':>9s} "
      f"{'whole call':>10s} | {'zlib.decompress':>15s} {'Pillow load':>11s}")
for name, make in CASES:
    data = make()
    f = ref.parse(data)
    z = f["z"]
    raw_len = len(zlib.decompress(z))
    types = ref.filter_types(data)
    chains = 1 + sum(1 for t in types[1:] if t <= 1)
    for _ in range(2):
        img = ctx.png_decode(data, "device")
    ctx.sync()
    assert ctx.last_kernel() == "png_unfilter_kernel, png_expand_kernel"

    def whole():
        ctx.png_decode(data, "device")
        ctx.sync()
    wall = med(whole)
    ctx.profile(True)
    ks = []
    for _ in range(REPS):
        ctx.png_decode(data, "device")
        ks.append([ctx.kernel_ms(), ctx.kernel_ms()])
    ctx.profile(False)
    k = np.median(np.array(ks), axis=0) * 1e3
    walk = med(lambda: ctx.png_decode_config(data))
    infl = med(lambda: fennec_amd.inflate(z, cap=raw_len))
    pinned = torch.empty(raw_len, dtype=torch.uint8).pin_memory()
    dev = torch.empty(raw_len, dtype=torch.uint8, device="cuda:0")
    ups = []
    for _ in range(REPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dev.copy_(pinned, non_blocking=True)
        e1.record()
        e1.synchronize()
        ups.append(e0.elapsed_time(e1))
    zl = med(lambda: zlib.decompress(z))
    pil = f"{med(lambda: Image.open(io.BytesIO(data)).load()):11.1f}" if Image is not None else f"{'-':>11s}"
    print(f"{name:30s} {len(data) / 1e6:8.1f} {raw_len / 1e6:9.1f} {chains:7d} | {walk:6.2f} {infl:8.1f} {np.median(ups):7.2f} {k[0]:11.0f} {k[1]:9.0f} "
          f"{wall:10.1f} | {zl:15.1f} {pil}")
