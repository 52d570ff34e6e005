"""Where the IDAT chunk's CRC of a device-made PNG file comes from (Context.set_png_crc), timed both ways on one ctx:

  host     FNX_PNG_CRC_HOST: the host walks the chunk's bytes once they have come down (png_frame.cpp's crc32_update)
  device   FNX_PNG_CRC_DEVICE: crc32.hip's kernels read the gathered stream on the device, the CRC word comes down with the sizes

through the single route (n calls of Context.compress_png(img, device_deflate=True)) and the batch (one call of
Context.png_compress_batch(imgs)), over tools/time_png_compress_batch.py's three image sets -- "icons" 64 x 64, "screens"
512 x 512, "photos" 3840 x 2160 -- at n = 1 and 32.  Per row, in ms per image: the wall time of each mode around work that ends
in a synchronise (the two modes alternate inside every round; median of --rounds medians of --reps calls after a warm-up of
both, and the spread max - min of those medians); "gpu": the library's own HIP-event time of a call's launches
(fnx_ctx_profile), summed, per mode, and "crc": the share of the device mode's that the two CRC kernels take (the last two
launches of a call, or of a chunk); "host crc": png_frame.cpp's tail -- crc32_update over "IDAT" and the body -- on the very
streams of the row, alone on the host, in a program of its own (tools/png_frame_crc_host.cpp built here with g++ -O3; the
library's copy is hipcc's).  Every device-mode file is checked against the host mode's, byte for byte, before it is timed.

Each row is measured by a child process of its own under --limit seconds; the first row that fails or runs out of time ends
the run, nothing is retried.

    python tools/time_png_crc.py [--reps 5] [--rounds 3] [--ns 1,32] [--sets icons,screens,photos] [--limit 300]
"""
from __future__ import annotations

import argparse
import os
import statistics
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from time_png_compress_batch import image_set, timed_pair  # noqa: E402


def idat_of(data: bytes) -> bytes:
    i = 8
    while i < len(data):
        n, = struct.unpack(">I", data[i:i + 4])
        if data[i + 4:i + 8] == b"IDAT":
            return data[i + 8:i + 8 + n]
        i += 12 + n
    raise ValueError("no IDAT chunk")


def launches_ms(ctx, calls):
    """per call of a list, the HIP-event times of its launches in launch order (the library keeps the last 32 launches)"""
    import fennec_amd
    ctx.profile(fennec_amd.PROF_MAIN)
    out = []
    for fn in calls:
        fn()
        ms = []
        while True:
            try:
                ms.append(ctx.kernel_ms())
            except fennec_amd.FennecError:
                break
        out.append(ms)
    ctx.profile(0)
    return out


def host_crc_ms(exe, files, reps):
    """png_frame_tail's computing form over the files' IDAT bodies, ms per pass over all of them (median of reps)"""
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "bodies.bin")
        with open(path, "wb") as f:
            for data in files:
                z = idat_of(data)
                f.write(struct.pack("<I", len(z)) + z)
        return float(subprocess.check_output([exe, "time", path, str(reps)]).decode().split()[0])


def row(name, n, route, reps, rounds, exe):
    import numpy as np
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
    group = 4 if name == "photos" else 32                # images of one chunk: its launches fit the library's 32 event pairs

    if route == "single":
        def call():
            return [ctx.compress_png(t, device_deflate=True) for t in imgs]
        parts = [lambda t=t: ctx.compress_png(t, device_deflate=True) for t in imgs]
    else:
        def call():
            return ctx.png_compress_batch(imgs)[0]
        parts = [lambda k=k: ctx.png_compress_batch(imgs[k:k + group]) for k in range(0, n, group)]

    def mode(m):
        def fn():
            ctx.set_png_crc(m)
            return call()
        return fn
    want = mode("host")()
    assert mode("device")() == want, f"{name} n={n} {route}: the device mode's files differ from the host mode's"
    (hm, hs), (dm, ds) = timed_pair(mode("host"), mode("device"), n, reps, rounds)
    ctx.set_png_crc("host")
    gh = sum(sum(ms) for ms in launches_ms(ctx, parts)) / n
    ctx.set_png_crc("device")
    per_call = launches_ms(ctx, parts)
    gd = sum(sum(ms) for ms in per_call) / n
    gc = sum(sum(ms[-2:]) for ms in per_call) / n
    ctx.set_png_crc("host")
    hc = host_crc_ms(exe, want, 21) / n
    kb = sum(len(f) for f in want) / n / 1024
    print(f"{name:>8} {n:>3} {route:>6} | {hm:>8.3f} {hs:>6.3f} | {dm:>8.3f} {ds:>6.3f} | {gh:>8.3f} {gd:>8.3f} {gc:>7.4f} | {hc:>8.4f} | {kb:>8.1f} | {hm / dm:>5.2f}x",
          flush=True)


def build_host_tool(tmp):
    exe = os.path.join(tmp, "png_frame_crc_host")
    csrc = os.path.join(ROOT, "fennec_amd", "csrc")
    subprocess.check_call(["g++", "-O3", "-std=c++17", "-pthread", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I" + csrc,
                           os.path.join(ROOT, "tools", "png_frame_crc_host.cpp")] +
                          [os.path.join(csrc, f) for f in ("png_frame.cpp", "png_parse.cpp", "png_compress_plan.cpp")] + ["-o", exe])
    return exe


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--ns", default="1,32")
    ap.add_argument("--sets", default="icons,screens,photos")
    ap.add_argument("--limit", type=int, default=300, help="seconds a row's process may take")
    ap.add_argument("--row", nargs=4, metavar=("SET", "N", "ROUTE", "EXE"), help="measure this row in this process (what the parent starts)")
    args = ap.parse_args()
    if args.row:
        row(args.row[0], int(args.row[1]), args.row[2], args.reps, args.rounds, args.row[3])
        return 0
    print(f"# ms per image: median of {args.rounds} medians of {args.reps} calls after a warm-up, the two modes alternating; +- = max - min of those"
          f" medians; gpu: HIP-event ms per image of one call's launches, crc: the two CRC kernels' share of the device mode's;"
          f" host crc: crc32_update over the row's IDAT chunks alone on the host; KiB: mean file size; x: host / device (wall)")
    print(f"{'set':>8} {'n':>3} {'route':>6} | {'host':>8} {'+-':>6} | {'device':>8} {'+-':>6} | {'gpu host':>8} {'gpu dev.':>8} {'crc':>7} | {'host crc':>8} |"
          f" {'KiB/file':>8} | {'x':>6}", flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_host_tool(tmp)
        for name in args.sets.split(","):
            for n in (int(v) for v in args.ns.split(",")):
                for route in ("single", "batch"):
                    cmd = [sys.executable, os.path.abspath(__file__), "--row", name, str(n), route, exe, "--reps", str(args.reps),
                           "--rounds", str(args.rounds)]
                    try:
                        rc = subprocess.run(cmd, timeout=args.limit).returncode
                    except subprocess.TimeoutExpired:
                        print(f"{name} n={n} {route}: no result within {args.limit} s; the run ends here", flush=True)
                        return 1
                    if rc != 0:
                        print(f"{name} n={n} {route}: exit status {rc}; the run ends here", flush=True)
                        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
