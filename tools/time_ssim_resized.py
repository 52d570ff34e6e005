"""computeSSIMNRGBA (targetsize.go:563-568) of a large `a` and a smaller `b`, per call, three legs in both spaces:

  (i)   baseline: fennec_lanczosResize(b -> a's size), then fnx_ssim_fast -- in host space the pair of calls the cgo shim made
        before fnx_ssim_fast_resized (the upscaled image comes down and goes up again), in device space the resize into a
        device image followed by the score.  Only entry points every earlier version has: the script runs unchanged on an
        older checkout, where legs (ii) and (iii) are skipped -- the comparison figure comes from there.
  (ii)  composed: fnx_ssim_fast_resized with the ctx's "resize_box" form "0" (lanczosResize into scratch, the box kernel)
  (iii) fused:    fnx_ssim_fast_resized with the form "1" (resize_box_kernel: the upscaled image is never stored)

Per leg: wall ms (host clock around the blocking call) and HIP-event ms (events on the stream the ctx launches on), each the
median of --reps calls after --warmup, with the 10th..90th percentile spread beside it.  The legs of one shape alternate call
by call, so that whatever else the machine is doing falls on all of them alike.

    python tools/time_ssim_resized.py [--reps 30] [--warmup 5]
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import fennec_amd  # noqa: E402
from fennec_amd import synth  # noqa: E402

SHAPES = [(3840, 2160, 0.25), (3840, 2160, 0.5), (3840, 2160, 0.75), (1920, 1080, 0.5)]


def stat(xs):
    xs = sorted(xs)
    lo, hi = xs[len(xs) // 10], xs[(len(xs) * 9) // 10]
    return f"{statistics.median(xs):8.3f} ({lo:7.3f}..{hi:7.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert args.reps >= 20, "a median of fewer than 20 calls is not reported"
    import torch
    ctx = fennec_amd.Context(0)
    # every call, host-space ones included, on torch's current stream: the events below then bracket the call's own work
    cur = torch.cuda.current_stream().cuda_stream
    ctx._chk(ctx._lib.fnx_ctx_use_stream(ctx._h, C.c_void_p(cur)), "fnx_ctx_use_stream")
    ctx._lent = cur
    new = hasattr(ctx, "ssim_fast_resized")
    print(f"# {torch.cuda.get_device_name(0)}; {fennec_amd.load_library().fnx_version().decode()}; ms per call: median of {args.reps} "
          f"(10th..90th percentile), {args.warmup} warm-up calls; new entry points: {'yes' if new else 'no (baseline leg only)'}")
    print(f"{'a':>11} {'b':>11} {'space':6} {'leg':9} {'wall ms':>26} {'HIP-event ms':>26} {'score':>15} {'resize route'}")
    for aw, ah, s in SHAPES:
        bw, bh = int(aw * s), int(ah * s)
        da = ctx.GaussianBlur(ctx.GaussianBlur(torch.from_numpy(synth.noise_image(aw, ah, 5)).cuda(), 2.0), 1.2)
        db = ctx.lanczosResize(da, bw, bh)
        ctx.sync()
        ha, hb = da.cpu().numpy(), db.cpu().numpy()
        for space, (a, b) in (("host", (ha, hb)), ("device", (da, db))):
            def baseline():
                return ctx.SSIMFast(a, ctx.lanczosResize(b, aw, ah))
            legs = [("baseline", baseline, None)]
            if new:
                legs += [("composed", lambda: ctx.computeSSIMNRGBA(a, b), 0), ("fused", lambda: ctx.computeSSIMNRGBA(a, b), 1)]
            wall = {n: [] for n, _, _ in legs}
            dev = {n: [] for n, _, _ in legs}
            val, route = {}, {}
            for rep in range(args.warmup + args.reps):
                for name, fn, form in legs:
                    if new:
                        ctx.set_form("resize_box", form)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record()
                    val[name] = fn()
                    e1.record()
                    e1.synchronize()
                    t1 = time.perf_counter()
                    route[name] = ctx.last_kernel(fennec_amd.PROF_RESIZE)
                    if rep >= args.warmup:
                        wall[name].append((t1 - t0) * 1e3)
                        dev[name].append(e0.elapsed_time(e1))
            if new:
                ctx.set_form("resize_box", None)
                assert val["fused"] == val["composed"], (val["fused"], val["composed"])
                assert abs(val["fused"] - val["baseline"]) <= 1e-9, (val["fused"], val["baseline"])
                assert route["fused"] == "resize_box_kernel" and route["composed"] != "resize_box_kernel", route
            for name, _, _ in legs:
                print(f"{f'{aw}x{ah}':>11} {f'{bw}x{bh}':>11} {space:6} {name:9} {stat(wall[name]):>26} {stat(dev[name]):>26} "
                      f"{val[name]:15.12f} {route[name]}")


if __name__ == "__main__":
    main()
