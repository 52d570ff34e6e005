"""Target-size mode's JPEG legs (hitTargetSize, targetsize.go:26-357) per 4K item, five routes:

  (a) the composed route the Go shim took before fnx_jpeg_target_size: host-space fnx_jpeg_size_search for strategy 1;
      a resident source with fnx_box_downsample(FNX_DEVICE_SRC) + a host-space size search per scale step; host-space
      Lanczos and SSIMFast for computeSSIMNRGBA
  (b) fnx_jpeg_target_size from a host source
  (c) the same from a device-resident source, size queries by the two-step route (form "jpeg_size" "0")
  (d) the same with the size queries answered in one wait (form "jpeg_size" "1": jpeg_ffcount_strips_kernel)
  (e) fennec_CompressFileTargetSize from the source's JPEG file (quality 95), form "jpeg_size" "1": decode, search and the
      winner's file, nothing but file bytes crossing (its image is the decoded file, so its winner is its own)

(a) and (b) run under the ctx's default form, which the first line names.  per row: ms per item (median of --reps, and the runs' minimum and maximum), size queries, the winning strategy and its file size.  Then the fused
box-downsample + colour conversion (fnx_jpeg_encode_scaled's size query) against box_tiled_kernel into an image followed
by jpeg_ycc_kernel (fennec_boxDownsample + fnx_jpeg_encode's size query) for the same geometries; both include the same
entropy-coded size query, so the difference is the kernels'.

    python tools/time_target_size.py [--reps 3]
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
from fennec_amd import FNX_TS_ALL, synth  # noqa: E402

MIN_Q = 20


def size_search(ctx, img, target, skip_ssim):
    """host-space fnx_jpeg_size_search -> (quality or 0, nbytes, ssim, steps)"""
    s = fennec_amd._Img(img)
    k = ctx.gaussianKernel()
    buf = np.empty(max(4096, target + 16), dtype=np.uint8)
    n, q, st, v = C.c_size_t(0), C.c_int(0), C.c_int(0), C.c_double(0)
    rc = ctx._lib.fnx_jpeg_size_search(ctx._h, s.space, s.ptr, s.stride, s.w, s.h, int(target), int(skip_ssim),
                                       k.ctypes.data_as(C.POINTER(C.c_double)), buf.ctypes.data, buf.size, C.byref(n),
                                       C.byref(q), C.byref(v), C.byref(st))
    ctx._chk(rc, "fnx_jpeg_size_search")
    return (q.value if rc == fennec_amd.FNX_OK else 0), n.value, v.value, st.value


def ssim_nrgba(ctx, src, img):
    h, w = src.shape[:2]
    if img.shape[:2] != (h, w):
        img = ctx.lanczosResize(img, w, h)
    return ctx.SSIMFast(src, img)


def route_a(ctx, img, dev, target):
    """hitTargetSize's JPEG legs composed from the per-op entry points -> (winner dict, size queries)"""
    h, w = img.shape[:2]
    nq = 0
    cands = []
    q, nb, s, n = size_search(ctx, img, target, False)              # strategy 1
    nq += n
    if q >= MIN_Q:
        cands.append(dict(strategy=1, quality=q, nbytes=nb, ssim=s))

    def scaled_fits(nw, nh):
        nonlocal nq
        small = ctx.boxDownsample(dev, nw, nh, to_host=True)        # FNX_DEVICE_SRC: the small image comes down
        q, nb, _, n = size_search(ctx, small, target, True)
        nq += n
        return q, q != 0 and nb <= target and q >= MIN_Q

    best, lo, hi = None, 0.05, 1.0                                   # strategy 3
    for _ in range(10):
        mid = (lo + hi) / 2
        nw, nh = int(w * mid), int(h * mid)
        if nw < 8 or nh < 8:
            lo = mid
            continue
        if scaled_fits(nw, nh)[1]:
            best, lo = mid, mid
        else:
            hi = mid
    for sc in (0.75, 0.5, 0.375, 0.25):
        nw, nh = int(w * sc), int(h * sc)
        if nw >= 8 and nh >= 8 and scaled_fits(nw, nh)[1] and (best is None or sc > best):
            best = sc
    if best is not None:
        fw, fh = int(w * best), int(h * best)
        fin = ctx.lanczosResize(img, fw, fh)
        q, nb, _, n = size_search(ctx, fin, target, False)
        nq += n
        if q >= MIN_Q:
            cands.append(dict(strategy=2, quality=q, nbytes=nb, ssim=ssim_nrgba(ctx, img, fin)))
    if not cands:                                                    # strategy 4
        best, best_q, lo, hi = 0.0, 0, 0.05, 1.0
        for _ in range(12):
            mid = (lo + hi) / 2
            nw, nh = int(w * mid), int(h * mid)
            if nw < 1 or nh < 1:
                lo = mid
                continue
            q, fits = scaled_fits(nw, nh)
            if fits:
                best, best_q, lo = mid, q, mid
            else:
                hi = mid
        if best:
            fw, fh = int(w * best), int(h * best)
            fin = ctx.lanczosResize(img, fw, fh)
            q, nb, _, n = size_search(ctx, fin, target, True)
            nq += n
            if q == 0:
                q, nb = best_q, ctx.jpeg_encoded_size(fin, best_q)
                nq += 1
            cands.append(dict(strategy=4, quality=q, nbytes=nb, ssim=ssim_nrgba(ctx, img, fin)))
    if not cands:                                                    # the fallback
        nq += 1
        cands.append(dict(strategy=8, quality=1, nbytes=ctx.jpeg_encoded_size(img, 1), ssim=ctx.SSIMFast(img, img)))
    best = cands[0]
    for c in cands[1:]:
        cu, bu = c["nbytes"] <= target, best["nbytes"] <= target
        if (cu and not bu) or (cu and bu and (c["ssim"], c["quality"]) > (best["ssim"], best["quality"])) or \
                (not cu and not bu and c["nbytes"] < best["nbytes"]):
            best = c
    return best, nq


class Ms(float):
    """the median of a timed() call's runs, their minimum and maximum beside it"""
    lo = hi = 0.0


def timed(fn, reps):
    out, ts = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    ms = Ms(statistics.median(ts))
    ms.lo, ms.hi = min(ts), max(ts)
    return out, ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import torch
    ctx = fennec_amd.Context(0)
    sources = {"photo": synth.large_photo(3840, 2160, 1),
               "noise": ctx.GaussianBlur(synth.noise_image(3840, 2160, 2), 1.0, exact=True)}
    print(f"# {torch.cuda.get_device_name(0)}; 3840 x 2160 sources; ms = median of {args.reps} (their minimum .. maximum)")
    print(f"{'source':6} {'target':>9} {'route':5} {'ms':>9} {'min .. max':>17} {'queries':>7} {'winner':>6} {'q':>3} {'bytes':>9}")
    files = {name: ctx.jpeg_encode(img, 95) for name, img in sources.items()}
    ctx.jpeg_encoded_size(sources["photo"][:64, :64].copy(), 50)
    print(f"# default size-query route of this build: {ctx.last_kernel(16)}")
    for name, img in sources.items():
        dev = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        q100 = ctx.jpeg_encoded_size(img, 100)
        # strategy 1 meets the first, only strategy 3 the second (full size at quality >= 20 does not fit), the third needs 4
        # or the fallback
        q20 = ctx.jpeg_encoded_size(img, 20)
        for target in (q100 // 4, q20 // 3, 700):
            wa, ms_a = timed(lambda: route_a(ctx, img, dev, target), args.reps)
            rb, ms_b = timed(lambda: ctx.jpeg_target_size(img, target, FNX_TS_ALL), args.reps)
            with ctx.forms(jpeg_size="0"):
                rc, ms_c = timed(lambda: ctx.jpeg_target_size(dev, target, FNX_TS_ALL), args.reps)
            with ctx.forms(jpeg_size="1"):
                rd, ms_d = timed(lambda: ctx.jpeg_target_size(dev, target, FNX_TS_ALL), args.reps)
                re_, ms_e = timed(lambda: ctx.compress_file_target_size(files[name], target), args.reps)
            assert (rc["candidates"], rc["winner"], rc["data"]) == (rd["candidates"], rd["winner"], rd["data"]), "forms disagree"
            for route, ms, res in (("a", ms_a, None), ("b", ms_b, rb), ("c", ms_c, rc), ("d", ms_d, rd), ("e", ms_e, re_)):
                if res is None:
                    c, nq = wa
                    win = {1: 1, 2: 3, 4: 4, 8: "fb"}[c["strategy"]]
                else:
                    c = res["candidates"][res["winner"]]
                    nq = sum(x["steps"] for x in res["candidates"])
                    win = {1: 1, 2: 3, 4: 4, 8: "fb"}[c["strategy"]]
                print(f"{name:6} {target:9d} {route:5} {ms:9.1f} {f'{ms.lo:.1f} .. {ms.hi:.1f}':>17} {nq:7d} {win!s:>6} {c['quality']:3d} {c['nbytes']:9d}")
            assert (wa[0]["quality"], wa[0]["nbytes"]) == (rb["candidates"][rb["winner"]]["quality"], len(rb["data"])), "routes disagree"
    # the fused kernel against box_tiled_kernel + jpeg_ycc_kernel (each with the same size query behind it)
    print("\n# one scale step's size query at quality 50: fused planes vs downsampled image + colour conversion (device source)")
    print(f"{'source':6} {'dw x dh':>11} {'fused ms':>9} {'composed ms':>12}")
    for name, img in sources.items():
        dev = torch.from_numpy(img).cuda()
        for s in (0.97, 0.5, 0.26, 0.05):
            dw, dh = int(3840 * s), int(2160 * s)
            ctx.jpeg_encode_scaled(dev, dw, dh, 50, size_only=True)
            n1, ms1 = timed(lambda: ctx.jpeg_encode_scaled(dev, dw, dh, 50, size_only=True), 10)
            n2, ms2 = timed(lambda: ctx.jpeg_encoded_size(ctx.boxDownsample(dev, dw, dh), 50), 10)
            assert n1 == n2
            print(f"{name:6} {f'{dw} x {dh}':>11} {ms1:9.3f} {ms2:12.3f}")


if __name__ == "__main__":
    main()
