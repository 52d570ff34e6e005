"""fnx_median_cut at the five palette sizes of quantizeStrategy (16, 32, 64, 128, 256; one run), per image: the device time of
median_cut_kernel (the library's HIP events, fnx_ctx_profile; median of 7), the fnx_download of the same image -- the crossing
the host route pays before it can sample -- (wall clock, median of 7), and the numpy restatement's wall time
(tests/median_cut_ref.py, once: the host's median cut, five palettes from one run as well).
    python tools/time_median_cut.py"""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch

import fennec_amd
import median_cut_ref as ref
from fennec_amd import synth

LEVELS = (16, 32, 64, 128, 256)
REPS = 7
CASES = [("4K photograph", synth.large_photo(3840, 2160, 0)),
         ("4K noise", synth.noise_image(3840, 2160, 1)),
         ("4K flat", synth.make_solid_image(3840, 2160, (37, 99, 200, 255))),
         ("447x447 noise", synth.noise_image(447, 447, 2))]

ctx = fennec_amd.Context(0)
print(f"device: {torch.cuda.get_device_name(0)}")
print(f"fnx_median_cut at levels {LEVELS}, device images; median of {REPS} after two warm-up calls")
print(f"{'image':16s} {'samples':>8s} {'colours':>8s} {'kernel us':>10s} {'download us':>12s} {'numpy ms':>9s} {'same bytes':>11s}")
for name, img in CASES:
    h, w = img.shape[:2]
    t = torch.from_numpy(np.ascontiguousarray(img)).cuda()
    torch.cuda.synchronize()
    for _ in range(2):
        got = ctx.median_cut(t, LEVELS)
    ctx.profile(True)
    ks = []
    for _ in range(REPS):
        ctx.median_cut(t, LEVELS)
        ks.append(ctx.kernel_ms() * 1e3)
    ctx.profile(False)
    host = np.empty_like(img)
    dl = []
    for _ in range(REPS + 2):
        t0 = time.perf_counter()
        rc = ctx._lib.fnx_download(ctx._h, host.ctypes.data, 4 * w, t.data_ptr(), 4 * w, w, h)
        dl.append((time.perf_counter() - t0) * 1e6)
        assert rc == 0
    assert np.array_equal(host, img)
    t0 = time.perf_counter()
    want, _ = ref.median_cut(img, LEVELS)
    np_ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(a, b) for a, b in zip(got, want))
    print(f"{name:16s} {len(ref.samples(img)):8d} {len(got[-1]):8d} {np.median(ks):10.1f} {np.median(dl[2:]):12.1f} {np_ms:9.1f} {str(same):>11s}")
