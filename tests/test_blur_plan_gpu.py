"""The host plan (csrc/blur_plan.cpp) against what launches: for the smallest shape of each route, the kernel the library
names after the call (Context.last_kernel) is the one tools/blur_plan_host.cpp prints for the same call, and the one-pass
blur + SSIMFast call returns the plain call's bytes.

    64 x 32 / 63 x 32 / 64 x 31   the smallest image of the matrix kernels, and its two neighbours (the direct kernel)
    radius 6 / 7                  blur_mfma_kernel / blur_mfma_wide_kernel<2>
    radius 24 / 25                the wide kernel's V window in one / two chained instructions (NKH = 4 / 5)
    radius 62 / 63                NKH = 8 / the generic fp64 passes
    2047 x 32                     the smallest shape with a one-pass form: narrow (radius 6), wide (7), direct (a weight >= 0.49)
    64 x 2048                     the one-pass narrow form over several segments
    1900 x 64                     boxes under 4 px: the matrix kernel alone, no one-pass form -- the two calls take the step

Reads the plan program's output and the library, nothing else."""
import numpy as np
import pytest
import torch

import fennec_amd
from fennec_amd import synth
from test_blur_plan import build_program, case, run

pytestmark = pytest.mark.gpu

# (w, h, sigma): radius = ceil(3 sigma)
CASES = [(64, 32, 2.0), (63, 32, 2.0), (64, 31, 2.0), (64, 32, 2.3), (64, 32, 8.0), (64, 32, 8.3), (64, 32, 20.6), (64, 32, 20.9),
         (2047, 32, 2.0), (2047, 32, 2.3), (2047, 32, 0.3), (64, 2048, 2.0), (1900, 64, 2.0)]
# what the docstring says of each case, checked against the plan: plain family, NKH, one-pass family
WANT = [("mfma", 0, None), ("direct", 0, None), ("direct", 0, None), ("mfma_wide", 2, None), ("mfma_wide", 4, None), ("mfma_wide", 5, None),
        ("mfma_wide", 8, None), ("generic_f64", 0, None), ("mfma", 0, "mfma"), ("mfma_wide", 2, "mfma_wide"), ("direct", 0, "direct"),
        ("mfma", 0, "mfma"), ("mfma", 0, None)]


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


@pytest.fixture(scope="module")
def plans(tmp_path_factory, ctx):
    program = build_program(tmp_path_factory.mktemp("blur_plan_gpu"), [])       # a plain build: only its output is needed here
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    cases = []
    for (w, h, sigma) in CASES:
        radius, k = ctx.blurKernel(sigma)
        assert len(k) == 2 * radius + 1
        _, nw, nh = ctx.ssimFastDims(w, h)
        cases += [case(w, h, [float(v) for v in k], exact, 1, cus, (nw, nh)) for exact in (False, True)]
    out = run(program, cases)
    return {(c, exact): out[2 * i + exact] for i, c in enumerate(CASES) for exact in (0, 1)}


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("w,h,sigma", CASES)
def test_the_launch_is_the_plans(ctx, plans, w, h, sigma, exact):
    p = plans[((w, h, sigma), int(exact))]
    family, nkh, scored = WANT[CASES.index((w, h, sigma))]
    assert (p["family"], p["nkh"], p["scored"] and p["family"]) == (family, nkh, scored), p["line"]
    img = synth.noise_image(w, h, 5 * w + h, alpha=True)
    plain = ctx.GaussianBlur(img, sigma, exact=exact)
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == p["route"]
    both, _ = ctx.GaussianBlurSSIMFast(img, sigma, exact=exact)
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == p["route"]              # one image: the plain kernel, then the score
    assert np.array_equal(both, plain)
    d = torch.from_numpy(img.copy()).cuda()
    torch.cuda.synchronize()
    outs, _ = ctx.GaussianBlurSSIMFastBatch([d], sigma, exact=exact)
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == (p["scored"]["route"] if p["scored"] else p["route"])
    assert np.array_equal(outs[0].cpu().numpy(), plain)
