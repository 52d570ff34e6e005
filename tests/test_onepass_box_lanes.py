"""blur_mfma_kernel<SCORE, .> / blur_mfma_wide_kernel<., ., SCORE>: only the lanes whose indicator column is a box column issue
the box atomics (the `live` bit of score_mfma_tables' column word; the wide kernel derives it from bx).

A lane wrongly masked loses a box's sums and changes the score; a lane wrongly left live only adds into the spare column.
So every case asks for the one-pass call to equal the two-call route bit for bit -- images with torch.equal, scores with ==
(test_gpu_parity._one_pass_case's method, restated here) -- in fast and in exact mode, and for the kept form
(GaussianBlur(keep_box_sums=True), then SSIMFast) to equal it too.  Every case first asserts the route by name.

The shapes are the smallest that reach each lane pattern of a wave's five box-column slots (lane r = 3 slot + channel, lane 15
unused); the long side must exceed 1843 px for the one-pass geometry:

    8192 x 128   boxes 16 x 16: one live slot, 13 dead lanes of 16
    7680 x 160   boxes 15 px: two slots
    3840 x 112   boxes 7.5 px: three slots, the benchmark's pattern
    2560 x 96    boxes 5 px: four slots
    2200 x 120   boxes of 4 and 5 px: five slots, no dead slot
    2048 x 64    boxes of exactly 4 px
    3850 x 112   the last tile is 10 px wide: waves with no boxed pixel (first == 255), dead in all their lanes
    120 x 3840   tall: many box rows, one tile column
"""
import numpy as np
import pytest

import fennec_amd
from fennec_amd import synth

pytestmark = pytest.mark.gpu

SIGMA = 2.0
SIGMA_WIDE = 3.0

SHAPES = [(8192, 128), (7680, 160), (3840, 112), (2560, 96), (2200, 120), (2048, 64), (3850, 112), (120, 3840)]
WIDE_SHAPES = [(3840, 112), (7680, 160)]


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


_cache = {}


def _device_images(w, h):
    """one noise image with alpha (a lost box sum changes its score) and one large_photo, on the device; built once per shape"""
    import torch
    if (w, h) not in _cache:
        imgs = [synth.noise_image(w, h, 5 * w + h, alpha=True), synth.large_photo(w, h, 2)]
        _cache[(w, h)] = [torch.from_numpy(i).cuda() for i in imgs]
        torch.cuda.synchronize()
    return _cache[(w, h)]


def _route(exact, wide):
    name = "blur_mfma_wide_kernel<SCORE" if wide else "blur_mfma_kernel<SCORE"
    return name + (", GUARD>" if exact else ">")


def _equal_to_two_calls(ctx, d, sigma, exact, wide):
    import torch
    outs, ss = ctx.GaussianBlurSSIMFastBatch(d, sigma, exact=exact)
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == _route(exact, wide)
    ref = ctx.GaussianBlurBatch(d, sigma, exact=exact)
    assert "SCORE" not in ctx.last_kernel(fennec_amd.PROF_MAIN)
    ref_ss = ctx.SSIMFastBatch(d, ref)
    for k in range(len(d)):
        assert torch.equal(outs[k], ref[k])
        assert ss[k] == ref_ss[k]
    return ref, ref_ss


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("w,h", SHAPES)
def test_live_lanes_one_pass(ctx, w, h, exact):
    import torch
    d = _device_images(w, h)
    ref, ref_ss = _equal_to_two_calls(ctx, d, SIGMA, exact, wide=False)
    # the kept form: the blur keeps both sides' box sums for the scoring call that follows
    for k in range(len(d)):
        out = ctx.GaussianBlur(d[k], SIGMA, exact=exact, keep_box_sums=True)
        assert ctx.last_kernel(fennec_amd.PROF_MAIN) == _route(exact, False)
        s = ctx.SSIMFast(d[k], out)
        assert ctx.last_kernel(fennec_amd.PROF_SSIM).startswith("kept box planes")
        print(f"{w}x{h} exact={exact} image {k}: kept {s!r} two calls {ref_ss[k]!r}")
        assert torch.equal(out, ref[k])
        assert s == ref_ss[k]


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("w,h", WIDE_SHAPES)
def test_live_lanes_wide_kernel(ctx, w, h, exact):
    d = _device_images(w, h)
    _equal_to_two_calls(ctx, d, SIGMA_WIDE, exact, wide=True)


def test_inputs_untouched(ctx):
    """the shared device images are what they were built from (no case wrote into a source)"""
    for (w, h), d in _cache.items():
        assert np.array_equal(d[0].cpu().numpy(), synth.noise_image(w, h, 5 * w + h, alpha=True))
