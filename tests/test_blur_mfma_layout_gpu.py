"""csrc/blur_mfma.hip: which ring columns a V set filters, and the box sums next to them.

A V set of blur_mfma_kernel is one colour channel of the wave's 16 px (three sets per 16 output rows; the alpha columns of
the ring are read as bytes, never filtered), and the ring's 16-column groups are skewed for that read.  A wrong column,
channel or pixel pick shows on noise with an alpha channel: every sample of such an image differs from its neighbours.
The shapes are the smallest that put every form of the march into one image: first / last tile column (a last one 8 px
and 1 px wide), tile columns whose window stays inside the image, one segment, two segments with a short last one, a
height that is no multiple of 16, and three segments (the middle one addresses its rows from a scalar base).

The one-pass (SSIMFast) cases pick box geometries by the long side: 4-px boxes (five box rows in a 16-row block), uneven
4 / 5-px boxes, 7.5 px, 16 px (a block inside one box), a short last segment, and all-0 / all-255 images at 16-px boxes,
where a block's column sums of (p - 128) reach -2048 and +2032.

Exact mode's V fix-up follows the same map (flag bit 4 q + i, ring column 16 g + 4 i + q, patched byte 4 i + q), and only
about 6 samples in 100 000 are flagged at sigma = 2 -- a handful per small noise image, at whatever positions they fall.
_flagged_image arranges them: an image that is constant along x (the H pass then returns its input exactly) whose rows hold,
per channel, 13-row patterns found on the host with fnx_blur_fixed_point for which the kernel's own test flags the V sample.
Two output rows, one in an even and one in an odd V set, are flagged in every channel of every pixel of the row; the three
channels blur to different bytes there, so a patch that reads or writes another channel's or pixel's byte shows.

Every case first asserts the route by name (ctx.last_kernel).  Bars: exact mode equals the oracle's image; fast mode passes
test_gpu_parity's assert_blur_close; alpha is the source's; the one-pass call equals the two calls bit for bit and its
scores are within SSIM_TOL of the oracle's SSIMFast of the returned pair."""
import numpy as np
import pytest

import fennec_amd
from fennec_amd import synth
from test_gpu_parity import SSIM_TOL, _one_pass_case, assert_blur_close

pytestmark = pytest.mark.gpu

SIGMA = 2.0


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


_cache = {}


def _image(w, h):
    key = ("img", w, h)
    if key not in _cache:
        img = synth.noise_image(w, h, 3 * w + h, alpha=True)
        img.setflags(write=False)
        _cache[key] = img
    return _cache[key]


def _want(orc, w, h):
    """the oracle's blur of _image(w, h), computed once for the fast and the exact case"""
    key = ("blur", w, h)
    if key not in _cache:
        want = orc.gaussian_blur(_image(w, h), SIGMA)
        want.setflags(write=False)
        _cache[key] = want
    return _cache[key]


# 200 x 48:  four tile columns (two of them away from the x edges, the last 8 px wide), one segment
# 65 x 40:   a last tile column one pixel wide, a height that is no multiple of 16
# 200 x 72:  two segments of 48 rows, the last one 24 rows short
# 200 x 112: three segments; the middle one's staged rows all lie inside the image
PLAIN = [(200, 48), (65, 40), (200, 72), (200, 112)]


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("w,h", PLAIN)
def test_v_sets_plain_blur(ctx, orc, w, h, exact):
    img = _image(w, h)
    got = ctx.GaussianBlur(img, SIGMA, exact=exact)
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == ("blur_mfma_kernel<GUARD>" if exact else "blur_mfma_kernel")
    want = _want(orc, w, h)
    if exact:
        assert np.array_equal(got, want)
    else:
        assert_blur_close(got, want)
    assert np.array_equal(got[..., 3], img[..., 3])


FLAGGED_ROWS = (8, 28)      # output rows of V set 0 (even) and V set 1 (odd); their 13 source rows do not overlap


def _flagged_image(orc, w, h):
    """(image, flagged output rows): constant along x; at FLAGGED_ROWS the V sample of every channel of every pixel has its
    fraction within the guard distance of the rounding boundary, by the kernel's own test: (sum wq p + 2^23 + G) mod 2^24 < 2 G"""
    import math
    key = ("flagged", w, h)
    if key in _cache:
        return _cache[key]
    radius, k = orc.blur_kernel(SIGMA)
    wq, err255 = fennec_amd.blur_fixed_point(k)
    wq = np.array(wq, dtype=np.int64)
    assert radius == 6 and int(wq.sum()) == 1 << 24
    gq = math.ceil(err255) + 2
    rng = np.random.default_rng(8)
    cand = rng.integers(0, 256, size=(600_000, 13), dtype=np.int64)
    frac = ((cand @ wq) + (1 << 23) + gq) & 0xffffff
    hits = cand[frac < 2 * gq]
    # six patterns whose blurred bytes differ from one another (3 channels x 2 rows)
    picked, seen = [], set()
    for pat in hits:
        byte = int((int(pat @ wq) + (1 << 23)) >> 24)
        if byte not in seen:
            seen.add(byte)
            picked.append(pat)
        if len(picked) == 6:
            break
    assert len(picked) == 6
    col = rng.integers(0, 256, size=(h, 4), dtype=np.int64)          # one pixel per row, repeated along x
    for n, y in enumerate(FLAGGED_ROWS):
        for ch in range(3):
            col[y - 6:y + 7, ch] = picked[3 * n + ch]
    img = np.ascontiguousarray(np.broadcast_to(col[:, None, :], (h, w, 4)).astype(np.uint8))
    for y in FLAGGED_ROWS:                                           # what was arranged, checked
        for ch in range(3):
            f = (int(col[y - 6:y + 7, ch] @ wq) + (1 << 23) + gq) & 0xffffff
            assert f < 2 * gq
    img.setflags(write=False)
    _cache[key] = img
    return img


@pytest.mark.parametrize("w,h", [(200, 48)])
def test_v_fixup_every_position_plain(ctx, orc, w, h):
    img = _flagged_image(orc, w, h)
    got = ctx.GaussianBlur(img, SIGMA, exact=True)
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == "blur_mfma_kernel<GUARD>"
    want = orc.gaussian_blur(img, SIGMA)
    for y in FLAGGED_ROWS:
        assert len(set(int(v) for v in want[y, w // 2, :3])) == 3
    assert np.array_equal(got, want)


def test_v_fixup_every_position_one_pass(ctx, orc):
    w, h = 2048, 96
    img = _flagged_image(orc, w, h)
    got = _one_pass(ctx, orc, img, True)
    assert np.array_equal(got, orc.gaussian_blur(img, SIGMA))


def _one_pass(ctx, orc, img, exact):
    import torch
    d = torch.from_numpy(img.copy()).cuda()
    torch.cuda.synchronize()
    outs, ss = ctx.GaussianBlurSSIMFastBatch([d], SIGMA, exact=exact)
    assert ctx.last_kernel(fennec_amd.PROF_MAIN) == ("blur_mfma_kernel<SCORE, GUARD>" if exact else "blur_mfma_kernel<SCORE>")
    got = outs[0].cpu().numpy()
    assert np.array_equal(got[..., 3], img[..., 3])
    _one_pass_case(ctx, orc, [img.copy()], SIGMA, exact=exact, check_oracle=(0,))
    return got


# 2048 x 96:  boxes of exactly 4 px -- five box rows in a 16-row block that starts inside a box
# 2200 x 80:  uneven boxes of 4 and 5 px
# 3840 x 64:  7.5 px, the benchmark's geometry
# 8192 x 48:  16-px boxes: a 16 x 16 block lies inside one box
# 2048 x 104: a last segment of 8 rows
ONE_PASS = [(2048, 96), (2200, 80), (3840, 64), (8192, 48), (2048, 104)]


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("w,h", ONE_PASS)
def test_v_sets_one_pass(ctx, orc, w, h, exact):
    got = _one_pass(ctx, orc, _image(w, h), exact)
    want = _want(orc, w, h)
    if exact:
        assert np.array_equal(got, want)
    else:
        assert_blur_close(got, want)


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("value", [0, 255])
def test_one_pass_flat_extremes(ctx, orc, value, exact):
    """every byte 0 / 255, 16-px boxes: the column sums of a block are -2048 / +2032 before the seed; a flat image blurs to itself"""
    w, h = 8192, 48
    img = np.full((h, w, 4), value, dtype=np.uint8)
    got = _one_pass(ctx, orc, img, exact)
    assert np.array_equal(got, img)
