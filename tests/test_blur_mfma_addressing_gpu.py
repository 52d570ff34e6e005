"""csrc/blur_mfma.hip: how a workgroup addresses its rows and where the one-pass form's set-up comes from.

A workgroup whose whole source window lies inside the image addresses its row sets from a scalar base with 32-bit lane
offsets; the ones on an edge clamp per lane; a launch whose row offsets do not fit 31 bits keeps 64-bit addresses everywhere.
The one-pass (SSIMFast) form reads its column and row look-ups from tables the host builds once per geometry.  The shapes
below put interior workgroups and every kind of edge workgroup into one image (first / last tile column, first / last
segment, a last tile column one pixel wide, a short last segment, a single segment that is an edge on both sides), and run
them through pitched views, unaligned bases, differing strides and a stride past 2^31 / 33 rows.

Bars: the one-pass call equals the two calls bit for bit; exact mode equals the oracle's image; fast mode passes
test_gpu_parity's assert_blur_close; scores are within SSIM_TOL of the oracle's SSIMFast of the returned pair."""
import numpy as np
import pytest

import fennec_amd
from fennec_amd import synth
from test_gpu_parity import SSIM_TOL, _one_pass_case, assert_blur_close

pytestmark = pytest.mark.gpu

SIGMA = 2.0
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


_cache = {}


def _image(w, h, k=0):
    key = ("img", w, h, k)
    if key not in _cache:
        img = synth.noise_image(w, h, 5 * w + h + k, alpha=True)
        img.setflags(write=False)
        _cache[key] = img
    return _cache[key]


def _want(orc, w, h, k=0):
    """the oracle's blur of _image(w, h, k), computed once for the fast and the exact case"""
    key = ("blur", w, h, k)
    if key not in _cache:
        want = orc.gaussian_blur(_image(w, h, k), SIGMA, procs=8)
        want.setflags(write=False)
        _cache[key] = want
    return _cache[key]


def _check_image(got, want, exact):
    if exact:
        assert np.array_equal(got, want)
    else:
        assert_blur_close(got, want)


def _view(big, y0, x0, h, w):
    return big[y0:y0 + h, x0:x0 + w]


def _put(img, rows, cols, y0, x0, fill=None):
    """img as a sub-rectangle at (y0, x0) of a fresh rows x cols device tensor"""
    import torch
    big = torch.empty((rows, cols, 4), dtype=torch.uint8, device="cuda")
    if fill is not None:
        big.fill_(fill)
    h, w = img.shape[:2]
    view = _view(big, y0, x0, h, w)
    view.copy_(torch.from_numpy(np.array(img)).cuda())
    torch.cuda.synchronize()
    return big, view


def _one_pass_views(ctx, orc, hosts, srcs, dsts, exact, wants):
    """_one_pass_case's check for device views: the one-pass call into `dsts` equals the two calls, bit for bit, the images
    are the oracle's (exact) or close to them (fast), the scores the oracle's SSIMFast of the returned pairs"""
    import torch
    outs, ss = ctx.GaussianBlurSSIMFastBatch(srcs, SIGMA, outs=dsts, exact=exact)
    ref = ctx.GaussianBlurBatch(srcs, SIGMA, exact=exact)
    if max(hosts[0].shape[:2]) > 512:
        ref_ss = ctx.SSIMFastBatch(srcs, ref)
    else:
        ref_ss = np.array([ctx.SSIMFast(a, b) for a, b in zip(srcs, ref)])
    for k, host in enumerate(hosts):
        assert torch.equal(outs[k], ref[k])
        assert ss[k] == ref_ss[k]
        got = outs[k].cpu().numpy()
        _check_image(got, wants[k], exact)
        assert abs(ss[k] - orc.ssim_fast(host, got)) <= SSIM_TOL


# 2048 x 600: 32 tile columns and three or more segments -- interior workgroups, both x edges, both y edges, the corners
# 192 x 2048: three tile columns (one interior) and 8 segments
# 2049 x 560: a last tile column one pixel wide, a last segment that is no multiple of 16 rows
# 2048 x 33:  one short segment, an edge at the top and at the bottom
ONE_PASS = [(2048, 600), (192, 2048), (2049, 560), (2048, 33)]


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("w,h", ONE_PASS)
def test_one_pass(ctx, orc, w, h, exact):
    import torch
    img = _image(w, h)
    _one_pass_case(ctx, orc, [img.copy()], SIGMA, exact=exact, check_oracle=(0,))
    d = torch.from_numpy(img.copy()).cuda()
    torch.cuda.synchronize()
    outs, ss = ctx.GaussianBlurSSIMFastBatch([d], SIGMA, exact=exact)
    got = outs[0].cpu().numpy()
    _check_image(got, _want(orc, w, h), exact)
    assert abs(ss[0] - orc.ssim_fast(img, got)) <= SSIM_TOL


# 320 x 1700: at least four segments of at most 544 rows; 64 x 32: the smallest image the kernel takes
@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("w,h", [(320, 1700), (64, 32)])
def test_plain_blur(ctx, orc, w, h, exact):
    got = ctx.GaussianBlur(_image(w, h), SIGMA, exact=exact)
    _check_image(got, _want(orc, w, h), exact)


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_one_pass_strided_batch(ctx, orc, exact):
    """three separately allocated sources and destinations, all sub-rectangles of larger tensors: an odd pixel offset (4-byte
    alignment only), a 16-byte aligned one and one at the origin; the destinations' stride is not the sources'"""
    w, h = 2048, 600
    hosts = [_image(w, h, k) for k in range(3)]
    wants = [_want(orc, w, h, k) for k in range(3)]
    src_at = [(7, 13), (0, 0), (3, 4)]
    dst_at = [(1, 5), (9, 1), (0, 0)]
    srcs = [_put(img, h + 11, w + 40, y0, x0)[1] for img, (y0, x0) in zip(hosts, src_at)]
    dsts = [_put(np.zeros_like(img), h + 9, w + 72, y0, x0)[1] for img, (y0, x0) in zip(hosts, dst_at)]
    assert srcs[0].stride(0) != dsts[0].stride(0)
    _one_pass_views(ctx, orc, hosts, srcs, dsts, exact, wants)


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_plain_blur_strided_batch(ctx, orc, exact):
    w, h = 320, 1700
    hosts = [_image(w, h, k) for k in range(3)]
    src_at = [(7, 13), (0, 0), (3, 4)]
    dst_at = [(1, 5), (9, 1), (0, 0)]
    srcs = [_put(img, h + 11, w + 40, y0, x0)[1] for img, (y0, x0) in zip(hosts, src_at)]
    dsts = [_put(np.zeros_like(img), h + 9, w + 72, y0, x0)[1] for img, (y0, x0) in zip(hosts, dst_at)]
    outs = ctx.GaussianBlurBatch(srcs, SIGMA, outs=dsts, exact=exact)
    ctx.sync()
    for k in range(3):
        _check_image(outs[k].cpu().numpy(), _want(orc, w, h, k), exact)


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
@pytest.mark.parametrize("one_pass", [True, False], ids=["one_pass", "plain"])
def test_no_stray_stores(ctx, orc, one_pass, exact):
    """the destination is a view inside a tensor full of a sentinel byte: every byte outside the view still holds it afterwards"""
    w, h = 2049, 560
    img = _image(w, h)
    y0, x0 = 5, 3
    _, src = _put(img, h + 4, w + 9, 2, 1)
    big, dst = _put(np.zeros_like(img), h + 12, w + 8, y0, x0, fill=SENTINEL)
    if one_pass:
        outs, ss = ctx.GaussianBlurSSIMFastBatch([src], SIGMA, outs=[dst], exact=exact)
        assert abs(ss[0] - orc.ssim_fast(img, outs[0].cpu().numpy())) <= SSIM_TOL
    else:
        outs = ctx.GaussianBlurBatch([src], SIGMA, outs=[dst], exact=exact)
        ctx.sync()
    after = big.cpu().numpy()
    _check_image(after[y0:y0 + h, x0:x0 + w], _want(orc, w, h), exact)
    outside = np.ones(after.shape[:2], dtype=bool)
    outside[y0:y0 + h, x0:x0 + w] = False
    assert (after[outside] == SENTINEL).all()


@pytest.mark.parametrize("exact", [False, True], ids=["fast", "exact"])
def test_row_offsets_past_31_bits(ctx, orc, exact):
    """a 64 x 33 view whose rows lie 70 MB apart (allocated, touched in the view only): the last rows' offsets pass 2^31, the
    launch keeps 64-bit addresses; plain blur, and the one-pass call (no matrix one-pass form at this size: its fallback route)"""
    import torch
    w, h = 64, 33
    img = _image(w, h)
    want = _want(orc, w, h)
    big = torch.empty((h, 17_500_000, 4), dtype=torch.uint8, device="cuda")
    src = big[:, 1000:1000 + w]
    src.copy_(torch.from_numpy(img.copy()).cuda())
    torch.cuda.synchronize()
    assert src.stride(0) * (h - 1) >= 2 ** 31
    tight = src.contiguous()
    got = ctx.GaussianBlurBatch([src], SIGMA, exact=exact)[0]
    ref = ctx.GaussianBlurBatch([tight], SIGMA, exact=exact)[0]
    ctx.sync()
    assert torch.equal(got, ref)
    _check_image(got.cpu().numpy(), want, exact)
    # into a destination view with the same 70 MB stride
    dst = big[:, 5000:5000 + w]
    ctx.GaussianBlurBatch([tight], SIGMA, outs=[dst], exact=exact)
    ctx.sync()
    assert torch.equal(dst, ref)
    _one_pass_views(ctx, orc, [img], [src], [big[:, 9000:9000 + w]], exact, [want])
    del big
