"""The device JPEG encoder's entropy coder on crafted images that reach every Huffman symbol (tests/jpeg_enc_cases.py; what they
reach is proved on the CPU in test_jpeg_enc_cases.py): every file byte for byte the oracle's, from a host array and from a device
tensor; the size query under both "jpeg_size" forms; the round trip's pixels; and the batched coder through
fnx_jpeg_compress_batch on lists ordered against a predictor or a string leaking from one image into the next.  Every comparison
is byte equality.  A mismatch names the first differing byte and, from the plain-Python writer's symbol map of the oracle's
coefficients, the block and the symbol that hold it."""
from __future__ import annotations

import numpy as np
import pytest

import fennec_amd
import jpeg_enc_cases as ec
from oracle import oracle as orc
from test_jpeg_roundtrip import _oracle_search

pytestmark = pytest.mark.gpu

PROF_JPEG = 16
ONE_WAIT, TWO_STEP = "jpeg_ffcount_strips_kernel", "jpeg_pack_kernel"


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def _same_file(got, want, img, coef, what):
    if got != want:
        h, w = img.shape[:2]
        raise AssertionError(f"{what}: {ec.first_difference(got, want, coef, w, h)}")


@pytest.mark.parametrize("name", list(ec.cases()))
def test_file_size_and_pixels_are_the_oracles(ctx, name):
    import torch
    case = ec.cases()[name]
    img = np.ascontiguousarray(case.img)
    dev = torch.from_numpy(img).cuda()
    for q in case.qualities:
        want, coef = orc.jpeg_encode(img, q, with_coefficients=True)
        _same_file(ctx.jpeg_encode(img, q), want, img, coef, f"{name} at {q}, host array")
        _same_file(ctx.jpeg_encode(dev, q), want, img, coef, f"{name} at {q}, device tensor")
        for form, kernel in (("1", ONE_WAIT), ("0", TWO_STEP)):
            with ctx.forms(jpeg_size=form):
                assert ctx.jpeg_encoded_size(img, q) == len(want), (name, q, form)
                assert ctx.last_kernel(PROF_JPEG) == kernel, (name, q, form)
                assert ctx.jpeg_encoded_size(dev, q) == len(want), (name, q, form)
        assert np.array_equal(ctx.jpeg_roundtrip(img, q), orc.jpeg_decode(want)), (name, q)


@pytest.mark.parametrize("name", list(ec.batches()))
def test_the_batched_coder_on_ordered_lists(ctx, name):
    import torch
    items = ec.batches()[name]
    host = [np.ascontiguousarray(img) for img, _ in items]
    targets = [t for _, t in items]
    dev = [torch.from_numpy(img).cuda() for img in host]
    torch.cuda.synchronize()
    got = ctx.jpeg_compress_batch(dev, targets)
    assert len(got) == len(items)
    covs, coefs = [], []
    for i, (img, t) in enumerate(zip(host, targets)):
        data, q, s, n = got[i]
        want, coef = orc.jpeg_encode(img, q, with_coefficients=True)
        _same_file(data, want, img, coef, f"{name}[{i}] at the returned quality {q}")
        assert len(want) <= 4096 + img.shape[0] * img.shape[1] * 3 // 2   # it fitted the call's buffer: these are the batched coder's bytes
        assert got[i] == ctx.jpeg_compress(dev[i], t), (name, i)
        assert q == _oracle_search(img, t)[0], (name, i, q)           # the targets were chosen with the oracle-driven search
        covs.append(ec.coverage(coef))
        coefs.append(coef)
    # at the RETURNED qualities, from the oracle's coefficients: the list still holds a DC category 11 in both tables and an AC
    # size 10, its neighbours' strings differ mod 32 bits, and flat gray follows an image that ends on large DCs
    for t in (0, 1):
        assert any(11 in cov["dc"][t] for cov in covs), (name, t)
    assert any(size == 10 for cov in covs for t in (0, 1) for _, size in cov["ac"][t]), name
    residues = [int(cov["bits"].sum()) % 32 for cov in covs]
    assert all(a != b for a, b in zip(residues, residues[1:])), residues
    leaks_would_show = 0
    for i in range(len(items) - 1):
        last = [abs(int(v)) for v in coefs[i][-3:, 0]]                # the last MCU's Y3, Cb and Cr
        if min(last) >= 128 and (host[i + 1][..., :3] == 128).all():
            assert not coefs[i + 1].any()
            leaks_would_show += 1
    assert leaks_would_show >= 1, name
