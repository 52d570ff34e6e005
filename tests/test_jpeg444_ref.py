"""tests/jpeg444_ref.py -- the CPU restatement of FNX_JPEG_SUBSAMPLING_444 the GPU tests hold the library to -- against what can
be checked without the library: the oracle's decoder reads its files as 4:4:4, to its coefficients and its round trip; Pillow
(libjpeg-turbo) opens them as three components at 4:4:4; and where 4:2:0 and 4:4:4 must agree -- the Y blocks of an opaque gray
image whose dims are multiples of 16 -- its coefficients are the oracle encoder's.  No GPU, no library."""
from __future__ import annotations

import io

import numpy as np
import pytest

import jpeg444_ref as ref
from oracle import oracle as orc

CASES = sorted(ref.cases())


@pytest.mark.parametrize("name", CASES)
def test_the_oracles_decoder_reads_the_restated_file(name):
    img, qualities = ref.cases()[name]
    for q in qualities:
        r = ref.ref(name, q)
        w, h, ratio, y, cb, cr, coef = orc.jpeg_decode_planes(r.file, with_coefficients=True)
        assert (w, h, ratio) == (img.shape[1], img.shape[0], 0), (name, q)
        assert np.array_equal(coef, r.coef), (name, q)
        assert np.array_equal(np.stack([y, cb, cr]), r.planes), (name, q)
        assert np.array_equal(orc.jpeg_decode(r.file), r.image), (name, q)
        # the writer's own file (its header is jpeg_craft's, the scan the same) says the same
        assert np.array_equal(orc.jpeg_decode_planes(r.crafted.data, with_coefficients=True)[6], r.coef), (name, q)


@pytest.mark.parametrize("name", CASES)
def test_pillow_opens_the_restated_file_as_444(name):
    from PIL import Image, JpegImagePlugin
    img, qualities = ref.cases()[name]
    for q in qualities:
        for data in (ref.ref(name, q).file, ref.ref(name, q).opt_file):
            im = Image.open(io.BytesIO(data))
            im.load()
            assert im.size == (img.shape[1], img.shape[0]) and im.mode == "RGB" and len(im.layer) == 3, (name, q)
            assert JpegImagePlugin.get_sampling(im) == 0, (name, q)                 # 0: 4:4:4


@pytest.mark.parametrize("name", CASES)
def test_the_optimised_file_decodes_to_the_same_coefficients(name):
    for q in ref.cases()[name][1]:
        r = ref.ref(name, q)
        got = orc.jpeg_decode_planes(r.opt_file, with_coefficients=True)
        assert got[2] == 0 and np.array_equal(got[6], r.coef), (name, q)
        assert len(r.opt_file) <= len(r.file) + 4 * 17 + 4 * 256, (name, q)      # (tiny images: the tables may cost more than they save)


def _gray(w, h, seed):
    g = np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)
    img = np.full((h, w, 4), 255, np.uint8)
    img[..., 0] = img[..., 1] = img[..., 2] = g
    return img


@pytest.mark.parametrize("w,h", [(16, 16), (48, 32), (32, 64)])
def test_y_blocks_are_the_oracle_encoders_on_gray_images(w, h):
    """R = G = B, opaque, dims multiples of 16: no clamp and no chroma in Y, so 4:2:0's Y blocks are 4:4:4's, mapped by (bx, by)"""
    img = _gray(w, h, w + h)
    for q in ref.QUALITIES:
        _, coef420 = orc.jpeg_encode(img, q, with_coefficients=True)
        coef444 = ref.Ref(img, q).coef
        mx8, mx16 = w // 8, w // 16
        for by in range(h // 8):
            for bx in range(mx8):
                at420 = ((by >> 1) * mx16 + (bx >> 1)) * 6 + (by & 1) * 2 + (bx & 1)
                assert np.array_equal(coef444[(by * mx8 + bx) * 3], coef420[at420]), (q, bx, by)


def test_the_quantiser_rounds_halves_away_from_zero():
    fd = np.zeros((3, 1, 1, 64), np.int32)
    q = ref.quantisers(50)
    fd[0, 0, 0, :4] = [4 * q[0, 0], -4 * q[0, 1], 4 * q[0, 2] - 1, -(4 * q[0, 3] - 1)]      # +-half a step, and just under it
    fd[1, 0, 0, :2] = [12 * q[1, 0], -12 * q[1, 1]]                                        # +-one and a half steps
    got = ref.quantise(fd, 50)
    assert got[0, 0, 0, :4].tolist() == [1, -1, 0, 0] and got[1, 0, 0, :2].tolist() == [2, -2]


def test_the_cases_reach_what_they_are_there_for():
    c = ref.cases()
    assert {(img.shape[1], img.shape[0]) for img, _ in c.values()} >= set(ref.SMALL + ref.LARGE)
    assert 3 * 33 * 3 == 297 > 256                                                       # 264 x 24: a prediction crosses the coder's workgroup
    assert set(np.unique(c["translucent_17x23"][0][..., 3])) == {0, 1, 128, 254, 255}
    runs = ref.ref("runs_gray", c["runs_gray"][1][0]).hist
    assert runs[1, 0xF0] >= 3, "the luminance scan codes ZRLs"
    ac = ref.ref("ac_gray_q100", 100).hist
    assert all(ac[1, (run << 4) | 10] > 0 for run in (0, 5, 15)), "AC values of size 10"
    # the padding is to 8: a 17 x 23 image has 3 x 3 MCUs of three blocks
    assert ref.ref("noise_17x23", 75).coef.shape == (27, 64)


def test_the_header_differs_from_420s_in_one_byte():
    r = ref.ref("noise_17x23", 75)
    n = len(r.header)
    diff = [i for i in range(n) if r.header[i] != r.std_420[i]]
    assert len(diff) == 1 and (r.std_420[diff[0]], r.header[diff[0]]) == (0x22, 0x11)
