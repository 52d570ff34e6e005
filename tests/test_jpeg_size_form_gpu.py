"""The "jpeg_size" form (fnx_ctx_set_form): a size-only JPEG query answered from the blocks' strips in one wait
(jpeg_ffcount_strips_kernel, "1") against the packed and stuffed string (jpeg_pack_kernel ..., "0").  Both must give the
oracle's file length for every quality, on images chosen for the byte-ownership rule: minimal blocks (every byte of the
string straddles blocks), MCU padding, dense noise at quality 100 (stuffed 0xff bytes), a translucent half."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
from fennec_amd import FNX_TS_ALL, synth
from oracle import oracle as orc

PROF_JPEG = 16
ONE_WAIT, TWO_STEP = "jpeg_ffcount_strips_kernel", "jpeg_pack_kernel"


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def _translucent_half():
    img = synth.noise_image(33, 31, 9)
    img[:, 16:, 3] = synth.noise_image(33, 31, 10)[:, 16:, 0]
    return np.ascontiguousarray(img)


IMAGES = {
    "flat_8x8": lambda: synth.make_solid_image(8, 8, (90, 160, 30, 255)),
    "padded_17x9": lambda: synth.noise_image(17, 9, 4),
    "flat_colour_64x64": lambda: synth.make_solid_image(64, 64, (200, 40, 120, 255)),
    "noise_48x32": lambda: synth.noise_image(48, 32, 7),
    "translucent_half_33x31": _translucent_half,
}


@pytest.fixture(scope="module")
def oracle_sizes():
    """len(jpeg.Encode(img, q)) of every image and quality, computed once"""
    return {name: [len(orc.jpeg_encode(np.ascontiguousarray(make()), q)) for q in range(1, 101)] for name, make in IMAGES.items()}


def _scan(data: bytes) -> bytes:
    """the entropy-coded segment of a baseline file: behind the SOS header, in front of EOI"""
    i = 2
    while True:
        assert data[i] == 0xff
        length = int.from_bytes(data[i + 2:i + 4], "big")
        if data[i + 1] == 0xda:
            return data[i + 2 + length:-2]
        i += 2 + length


def test_the_noise_at_quality_100_has_stuffed_bytes():
    orc.build()
    scan = _scan(orc.jpeg_encode(IMAGES["noise_48x32"](), 100))
    assert scan.count(b"\xff\x00") >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_size_query_is_the_oracle_length_under_both_forms(ctx, oracle_sizes, name):
    img = np.ascontiguousarray(IMAGES[name]())
    want = oracle_sizes[name]
    got = {}
    for form, kernel in (("1", ONE_WAIT), ("0", TWO_STEP)):
        with ctx.forms(jpeg_size=form):
            got[form] = [ctx.jpeg_encoded_size(img, q) for q in range(1, 101)]
            assert ctx.last_kernel(PROF_JPEG) == kernel, form
    assert got["1"] == got["0"], [(q + 1, a, b) for q, (a, b) in enumerate(zip(got["1"], got["0"])) if a != b]
    assert got["1"] == want, [(q + 1, a, b) for q, (a, b) in enumerate(zip(got["1"], want)) if a != b]


@pytest.mark.gpu
def test_the_form_is_opt_in(ctx):
    img = IMAGES["noise_48x32"]()
    ctx.set_form("jpeg_size", None)
    assert ctx.jpeg_encoded_size(img, 100) == len(orc.jpeg_encode(img, 100)) and ctx.last_kernel(PROF_JPEG) == TWO_STEP
    fresh = fennec_amd.Context(0)
    assert fresh.last_kernel(PROF_JPEG) == ""
    assert fresh.jpeg_encoded_size(img, 100) == len(orc.jpeg_encode(img, 100)) and fresh.last_kernel(PROF_JPEG) == TWO_STEP
    fresh.close()


@pytest.mark.gpu
def test_files_keep_the_two_step_route_and_their_bytes(ctx):
    img = IMAGES["noise_48x32"]()
    for q in (1, 50, 100):
        with ctx.forms(jpeg_size="1"):
            data = ctx.jpeg_encode(img, q)
            assert ctx.last_kernel(PROF_JPEG) == TWO_STEP
            assert ctx.jpeg_encoded_size(img, q) == len(data) and ctx.last_kernel(PROF_JPEG) == ONE_WAIT
        assert data == orc.jpeg_encode(img, q)


@pytest.mark.gpu
def test_scaled_size_query_and_device_sources(ctx):
    import torch
    img = synth.large_photo(160, 120, 5)
    dev = torch.from_numpy(img).cuda()
    for dw, dh, q in ((159, 119, 90), (80, 60, 50), (25, 18, 20), (1, 1, 100)):
        want = len(orc.jpeg_encode(orc.box_downsample(img, dw, dh), q))
        for form, kernel in (("1", ONE_WAIT), ("0", TWO_STEP)):
            with ctx.forms(jpeg_size=form):
                assert ctx.jpeg_encode_scaled(img, dw, dh, q, size_only=True) == want, (dw, dh, q, form)
                assert ctx.jpeg_encode_scaled(dev, dw, dh, q, size_only=True) == want, (dw, dh, q, form)
                assert ctx.last_kernel(PROF_JPEG) == kernel


@pytest.mark.gpu
def test_more_than_one_workgroup_and_wave(ctx):
    """640 x 480: 7200 blocks, 29 workgroups -- the last workgroup's hand-over and the counters it puts back, call after call"""
    img = synth.noise_image(640, 480, 3)
    for q in (100, 97, 100, 35):
        want = len(orc.jpeg_encode(img, q))
        with ctx.forms(jpeg_size="1"):
            assert [ctx.jpeg_encoded_size(img, q) for _ in range(3)] == [want] * 3, q
        with ctx.forms(jpeg_size="0"):
            assert ctx.jpeg_encoded_size(img, q) == want, q


@pytest.mark.gpu
def test_target_size_is_the_same_under_both_forms(ctx):
    """a photo-like 160 x 120 source; the targets reach strategy 1, strategy 3, strategy 4 (its encode at bestQ) and the fallback"""
    img = synth.large_photo(160, 120, 5)
    winners = []
    for target in (12107, 3026, 690, 10):
        with ctx.forms(jpeg_size="1"):
            a = ctx.jpeg_target_size(img, target, FNX_TS_ALL)
        with ctx.forms(jpeg_size="0"):
            b = ctx.jpeg_target_size(img, target, FNX_TS_ALL)
        assert a["candidates"] == b["candidates"] and a["winner"] == b["winner"] and a["data"] == b["data"], target
        assert a["data"] == orc.jpeg_encode(np.ascontiguousarray(a["image"]), a["candidates"][a["winner"]]["quality"]), target
        winners.append(a["winner"])
    assert winners[0] != winners[1] and 3 not in winners[:2] and winners[3] == 3, winners


@pytest.mark.gpu
def test_the_form_takes_values_as_the_other_names_do(ctx):
    L = ctx._lib
    for name in (b"jpeg_size", b"resize_box"):
        assert L.fnx_ctx_set_form(ctx._h, name, b"1") == fennec_amd.FNX_OK
        assert L.fnx_ctx_set_form(ctx._h, name, b"other") == fennec_amd.FNX_OK           # values are not policed, only their length
        assert L.fnx_ctx_set_form(ctx._h, name, b"12345678") == fennec_amd.FNX_ERR_INVALID
        assert L.fnx_ctx_set_form(ctx._h, name, None) == fennec_amd.FNX_OK
    assert L.fnx_ctx_set_form(ctx._h, b"jpeg_sizes", b"1") == fennec_amd.FNX_ERR_INVALID
