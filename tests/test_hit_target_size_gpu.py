"""fnx_hit_target_size and fennec_CompressFileHitTargetSize on the GPU: all of hitTargetSize (targetsize.go:26-75) in one call.
Format JPEG is fnx_jpeg_target_size with all four bits, format PNG is fnx_png_target_size with all three (both pinned by their
own tests), Auto lets the source's opacity pick the legs and betterFit pick the winner; the file entry is its staging followed
by the call on the staged image."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
import png_filter_ref as pref
import png_target_ref as ptr
from fennec_amd import (FNX_FORMAT_AUTO, FNX_FORMAT_JPEG, FNX_FORMAT_PNG, FNX_TS_ALL, FNX_TS_FALLBACK, FNX_TS_FALLBACK_PNG, FNX_TS_PNG_ALL,
                        FNX_TS_QUALITY, FNX_TS_QUALITY_SCALE, FNX_TS_QUANTIZE, FNX_TS_SCALE, FNX_TS_SCALE_PNG, synth)
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

JPEG_BITS = (FNX_TS_QUALITY, FNX_TS_QUALITY_SCALE, FNX_TS_SCALE, FNX_TS_FALLBACK)
EMPTY = dict(strategy=0, quality=0, final_w=0, final_h=0, steps=0, nbytes=0, ssim=0.0)


@pytest.fixture(scope="module")
def ctx():
    c = fennec_amd.Context(0)
    c.set_deflate_level("dense")
    return c


@pytest.fixture(scope="module")
def opaque():
    return orc.gaussian_blur(synth.noise_image(96, 80, 1), 2.0)


@pytest.fixture(scope="module")
def translucent():
    img = orc.gaussian_blur(synth.noise_image(64, 48, 2), 2.0).copy()
    img[20, 30, 3] = 254
    return img


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def replay_better_fit(cands, target):
    win = None
    for i, c in enumerate(cands):
        if c["strategy"] and (win is None or ptr.better_fit(c, cands[win], target)):
            win = i
    return win


def same_call(got, want, at):
    """got: hit_target_size's answer; want: the sub-entry's, whose candidate k is hit_target_size's candidate at[k]"""
    for k, i in enumerate(at):
        assert got["candidates"][i] == want["candidates"][k], (i, got["candidates"][i], want["candidates"][k])
    for i in range(5):
        if i not in at:
            assert got["candidates"][i] == EMPTY
    assert got["status"] == want["status"]
    assert got["winner"] == (None if want["winner"] is None else at[want["winner"]])
    assert got["data"] == want["data"]
    if want["winner"] is not None:
        assert np.array_equal(host(got["image"]), host(want["image"]))


@pytest.mark.parametrize("target", [1 << 20, 2500, 900, 1])
def test_format_jpeg_is_the_jpeg_entry_with_all_four_bits(ctx, opaque, translucent, target):
    for img in (opaque, translucent):                                # wantJPEG: the JPEG legs also for a translucent source
        want = ctx.jpeg_target_size(img, target, FNX_TS_ALL)
        got = ctx.hit_target_size(img, target, FNX_FORMAT_JPEG)
        same_call(got, want, (0, 2, 3, 4))
        print(f"target {target}: winner {got['winner']}, strategies {[c['strategy'] for c in got['candidates']]}")


@pytest.mark.parametrize("target", [1 << 20, 4000, 300, 1])
def test_format_png_is_the_png_entry_with_all_three_bits(ctx, opaque, target):
    import torch
    want = ctx.png_target_size(opaque, target, FNX_TS_PNG_ALL)
    got = ctx.hit_target_size(opaque, target, FNX_FORMAT_PNG)
    same_call(got, want, (1, 3, 4))
    dev = ctx.hit_target_size(torch.from_numpy(opaque).cuda(), target, FNX_FORMAT_PNG)
    assert dev["candidates"] == got["candidates"] and dev["data"] == got["data"] and dev["winner"] == got["winner"]
    print(f"target {target}: winner {got['winner']}, strategies {[c['strategy'] for c in got['candidates']]}")


def test_auto_on_an_opaque_image_with_a_generous_target(ctx, opaque):
    target = 1 << 20
    got = ctx.hit_target_size(opaque, target, FNX_FORMAT_AUTO)
    cands = got["candidates"]
    print(cands)
    assert [c["strategy"] for c in cands] == [FNX_TS_QUALITY, FNX_TS_QUANTIZE, FNX_TS_QUALITY_SCALE, 0, 0], "three candidates"
    # each leg is its own entry's leg
    jpeg = ctx.jpeg_target_size(opaque, target, FNX_TS_QUALITY | FNX_TS_QUALITY_SCALE)["candidates"]
    png = ctx.png_target_size(opaque, target, FNX_TS_QUANTIZE)["candidates"]
    assert cands[0] == jpeg[0] and cands[2] == jpeg[1] and cands[1] == png[0]
    win = replay_better_fit(cands, target)
    assert got["winner"] == win and got["status"] == fennec_amd.FNX_OK
    # the output's format is read off the winner's strategy bit
    is_png = bool(cands[win]["strategy"] & FNX_TS_PNG_ALL)
    assert (got["data"][:8] == b"\x89PNG\r\n\x1a\n") == is_png and (got["data"][:2] == b"\xff\xd8") == (not is_png)
    assert len(got["data"]) == cands[win]["nbytes"]
    again = ctx.hit_target_size(opaque, target, FNX_FORMAT_AUTO)
    assert again["candidates"] == cands and again["data"] == got["data"]


@pytest.mark.parametrize("target", [1 << 20, 300, 1])
def test_auto_on_an_opaque_image_is_betterfit_over_its_legs(ctx, opaque, target):
    got = ctx.hit_target_size(opaque, target, FNX_FORMAT_AUTO)
    cands = got["candidates"]
    # canUseJPEG: strategy 4 and the fallback are the JPEG ones
    assert cands[3]["strategy"] in (0, FNX_TS_SCALE) and cands[4]["strategy"] in (0, FNX_TS_FALLBACK)
    assert got["winner"] == replay_better_fit(cands, target)
    if not any(c["strategy"] for c in cands[:3]):
        want = ctx.jpeg_target_size(opaque, target, FNX_TS_SCALE | FNX_TS_FALLBACK)
        assert cands[3] == want["candidates"][2] and cands[4] == want["candidates"][3] and got["data"] == want["data"]


@pytest.mark.parametrize("target", [1 << 20, 300, 1])
def test_auto_on_a_translucent_image_runs_no_jpeg_leg(ctx, translucent, target):
    got = ctx.hit_target_size(translucent, target, FNX_FORMAT_AUTO)
    cands = got["candidates"]
    print(f"target {target}: {[c['strategy'] for c in cands]}")
    assert cands[0] == EMPTY and cands[2] == EMPTY
    assert not any(c["strategy"] in JPEG_BITS for c in cands), "no JPEG leg has strategy != 0"
    same_call(got, ctx.png_target_size(translucent, target, FNX_TS_PNG_ALL), (1, 3, 4))
    assert got["data"][:8] == b"\x89PNG\r\n\x1a\n"
    if cands[got["winner"]]["strategy"] != FNX_TS_FALLBACK_PNG:
        assert np.array_equal(pref.decode_png(got["data"]), host(got["image"]))


def test_the_old_entry_still_refuses_the_new_bits(ctx, opaque):
    for bits in (FNX_TS_QUANTIZE, FNX_TS_ALL | FNX_TS_SCALE_PNG, FNX_TS_FALLBACK_PNG):
        with pytest.raises(fennec_amd.FennecError, match="strategies"):
            ctx.jpeg_target_size(opaque, 1000, bits)
    lib = fennec_amd.load_library()
    _, pk = fennec_amd._f64(ctx.gaussianKernel())
    cand = (fennec_amd.SizeCandidate * 4)()
    win, n = C.c_int(7), C.c_size_t(7)
    rc = lib.fnx_jpeg_target_size(ctx._h, fennec_amd.FNX_HOST, opaque.ctypes.data, opaque.strides[0], 96, 80, 1000, FNX_TS_ALL | FNX_TS_QUANTIZE, pk, None,
                                  cand, C.byref(win), None, 0, C.byref(n), None, 0)
    assert rc == fennec_amd.FNX_ERR_INVALID and "strategies" in lib.fnx_last_error().decode() and (win.value, n.value) == (7, 7)


# ---- the file entry -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sources(ctx):
    jpg = ctx.jpeg_encode(synth.large_photo(160, 120, 3), 90)
    rgba = synth.large_photo(96, 64, 4).copy()
    rgba[5, 7, 3] = 100                                              # a translucent PNG source: Auto takes the PNG legs
    png = ctx.png_encode(rgba)
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and jpg[:2] == b"\xff\xd8"
    return {"jpeg": jpg, "png": png}


@pytest.mark.parametrize("fmt", [FNX_FORMAT_AUTO, FNX_FORMAT_JPEG, FNX_FORMAT_PNG])
@pytest.mark.parametrize("kind", ["jpeg", "png"])
def test_file_entry_is_its_staging_and_the_call(ctx, sources, kind, fmt):
    data = sources[kind]
    img = ctx.jpeg_decode(data) if kind == "jpeg" else ctx.png_decode(data, "host")
    img = np.ascontiguousarray(ctx.ApplyOrientation(img, 6))
    original = (img.shape[1], img.shape[0])
    img = np.ascontiguousarray(ctx.smartResize(img, 64, 0))
    assert original == ((120, 160) if kind == "jpeg" else (64, 96)) and img.shape[1] == 64
    for target in (1 << 20, 1500, 10):
        want = ctx.hit_target_size(img, target, fmt)
        got = ctx.compress_file_hit_target_size(data, target, fmt, orient=6, max_w=64)
        assert got["candidates"] == want["candidates"]
        assert got["winner"] == want["winner"] and got["status"] == want["status"] and got["data"] == want["data"]
        c = want["candidates"][want["winner"]]
        assert got["dims"] == (original, (c["final_w"], c["final_h"]))
        print(f"{kind} format {fmt} target {target}: winner {got['winner']} strategies {[c['strategy'] for c in got['candidates']]}")
        if fmt == FNX_FORMAT_AUTO:                                    # the staged image's opacity picks the legs
            assert orc.is_opaque(img) == (kind == "jpeg")
            assert any(c["strategy"] in JPEG_BITS for c in got["candidates"]) == (kind == "jpeg")
        if fmt == FNX_FORMAT_JPEG:
            old = ctx.compress_file_target_size(data, target, orient=6, max_w=64)
            assert [got["candidates"][i] for i in (0, 2, 3, 4)] == old["candidates"] and got["data"] == old["data"]
