"""fnx_png_target_size on the GPU: hitTargetSize's PNG legs (quantize, scale with format PNG, the PNG fallback) against the
restatement of png_target_ref -- the reference's control flow over the oracle's pixel steps and the single route's files on the
same context.  The targets are derived here from the image's five measured level sizes; nothing is written down in advance."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
import png_filter_ref as pref
import png_target_ref as ptr
from fennec_amd import (FNX_TS_FALLBACK_PNG, FNX_TS_PNG_ALL, FNX_TS_QUANTIZE, FNX_TS_SCALE_PNG, synth)
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


def blurred_noise(w, h, seed):
    return orc.gaussian_blur(synth.noise_image(w, h, seed), 2.0)


def flat_colours():
    """40 x 40, twelve flat colours in blocks of 10 x 14 (the last row of blocks 10 x 12)"""
    rng = np.random.default_rng(12)
    colours = rng.integers(0, 256, size=(12, 4), dtype=np.uint8)
    colours[:, 3] = 255
    img = np.empty((40, 40, 4), np.uint8)
    for y in range(40):
        for x in range(40):
            img[y, x] = colours[(y // 14) * 4 + x // 10]
    return img


def one_translucent_pixel():
    img = blurred_noise(64, 48, 2).copy()
    img[20, 30, 3] = 254
    return img


IMAGES = {
    "noise_96x80": lambda: blurred_noise(96, 80, 1),
    "noise_64x48": lambda: blurred_noise(64, 48, 2),
    "alpha254_64x48": one_translucent_pixel,
    "flat12_40x40": flat_colours,
    "noise_9x7": lambda: blurred_noise(9, 7, 3),
}
_LEGS = {}


@pytest.fixture(scope="module")
def ctxs():
    fast, dense = fennec_amd.Context(0), fennec_amd.Context(0)
    dense.set_deflate_level("dense")
    return {"fast": fast, "dense": dense}


def legs(ctxs, level, name):
    """the restatement's images and files of one image on one context: made once, shared by every test"""
    if (level, name) not in _LEGS:
        img = IMAGES[name]()
        assert img.flags.c_contiguous and img.shape[2] == 4
        _LEGS[level, name] = ptr.PngLegs(ctxs[level], img)
    return _LEGS[level, name]


def host(x):
    return x.cpu().numpy() if hasattr(x, "cpu") else x


def composed_ssim(ctx, src, image):
    """computeSSIMNRGBA through the library's own separate calls: the prepared source, lanczosResize, SSIMFast against it"""
    h, w = src.shape[:2]
    if image.shape[:2] != (h, w):
        image = host(ctx.lanczosResize(np.ascontiguousarray(image), w, h))
    p = ctx.ssim_fast_prepare(src)
    try:
        return p.against(np.ascontiguousarray(image))
    finally:
        p.close()


def check(ctx, lg: ptr.PngLegs, target, strategies, device=False):
    import torch
    src = lg.src
    arg = torch.from_numpy(src).cuda() if device else src
    got = ctx.png_target_size(arg, target, strategies)
    cands, win, image, file = ptr.restate(lg, target, strategies)
    for g, w in zip(got["candidates"], cands):
        print(f"target {target} strategies {strategies}: got {g} want {w}")
        assert {k: g[k] for k in w if k != "ssim"} == {k: w[k] for k in w if k != "ssim"}
        assert abs(g["ssim"] - w["ssim"]) <= 1e-9
    assert got["winner"] == win
    if win is None:
        assert got["status"] == fennec_amd.FNX_NOOP and got["data"] is None
        return got
    assert got["status"] == fennec_amd.FNX_OK
    assert got["data"] == file, "the single route's file, byte for byte"
    gi = host(got["image"])
    assert np.array_equal(gi, image), "img is the winner's image"
    c = cands[win]
    if c["strategy"] == FNX_TS_FALLBACK_PNG:
        assert got["candidates"][win]["ssim"] == 1.0
    else:
        assert np.array_equal(pref.decode_png(got["data"]), image), "the file decodes to the winner's image"
        assert got["candidates"][win]["ssim"] == composed_ssim(ctx, src, image), "== the composed device calls"
    return got


def strict_first_fits(sizes):
    """the levels (indices into LEVELS) that some target makes the FIRST fit of the walk from 256 down: smaller than every level above"""
    return [l for l in range(5) if all(sizes[l] < sizes[k] for k in range(l + 1, 5))]


@pytest.mark.parametrize("level", ["fast", "dense"])
@pytest.mark.parametrize("name", ["noise_96x80", "noise_64x48", "alpha254_64x48", "flat12_40x40", "noise_9x7"])
def test_targets_from_the_measured_level_sizes(ctxs, level, name):
    ctx, lg = ctxs[level], legs(ctxs, level, name)
    sizes = lg.level_sizes()
    firsts = strict_first_fits(sizes)
    print(f"{level} {name}: level sizes s16..s256 {sizes}, colours {[len(p) for p in lg.palettes()]}, strict first fits {firsts}")
    assert 4 in firsts
    if name == "noise_96x80":
        assert len(firsts) >= 3, "the test's precondition: at least three levels are strict first fits"
    for l in firsts:                                                  # one target per level that is a strict first fit
        got = check(ctx, lg, sizes[l], FNX_TS_PNG_ALL)
        assert got["winner"] == 0 and got["candidates"][0]["nbytes"] == sizes[l]
        assert pref.chunks(got["data"])[1][0] == b"PLTE" and len(pref.chunks(got["data"])[1][1]) == 3 * len(lg.palettes()[l])
    smallest = min(sizes)
    # under every level: quantize alone finds nothing; with all three bits the scale leg answers
    got = check(ctx, lg, smallest - 1, FNX_TS_QUANTIZE)
    assert got["status"] == fennec_amd.FNX_NOOP and got["candidates"][0]["steps"] == len(set(len(p) for p in lg.palettes()))
    got = check(ctx, lg, smallest - 1, FNX_TS_PNG_ALL)
    assert got["candidates"][1]["strategy"] == FNX_TS_SCALE_PNG and got["winner"] == 1
    # one byte: no scale fits, the fallback answers over the target
    got = check(ctx, lg, 1, FNX_TS_PNG_ALL)
    assert [c["strategy"] for c in got["candidates"]] == [0, 0, FNX_TS_FALLBACK_PNG] and got["candidates"][2]["nbytes"] > 1
    if name == "noise_9x7":
        assert got["candidates"][1]["steps"] < 12, "the bisection's skip branch: a step whose scaled image has no pixels runs no query"
    else:
        assert got["candidates"][1]["steps"] == 12
    # a huge target: level 256
    got = check(ctx, lg, 1 << 30, FNX_TS_PNG_ALL)
    assert got["candidates"][0]["nbytes"] == sizes[4] and got["candidates"][0]["steps"] == 1


@pytest.mark.parametrize("name", ["noise_64x48", "alpha254_64x48"])
def test_host_and_device_sources_and_a_second_call(ctxs, name):
    ctx, lg = ctxs["dense"], legs(ctxs, "dense", name)
    sizes = lg.level_sizes()
    for target, strategies in ((sizes[2], FNX_TS_PNG_ALL), (min(sizes) - 1, FNX_TS_SCALE_PNG), (1, FNX_TS_FALLBACK_PNG)):
        a = check(ctx, lg, target, strategies)
        b = check(ctx, lg, target, strategies, device=True)
        c = check(ctx, lg, target, strategies)
        assert a["data"] == b["data"] == c["data"]
        assert a["candidates"] == b["candidates"] == c["candidates"]


def test_the_deflate_level_decides_between_the_two_s256(ctxs):
    fast, dense = legs(ctxs, "fast", "noise_96x80"), legs(ctxs, "dense", "noise_96x80")
    f256, d256 = fast.level_sizes()[4], dense.level_sizes()[4]
    print(f"s256: fast {f256}, dense {d256}")
    assert d256 < f256, "the test's precondition: the dense level's file of the 256-colour level is the smaller one"
    target = f256 - 1                                                 # between the two: fits the dense file, not the fast one
    a = check(ctxs["fast"], fast, target, FNX_TS_PNG_ALL)
    b = check(ctxs["dense"], dense, target, FNX_TS_PNG_ALL)
    assert b["candidates"][0]["nbytes"] == d256
    na = len(pref.chunks(a["data"])[1][1]) // 3 if a["candidates"][0]["strategy"] else 0
    assert na < len(pref.chunks(b["data"])[1][1]) // 3 == len(dense.palettes()[4]), "the fast level picks a lower level"


def test_cancelled_before_the_call(ctxs):
    ctx, lg = ctxs["fast"], legs(ctxs, "fast", "noise_64x48")
    cancel = C.c_int(1)
    got = ctx.png_target_size(lg.src, 1 << 30, FNX_TS_PNG_ALL, cancel=cancel)
    cands, win, image, file = ptr.restate(lg, 1 << 30, FNX_TS_PNG_ALL, cancelled=True)
    assert [c["strategy"] for c in cands] == [0, 0, FNX_TS_FALLBACK_PNG] and win == 2
    assert [{k: v for k, v in g.items() if k in w} for g, w in zip(got["candidates"], cands)] == cands
    assert got["winner"] == 2 and got["data"] == file
    assert ctx.png_target_size(lg.src, 1 << 30, FNX_TS_QUANTIZE | FNX_TS_SCALE_PNG, cancel=cancel)["status"] == fennec_amd.FNX_NOOP


def test_cap_too_small(ctxs):
    """fnx_jpeg_target_size's protocol: FNX_ERR_INVALID with *nbytes, cand and *winner filled, nothing written; the size alone with out == NULL"""
    ctx, lg = ctxs["fast"], legs(ctxs, "fast", "noise_64x48")
    lib = fennec_amd.load_library()
    src = lg.src
    file = lg.fallback()
    win_k, pk = fennec_amd._f64(ctx.gaussianKernel())
    cand = (fennec_amd.SizeCandidate * 3)()
    win, n = C.c_int(-1), C.c_size_t(0)
    out = np.full(len(file) + 16, 0xAB, np.uint8)
    args = (ctx._h, fennec_amd.FNX_HOST, src.ctypes.data, src.strides[0], 64, 48, 1, FNX_TS_PNG_ALL, pk, None, cand, C.byref(win))
    assert lib.fnx_png_target_size(*args, out.ctypes.data_as(fennec_amd._u8p), len(file) - 1, C.byref(n), None, 0) == fennec_amd.FNX_ERR_INVALID
    assert n.value == len(file) and win.value == 2 and cand[2].strategy == FNX_TS_FALLBACK_PNG and cand[2].nbytes == len(file)
    assert (out == 0xAB).all()
    assert lib.fnx_png_target_size(*args, None, 0, C.byref(n), None, 0) == fennec_amd.FNX_OK
    assert n.value == len(file) and win.value == 2
    assert lib.fnx_png_target_size(*args, out.ctypes.data_as(fennec_amd._u8p), len(out), C.byref(n), None, 0) == fennec_amd.FNX_OK
    assert out[:n.value].tobytes() == file and (out[n.value:] == 0xAB).all()
