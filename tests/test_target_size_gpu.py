"""Target-size mode's JPEG legs on the device: fnx_jpeg_encode_scaled (jpeg.Encode of boxDownsample without the scaled
image) and fnx_jpeg_target_size (hitTargetSize's strategies 1, 3, 4 and the JPEG fallback, targetsize.go:26-357) against
a restatement of the reference's control flow built from the CPU oracle's primitives."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
from fennec_amd import FNX_TS_ALL, FNX_TS_FALLBACK, FNX_TS_QUALITY, FNX_TS_QUALITY_SCALE, FNX_TS_SCALE, synth
from oracle import oracle as orc

MIN_Q = 20      # minJPEGQuality (targetsize.go:14)


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def _blurred_noise(w, h, seed):
    return orc.gaussian_blur(synth.noise_image(w, h, seed), 2.0)


# ---- the restatement ---------------------------------------------------------------------------------------------
class Sizes:
    """len(jpeg.Encode(...)) of the source, its boxDownsample'd and its Lanczos-resized copies, memoised by (kind, dims,
    quality).  device=ctx: the sizes come from the device's encoder (pinned against the oracle by the tests of
    fnx_jpeg_encode_scaled below and of fnx_jpeg_encode elsewhere) -- for 4K sources, whose oracle encodes are slow."""

    def __init__(self, src, device=None):
        self.src, self.device = src, device
        self.memo, self.imgs = {}, {}

    def image(self, kind, w, h):
        key = (kind, w, h)
        if key not in self.imgs:
            if kind == "src":
                self.imgs[key] = self.src
            elif kind == "box":
                self.imgs[key] = orc.box_downsample(self.src, w, h)
            else:
                self.imgs[key] = orc.lanczos_resize(self.src, w, h, procs=8)
        return self.imgs[key]

    def size(self, kind, w, h, q):
        key = (kind, w, h, q)
        if key not in self.memo:
            if self.device is not None and kind == "box":
                self.memo[key] = self.device.jpeg_encode_scaled(self.src, w, h, q, size_only=True)
            elif self.device is not None:
                self.memo[key] = self.device.jpeg_encoded_size(self.image(kind, w, h), q)
            else:
                self.memo[key] = len(orc.jpeg_encode(self.image(kind, w, h), q))
        return self.memo[key]


def _bisect(size_of, w, h, target):
    """jpegQualitySearchOpt's bisection (targetsize.go:129-165) -> (quality or 0, its size, encodes)."""
    bpp = float(target * 8) / float(w * h)
    lo, hi = 1, 100
    if bpp < 0.5:
        hi = 40
    elif bpp < 1.0:
        lo, hi = 10, 70
    elif bpp < 2.0:
        lo, hi = 30, 90
    elif bpp > 4.0:
        lo = 60
    q, sz, n = 0, 0, 0
    while lo <= hi:
        mid = (lo + hi) // 2
        s = size_of(mid)
        n += 1
        if s <= target:
            q, sz, lo = mid, s, mid + 1
        else:
            hi = mid - 1
    return q, sz, n


def _ssim_nrgba(src, img):
    """computeSSIMNRGBA (targetsize.go:534-539)."""
    h, w = src.shape[:2]
    if img.shape[:2] != (h, w):
        img = orc.lanczos_resize(img, w, h, procs=8)
    return orc.ssim_fast(src, img, procs=8)


def _empty():
    return dict(strategy=0, quality=0, final_w=0, final_h=0, steps=0, nbytes=0, ssim=0.0)


def _better_fit(c, b, t):
    """betterFit (targetsize.go:92-115)."""
    cu, bu = c["nbytes"] <= t, b["nbytes"] <= t
    if cu and not bu:
        return True
    if not cu and bu:
        return False
    if cu and bu:
        if c["ssim"] != b["ssim"]:
            return c["ssim"] > b["ssim"]
        return c["quality"] > b["quality"]
    return c["nbytes"] < b["nbytes"]


def restate(sz: Sizes, target, strategies, cancelled=False):
    """hitTargetSize's JPEG legs (targetsize.go:26-90, 117-357) -> (candidates, winner index or None, winner's image)."""
    src = sz.src
    h, w = src.shape[:2]
    cands = [_empty() for _ in range(4)]
    scaled = None
    if strategies & FNX_TS_QUALITY and not cancelled:                      # strategy 1
        q, n_bytes, n = _bisect(lambda q: sz.size("src", w, h, q), w, h, target)
        cands[0]["steps"] = n
        if q >= MIN_Q:
            cands[0].update(strategy=FNX_TS_QUALITY, quality=q, final_w=w, final_h=h, nbytes=n_bytes,
                            ssim=orc.ssim_fast(src, orc.jpeg_roundtrip(src, q), procs=8))
    if strategies & FNX_TS_QUALITY_SCALE and not cancelled:                # strategy 3
        n, best = 0, None

        def fits(nw, nh):
            nonlocal n
            q, s, k = _bisect(lambda q: sz.size("box", nw, nh, q), nw, nh, target)
            n += k
            return q != 0 and s <= target and q >= MIN_Q

        lo, hi = 0.05, 1.0
        for _ in range(10):
            mid = (lo + hi) / 2
            nw, nh = int(float(w) * mid), int(float(h) * mid)
            if nw < 8 or nh < 8:
                lo = mid
                continue
            if fits(nw, nh):
                best, lo = mid, mid
            else:
                hi = mid
        for scale in (0.75, 0.50, 0.375, 0.25):
            nw, nh = int(float(w) * scale), int(float(h) * scale)
            if nw < 8 or nh < 8:
                continue
            if fits(nw, nh) and (best is None or scale > best):
                best = scale
        cands[1]["steps"] = n
        if best is not None:
            fw, fh = int(float(w) * best), int(float(h) * best)
            q, s, k = _bisect(lambda q: sz.size("lanczos", fw, fh, q), fw, fh, target)
            n += k
            cands[1]["steps"] = n
            if q >= MIN_Q:
                scaled = sz.image("lanczos", fw, fh)
                cands[1].update(strategy=FNX_TS_QUALITY_SCALE, quality=q, final_w=fw, final_h=fh, nbytes=s,
                                ssim=_ssim_nrgba(src, scaled))
    none = not any(c["strategy"] for c in cands)
    if strategies & FNX_TS_SCALE and none and not cancelled:               # strategy 4
        n, best, best_q = 0, 0.0, 0
        lo, hi = 0.05, 1.0
        for _ in range(12):
            mid = (lo + hi) / 2
            nw, nh = int(float(w) * mid), int(float(h) * mid)
            if nw < 1 or nh < 1:
                lo = mid
                continue
            q, s, k = _bisect(lambda q: sz.size("box", nw, nh, q), nw, nh, target)
            n += k
            if q != 0 and s <= target and q >= MIN_Q:
                best, best_q, lo = mid, q, mid
            else:
                hi = mid
        cands[2]["steps"] = n
        if best != 0.0:
            fw, fh = int(float(w) * best), int(float(h) * best)
            q, s, k = _bisect(lambda q: sz.size("lanczos", fw, fh, q), fw, fh, target)
            n += k
            if q == 0:
                q, s = best_q, sz.size("lanczos", fw, fh, best_q)
                n += 1
            scaled = sz.image("lanczos", fw, fh)
            cands[2].update(strategy=FNX_TS_SCALE, quality=q, final_w=fw, final_h=fh, steps=n, nbytes=s,
                            ssim=_ssim_nrgba(src, scaled))
    if strategies & FNX_TS_FALLBACK and not any(c["strategy"] for c in cands):   # fallbackTargetSizeEncode
        cands[3].update(strategy=FNX_TS_FALLBACK, quality=1, final_w=w, final_h=h, steps=1, nbytes=sz.size("src", w, h, 1),
                        ssim=orc.ssim_fast(src, src, procs=8))
    win = None
    for i, c in enumerate(cands):
        if c["strategy"] and (win is None or _better_fit(c, cands[win], target)):
            win = i
    image = None if win is None else (scaled if win in (1, 2) else src)
    return cands, win, image


def _check(ctx, img, target, strategies, sz: Sizes, file_check=True):
    got = ctx.jpeg_target_size(img, target, strategies)
    cands, win, image = restate(sz, target, strategies)
    for g, w in zip(got["candidates"], cands):
        assert {k: g[k] for k in w if k != "ssim"} == {k: w[k] for k in w if k != "ssim"}, (target, strategies, g, w)
        assert abs(g["ssim"] - w["ssim"]) <= 1e-9, (target, strategies, g, w)
    assert got["winner"] == win, (target, strategies)
    if win is None:
        assert got["status"] == fennec_amd.FNX_NOOP and got["data"] is None
        return got
    c = cands[win]
    assert len(got["data"]) == c["nbytes"]
    gi = got["image"]
    gi = gi.cpu().numpy() if hasattr(gi, "cpu") else gi
    assert np.array_equal(gi, image), (target, strategies, win)
    if file_check:
        assert got["data"] == orc.jpeg_encode(image, c["quality"]), (target, strategies, win)
    return got


# ---- fnx_jpeg_encode_scaled --------------------------------------------------------------------------------------
SCALES = (0.97, 0.75, 0.5, 0.375, 0.26, 0.05)
QUALITIES = (1, 20, 50, 90, 100)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,kind", [(640, 480, "photo"), (1280, 720, "photo"), (333, 217, "noise"), (640, 480, "alpha"),
                                      (333, 217, "alpha_test")])
def test_encode_scaled_is_the_oracle_file_of_the_box_downsample(ctx, w, h, kind):
    import torch
    if kind == "photo":
        img = synth.large_photo(w, h, 2)
    elif kind == "noise":
        img = _blurred_noise(w, h, 3)
    elif kind == "alpha":
        img = synth.noise_image(w, h, 5, alpha=True)
    else:
        img = np.ascontiguousarray(synth.make_test_image_with_alpha(w, h))
    assert img.shape == (h, w, 4)
    dev = torch.from_numpy(img).cuda()
    for i, s in enumerate(SCALES):
        dw, dh = max(1, int(w * s)), max(1, int(h * s))
        box = orc.box_downsample(img, dw, dh)
        for q in (QUALITIES if i in (0, 4) else QUALITIES[i % 5:i % 5 + 1]):
            want = orc.jpeg_encode(box, q)
            got = ctx.jpeg_encode_scaled(img, dw, dh, q)
            assert got == want, (w, h, kind, dw, dh, q)
            assert ctx.jpeg_encode_scaled(img, dw, dh, q, size_only=True) == len(want)
        assert ctx.jpeg_encode_scaled(dev, dw, dh, 50) == orc.jpeg_encode(box, 50), (dw, dh)


@pytest.mark.gpu
def test_encode_scaled_edge_shapes(ctx):
    import torch
    img = _blurred_noise(333, 217, 4)
    # 1 x 1, 7 x 5, odd sizes, and dw / dh above the source's (boxDownsample's "upsampling": empty boxes are zero pixels)
    for dw, dh in ((1, 1), (7, 5), (17, 9), (31, 217), (333, 1), (400, 300), (700, 100), (50, 500)):
        box = orc.box_downsample(img, dw, dh)
        for q in (1, 50, 100):
            assert ctx.jpeg_encode_scaled(img, dw, dh, q) == orc.jpeg_encode(box, q), (dw, dh, q)
    # a strided view (rows of a larger array), host and device
    big = synth.large_photo(700, 500, 6)
    view = big[13:13 + 430, 21:21 + 611]
    assert view.strides[0] == 700 * 4
    for dw, dh in ((305, 215), (160, 112), (611, 430)):
        want = orc.jpeg_encode(orc.box_downsample(np.ascontiguousarray(view), dw, dh), 75)
        assert ctx.jpeg_encode_scaled(view, dw, dh, 75) == want, (dw, dh)
        dview = torch.from_numpy(big).cuda()[13:13 + 430, 21:21 + 611]
        assert ctx.jpeg_encode_scaled(dview, dw, dh, 75) == want, (dw, dh)


@pytest.mark.gpu
def test_encode_scaled_4k(ctx):
    img = synth.large_photo(3840, 2160, 1)
    for s, q in ((0.5, 50), (0.26, 90), (0.05, 20), (0.97, 75)):
        dw, dh = int(3840 * s), int(2160 * s)
        want = orc.jpeg_encode(orc.box_downsample(img, dw, dh), q)
        assert ctx.jpeg_encode_scaled(img, dw, dh, q) == want, (dw, dh, q)


# ---- fnx_jpeg_target_size ----------------------------------------------------------------------------------------
def _targets(img):
    q100 = len(orc.jpeg_encode(img, 100))
    return [2 * q100, q100 // 2, q100 // 5, q100 // 20, q100 // 200, 700, 10]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["photo640", "noise333"])
def test_target_size_matches_the_restatement_per_strategy(ctx, name):
    img = synth.large_photo(640, 480, 7) if name == "photo640" else _blurred_noise(333, 217, 8)
    sz = Sizes(img)
    seen = set()
    for t in _targets(img):
        for mask in (FNX_TS_ALL, FNX_TS_QUALITY, FNX_TS_QUALITY_SCALE, FNX_TS_SCALE, FNX_TS_FALLBACK,
                     FNX_TS_QUALITY | FNX_TS_QUALITY_SCALE):
            got = _check(ctx, img, t, mask, sz)
            if mask == FNX_TS_ALL:
                seen.add(got["winner"])
    if name == "photo640":                  # the targets reach the strategies they are for (on the noise, 3 beats 1 throughout)
        assert {0, 1}.issubset(seen) and (2 in seen or 3 in seen), seen
    assert 1 in seen and (2 in seen or 3 in seen), seen


@pytest.mark.gpu
def test_target_size_720p_host_and_device(ctx):
    import torch
    img = synth.large_photo(1280, 720, 4)
    sz = Sizes(img)
    dev = torch.from_numpy(img).cuda()
    for t in _targets(img):
        got = _check(ctx, img, t, FNX_TS_ALL, sz)
        d = ctx.jpeg_target_size(dev, t, FNX_TS_ALL)
        assert d["candidates"] == got["candidates"] and d["winner"] == got["winner"] and d["data"] == got["data"]
        if got["winner"] in (1, 2):
            assert d["image"].is_cuda and np.array_equal(d["image"].cpu().numpy(), got["image"])


@pytest.mark.gpu
def test_target_size_translucent_source(ctx):
    img = synth.noise_image(480, 320, 11, alpha=True)
    sz = Sizes(img)
    for t in _targets(img):
        _check(ctx, img, t, FNX_TS_ALL, sz)


@pytest.mark.gpu
def test_target_size_4k(ctx):
    """One 4K source; the restatement takes its sizes from the device's encoder (pinned above), its pixels, SSIMs and the
    winner's file from the oracle."""
    img = synth.large_photo(3840, 2160, 2)
    sz = Sizes(img, device=ctx)
    q100 = ctx.jpeg_encoded_size(img, 100)
    for t in (q100 // 2, q100 // 20, 700):
        _check(ctx, img, t, FNX_TS_ALL, sz, file_check=t < q100 // 10)


# ---- the contract ------------------------------------------------------------------------------------------------
def _raw(ctx, img, target, strategies, cap, cancel=None, window=None, istride=None):
    L = ctx._lib
    s = fennec_amd._Img(img)
    k = np.ascontiguousarray(ctx.gaussianKernel() if window is None else window)
    cand = (fennec_amd.SizeCandidate * 4)()
    win, n = C.c_int(-1), C.c_size_t(0)
    buf = np.zeros(max(cap, 1), dtype=np.uint8)
    out = np.zeros_like(img)
    rc = L.fnx_jpeg_target_size(ctx._h, s.space, s.ptr, s.stride, s.w, s.h, int(target), int(strategies),
                                k.ctypes.data_as(C.POINTER(C.c_double)) if window is not False else None,
                                C.byref(cancel) if cancel is not None else None, cand, C.byref(win),
                                buf.ctypes.data, cap, C.byref(n), out.ctypes.data, s.w * 4 if istride is None else istride)
    return rc, [c.as_dict() for c in cand], win.value, buf[:n.value].tobytes(), n.value, out


@pytest.mark.gpu
def test_target_size_cancelled_before_the_call(ctx):
    img = synth.large_photo(640, 480, 3)
    flag = C.c_int(1)
    got = ctx.jpeg_target_size(img, 20000, FNX_TS_ALL, cancel=flag)
    assert got["winner"] == 3 and [c["strategy"] for c in got["candidates"]] == [0, 0, 0, FNX_TS_FALLBACK]
    assert got["data"] == orc.jpeg_encode(img, 1)
    assert got["candidates"][3]["ssim"] == orc.ssim_fast(img, img, procs=8) or \
        abs(got["candidates"][3]["ssim"] - orc.ssim_fast(img, img, procs=8)) <= 1e-9
    got = ctx.jpeg_target_size(img, 20000, FNX_TS_QUALITY | FNX_TS_QUALITY_SCALE | FNX_TS_SCALE, cancel=flag)
    assert got["status"] == fennec_amd.FNX_NOOP and got["winner"] is None
    assert all(c["strategy"] == 0 and c["steps"] == 0 for c in got["candidates"])
    flag.value = 0
    assert ctx.jpeg_target_size(img, 20000, FNX_TS_ALL, cancel=flag)["winner"] in (0, 1)


@pytest.mark.gpu
def test_target_size_small_cap_fills_everything(ctx):
    img = synth.large_photo(640, 480, 5)
    q100 = len(orc.jpeg_encode(img, 100))
    for t in (q100 // 5, q100 // 20, 700):
        full = ctx.jpeg_target_size(img, t, FNX_TS_ALL)
        rc, cands, win, _, n, out = _raw(ctx, img, t, FNX_TS_ALL, 16)
        assert rc == fennec_amd.FNX_ERR_INVALID and "needs" in ctx._err()
        assert n == len(full["data"]) and win == full["winner"] and cands == full["candidates"]
        c = cands[win]
        src = out[:c["final_h"], :c["final_w"]] if win in (1, 2) else img
        if win in (1, 2):
            assert np.array_equal(src, full["image"])
        assert ctx.jpeg_encode(np.ascontiguousarray(src), c["quality"]) == full["data"]


@pytest.mark.gpu
def test_target_size_refuses_bad_arguments(ctx):
    img = synth.large_photo(64, 48, 1)
    for target, strategies, window, istride in ((0, FNX_TS_ALL, None, None), (-5, FNX_TS_ALL, None, None), (1000, 0, None, None),
                                                (1000, 16, None, None), (1000, FNX_TS_ALL, False, None), (1000, FNX_TS_ALL, None, 4)):
        rc = _raw(ctx, img, target, strategies, 4096, window=window, istride=istride)[0]
        assert rc == fennec_amd.FNX_ERR_INVALID and ctx._err().startswith("invalid argument"), (target, strategies)
    L = ctx._lib
    cand = (fennec_amd.SizeCandidate * 4)()
    win, n = C.c_int(), C.c_size_t()
    k = ctx.gaussianKernel()
    big = np.zeros((1, 4), dtype=np.uint8)
    rc = L.fnx_jpeg_target_size(ctx._h, 0, big.ctypes.data, 65536 * 4, 65536, 1, 1000, FNX_TS_ALL, k.ctypes.data_as(C.POINTER(C.c_double)),
                                None, cand, C.byref(win), None, 0, C.byref(n), None, 0)
    assert rc == fennec_amd.FNX_ERR_INVALID and "65535" in ctx._err()
    rc = L.fnx_jpeg_encode_scaled(ctx._h, 0, img.ctypes.data, 64 * 4, 64, 48, 65536, 10, 50, None, 0, C.byref(n))
    assert rc == fennec_amd.FNX_ERR_INVALID and "16-bit" in ctx._err()
    with pytest.raises(fennec_amd.FennecError):
        ctx.jpeg_target_size(img, 0)
    with pytest.raises(fennec_amd.FennecError):
        ctx.jpeg_target_size(img, 1000, strategies=0)
    with pytest.raises(fennec_amd.FennecError):
        ctx.jpeg_encode_scaled(img, 0, 10, 50)


@pytest.mark.gpu
def test_target_size_second_call_is_the_same(ctx):
    img = synth.large_photo(800, 600, 9)
    t = len(orc.jpeg_encode(img, 100)) // 20
    a = ctx.jpeg_target_size(img, t, FNX_TS_ALL)
    b = ctx.jpeg_target_size(img, t, FNX_TS_ALL)
    assert a["candidates"] == b["candidates"] and a["winner"] == b["winner"] and a["data"] == b["data"]
    assert np.array_equal(np.asarray(a["image"]), np.asarray(b["image"]))
