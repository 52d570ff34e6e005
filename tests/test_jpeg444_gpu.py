"""FNX_JPEG_SUBSAMPLING_444 on the GPU (-m gpu): the single-image JPEG entries on a ctx set to 4:4:4 against the plain-numpy
statement of the rule (tests/jpeg444_ref.py, itself held by tests/test_jpeg444_ref.py) -- the file's entropy-coded segment byte
for byte, its header, the round trip, both size-query routes, the symbol histogram and the optimised tables, the two searches --
the default's bytes again after switching back, and the refusal of every JPEG-writing entry that has no 4:4:4 form."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
import jpeg444_ref as ref
import jpeg_hufftab_ref as href
from oracle import oracle as orc

PROF_JPEG = 16
ONE_WAIT, TWO_STEP, YCC444 = "jpeg_ffcount_strips_kernel", "jpeg_pack_kernel", "jpeg_ycc444_kernel"
CASES = sorted(ref.cases())
_u8p = C.POINTER(C.c_uint8)


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


@pytest.fixture()
def c444(ctx):
    ctx.set_jpeg_subsampling("444")
    yield ctx
    ctx.set_jpeg_subsampling("420")
    ctx.set_jpeg_huffman("standard")


def _scan(data):
    i, end = href._segment_at(data, 0xDA)
    return data[:end], data[end:-2]


# ---------------------------------------------------------------------------------------------------------------- 1. file bytes
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_files_are_the_restatements_byte_for_byte(ctx, name):
    img, qualities = ref.cases()[name]
    for q in qualities:
        r = ref.ref(name, q)
        ctx.set_jpeg_subsampling("420")
        header_420, _ = _scan(ctx.jpeg_encode(img, q))
        ctx.set_jpeg_subsampling("444")
        try:
            data = ctx.jpeg_encode(img, q)
        finally:
            ctx.set_jpeg_subsampling("420")
        header, scan = _scan(data)
        assert scan == r.scan, (name, q, ref.first_difference(scan, r.scan, r.crafted))
        assert data[-2:] == b"\xff\xd9"
        # the header: the same ctx's 4:2:0 header except the Y component's sampling byte in SOF0
        diff = [i for i in range(max(len(header), len(header_420))) if header[i:i + 1] != header_420[i:i + 1]]
        at = ref._sof0_y_sampling(header_420)
        assert diff == [at] and (header_420[at], header[at]) == (0x22, 0x11), (name, q, diff)
        assert data == r.file, (name, q)
        w, h, ratio, _, _, _, coef = orc.jpeg_decode_planes(data, with_coefficients=True)
        assert (w, h, ratio) == (img.shape[1], img.shape[0], 0) and np.array_equal(coef, r.coef), (name, q)


# ---------------------------------------------------------------------------------------------------------------- 2. round trip
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_round_trip_is_the_decoded_file(c444, name):
    img, qualities = ref.cases()[name]
    for q in qualities:
        got = c444.jpeg_roundtrip(img, q)
        assert c444.last_kernel(PROF_JPEG) == YCC444                                   # (9) the new colour kernel ran
        assert np.array_equal(got, ref.ref(name, q).image), (name, q)
        assert np.array_equal(got, orc.jpeg_decode(c444.jpeg_encode(img, q))), (name, q)
        assert np.array_equal(c444.jpeg_decode(ref.ref(name, q).file), got), (name, q)  # the device's decoder reads it as 4:4:4 too


@pytest.mark.gpu
def test_round_trip_of_a_device_tensor_and_a_strided_view(c444):
    import torch
    img = ref.image("noise_17x23")
    want = ref.ref("noise_17x23", 75).image
    d = torch.from_numpy(np.array(img)).cuda()
    torch.cuda.synchronize()
    assert np.array_equal(c444.jpeg_roundtrip(d, 75).cpu().numpy(), want)
    wide = torch.zeros((23, 32, 4), dtype=torch.uint8, device="cuda")
    wide[:, 5:22] = d
    torch.cuda.synchronize()
    assert np.array_equal(c444.jpeg_roundtrip(wide[:, 5:22], 75).cpu().numpy(), want)   # an unaligned source, a stride beyond 4 w


# -------------------------------------------------------------------------------------------------------------- 3. size queries
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_both_size_routes_return_the_files_length(c444, name):
    img, qualities = ref.cases()[name]
    for huffman in ("standard", "optimized"):
        c444.set_jpeg_huffman(huffman)
        for q in qualities:
            r = ref.ref(name, q)
            n = len(r.file if huffman == "standard" else r.opt_file)
            for form, kernel in (("1", ONE_WAIT), ("0", TWO_STEP)):
                with c444.forms(jpeg_size=form):
                    assert c444.jpeg_encoded_size(img, q) == n, (name, huffman, q, form)
                    assert c444.last_kernel(PROF_JPEG) == kernel, (name, huffman, q, form)


# ---------------------------------------------------------------------------------------------------------- 4. optimised tables
@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_symbol_histogram_and_optimised_files(c444, name):
    img, qualities = ref.cases()[name]
    for q in qualities:
        r = ref.ref(name, q)
        got = c444.jpeg_symbol_histogram(img, q).astype(np.int64)
        assert c444.last_kernel(PROF_JPEG) == "jpeg_symhist_kernel"
        bad = np.argwhere(got != r.hist)
        assert len(bad) == 0, (name, q, [(f"table {t}", f"symbol {s:#04x}", int(got[t, s]), int(r.hist[t, s])) for t, s in bad[:8]])
    c444.set_jpeg_huffman("optimized")
    for q in qualities:
        r = ref.ref(name, q)
        data = c444.jpeg_encode(img, q)
        assert data == r.opt_file, (name, q, href.first_difference(data, r.opt_file, r.opt_crafted))
        dec = orc.jpeg_decode_planes(data, with_coefficients=True)
        assert dec[2] == 0 and np.array_equal(dec[6], r.coef), (name, q)


# -------------------------------------------------------------------------------------------------------------- 5. quality search
SEARCHES = (("photo_48x40", (0.90, 0.95, 0.98)), ("noise_17x23", (0.93,)), ("photo_528x40", (0.92, 0.97)))


def _cpu_search(name, target):
    img = ref.image(name)
    return ref.quality_search(lambda q: orc.ssim_fast(img, ref.ref(name, q).image), target)


def test_the_search_images_reach_both_branches_of_ssim_fast():
    assert not orc.ssim_fast_dims(48, 40)[0] and not orc.ssim_fast_dims(17, 23)[0] and orc.ssim_fast_dims(528, 40)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("name,targets", SEARCHES)
def test_quality_search_and_compress_follow_the_bisection(c444, name, targets):
    img = ref.image(name)
    for target in targets:
        q, s, steps, found, tried = _cpu_search(name, target)
        # the precondition: no candidate's score within 1e-6 of the target (the device's 1e-9 cannot flip a comparison)
        assert all(abs(v - target) > 1e-6 for v in tried.values()), (name, target, tried)
        gq, gs, gsteps, gfound = c444.jpeg_quality_search(img, target)
        assert c444.last_kernel(PROF_JPEG) == YCC444
        assert (gq, gsteps, gfound) == (q, steps, found), (name, target)
        assert abs(gs - s) <= 1e-9, (name, target, gs, s)
        if found:
            assert gs == c444.SSIMFast(img, c444.jpeg_roundtrip(img, q)), (name, target)
        data, cq, cs, csteps = c444.jpeg_compress(img, target)
        assert (cq, cs, csteps) == (gq, gs, gsteps), (name, target)
        assert data == c444.jpeg_encode(img, q) == ref.ref(name, q).file, (name, target)


@pytest.mark.gpu
def test_an_unreachable_target_ends_at_quality_100(c444):
    img = ref.image("noise_17x23")
    target = 0.99999
    q, s, steps, found, tried = _cpu_search("noise_17x23", target)
    assert not found and (q, s) == (100, 1.0) and all(abs(v - target) > 1e-6 for v in tried.values())
    assert c444.jpeg_quality_search(img, target) == (100, 1.0, steps, False)
    data, cq, cs, csteps = c444.jpeg_compress(img, target)
    assert (cq, cs, csteps) == (100, 1.0, steps) and data == ref.ref("noise_17x23", 100).file


# ----------------------------------------------------------------------------------------------------------------- 6. size search
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["photo_48x40", "photo_528x40"])
def test_size_search_returns_the_highest_quality_that_fits(c444, name):
    img = ref.image(name)
    h, w = img.shape[:2]
    for huffman in ("standard", "optimized"):
        c444.set_jpeg_huffman(huffman)
        file_of = (lambda q: ref.ref(name, q).file) if huffman == "standard" else (lambda q: ref.ref(name, q).opt_file)
        for tq in (35, 80):
            target = len(ref.ref(name, tq).file) + 3
            q, sz, steps = href.size_bisect(lambda quality: len(file_of(quality)), w, h, target)
            assert q > 0
            data, gq, gs, gsteps = c444.jpeg_size_search(img, target, skip_ssim=False)
            assert (gq, len(data), gsteps) == (q, sz, steps), (name, huffman, tq)
            assert data == file_of(q), (name, huffman, tq)
            assert abs(gs - orc.ssim_fast(img, ref.ref(name, q).image)) <= 1e-9, (name, huffman, tq)
            assert gs == c444.SSIMFast(img, c444.jpeg_roundtrip(img, q)), (name, huffman, tq)
            skipped = c444.jpeg_size_search(img, target, skip_ssim=True)
            assert (skipped[0], skipped[1], skipped[3]) == (data, gq, gsteps)
    assert c444.jpeg_size_search(img, 300, skip_ssim=True) is None                      # nothing fits: the header alone is larger


# ------------------------------------------------------------------------------------------------------------ 7. default untouched
@pytest.mark.gpu
def test_the_default_is_untouched(ctx):
    name = "noise_17x23"
    img = ref.image(name)
    fresh = fennec_amd.Context(0)
    want = orc.jpeg_encode(img, 75)
    assert fresh.jpeg_encode(img, 75) == want
    ctx.set_jpeg_subsampling("444")
    try:
        assert ctx.jpeg_encode(img, 75) == ref.ref(name, 75).file
        # a second ctx stays at 4:2:0 while the first is at 4:4:4
        assert fresh.jpeg_encode(img, 75) == want
        assert np.array_equal(fresh.jpeg_roundtrip(img, 75), orc.jpeg_roundtrip(img, 75))
        assert fresh.jpeg_compress(img, 0.93) == ctx_420_compress(fresh, img)
    finally:
        ctx.set_jpeg_subsampling(fennec_amd.FNX_JPEG_SUBSAMPLING_420)
    # set to 4:4:4 and back: the bytes of a fresh ctx
    assert ctx.jpeg_encode(img, 75) == want
    assert np.array_equal(ctx.jpeg_roundtrip(img, 75), orc.jpeg_roundtrip(img, 75))
    assert np.array_equal(ctx.jpeg_symbol_histogram(img, 75), fresh.jpeg_symbol_histogram(img, 75))
    assert ctx.jpeg_compress(img, 0.93) == fresh.jpeg_compress(img, 0.93)
    assert ctx.jpeg_size_search(img, 2000) == fresh.jpeg_size_search(img, 2000)
    with pytest.raises(fennec_amd.FennecError):
        ctx.set_jpeg_subsampling(2)
    assert ctx.jpeg_encode(img, 75) == want                                            # a refused mode changes nothing


def ctx_420_compress(c, img):
    data, q, s, steps = c.jpeg_compress(img, 0.93)
    assert data == orc.jpeg_encode(img, q)
    return data, q, s, steps


# -------------------------------------------------------------------------------------------------------------------- 8. refusals
SENTINEL = 0x5a


def _refusing_calls(ctx, img_dev, file_bytes):
    """name -> (call, outputs): every entry on the refusal list through the C ABI, its outputs filled with a sentinel"""
    L, h = ctx._lib, ctx._h
    H, W = img_dev.shape[:2]
    ptr = C.cast(C.c_void_p(img_dev.data_ptr()), _u8p)
    win, pk = fennec_amd._f64(ctx.gaussianKernel())
    src = np.frombuffer(file_bytes, dtype=np.uint8)
    fp, fn = src.ctypes.data_as(_u8p), len(file_bytes)
    out = np.full(1 << 16, SENTINEL, np.uint8)
    op, cap = out.ctypes.data_as(_u8p), out.size
    n, q, st, w_, h_, winner = C.c_size_t(SENTINEL), C.c_int(SENTINEL), C.c_int(SENTINEL), C.c_int(SENTINEL), C.c_int(SENTINEL), C.c_int(SENTINEL)
    v = C.c_double(float(SENTINEL))
    cand = (fennec_amd.SizeCandidate * 5)()
    for c in cand:
        c.strategy = c.quality = SENTINEL
    dims = (C.c_int * 4)(*([SENTINEL] * 4))
    fo = fennec_amd.FileOptions(1, 0, 0, 0, 0.94)
    to = fennec_amd.TargetOptions.make(4000)
    one = lambda t, val: (t * 1)(val)
    srcs, outs, files = one(C.c_void_p, img_dev.data_ptr()), one(C.c_void_p, out.ctypes.data), one(C.c_void_p, src.ctypes.data)
    caps, sizes, nb = one(C.c_size_t, cap), one(C.c_size_t, fn), one(C.c_size_t, SENTINEL)
    tg, ptg = fennec_amd._f64([0.94])
    qs, sts, status, ws, hs = (one(C.c_int, SENTINEL) for _ in range(5))
    vs = one(C.c_double, float(SENTINEL))
    D = 1                                            # FNX_DEVICE
    scalars = lambda: (n.value, q.value, st.value, w_.value, h_.value, winner.value, v.value, nb[0], qs[0], sts[0], status[0], ws[0], hs[0], vs[0],
                       tuple(dims), tuple((c.strategy, c.quality) for c in cand))
    keep = (win, src, out, tg)
    calls = {
        "fnx_jpeg_encode_scaled": lambda: L.fnx_jpeg_encode_scaled(h, D, ptr, W * 4, W, H, 8, 8, 75, op, cap, C.byref(n)),
        "fnx_jpeg_target_size": lambda: L.fnx_jpeg_target_size(h, D, ptr, W * 4, W, H, 4000, 15, pk, None, cand, C.byref(winner), op, cap, C.byref(n),
                                                               None, 0),
        "fnx_hit_target_size": lambda: L.fnx_hit_target_size(h, D, ptr, W * 4, W, H, 4000, fennec_amd.FNX_FORMAT_PNG, pk, None, cand, C.byref(winner),
                                                             op, cap, C.byref(n), None, 0),
        "fnx_jpeg_recompress": lambda: L.fnx_jpeg_recompress(h, fp, fn, 0.94, pk, op, cap, C.byref(n), C.byref(q), C.byref(v), C.byref(st),
                                                             C.byref(w_), C.byref(h_)),
        "fnx_jpeg_compress_batch": lambda: L.fnx_jpeg_compress_batch(h, 1, srcs, W * 4, W, H, ptg, pk, outs, caps, nb, qs, vs, sts, status),
        "fnx_jpeg_recompress_batch": lambda: L.fnx_jpeg_recompress_batch(h, 1, files, sizes, ptg, pk, outs, caps, nb, qs, vs, sts, ws, hs, status),
        "fennec_CompressFileJPEG": lambda: L.fennec_CompressFileJPEG(h, fp, fn, C.byref(fo), op, cap, C.byref(n), C.byref(q), C.byref(v), C.byref(st),
                                                                     dims),
        "fennec_CompressFileTargetSize": lambda: L.fennec_CompressFileTargetSize(h, fp, fn, C.byref(to), None, cand, C.byref(winner), op, cap,
                                                                                 C.byref(n), dims),
        "fennec_CompressFileHitTargetSize": lambda: L.fennec_CompressFileHitTargetSize(h, fp, fn, C.byref(fo), 4000, fennec_amd.FNX_FORMAT_JPEG, None,
                                                                                       cand, C.byref(winner), op, cap, C.byref(n), dims),
    }
    return calls, out, scalars, keep


@pytest.mark.gpu
def test_the_other_jpeg_entries_refuse_a_444_ctx_and_work_again_after(ctx):
    import torch
    img = ref.photo_like(32, 32, 31)
    dev = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    source = orc.jpeg_encode(img, 92)
    calls, out, scalars, keep = _refusing_calls(ctx, dev, source)
    before = scalars()
    ctx.set_jpeg_subsampling("444")
    try:
        for name, call in calls.items():
            assert call() == fennec_amd.FNX_ERR_UNSUPPORTED, name
            msg = ctx._lib.fnx_last_error().decode()
            assert name in msg and "4:4:4" in msg, (name, msg)
            assert scalars() == before and (out == SENTINEL).all(), name
        # the binding raises what it raises for any unsupported call
        with pytest.raises(fennec_amd.FennecUnsupported, match="fnx_jpeg_encode_scaled.*4:4:4"):
            ctx.jpeg_encode_scaled(dev, 8, 8, 75)
        # the decoders and the PNG entries ignore the mode
        assert np.array_equal(ctx.jpeg_decode(source), orc.jpeg_decode(source))
    finally:
        ctx.set_jpeg_subsampling("420")
    # ... and every one of them succeeds again
    for name, call in calls.items():
        assert call() == fennec_amd.FNX_OK, (name, ctx._lib.fnx_last_error())
    ctx.sync()
    assert ctx.jpeg_encode_scaled(dev, 8, 8, 75) == orc.jpeg_encode(np.ascontiguousarray(orc.box_downsample(img, 8, 8)), 75)
    data, q, s, steps, wh = ctx.jpeg_recompress(source, 0.94)
    assert wh == (32, 32) and data == orc.jpeg_encode(orc.jpeg_decode(source), q)
