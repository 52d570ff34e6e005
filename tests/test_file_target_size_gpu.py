"""Target-size mode from a file's bytes (fennec_CompressFileTargetSize) and the pool over such files
(fennec_CompressBatchTargetSize) against the composition of the entries they assemble: jpeg_decode / png_decode, then
ApplyOrientation, then smartResize, then jpeg_target_size -- candidates, winner, file bytes and dims."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import fennec_amd
import png_decode_ref as ref
from fennec_amd import FNX_TS_ALL, SizeCandidate, TargetOptions, batch, synth

OPTION_SETS = {"plain": {}, "orient6": dict(orient=6), "max_w64": dict(max_w=64)}
TARGETS = {"jpeg": (4000, 1500, 10), "png": (2500, 1500, 10)}      # strategy 1 or 3 wins the first two, the fallback the last


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


@pytest.fixture(scope="module")
def sources(ctx):
    jpg = ctx.jpeg_encode(synth.large_photo(160, 120, 3), 90)
    png = ctx.compress_png(synth.large_photo(96, 64, 4))
    assert png[:8] == b"\x89PNG\r\n\x1a\n" and jpg[:2] == b"\xff\xd8"
    return {"jpeg": jpg, "png": png}


def _decoded(ctx, kind, data):
    return ctx.jpeg_decode(data) if kind == "jpeg" else ctx.png_decode(data, "host")


def _composed(ctx, kind, data, target, orient=1, max_w=0, max_h=0, strategies=FNX_TS_ALL, cancel=None):
    img = np.ascontiguousarray(ctx.ApplyOrientation(_decoded(ctx, kind, data), orient))
    original = (img.shape[1], img.shape[0])
    if max_w > 0 or max_h > 0:
        img = np.ascontiguousarray(ctx.smartResize(img, max_w, max_h))
    got = ctx.jpeg_target_size(img, target, strategies, cancel=cancel)
    final = (img.shape[1], img.shape[0])
    if got["winner"] is not None:
        c = got["candidates"][got["winner"]]
        final = (c["final_w"], c["final_h"])
    return got, (original, final)


def _same(got, want, dims):
    assert got["candidates"] == want["candidates"]
    assert got["winner"] == want["winner"] and got["status"] == want["status"]
    assert got["data"] == want["data"]
    assert got["dims"] == dims


@pytest.mark.gpu
@pytest.mark.parametrize("opts", sorted(OPTION_SETS))
@pytest.mark.parametrize("kind", ["jpeg", "png"])
def test_file_entry_is_the_composition(ctx, sources, kind, opts):
    o = OPTION_SETS[opts]
    winners = []
    for target in TARGETS[kind]:
        want, dims = _composed(ctx, kind, sources[kind], target, **o)
        got = ctx.compress_file_target_size(sources[kind], target, **o)
        _same(got, want, dims)
        winners.append(got["winner"])
    assert winners[2] == 3 and 3 not in winners[:2], winners
    w, h = (160, 120) if kind == "jpeg" else (96, 64)
    assert got["dims"][0] == ((h, w) if opts == "orient6" else (w, h))


@pytest.mark.gpu
def test_a_strategy_subset_and_no_candidate(ctx, sources):
    want, dims = _composed(ctx, "jpeg", sources["jpeg"], 1500, strategies=fennec_amd.FNX_TS_QUALITY)
    got = ctx.compress_file_target_size(sources["jpeg"], 1500, strategies=fennec_amd.FNX_TS_QUALITY)
    assert got["status"] == fennec_amd.FNX_NOOP and got["winner"] is None and got["data"] is None
    _same(got, want, dims)
    assert got["dims"] == ((160, 120), (160, 120))                   # no winner: the staged image's size


def _raw(ctx, data, o, cap, cancel=None):
    src = np.frombuffer(data, dtype=np.uint8)
    cand = (SizeCandidate * 4)()
    win, n = C.c_int(-1), C.c_size_t(0)
    dims = (C.c_int * 4)()
    buf = np.zeros(max(cap, 1), dtype=np.uint8)
    rc = ctx._lib.fennec_CompressFileTargetSize(ctx._h, src.ctypes.data_as(C.POINTER(C.c_uint8)), len(data), C.byref(o),
                                                C.byref(cancel) if cancel is not None else None, cand, C.byref(win),
                                                buf.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n), dims)
    return rc, [c.as_dict() for c in cand], win.value, n.value, list(dims), buf[:min(n.value, cap)].tobytes()


@pytest.mark.gpu
def test_a_small_cap_fills_everything(ctx, sources):
    for target in (1500, 10):
        full = ctx.compress_file_target_size(sources["jpeg"], target, orient=6)
        rc, cands, win, n, dims, _ = _raw(ctx, sources["jpeg"], TargetOptions.make(target, orient=6), 16)
        assert rc == fennec_amd.FNX_ERR_INVALID and "needs" in ctx._err()
        assert cands == full["candidates"] and win == full["winner"] and n == len(full["data"])
        assert (tuple(dims[:2]), tuple(dims[2:])) == full["dims"]
    # the size alone: out == NULL with cap == 0
    src = np.frombuffer(sources["jpeg"], dtype=np.uint8)
    o = TargetOptions.make(1500)
    cand, win, n, dims = (SizeCandidate * 4)(), C.c_int(-1), C.c_size_t(0), (C.c_int * 4)()
    rc = ctx._lib.fennec_CompressFileTargetSize(ctx._h, src.ctypes.data_as(C.POINTER(C.c_uint8)), len(src), C.byref(o), None, cand,
                                                C.byref(win), None, 0, C.byref(n), dims)
    full = ctx.compress_file_target_size(sources["jpeg"], 1500)
    assert rc == fennec_amd.FNX_OK and n.value == len(full["data"]) and win.value == full["winner"]


@pytest.mark.gpu
def test_an_adam7_png_is_unsupported_on_a_default_ctx(ctx):
    il = ref.write_png(ref.random_samples(9, 5, 2, 8, 1), 2, 8, interlace=1)
    with pytest.raises(fennec_amd.FennecUnsupported):
        ctx.compress_file_target_size(il, 1000)
    rc = _raw(ctx, il, TargetOptions.make(1000), 4096)[0]
    assert rc == fennec_amd.FNX_ERR_UNSUPPORTED


@pytest.mark.gpu
def test_cancelled_before_the_call(ctx, sources):
    flag = C.c_int(1)
    want, dims = _composed(ctx, "jpeg", sources["jpeg"], 4000, cancel=flag)
    got = ctx.compress_file_target_size(sources["jpeg"], 4000, cancel=flag)
    _same(got, want, dims)
    assert got["winner"] == 3 and [c["strategy"] for c in got["candidates"]] == [0, 0, 0, fennec_amd.FNX_TS_FALLBACK]
    flag.value = 0
    assert ctx.compress_file_target_size(sources["jpeg"], 4000, cancel=flag)["winner"] in (0, 1)


@pytest.mark.gpu
def test_refusals_with_a_ctx_touch_nothing(ctx, sources):
    for o in (TargetOptions.make(0), TargetOptions.make(1000, strategies=0), TargetOptions.make(1000, strategies=16)):
        assert _raw(ctx, sources["jpeg"], o, 4096)[0] == fennec_amd.FNX_ERR_INVALID and ctx._err().startswith("invalid argument")
    o = TargetOptions.make(1000)
    o.reserved = 1
    assert _raw(ctx, sources["jpeg"], o, 4096)[0] == fennec_amd.FNX_ERR_INVALID and "reserved" in ctx._err()


@pytest.mark.gpu
def test_pool_items_are_the_single_entry(ctx, sources):
    jpg2 = ctx.jpeg_encode(synth.large_photo(120, 88, 6), 85)
    files = [sources["jpeg"], sources["png"], jpg2, sources["jpeg"][:len(sources["jpeg"]) // 2], sources["png"], jpg2]
    own = [None] * 6
    own[2] = TargetOptions.make(10, orient=6)                           # its own target (the fallback: over its buffer) and orientation
    own[4] = TargetOptions.make(2500, max_w=64, strategies=fennec_amd.FNX_TS_QUALITY_SCALE | fennec_amd.FNX_TS_FALLBACK)
    results, out_files, summary = batch.compress_batch_target_size_native(files, 1500, workers=3, device=0, item_opts=own)
    assert [r.Index for r in results] == list(range(6))
    for i, r in enumerate(results):
        if i == 3:
            continue
        o = own[i]
        kw = dict(orient=o.file.orient, max_w=o.file.max_w, max_h=o.file.max_h, strategies=o.strategies) if o is not None else {}
        want = ctx.compress_file_target_size(files[i], o.target_bytes if o is not None else 1500, **kw)
        assert r.Err is None and r.status == fennec_amd.FNX_OK and r.has_result, (i, r)
        assert out_files[i] == want["data"], i
        assert r.candidates == want["candidates"] and r.winner == want["winner"] and r.dims == want["dims"], i
        c = want["candidates"][want["winner"]]
        assert (r.Quality, r.SSIM, r.CompressedSize, r.OriginalSize) == (c["quality"], c["ssim"], len(want["data"]), len(files[i])), i
        assert r.steps == sum(x["steps"] for x in want["candidates"]), i
    assert results[2].winner == 3 and results[2].dims[0] == (88, 120)
    bad = results[3]                                                     # the truncated file fails alone
    assert bad.Err is not None and bad.status < 0 and out_files[3] == b"" and bad.OriginalSize == len(files[3])
    assert (summary.Total, summary.Succeeded, summary.Failed) == (6, 5, 1)
    assert summary.TotalSaved == sum(len(files[i]) - len(out_files[i]) for i in range(6) if i != 3)
    assert abs(summary.AvgSSIM - sum(r.SSIM for r in results if r.Err is None) / 5) <= 1e-15


@pytest.mark.gpu
def test_pool_results_through_the_c_summary(ctx, sources):
    """fennec_SummarizeResults over the pool's own result array, the cancel word handed to every item"""
    L = ctx._lib
    files = [sources["jpeg"], sources["png"]]
    n = len(files)
    arrs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    outs = [np.zeros(8192, dtype=np.uint8) for _ in files]
    res = (fennec_amd.NativeBatchResult * n)()
    cands = (SizeCandidate * (4 * n))()
    dims = (C.c_int * (4 * n))()
    default = TargetOptions.make(1500)
    flag = C.c_int(0)
    rc = L.fennec_CompressBatchTargetSize(0, 2, n, (C.c_void_p * n)(*[a.ctypes.data for a in arrs]), (C.c_size_t * n)(*[len(f) for f in files]),
                                          C.byref(default), None, (C.c_void_p * n)(*[o.ctypes.data for o in outs]), (C.c_size_t * n)(8192, 8192),
                                          res, cands, dims, C.byref(flag), None, None)
    assert rc == fennec_amd.FNX_OK
    out4 = (C.c_int64 * 4)()
    avg = L.fennec_SummarizeResults(n, res, out4)
    assert list(out4) == [2, 2, 0, sum(len(f) for f in files) - sum(int(r.compressed_size) for r in res)]
    assert abs(avg - (res[0].ssim + res[1].ssim) / 2) <= 1e-15
    for i in range(n):
        want = ctx.compress_file_target_size(files[i], 1500)
        assert outs[i][:int(res[i].compressed_size)].tobytes() == want["data"]
        assert res[i].steps == sum(cands[4 * i + k].steps for k in range(4)) == sum(c["steps"] for c in want["candidates"])
        assert res[i].original_size == len(files[i]) and res[i].failed == 0 and res[i].status == fennec_amd.FNX_OK
