"""fnx_jpeg_decode_batch / fnx_jpeg_recompress_batch on the GPU (-m gpu): a chunk of JPEG files through ONE set of the
decoder's launches (jpeg_dec.hip: jpeg_decode_planes_chunk).  Per file the batch must give what fnx_jpeg_decode gives -- the
oracle's pixels bit for bit, the same refusals -- whatever its neighbours in the chunk are: files of every geometry, with and
without restart intervals, with their own Huffman tables, of one workgroup and of several (a scan above ~30.7 KB spans more
than one: 240 spans of 1024 bits each), damaged files beside good ones, strided destinations, chunk boundaries."""
from __future__ import annotations

import ctypes as C
import io

import numpy as np
import pytest

import fennec_amd
from fennec_amd import FNX_ERR_INVALID, FNX_ERR_UNSUPPORTED, FNX_OK
from oracle import oracle as orc

pytestmark = pytest.mark.gpu
PROF_JPEG = 16
CHUNK = 32          # FNX_JPEG_DECODE_CHUNK


def _pil(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., :3]), "RGB").save(buf, "JPEG", **kw)
    return buf.getvalue()


def _pil_grey(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., 1]), "L").save(buf, "JPEG", **kw)
    return buf.getvalue()


def _as_440(data):
    """a 4:2:2 file relabelled as 4:4:0 (tests/test_jpeg_decode.py)"""
    i = data.index(b"\xff\xc0")
    b = bytearray(data)
    assert b[i + 9] == 3 and b[i + 11] == 0x21
    b[i + 5:i + 9] = b[i + 7:i + 9] + b[i + 5:i + 7]
    b[i + 11] = 0x12
    return bytes(b)


def _noise(w, h, seed=0):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    a[..., 3] = 255
    return a


def _photo(w, h, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 60 * np.sin(x / 37.0) * np.cos(y / 23.0) + 40 * np.sin((x + y) / 91.0)
    img = np.stack([base + rng.normal(0, s, (h, w)) for s in (6, 9, 12)], axis=-1)
    out = np.empty((h, w, 4), dtype=np.uint8)
    out[..., :3] = np.clip(img, 0, 255).astype(np.uint8)
    out[..., 3] = 255
    return out


def _workgroups(data):
    """workgroups of the decoder's first pass for a baseline file: its scan without stuffing and markers, in spans of 1024
    bits, 240 spans per workgroup"""
    i = data.index(b"\xff\xda")
    scan = data[i + 2 + ((data[i + 2] << 8) | data[i + 3]):data.rindex(b"\xff\xd9")]
    nb = len(scan) - scan.count(b"\xff\x00") - 2 * sum(scan.count(bytes([0xff, 0xd0 + k])) for k in range(8))
    lanes = (8 * nb + 1023) // 1024
    return (lanes + 239) // 240


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


@pytest.fixture(scope="module")
def mixed():
    """(name, file, the oracle's decode) of the mixed chunk; made and decoded on the CPU once"""
    import jpeg_mini
    files = []
    for (w, h) in ((1, 1), (16, 16), (17, 9), (8, 300)):
        files.append((f"oracle {w}x{h}", orc.jpeg_encode(_photo(w, h, w + h), 75)))
    src = _photo(203, 117, 5)
    files.append(("pil 420 optimize", _pil(src, quality=92, subsampling=2, optimize=True)))
    d422 = _pil(_photo(333, 217, 6), quality=88, subsampling=1)
    files.append(("pil 422", d422))
    files.append(("pil 440", _as_440(d422)))
    files.append(("pil grey", _pil_grey(src, quality=80)))
    files.append(("pil rst rows", _pil(src, quality=88, subsampling=2, restart_marker_rows=1)))
    files.append(("pil rst blocks 7", _pil(src, quality=88, subsampling=0, restart_marker_blocks=7)))
    small = _photo(64, 16, 1)
    for (hy, vy) in ((4, 1), (4, 2)):
        for rst in (0, 7):
            files.append((f"mini {hy}x{vy} rst {rst}", jpeg_mini.encode(small, hy, vy, 88, rst)))
    files.append(("noise 128 q100", orc.jpeg_encode(_noise(128, 128, 1), 100)))
    files.append(("noise 256 q100", orc.jpeg_encode(_noise(256, 256, 2), 100)))
    flat = np.full((1024, 2048, 4), 255, dtype=np.uint8)
    flat[..., 1] = 77
    files.append(("flat 2048x1024 q50", orc.jpeg_encode(flat, 50)))
    files.append(("photo 640x480 q95", _pil(_photo(640, 480, 9), quality=95, subsampling=2)))
    for name, data in files[-4:]:
        assert _workgroups(data) >= 2, (name, _workgroups(data))
    assert len(files) >= 14
    return [(name, data, orc.jpeg_decode(data)) for name, data in files]


def _check(ctx, items):
    images, statuses = ctx.jpeg_decode_batch([data for _, data, _ in items])
    for (name, _, want), got, st in zip(items, images, statuses):
        assert st == FNX_OK, (name, st)
        assert got.shape == want.shape and np.array_equal(got, want), name


def test_mixed_chunk_is_the_oracles_and_the_single_calls(ctx, mixed):
    _check(ctx, mixed)
    assert ctx.last_kernel(PROF_JPEG) == "jpeg_dsync_batch_kernel"
    for name, data, want in mixed:
        assert np.array_equal(ctx.jpeg_decode(data), want), name


def test_neighbours_do_not_matter(ctx, mixed):
    _check(ctx, mixed[::-1])
    _check(ctx, mixed[5:] + mixed[:5])


def test_a_batch_of_one_equals_the_single_call(ctx, mixed):
    for name in ("pil 422", "noise 256 q100"):
        item = next(m for m in mixed if m[0] == name)
        images, statuses = ctx.jpeg_decode_batch([item[1]])
        assert statuses == [FNX_OK] and np.array_equal(images[0], ctx.jpeg_decode(item[1])) and np.array_equal(images[0], item[2])


def test_two_1080p_files_in_one_call(ctx):
    files = [_pil(_photo(1920, 1080, s), quality=90, subsampling=2) for s in (1, 2)]
    assert all(_workgroups(f) >= 12 for f in files)
    images, statuses = ctx.jpeg_decode_batch(files, device=True)
    assert statuses == [FNX_OK, FNX_OK]
    for f, t in zip(files, images):
        assert t.is_cuda and np.array_equal(t.cpu().numpy(), orc.jpeg_decode(f))


def test_chunk_boundaries(ctx):
    n = 2 * CHUNK + 3
    files = [orc.jpeg_encode(_photo(16 + i % 9, 16 + (i * 5) % 9, i), 60 + i % 40) for i in range(n)]
    assert len(set(files)) == n
    images, statuses = ctx.jpeg_decode_batch(files)
    assert statuses == [FNX_OK] * n
    for i, (f, got) in enumerate(zip(files, images)):
        assert np.array_equal(got, orc.jpeg_decode(f)), i


def test_per_item_failures_beside_good_files(ctx, mixed):
    src = _photo(160, 120, 4)
    good = _pil(src, quality=80, subsampling=2)
    big = next(m for m in mixed if m[0] == "noise 256 q100")[1]
    files = [good,
             good[: len(good) * 3 // 4] + b"\xff\xd9",
             big,
             good[: len(good) // 2],
             _pil(src, quality=80, progressive=True, subsampling=2),
             _pil(src, quality=80, progressive=True, subsampling=2, restart_marker_blocks=3),
             b"\x89PNG\r\n\x1a\n" + good,
             good]
    want = [FNX_OK, FNX_ERR_INVALID, FNX_OK, FNX_ERR_INVALID, FNX_OK, FNX_ERR_UNSUPPORTED, FNX_ERR_INVALID, FNX_OK]
    images, statuses = ctx.jpeg_decode_batch(files)
    assert statuses == want
    for f, got, st in zip(files, images, statuses):
        if st == FNX_OK:
            assert np.array_equal(got, orc.jpeg_decode(f))
        else:
            assert got is None
    assert np.array_equal(ctx.jpeg_decode(good), orc.jpeg_decode(good))


def _raw_decode_batch(ctx, files, ptrs, strides):
    n = len(files)
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in files]
    pf = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    ps = (C.c_size_t * n)(*[len(f) for f in files])
    pd = (C.c_void_p * n)(*ptrs)
    pst = (C.c_int * n)(*strides)
    ws, hs, status = (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    rc = ctx._lib.fnx_jpeg_decode_batch(ctx._h, n, pf, ps, pd, pst, ws, hs, status)
    return rc, list(ws), list(hs), list(status)


def test_strided_and_offset_destinations(ctx, mixed):
    import torch
    items = [next(m for m in mixed if m[0] == name) for name in ("pil 420 optimize", "oracle 17x9", "noise 128 q100", "pil grey")]
    cases = [(16, 0), (5, 1), (16, 1), (5, 0)]                  # (pad px, offset px)
    bigs, ptrs, strides = [], [], []
    for (_, _, want), (pad, off) in zip(items, cases):
        h, w = want.shape[:2]
        big = torch.full((h + 2, w + pad, 4), 0xAB, dtype=torch.uint8, device="cuda:0")
        bigs.append(big)
        strides.append((w + pad) * 4)
        ptrs.append(big.data_ptr() + strides[-1] + 4 * off)     # one row down, `off` pixels in
    torch.cuda.synchronize()
    with ctx._ordered(*bigs):
        rc, ws, hs, status = _raw_decode_batch(ctx, [it[1] for it in items], ptrs, strides)
    assert rc == FNX_OK and status == [FNX_OK] * 4
    for (_, _, want), (pad, off), big, w_, h_ in zip(items, cases, bigs, ws, hs):
        h, w = want.shape[:2]
        assert (w_, h_) == (w, h)
        got = big.cpu().numpy()
        assert np.array_equal(got[1:h + 1, off:off + w], want)
        got[1:h + 1, off:off + w] = 0xAB
        assert (got == 0xAB).all()                               # nothing outside each row was touched


def test_bad_arguments(ctx, mixed):
    import torch
    good = mixed[1][1]
    want = mixed[1][2]
    h, w = want.shape[:2]
    t = [torch.zeros((h, w, 4), dtype=torch.uint8, device="cuda:0") for _ in range(2)]
    torch.cuda.synchronize()
    L, H = ctx._lib, ctx._h
    bufs = np.frombuffer(good, dtype=np.uint8)
    pf = (C.c_void_p * 2)(bufs.ctypes.data, bufs.ctypes.data)
    ps = (C.c_size_t * 2)(len(good), len(good))
    pd = (C.c_void_p * 2)(t[0].data_ptr(), t[1].data_ptr())
    pst = (C.c_int * 2)(4 * w, 4 * w)
    ws, hs, status = (C.c_int * 2)(), (C.c_int * 2)(), (C.c_int * 2)()
    with ctx._ordered(*t):
        assert L.fnx_jpeg_decode_batch(H, 0, pf, ps, pd, pst, ws, hs, status) == FNX_ERR_INVALID
        assert L.fnx_jpeg_decode_batch(H, 2, pf, None, pd, pst, ws, hs, status) == FNX_ERR_INVALID
        assert L.fnx_jpeg_decode_batch(H, 2, pf, ps, pd, pst, ws, hs, None) == FNX_ERR_INVALID
        # a result waiting in the FIFO: the blocking batch refuses to run past it
        a = torch.from_numpy(_photo(64, 64, 1)).cuda()
        k, pk = fennec_amd._f64(ctx.gaussianKernel())
        pa = (C.c_void_p * 1)(a.data_ptr())
        assert L.fnx_ssim_fast_batch_enqueue(H, 1, pa, 256, pa, 256, 64, 64, pk) == FNX_OK
        assert L.fnx_jpeg_decode_batch(H, 2, pf, ps, pd, pst, ws, hs, status) == FNX_ERR_INVALID
        out = (C.c_double * 1)()
        assert L.fnx_results_fetch(H, 1, out) == FNX_OK
        # a NULL destination: that item only
        pd[0] = None
        assert L.fnx_jpeg_decode_batch(H, 2, pf, ps, pd, pst, ws, hs, status) == FNX_OK
        assert list(status) == [FNX_ERR_INVALID, FNX_OK] and (ws[0], hs[0]) == (w, h)
    assert np.array_equal(t[1].cpu().numpy(), want) and not t[0].any()


def test_recompress_batch_is_the_single_call_per_item(ctx):
    import jpeg_mini
    a, b, c = _photo(320, 200, 6), _photo(203, 117, 5), _photo(640, 480, 2)
    files = [_pil(a, quality=93, subsampling=2),
             _pil(b, quality=92, subsampling=0, optimize=True),
             _pil_grey(a, quality=90),
             _pil(c, quality=93, subsampling=2, restart_marker_rows=1),
             jpeg_mini.encode(a, 4, 2, 91),
             _pil(c, quality=95, subsampling=1),
             _pil(b, quality=85, subsampling=2),
             orc.jpeg_encode(a, 88)]
    for targets in (0.94, [0.9, 0.94, 0.97, 0.94, 0.92, 0.99, 0.94, 0.95]):
        res = ctx.jpeg_recompress_batch(files, targets)
        tl = [targets] * len(files) if isinstance(targets, float) else targets
        for i, (f, t, r) in enumerate(zip(files, tl, res)):
            assert r == ctx.jpeg_recompress(f, t), i
    # one unsupported item keeps its status while the others finish
    bad = _pil(b, quality=80, progressive=True, subsampling=2, restart_marker_blocks=3)
    res = ctx.jpeg_recompress_batch([files[0], bad, files[1]], 0.94)
    assert isinstance(res[1], fennec_amd.FennecUnsupported)
    assert res[0] == ctx.jpeg_recompress(files[0], 0.94) and res[2] == ctx.jpeg_recompress(files[1], 0.94)
    # a deliberately small buffer through the raw ABI: FNX_ERR_INVALID with the size and the quality set
    sub = files[:3]
    n = len(sub)
    single = [ctx.jpeg_recompress(f, 0.94) for f in sub]
    bufs = [np.frombuffer(f, dtype=np.uint8) for f in sub]
    outs = [np.empty(len(f) + 4096, dtype=np.uint8) for f in sub]
    capl = [len(o) for o in outs]
    capl[1] = 100
    k, pk = fennec_amd._f64(ctx.gaussianKernel())
    tg, ptg = fennec_amd._f64([0.94] * n)
    pf = (C.c_void_p * n)(*[x.ctypes.data for x in bufs])
    ps = (C.c_size_t * n)(*[len(f) for f in sub])
    po = (C.c_void_p * n)(*[o.ctypes.data for o in outs])
    caps = (C.c_size_t * n)(*capl)
    nb, q, st, status = (C.c_size_t * n)(), (C.c_int * n)(), (C.c_int * n)(), (C.c_int * n)()
    ws, hs, v = (C.c_int * n)(), (C.c_int * n)(), (C.c_double * n)()
    assert ctx._lib.fnx_jpeg_recompress_batch(ctx._h, n, pf, ps, ptg, pk, po, caps, nb, q, v, st, ws, hs, status) == FNX_OK
    assert list(status) == [FNX_OK, FNX_ERR_INVALID, FNX_OK]
    assert nb[1] == len(single[1][0]) and q[1] == single[1][1]
    assert ctx.jpeg_encode(ctx.jpeg_decode(sub[1]), q[1]) == single[1][0]
    for i in (0, 2):
        assert (outs[i][:nb[i]].tobytes(), q[i], v[i], st[i], (ws[i], hs[i])) == single[i]
