"""The dense deflate level (fnx_ctx_set_deflate_level(ctx, FNX_DEFLATE_LEVEL_DENSE)) on the GPU: round trips through Python's
zlib in every space, contract_dense and the certificates of deflate_dense_contract.py on the device's streams, the three
size-table streams held byte for byte (size and SHA-256) to what the kernels' source gave on the CPU
(test_deflate_dense_hostsim.TABLE), level switching on one ctx, the capacity rule, and the PNG entries -- single and batched --
on a dense ctx."""
from __future__ import annotations

import ctypes as C
import hashlib
import zlib

import numpy as np
import pytest

import deflate_contract as dc
import deflate_dense_contract as dd
import fennec_amd
import inflate_probe as ip
import png_filter_ref as ref
from fennec_amd import FNX_DEFLATE_CHUNK as CH, FNX_PNG_GRAY, FNX_PNG_NRGBA, FNX_PNG_PALETTED
from test_deflate_dense_hostsim import TABLE
from test_deflate_gpu import RATIO_CASES, ROW

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 258, 259, CH - 1, CH, CH + 1, 2 * CH + 3]


@pytest.fixture(scope="module")
def ctx():
    c = fennec_amd.Context(0)
    c.set_deflate_level("dense")
    return c


@pytest.fixture(scope="module")
def fast():
    return fennec_amd.Context(0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def filtered_rgb(n):
    stream = ref.png_stream(ref.smooth_rgba(67, 330, 5, opaque=True), FNX_PNG_NRGBA)[0]
    assert stream.shape[1] == ROW
    return np.ascontiguousarray(stream).reshape(-1)[:n].copy()


CONTENTS = {
    "zeros": (lambda n: np.zeros(n, np.uint8), 0),
    "period_row": (lambda n: np.resize((np.arange(ROW) * 37 + 11).astype(np.uint8), n), ROW),
    "noise": (lambda n: np.random.default_rng(n).integers(0, 256, size=n, dtype=np.uint8), 0),
    "filtered_rgb": (filtered_rgb, ROW),
}


def device_src(ctx, d, n, row):
    """fnx_deflate with a device source and a host stream"""
    lib = fennec_amd.load_library()
    out = np.empty(fennec_amd.deflate_bound(n), np.uint8)
    nb = C.c_size_t(0)
    rc = lib.fnx_deflate(ctx._h, fennec_amd.FNX_DEVICE_SRC, d.data_ptr(), n, row, out.ctypes.data, out.size, C.byref(nb))
    assert rc == 0, lib.fnx_last_error()
    return out[:nb.value].tobytes()


def round_trip(ctx, x, row=0):
    want = x.tobytes()
    d = dev(x)
    outs = []
    for _ in range(2):
        outs.append(ctx.deflate(x, row))
        t = ctx.deflate(d, row)
        ctx.sync()
        outs.append(t.cpu().numpy().tobytes())
        outs.append(device_src(ctx, d, x.size, row))
    assert all(o == outs[0] for o in outs), "host, device and device-source space, first and second call: identical bytes"
    assert zlib.decompress(outs[0]) == want, f"n = {len(x)}"
    assert len(outs[0]) <= fennec_amd.deflate_bound(len(x))
    return outs[0]


@pytest.mark.parametrize("name", sorted(CONTENTS))
def test_round_trip(ctx, name):
    gen, row = CONTENTS[name]
    for n in LENGTHS:
        round_trip(ctx, gen(n), row)
    assert ctx.last_kernel() == "deflate_dense_chunk_kernel"


# ---- the contract and the certificates on the device's streams -------------------------------------------------------------------
def run(ctx, x, row=0, label=""):
    stream = ctx.deflate(x, row)
    return stream, dd.contract_dense(stream, x.tobytes(), None, label)[1]


def test_code_limits_and_ties(ctx):
    dc.certify_limit15(run(ctx, dc.limit15(), 0, "limit15")[1], 0)
    stream, info = run(ctx, dc.ties(), 0, "ties")
    dc.certify_ties(info, 0, ip.probe(stream).blocks[0].ll_lengths)
    dc.certify_limit7(run(ctx, dc.limit7(), 0, "limit7")[1], 0)


def test_far_and_three_byte_matches(ctx):
    for name in sorted(dc.FAR):
        dc.certify_far(run(ctx, dc.far_match(name), 0, f"far {name}")[1], name)
    for dist in (4096, 4097):
        x, site = dc.three_bytes(dist)
        dc.certify_three_bytes(run(ctx, x, 0, f"three bytes {dist} back")[1], dist, site)


def test_forms_and_five_chunks(ctx):
    dc.certify_forms(run(ctx, dc.forms(), 0, "forms")[1])
    x = dc.many_chunks()[252 * CH:]
    assert x.size == 5 * CH + 5
    info = run(ctx, x, ROW, "many_chunks")[1]
    assert [r["btype"] for r in info[3:5]] == [ip.STORED, ip.STORED]


def test_what_the_dense_parse_adds(ctx):
    dd.certify_uncut(run(ctx, np.full(CH, 0x5A, np.uint8), 0, "constant")[1])
    dd.certify_edge_exact(run(ctx, dd.edge_exact(), 0, "A A")[1])
    dd.certify_edge_beyond(run(ctx, dd.edge_beyond(), 0, "A x A")[1])
    dd.certify_edge_two_back(run(ctx, dd.edge_two_back(), 0, "A B A")[1])
    dd.certify_lazy(run(ctx, dd.lazy_input(), 0, "lazy")[1])
    dd.certify_chain(run(ctx, dd.chain_input(), 0, "chain")[1])


@pytest.mark.parametrize("off", [1, 2, 3])
def test_pointers_that_are_not_dword_aligned(ctx, off):
    x = filtered_rgb(CH + 777)
    want = ctx.deflate(x, ROW)
    big = dev(np.concatenate([np.zeros(off, np.uint8), x]))
    out = dev(np.full(fennec_amd.deflate_bound(x.size) + 8, 0xAB, np.uint8))
    got = ctx.deflate(big[off:], ROW, out=out[off:])
    ctx.sync()
    assert got.cpu().numpy().tobytes() == want


# ---- against the host simulation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(RATIO_CASES))
def test_the_size_table_streams_are_the_host_simulations(ctx, name):
    stream = RATIO_CASES[name]()[0]
    flat = np.ascontiguousarray(stream).reshape(-1)
    out = ctx.deflate(dev(flat), stream.shape[1])
    ctx.sync()
    out = out.cpu().numpy().tobytes()
    assert zlib.decompress(out) == flat.tobytes()
    print(f"{name}: {flat.size} bytes -> dense {len(out)}, sha256 {hashlib.sha256(out).hexdigest()}")
    assert (flat.size, len(out), hashlib.sha256(out).hexdigest()) == TABLE[name]


# ---- level switching ---------------------------------------------------------------------------------------------------------
def test_level_switching(fast):
    lib = fennec_amd.load_library()
    c = fennec_amd.Context(0)
    x = filtered_rgb(2 * CH + 3)
    want_fast = fast.deflate(x, ROW)
    assert c.deflate(x, ROW) == want_fast and c.last_kernel() == "deflate_chunk_kernel"
    c.set_deflate_level(fennec_amd.FNX_DEFLATE_LEVEL_DENSE)
    dense = c.deflate(x, ROW)
    assert c.last_kernel() == "deflate_dense_chunk_kernel"
    assert len(dense) < len(want_fast) and zlib.decompress(dense) == x.tobytes()
    for bad in (-1, 2):                                               # refused, and the level stays
        assert lib.fnx_ctx_set_deflate_level(c._h, bad) == fennec_amd.FNX_ERR_INVALID and lib.fnx_last_error()
    with pytest.raises(fennec_amd.FennecError):
        c.set_deflate_level("densest")
    assert c.deflate(x, ROW) == dense
    c.set_deflate_level("fast")
    assert c.deflate(x, ROW) == want_fast and c.last_kernel() == "deflate_chunk_kernel"
    c.set_deflate_level("dense")
    assert c.deflate(x, ROW) == dense


# ---- capacity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("space", ["host", "device", "device_src"])
def test_capacity(ctx, space):
    lib = fennec_amd.load_library()
    x = filtered_rgb(CH + 777)
    want = ctx.deflate(x, ROW)
    src = x if space == "host" else dev(x)
    sptr = x.ctypes.data if space == "host" else src.data_ptr()
    sp = {"host": fennec_amd.FNX_HOST, "device": fennec_amd.FNX_DEVICE, "device_src": fennec_amd.FNX_DEVICE_SRC}[space]

    def call(cap):
        out = np.full(len(want) + 64, 0xAB, np.uint8)
        out = dev(out) if space == "device" else out
        nb = C.c_size_t(0)
        rc = lib.fnx_deflate(ctx._h, sp, sptr, len(x), ROW, out.data_ptr() if space == "device" else out.ctypes.data, cap, C.byref(nb))
        ctx.sync()
        return rc, nb.value, out if isinstance(out, np.ndarray) else out.cpu().numpy()
    rc, nb, out = call(len(want) - 1)                                # one byte short: the size, and nothing written
    assert rc == fennec_amd.FNX_ERR_INVALID and nb == len(want)
    assert (out == 0xAB).all()
    rc, nb, out = call(len(want))
    assert rc == 0 and nb == len(want) and out[:nb].tobytes() == want
    assert (out[nb:] == 0xAB).all(), "bytes behind the stream were written"


# ---- the PNG entries on a dense ctx --------------------------------------------------------------------------------------------
def palette_of(n, seed):
    pal = np.random.default_rng(seed).integers(0, 256, size=(n, 4), dtype=np.uint8)
    pal[:, 3] = 255
    if n > 2:
        pal[1, 3] = 40                                               # tRNS: up to and including entry 1
    return pal


def png_sources(w, h):
    """(name, source, kind, ncolors, palette): NRGBA, RGB (an opaque NRGBA image), gray, paletted with a tRNS"""
    rng = np.random.default_rng(1000 * w + h)
    ncolors = 2 if w * h == 1 else 16
    pal = palette_of(16, w)[:ncolors]
    if ncolors == 2:
        pal[0, 3] = 40
    return [("nrgba", ref.smooth_rgba(w, h, 31, opaque=False), FNX_PNG_NRGBA, 0, None),
            ("rgb", ref.smooth_rgba(w, h, 32, opaque=True), FNX_PNG_NRGBA, 0, None),
            ("gray", (rng.integers(0, 8, size=(h, w)) * 3 + np.arange(w)[None, :]).astype(np.uint8), FNX_PNG_GRAY, 0, None),
            ("paletted", ((np.arange(w)[None, :] // 4 + np.arange(h)[:, None] // 3) % ncolors).astype(np.uint8), FNX_PNG_PALETTED, ncolors, pal)]


@pytest.mark.parametrize("w,h", [(67, 41), (1, 1)])
def test_png_encode(ctx, fast, w, h):
    for name, src, kind, ncolors, pal in png_sources(w, h):
        file = ctx.png_encode(src, kind, ncolors, -1, pal)
        assert file == ctx.png_encode(dev(src), kind, ncolors, -1, pal), name
        assert ctx.last_kernel() == "deflate_dense_chunk_kernel"
        pixels = ref.decode_png(file)
        if kind == FNX_PNG_NRGBA:
            assert np.array_equal(pixels, src), name
        elif kind == FNX_PNG_GRAY:
            assert np.array_equal(pixels[..., 0], src) and np.array_equal(pixels[..., 2], src) and (pixels[..., 3] == 255).all()
        else:
            assert np.array_equal(pixels, pal[src]), name
            assert b"tRNS" in dict(ref.chunks(file))
        wstream = ref.png_stream(src, kind, ncolors)[0]
        idat = dict(ref.chunks(file))[b"IDAT"]
        dd.contract_dense(idat, np.ascontiguousarray(wstream).tobytes(), None, f"{name} {w} x {h}")
        other = fast.png_encode(src, kind, ncolors, -1, pal)
        assert len(file) <= len(other), f"{name} {w} x {h}: dense {len(file)} bytes, fast {len(other)}"
        assert ref.chunks(file)[:-2] == ref.chunks(other)[:-2]          # everything in front of IDAT


def compress_images():
    import test_png_filter_gpu as filter_tests
    two = filter_tests.two_colour(67, 41)
    gray = np.repeat(((np.arange(67)[None, :] * 3 + np.arange(41)[:, None] * 5) % 256).astype(np.uint8)[..., None], 4, axis=2)
    gray[..., 3] = 255
    return [ref.smooth_rgba(67, 41, 41, opaque=False), ref.smooth_rgba(67, 41, 42, opaque=True), gray, two,
            ref.smooth_rgba(1, 1, 43, opaque=False)]


def test_compress_png_with_the_device_deflate(ctx, fast):
    for i, img in enumerate(compress_images()):
        file = ctx.compress_png(img, device_deflate=True)
        assert file == ctx.compress_png(dev(img), device_deflate=True)
        assert np.array_equal(ref.decode_png(file), img), i
        assert len(file) <= len(fast.compress_png(img, device_deflate=True)), i
        assert ctx.compress_png(img) == fast.compress_png(img), "the host's deflate does not follow the level"


def test_png_compress_batch(ctx, fast):
    import test_png_filter_gpu as filter_tests
    imgs = [ref.smooth_rgba(1, 1, 51, opaque=True), filter_tests.two_colour(67, 41), ref.smooth_rgba(200, 100, 52, opaque=False)]
    files, kinds = ctx.png_compress_batch([dev(a) for a in imgs])
    assert "deflate_dense_chunk_batch_kernel" in ctx.last_kernel()
    assert kinds[1] == FNX_PNG_PALETTED and kinds[2] == FNX_PNG_NRGBA
    assert len(ip.probe(dict(ref.chunks(files[2]))[b"IDAT"]).blocks) == 5       # a stream of three chunks
    for i, img in enumerate(imgs):
        single = ctx.compress_png(dev(img), device_deflate=True)
        assert files[i] == single, f"image {i}: {len(files[i])} bytes, the single dense route {len(single)}"
        assert np.array_equal(ref.decode_png(files[i]), img), i
    other, _ = fast.png_compress_batch([dev(a) for a in imgs])
    assert len(files[2]) < len(other[2])
    assert "deflate_chunk_batch_kernel" in fast.last_kernel()
