"""fnx_crc32 on the GPU (Context.crc32; crc32.hip): crc32_cases.py's list -- the one tools/crc32_hostsim runs on the CPU -- from
device tensors sliced at every alignment and from host arrays, against zlib.crc32."""
from __future__ import annotations

import zlib

import numpy as np
import pytest

import crc32_cases as cc
import fennec_amd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


@pytest.fixture(scope="module")
def resident():
    """blob -> [the blob 0..7 bytes behind an aligned address, as device tensors of 16 + len bytes]"""
    import torch
    out = {}
    for key, data in cc.blobs().items():
        out[key] = []
        for offset in range(8):
            host = np.full(16 + len(data), 0x5a, np.uint8)
            host[offset:offset + len(data)] = np.frombuffer(data, np.uint8)
            out[key].append(torch.from_numpy(host).cuda())
    torch.cuda.synchronize()
    return out


def test_device_tensors_at_every_alignment(ctx, resident):
    wrong = []
    for name, offset, length, seed, key, want in cc.cases():
        t = resident[key][offset]
        assert t.data_ptr() % 16 == 0
        got = ctx.crc32(t[offset:offset + length], seed)
        if got != want:
            wrong.append((name, f"{got:08x}", f"{want:08x}"))
    assert not wrong, wrong[:10]
    assert ctx.last_kernel() == "crc32_pieces_kernel"


def test_host_arrays_and_bytes(ctx):
    blobs = cc.blobs()
    wrong = []
    for name, offset, length, seed, key, want in cc.cases():
        if offset not in (0, 3) and length not in (cc.RUN + 1, cc.PIECE + 1):      # (the host bytes are uploaded to an aligned slot)
            continue
        host = np.frombuffer(blobs[key], np.uint8)[:length]
        got = ctx.crc32(host if offset else bytes(host), seed)
        if got != want:
            wrong.append((name, f"{got:08x}", f"{want:08x}"))
    assert not wrong, wrong[:10]
    assert ctx.last_kernel() == "crc32_pieces_kernel"


def test_no_byte_answers_the_seed_without_a_launch():
    import torch
    ctx = fennec_amd.Context(0)
    for seed in cc.SEEDS:
        assert ctx.crc32(b"", seed) == seed
        assert ctx.crc32(torch.empty(0, dtype=torch.uint8, device="cuda"), seed) == seed
    assert ctx.last_kernel() == ""


def test_a_crc_continues_across_calls_and_more_pieces_than_lanes(ctx):
    """5 MiB: more pieces than the fold kernel has lanes; and the split law through the seed of a second call"""
    import torch
    data = np.random.default_rng(8).integers(0, 256, 5 * (1 << 20) + 77, dtype=np.uint8)
    t = torch.from_numpy(data).cuda()
    torch.cuda.synchronize()
    want = zlib.crc32(data.tobytes())
    assert ctx.crc32(t) == want
    cut = 3 * cc.PIECE + 1
    assert ctx.crc32(t[cut:], ctx.crc32(t[:cut])) == want


def test_bad_arguments_are_refused(ctx):
    import ctypes as C
    lib, out = fennec_amd.load_library(), C.c_uint32(7)
    data = np.zeros(4, np.uint8)
    assert lib.fnx_crc32(ctx._h, fennec_amd.FNX_DEVICE_SRC, data.ctypes.data, 4, 0, C.byref(out)) == fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_crc32(ctx._h, fennec_amd.FNX_HOST, None, 4, 0, C.byref(out)) == fennec_amd.FNX_ERR_INVALID
    assert lib.fnx_crc32(ctx._h, fennec_amd.FNX_HOST, data.ctypes.data, 4, 0, None) == fennec_amd.FNX_ERR_INVALID
    assert out.value == 7
    with pytest.raises(fennec_amd.FennecError):
        ctx.crc32(np.zeros((2, 2), np.uint8))
