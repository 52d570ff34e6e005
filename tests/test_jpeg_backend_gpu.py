"""The back half of the device JPEG decoder -- jpeg_dc_gather_kernel, the DC prefix sum, jpeg_didct_kernel /
jpeg_didct_batch_kernel (dec_idct_body) and jpeg_idct.hpp's passes -- against the arithmetic-level reference
(tests/jpeg_backend_ref.py) on the files of tests/jpeg_backend_cases.py: DC chains beyond 16 bits, products and IDCT operations
that wrap int32, AC sizes up to 15, restart intervals across MCU rows for every sampling.  What each file reaches is proved on
the CPU (test_jpeg_backend.py); here the pixels, byte for byte, with the route asserted by name."""
from __future__ import annotations

import numpy as np
import pytest

import jpeg_backend_cases as bc
from fennec_amd import synth
from oracle import oracle as orc

DEVICE_ROUTE, BATCH_ROUTE = "jpeg_dsync_kernel", "jpeg_dsync_batch_kernel"
GROUPS = ["a", "b", "c", "d", "e", "f"]


@pytest.fixture(scope="module")
def ctx():
    import fennec_amd
    return fennec_amd.Context(0)


@pytest.fixture(scope="module")
def want():
    """name -> the reference's image: toNRGBARef of its planes, cropped (the colour conversion has its own tests)"""
    out = {}
    for name, case in bc.all_cases().items():
        r = case.ref
        out[name] = np.ascontiguousarray(orc.ycbcr_to_nrgba(r.y, r.cb, r.cr, r.ratio)[:case.h, :case.w])
    return out


@pytest.fixture(scope="module")
def ordinary():
    """files of the project's own encoder, for the mixed lists"""
    return [orc.jpeg_encode(synth.large_photo(200 + 24 * k, 136 + 8 * k, k), 60 + 15 * k) for k in range(2)]


def _drifts(name):
    """the files whose DC sums leave 16 bits: (a)'s chains and (c)"""
    return bc.all_cases()[name].leaves16 and name[0] in "ac"


@pytest.mark.gpu
@pytest.mark.parametrize("group", GROUPS)
def test_gpu_single_decodes_equal_the_reference(ctx, want, group):
    import fennec_amd
    for name, case in getattr(bc, "group_" + group)().items():
        got = ctx.jpeg_decode(case.data)
        assert ctx.last_kernel(fennec_amd.PROF_JPEG) == DEVICE_ROUTE, name
        assert got.shape == want[name].shape, name
        bad = np.argwhere((got != want[name]).any(axis=2))
        assert len(bad) == 0, (name, len(bad), bad[:4].tolist(), got[tuple(bad[0])].tolist(), want[name][tuple(bad[0])].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_gpu_batch_decodes_keep_each_files_dc_sums_apart(ctx, want, ordinary, where):
    """the batch IDCT takes a file's DC as a difference of two bases of a prefix sum over the whole chunk's blocks: (c)'s 8.5
    million and (a)'s chains in front of, between and behind the other files must not reach them"""
    import fennec_amd
    names = list(bc.all_cases())
    drift, rest = [n for n in names if _drifts(n)], [n for n in names if not _drifts(n)]
    assert {"a_up_40", "a_down_40", "a_cross_and_back", "a_until_the_idct_wraps", "a_cb_only", "a_cr_only", "c_product_wraps"} == set(drift)
    half = len(rest) // 2
    order = {"first": drift + rest, "middle": rest[:half] + drift + rest[half:], "last": rest + drift}[where]
    files = [(n, bc.all_cases()[n].data) for n in order]
    files.insert(len(files) // 3, ("ordinary 0", ordinary[0]))
    files.insert(2 * len(files) // 3, ("ordinary 1", ordinary[1]))
    single = [ctx.jpeg_decode(f) for _, f in files]
    images, status = ctx.jpeg_decode_batch([f for _, f in files])
    assert ctx.last_kernel(fennec_amd.PROF_JPEG) == BATCH_ROUTE
    assert status == [fennec_amd.FNX_OK] * len(files)
    for (name, f), img, one in zip(files, images, single):
        assert np.array_equal(img, one), name
        assert np.array_equal(img, want[name] if name in want else orc.jpeg_decode(f)), name


@pytest.mark.gpu
def test_gpu_host_scan_route_gives_the_reference_or_refuses(ctx, want):
    """the same scans under an SOF1 marker are the host decoder's to read (jpeg_prog.cpp), into int16: the reference's pixels or
    FennecUnsupported, never other pixels -- and FennecUnsupported ("coefficients beyond 16 bits") where a DC leaves 16 bits"""
    import fennec_amd
    decoded = refused = 0
    for name, case in bc.all_cases().items():
        i = case.data.index(b"\xff\xc0")
        sof1 = case.data[:i + 1] + b"\xc1" + case.data[i + 2:]
        try:
            got = ctx.jpeg_decode(sof1)
        except fennec_amd.FennecUnsupported:
            refused += 1
            continue
        route = ctx.last_kernel(fennec_amd.PROF_JPEG)
        assert "host" in route and "dsync" not in route, (name, route)
        assert not case.leaves16, name
        assert np.array_equal(got, want[name]), name
        decoded += 1
    print(f"host scan route: {decoded} files decoded to the reference's pixels, {refused} refused")
    assert refused >= sum(c.leaves16 for c in bc.all_cases().values()) and decoded >= 7, (decoded, refused)
