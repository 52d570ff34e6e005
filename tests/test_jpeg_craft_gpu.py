"""The crafted JPEG files of tests/jpeg_craft_cases.py on the device: fnx_jpeg_decode and fnx_jpeg_decode_batch against the
checker's decode, byte for byte, with the route asserted by name -- the crafted tables must go through jpeg_dec.hip's Huffman
decoder, not the host's scans.  What each file reaches is proved on the CPU (test_jpeg_craft.py: the symbol map;
test_jpeg_dec_hostsim.py: the lane body per coefficient)."""
from __future__ import annotations

import os
import re
import time

import numpy as np
import pytest

import jpeg_craft_cases as cs
from fennec_amd import synth
from oracle import oracle as orc

DEVICE_ROUTE, BATCH_ROUTE = "jpeg_dsync_kernel", "jpeg_dsync_batch_kernel"


@pytest.fixture(scope="module")
def ctx():
    import fennec_amd
    return fennec_amd.Context(0)


@pytest.fixture(scope="module")
def ordinary():
    """files of the project's own encoder, for the mixed lists"""
    return [orc.jpeg_encode(synth.large_photo(200 + 24 * k, 136 + 8 * k, k), 60 + 15 * k) for k in range(2)]


def _decode_on_the_device_route(ctx, data):
    import fennec_amd
    got = ctx.jpeg_decode(data)
    assert ctx.last_kernel(fennec_amd.PROF_JPEG) == DEVICE_ROUTE
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("group", ["a", "b", "c", "d", "e", "f_small"])
def test_gpu_decode_of_the_crafted_files(ctx, group):
    for name, cr in getattr(cs, "group_" + group)().items():
        got = _decode_on_the_device_route(ctx, cr.data)
        assert np.array_equal(got, orc.jpeg_decode(cr.data)), name


@pytest.mark.gpu
def test_gpu_batch_of_a_mixed_list_equals_the_single_calls(ctx, ordinary):
    import fennec_amd
    pick = [cs.group_a()["a_all_and_gaps"], cs.group_a()["a_long_and_255"], cs.group_b()["b_shift_37"], cs.group_b()["b_big_16"],
            cs.group_c()["c_shift_1"], cs.group_c()["c_shift_1_rst"], cs.group_d()["d_4096_blocks"], cs.group_d()["d_last_byte_padded"],
            cs.group_e()["e_grey"], cs.group_e()["e_410"], cs.group_e()["e_every_byte"], cs.group_f_small()["f_4wg"],
            cs.group_f_small()["f_4wg_rst"]]
    files = [ordinary[0]] + [cr.data for cr in pick[:7]] + [ordinary[1]] + [cr.data for cr in pick[7:]]
    single = [ctx.jpeg_decode(f) for f in files]
    images, status = ctx.jpeg_decode_batch(files)
    assert ctx.last_kernel(fennec_amd.PROF_JPEG) == BATCH_ROUTE
    assert status == [fennec_amd.FNX_OK] * len(files)
    for i, (a, b) in enumerate(zip(images, single)):
        assert np.array_equal(a, b), i
    # the stream that never falls into step without restart intervals around it: a list whose launches take the plain forms
    files = [ordinary[0], cs.group_f_small()["f_4wg"].data, cs.group_c()["c_shift_2"].data]
    images, status = ctx.jpeg_decode_batch(files)
    assert status == [fennec_amd.FNX_OK] * 3 and all(np.array_equal(a, ctx.jpeg_decode(f)) for a, f in zip(images, files))


@pytest.mark.gpu
def test_gpu_the_stream_that_never_falls_into_step(ctx, capfd):
    """(f) at 3648 x 3648: 68 workgroups, each one's chain of corrections takes all 256 passes, and every round across workgroups
    rights exactly one of them -- beyond the 64 round flags, so the rewind runs.  The trace line says so."""
    big = cs.f_big()
    want = orc.jpeg_decode(big.data)
    old = os.environ.get("FNX_JPEG_TRACE")
    os.environ["FNX_JPEG_TRACE"] = "1"
    try:
        capfd.readouterr()
        t0 = time.perf_counter()
        got = _decode_on_the_device_route(ctx, big.data)
        wall = time.perf_counter() - t0
        err = capfd.readouterr().err
    finally:
        if old is None:
            del os.environ["FNX_JPEG_TRACE"]
        else:
            os.environ["FNX_JPEG_TRACE"] = old
    lines = [ln for ln in err.splitlines() if ln.startswith("[fennec jpeg] 3648 x 3648")]
    assert lines, err
    m = re.search(r"(\d+) lanes in (\d+) workgroups: passes max (\d+) .* cross-workgroup rounds (\d+)", lines[-1])
    assert m, lines[-1]
    lanes, nwg, passes, rounds = (int(v) for v in m.groups())
    print(f"never-in-step 3648 x 3648: {lanes} lanes, {nwg} workgroups, passes max {passes}, rounds {rounds}, decode call {wall * 1e3:.1f} ms")
    assert (lanes, nwg) == (16245, 68)
    assert passes == 256 and rounds > 64
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_gpu_damaged_by_construction(ctx):
    import fennec_amd
    g = cs.group_g()
    for name in ("g_run_past_63", "g_code_outside_table"):
        with pytest.raises(fennec_amd.FennecError) as e:
            ctx.jpeg_decode(g[name][0].data)
        assert not isinstance(e.value, fennec_amd.FennecUnsupported), name           # FNX_ERR_INVALID
    with pytest.raises(fennec_amd.FennecError) as e:                                # two bits a block, one byte short
        ctx.jpeg_decode(cs.d_cut())
    assert not isinstance(e.value, fennec_amd.FennecUnsupported)
    # an interval whose blocks end 16 (3) bytes before its marker: refused, or every block -- the next interval's too -- as written
    for name in ("g_ends_16_early", "g_ends_3_early"):
        cr, twin = g[name]
        try:
            got = ctx.jpeg_decode(cr.data)
        except fennec_amd.FennecError as e:
            assert not isinstance(e, fennec_amd.FennecUnsupported), name
            continue
        assert np.array_equal(got, orc.jpeg_decode(twin.data)), name
    images, status = ctx.jpeg_decode_batch([g["g_ends_16_early"][0].data, g["g_ends_16_early"][1].data, g["g_run_past_63"][0].data])
    assert status[1] == fennec_amd.FNX_OK and status[2] == fennec_amd.FNX_ERR_INVALID
    assert status[0] in (fennec_amd.FNX_OK, fennec_amd.FNX_ERR_INVALID)
    if status[0] == fennec_amd.FNX_OK:
        assert np.array_equal(images[0], images[1])
    # and the ctx still works
    cr = cs.group_c()["c_shift_0"]
    assert np.array_equal(ctx.jpeg_decode(cr.data), orc.jpeg_decode(cr.data))


@pytest.mark.gpu
def test_gpu_the_host_scan_route_says_so(ctx):
    """the same crafted scan under an SOF1 marker is the host decoder's to read (jpeg_prog.cpp): the same pixels, and a route name
    that cannot be mistaken for the device decoder's"""
    import fennec_amd
    cr = cs.group_c()["c_shift_0"]
    i = cr.data.index(b"\xff\xc0")
    sof1 = cr.data[:i + 1] + b"\xc1" + cr.data[i + 2:]
    got = ctx.jpeg_decode(sof1)
    route = ctx.last_kernel(fennec_amd.PROF_JPEG)
    assert "host" in route and "dsync" not in route, route
    assert np.array_equal(got, orc.jpeg_decode(cr.data))
    assert np.array_equal(_decode_on_the_device_route(ctx, cr.data), got)
