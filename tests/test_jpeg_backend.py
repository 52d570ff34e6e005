"""The JPEG decoder's back half on the CPU: the arithmetic-level reference (tests/jpeg_backend_ref.py) against the real inverse DCT
where nothing wraps, the cases (tests/jpeg_backend_cases.py) against what they claim to reach -- by the reference's own record of
every wrapped operation -- and the oracle's IDCT and decoder against the reference on all of them.  The device's side:
test_jpeg_backend_gpu.py."""
from __future__ import annotations

import numpy as np
import pytest

import jpeg_backend_cases as bc
import jpeg_backend_ref as ref
from oracle import oracle as orc


def _nrgba(case):
    r = case.ref
    return np.ascontiguousarray(orc.ycbcr_to_nrgba(r.y, r.cb, r.cr, r.ratio)[:case.h, :case.w])


# ------------------------------------------------------------------------------------------------------- the reference itself
def test_wrap32_is_twos_complement():
    x = np.array([0, 2**31 - 1, 2**31, -2**31, -2**31 - 1, 2**32 + 5, 2841 * 2**31], np.int64)
    assert ref.wrap32(x).tolist() == [0, 2**31 - 1, -2**31, -2**31, 2**31 - 1, 5, -2**31]
    o = ref.Ops((2,))
    assert o.shl(np.array([1, -1]), 31).tolist() == [-2**31, -2**31] and o.hit.tolist() == [True, False]
    assert o.shr(np.array([-1, -256]), 8).tolist() == [-1, -1]


def test_reference_against_the_real_idct_where_nothing_wraps():
    """test_jpeg_roundtrip.py's bound for idct.go's passes against the orthonormal inverse DCT: within 1"""
    fft = pytest.importorskip("scipy.fft")
    rng = np.random.default_rng(0)
    blocks = []
    for k in range(300):                                             # the coefficients a decoder meets, as that test makes them
        x = rng.integers(0, 256, (8, 8))
        if k % 4 == 1:
            x = np.tile(x[:1], (8, 1))                               # rows alike: rows 1 .. 7 of the coefficients are nothing
        elif k % 4 == 2:
            x = np.tile(x[:, :1], (1, 8))                            # columns alike: every row is its first entry alone
        elif k % 4 == 3:
            x = np.full((8, 8), x[0, 0])
        step = int(rng.integers(1, 64))
        blocks.append(np.rint(fft.dctn((x - 128).astype(float), norm="ortho") / step) * step)
    blocks = np.array(blocks).astype(np.int64).reshape(-1, 64)
    assert ((blocks.reshape(-1, 8, 8)[:, :, 1:] == 0).all(axis=2).sum(axis=1) == 8).sum() >= 100
    pre, hit = ref.idct(blocks)
    assert not hit.any()
    want = fft.idctn(blocks.reshape(-1, 8, 8).astype(np.float64), axes=(1, 2), norm="ortho").reshape(-1, 64)
    assert np.abs(pre - want).max() <= 1.0 + 1e-9
    # where nothing wraps the shortcut changes nothing: ((dc << 11) + 128) >> 8 is dc << 3
    assert np.array_equal(ref.idct(blocks, row_shortcut=False)[0], pre)


def test_reference_places_the_blocks_of_every_sampling():
    """a flat block per scan position whose level is its index: the planes must show the MCU's layout, restart or not"""
    for samp in [None] + list(bc.SAMPLINGS.values()):
        hy, vy = samp or (1, 1)
        per = hy * vy + (2 if samp else 0)
        n = 6 * per                                                  # 3 x 2 MCUs
        abs_dc = 8 * (np.arange(n) - 100)                            # level shift: sample = index + 28
        for restart in (0, 2):
            zz = np.zeros((n, 64), np.int64)
            comp = [0] * (hy * vy) + [1, 2][:per - hy * vy]
            pred = {}
            for i in range(n):
                if restart and i % (restart * per) == 0:
                    pred = {}
                c = comp[i % per]
                zz[i, 0] = abs_dc[i] - pred.get(c, 0)
                pred[c] = abs_dc[i]
            r = ref.decode(zz, [[1] * 64], 24 * hy, 16 * vy, samp, restart)
            assert r.dc.tolist() == abs_dc.tolist() and not r.wrapped.any()
            for m in range(6):
                my0, mx0 = divmod(m, 3)
                for j in range(hy * vy):
                    tile = r.y[8 * (vy * my0 + j // hy):, 8 * (hy * mx0 + j % hy):][:8, :8]
                    assert (tile == m * per + j + 28).all(), (samp, m, j)
                if samp:
                    assert (r.cb[8 * my0:8 * my0 + 8, 8 * mx0:8 * mx0 + 8] == m * per + hy * vy + 28).all()
                    assert (r.cr[8 * my0:8 * my0 + 8, 8 * mx0:8 * mx0 + 8] == m * per + hy * vy + 29).all()


# ------------------------------------------------------------------------------------------------------- what the cases reach
def test_a_chains_leave_16_bits_and_wrap_where_the_arithmetic_says():
    files = bc.group_a()
    for name in ("a_up_40", "a_down_40", "a_cross_and_back", "a_until_the_idct_wraps", "a_cb_only", "a_cr_only"):
        assert files[name].leaves16, name
    assert files["a_up_40"].ref.dc.tolist() == [2047 * k for k in range(1, 41)]
    assert (files["a_down_40"].ref.dc == -files["a_up_40"].ref.dc).all() and len(files["a_up_40"].data) == 472
    dc = files["a_cross_and_back"].ref.dc
    assert dc.max() > 32767 and dc.min() < -32768 and dc[-1] == 0
    for name, loud, quiet in (("a_cb_only", 1, 2), ("a_cr_only", 2, 1)):
        r = files[name].ref
        assert np.abs(r.dc[r.comp == loud]).max() > 32767 and r.dc[r.comp == loud][-1] == 0
        assert np.abs(r.dc[r.comp == quiet]).max() < 64 and np.abs(r.dc[r.comp == 0]).max() < 1024
    # every block of (a) is a DC alone: the reference's flags are exactly what dc_only_block_wraps works out
    for name, case in files.items():
        assert not case.zz[:, 1:].any() and case.qtabs == [bc.Q_ONES]
        assert np.array_equal(case.ref.wrapped, bc.dc_only_block_wraps(case.ref.dc)), name
    wrapped = files["a_until_the_idct_wraps"].ref.wrapped
    assert not wrapped[:512].any() and wrapped[512:].all() and len(wrapped) == 640            # 2047 x 513 >= 2^20
    for name, case in files.items():
        if name != "a_until_the_idct_wraps":
            assert not case.ref.wrapped.any(), name


def test_a_restart_files_start_the_dc_over_inside_an_mcu_row():
    files = bc.group_a()
    for tag in ["grey"] + list(bc.SAMPLINGS):
        case = files["a_rst_" + tag]
        cr = case.cr
        assert (cr.mx, cr.my, case.restart) == (3, 3, 2) and len(cr.rst) == 4
        assert case.w % 8 and case.h % 8                                    # the image ends inside its last blocks
        dc = case.ref.dc
        assert len(set(dc.tolist())) == len(dc) and 0 not in dc              # distinct, and a carried prediction would show
        assert np.abs(dc).max() <= 1016                                       # ... as a sample: none saturates under a quantiser of 1
        pix = case.ref.pix
        assert len({int(p[0]) for p in pix}) == len(dc) and (pix == pix[:, :1]).all()
        # without the restart the same differences give other DCs from the second interval on
        other = ref.decode(case.zz, case.qtabs, case.w, case.h, case.sampling, 0).dc
        first = 2 * cr.nslots
        assert (other[:first] == dc[:first]).all() and (other[first:] != dc[first:]).all()


def test_b_d_e_blocks_wrap_and_stay_unsaturated():
    total = {}
    for g in ("b", "d", "e"):
        for name, case in getattr(bc, "group_" + g)().items():
            r = case.ref
            uns = ref.unsaturated(r.pix)[case.kept]
            print(f"{name}: {len(case.kept)} kept of {len(case.zz)} blocks, unsaturated samples per kept block min {uns.min()} mean {uns.mean():.1f}")
            assert len(case.kept) and (uns >= bc.MIN_UNSATURATED).all(), (name, uns)
            assert r.wrapped[case.kept].all(), name
            total[g] = total.get(g, 0) + len(case.kept)
    assert total["d"] >= 32 and total["b"] >= 16 and total["e"] >= 16, total
    for name, case in bc.group_b().items():
        dcs = np.abs(case.ref.dc[case.kept])
        assert case.qtabs[0][0] == 255 and dcs.min() >= 3 * 2047 and (np.abs(dcs - 2047 * np.rint(dcs / 2047)) < 1024).all()
        assert (case.zz[case.kept, 1:] != 0).any(axis=1).all()            # AC beside it
    for name, case in bc.group_d().items():
        assert all(min(q) >= 192 and max(q) == 255 for q in case.qtabs) and np.abs(case.zz[:, 1:]).max() <= 1023
    assert len(bc.group_d()["d_420"].qtabs) == 2 and bc.group_d()["d_420"].sampling == (2, 2) and bc.group_d()["d_grey"].sampling is None


def test_c_the_product_passes_int32_after_block_4114():
    case = bc.group_c()["c_product_wraps"]
    assert (case.w, case.h, len(case.zz)) == (520, 512, 4160) and (case.zz[:, 0] == 2047).all() and case.qtabs[0][0] == 255
    assert 2047 * 4114 * 255 < 2**31 <= 2047 * 4115 * 255
    r = case.ref
    assert not r.wrapped_dequant[:4114].any() and r.wrapped_dequant[4114:].all()
    # the first two blocks fit throughout (2047 x 2 x 255 < 2^20: the column pass's << 8 of dc << 3 stays inside); every other wraps
    assert not r.wrapped[:2].any() and r.wrapped[2:].all()
    assert len(case.data) < 20000


def test_e_sizes_and_the_rows_that_need_the_shortcut():
    case = bc.group_e()["e_grey"]
    sizes = {int(abs(int(v))).bit_length() for v in case.zz[:, 1:].ravel() if v}
    assert {11, 12, 13, 14, 15} <= sizes, sizes
    assert all(s in bc.E_AC.codes for s in [0x00, 0xf0] + [(r << 4) | n for r in range(16) for n in range(1, 16)])
    with pytest.raises(AssertionError):                                  # the writer's default stays at size 10
        bc.jc.encode(case.coef, case.w, case.h, [bc.K_DC], [bc.E_AC], qtabs=case.qtabs)
    r = case.ref
    rows = bc.e_first_of_row_blocks()
    assert sorted({k for _, k in rows}) == [8, 16, 24, 32, 40, 48, 56]
    without = ref.decode(case.zz, case.qtabs, case.w, case.h, row_shortcut=False)
    # dc << 3 and ((dc << 11) + 128) >> 8 part ways here, by a multiple of 2^24.  The column pass multiplies rows 1, 2, 3, 5, 6, 7
    # by its constants, which keeps that apart; rows 0 and 4 it shifts by 8, where a multiple of 2^24 is gone: position 32 is
    # in the file for the decoding, and cannot tell the two paths apart
    shows = 0
    for i, k in rows:
        row = r.dequant[i, k:k + 8]
        assert abs(int(row[0])) >= 1 << 20 and not row[1:].any(), (i, k)
        assert (without.pre[i] != r.pre[i]).any() == (k != 32), (i, k)
        shows += int((without.pix[i] != r.pix[i]).any())
    # ... and in samples that are not saturated: a decoder without the shortcut cannot pass the comparison
    print(f"e_grey: the shortcut shows in the samples of {shows} of {len(rows)} first-of-row blocks")
    assert shows >= len(rows) // 2


def test_f_samples_far_beyond_the_clamp_in_both_directions():
    """The column pass ends in >> 14 of an int32: no sample before the clamp can lie beyond +-2^17, whatever the coefficients.
    These blocks reach beyond +-2^16, half of that range, below and above in the same block, and every sample of them saturates."""
    case = bc.group_f()["f_far_clamp"]
    r = case.ref
    assert np.abs(r.pre).max() < 1 << 17
    assert (r.pre.min(axis=1) < -bc.FAR).all() and (r.pre.max(axis=1) > bc.FAR).all()
    assert set(np.unique(r.pix).tolist()) == {0, 255}


# ------------------------------------------------------------------------------------------------------- the oracle
def test_oracle_idct_against_the_reference():
    """exact, and before the clamp: every sample counts"""
    n = 0
    for g in ("b", "d", "e", "f"):
        for name, case in getattr(bc, "group_" + g)().items():
            r = case.ref
            for i in range(len(r.dequant)):
                assert np.array_equal(orc.jpeg_idct(r.dequant[i]).reshape(64), r.pre[i]), (name, i)
                n += 1
    assert n >= 150


@pytest.mark.parametrize("group", ["a", "b", "c", "d", "e", "f"])
def test_oracle_decoder_against_the_reference(group):
    for name, case in getattr(bc, "group_" + group)().items():
        r = case.ref
        out = orc.jpeg_decode_planes(case.data, with_coefficients=True)
        assert out[:3] == (case.w, case.h, r.ratio), name
        assert np.array_equal(out[3], r.y), name
        if r.cb is not None:
            assert np.array_equal(out[4], r.cb) and np.array_equal(out[5], r.cr), name
        # the coefficients come back as int16: the DC's low 16 bits where the chain has left them
        coef = case.coef.copy()
        coef[:, 0] = r.dc
        assert np.array_equal(out[6], coef.astype(np.int16)), name
        assert np.array_equal(orc.jpeg_decode(case.data), _nrgba(case)), name


# ------------------------------------------------------------------------------------------------------- the front half on (e)
def test_hostsim_reads_ac_values_of_size_11_to_15(tmp_path):
    """what the back half is given: jpeg_dec_span.inc's write pass on the CPU (tools/jpeg_dec_hostsim, a stand-alone program under
    ASan and UBSan) leaves (e)'s coefficients as the writer coded them -- int16 holds every AC value up to size 15"""
    from test_jpeg_dec_hostsim import Sim
    sim = Sim(tmp_path)
    for name, case in bc.group_e().items():
        r = sim.run(name, case.data)
        assert r["exit"] == 0 and r["route"] == "device" and r["err"] == 0 and r["stderr"] == "", (name, r["exit"], r["stderr"])
        nat = np.zeros_like(case.zz)
        nat[:, bc.ZIG] = case.zz                                       # natural order, the DC still as the difference
        assert np.abs(nat).max() > 16384 and np.array_equal(r["coef"], nat), name
        assert r["replay_ok"] == 1, name
