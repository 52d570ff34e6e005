"""The crafted JPEG files of tests/jpeg_craft_cases.py on the CPU: the checker (the oracle's decoder) reads back exactly the
coefficients the writer coded, libjpeg (where Pillow imports) lands within the IDCTs' spread of the checker's pixels, and the symbol
map proves that every file puts its symbols where its case says -- the code lengths used, the bit phases, the pairs of the sync
tables, the paddings, the streams that never fall into step (by the state walker).  The device's side: test_jpeg_craft_gpu.py;
the lane body on the CPU: test_jpeg_dec_hostsim.py."""
from __future__ import annotations

import io

import numpy as np
import pytest

import jpeg_craft as jc
import jpeg_craft_cases as cs
from jpeg_craft import OWN, SPAN, WARM
from oracle import oracle as orc


def _ends(cr):
    s = cr.sym
    return s["start"] + s["clen"] + s["size"]


# ------------------------------------------------------------------------------------------------------- the writer and the checker
def test_writer_refuses_a_table_with_an_all_ones_code():
    with pytest.raises(ValueError):
        jc.Table([2] + [0] * 15, [0, 1])                       # 0 and 1
    with pytest.raises(ValueError):
        jc.Table([1, 2] + [0] * 14, [0, 1, 2])                 # 0, 10, 11
    jc.Table([1, 1] + [0] * 14, [0, 1])                        # 0, 10: 11 stays free


def test_oracle_reads_back_the_coefficients_of_every_case():
    cases = dict(cs.sound_groups())
    cases["f_big"] = cs.f_big()
    assert len(cases) >= 80
    for name, cr in cases.items():
        out = orc.jpeg_decode_planes(cr.data, with_coefficients=True)
        assert (out[0], out[1]) == (cr.w, cr.h), name
        assert np.array_equal(out[-1], cr.coef), name


def test_oracle_refuses_the_damaged_files():
    for name, (cr, twin) in cs.group_g().items():
        with pytest.raises(RuntimeError):
            orc.jpeg_decode(cr.data)
        if twin is not None:
            orc.jpeg_decode(twin.data)
    with pytest.raises(RuntimeError):
        orc.jpeg_decode(cs.d_cut())


def _within_libjpegs_range_limit(cr):
    """libjpeg clamps a sample through a table that is right for level-shifted IDCT outputs of -384 .. 639 and WRAPS beyond (jdmaster.c,
    prepare_range_limit_table), where Go -- and the checker -- clamp whatever the value: a file is comparable when every block's
    IDCT output, by the checker's own IDCT before its clamp, stays inside that range by 8 (the IDCTs differ by a level or two)"""
    nat = np.zeros((len(cr.coef), 64), np.int32)
    nat[:, jc.ZIG] = cr.coef                                         # (every case's quantisation tables are all ones)
    for blk in np.unique(nat, axis=0):
        out = orc.jpeg_idct(blk) + 128
        if out.min() < -376 or out.max() > 631:
            return False
    return True


def test_libjpeg_agrees_within_the_idct_spread():
    """test_jpeg_decode.py's bounds for libjpeg against the checker: one component max 2 (islow IDCT against idct.go's); 4:2:0
    mean < 1.6 and 99th percentile <= 12 (fancy upsampling); 4:1:0 mean < 0.3, max 4 -- for every sound case whose samples libjpeg's
    range limiting can represent (the files of wild coefficients are held by their coefficients above, not by pixels)"""
    Image = pytest.importorskip("PIL.Image")
    compared = set()
    for name, cr in cs.sound_groups().items():
        if not _within_libjpegs_range_limit(cr):
            continue
        ratio = orc.jpeg_decode_planes(cr.data)[2]
        im = Image.open(io.BytesIO(cr.data))
        want = orc.jpeg_decode(cr.data)
        if ratio < 0:
            d = np.abs(np.asarray(im.convert("L")).astype(int) - want[..., 0].astype(int))
            assert d.max() <= 2, (name, d.max())
        else:
            d = np.abs(np.asarray(im.convert("RGB")).astype(int) - want[..., :3].astype(int))
            if ratio == 5:
                assert d.mean() < 0.3 and d.max() <= 4, (name, d.mean(), d.max())
            else:
                assert d.mean() < 1.6 and np.percentile(d, 99) <= 12, (name, d.mean())
        compared.add((name[0], ratio))
    print("compared with libjpeg:", sorted(compared))
    assert {("c", -1), ("d", -1), ("e", -1), ("e", 5), ("f", -1)} <= compared, compared


# ------------------------------------------------------------------------------------------------------- (a) code lengths
def test_a_every_long_code_length_is_used_under_every_table_selector():
    files = cs.group_a()
    want = {"a_all_and_gaps": {0: {12, 13, 14, 15, 16}, 2: {12, 13, 14, 15, 16}, 1: {13, 16}, 3: {13, 16}},
            "a_long_and_255": {0: {12, 14}, 2: {12, 16}, 1: {12}, 3: {12}},
            "a_swapped": {0: {13, 16}, 2: {12}, 1: {12, 13, 14, 15, 16}, 3: {12, 16}}}
    for name, per_tab in want.items():
        s = files[name].sym
        assert (files[name].w, files[name].h, files[name].nslots) == (64, 64, 6)
        for tab, lengths in per_tab.items():
            used = set(np.unique(s["clen"][s["tab"] == tab]).tolist())
            assert lengths <= used, (name, tab, used)
            if name == "a_long_and_255" and tab in (0, 2):
                assert min(used) == 12                               # no code the fast tables hold: every look-up counts
    s = files["a_all_and_gaps"].sym
    assert set(np.unique(s["clen"][s["tab"] == 2]).tolist()) == set(range(1, 17))
    s = files["a_long_and_255"].sym
    assert len(cs.A_AC_255.values) == 255 and len(np.unique(s["sym"][s["tab"] == 3])) > 60
    # the value index of a long code reaches past 127 and 240: delta[] + the code, & 255
    idx = [cs.A_AC_255.values.index(int(v)) for v in np.unique(s["sym"][(s["tab"] == 3) & (s["clen"] == 12)])]
    assert max(idx) > 240 and min(idx) < 40


# ------------------------------------------------------------------------------------------------------- (b) bit phase
def test_b_the_probe_lands_on_every_phase_and_on_the_borders():
    files = cs.group_b()
    assert len(files) == 64 + len(cs.BIG_SHIFTS)
    probe = cs.from_diffs(cs.probe_blocks())
    cats = {int(abs(int(d))).bit_length() for d in np.diff(np.concatenate([[0], probe[:, 0]]))}
    assert cats == set(range(12))
    ac = probe[:, 1:]
    for size in range(1, 11):                                        # each size at both ends of its range, both signs
        for v in (-(1 << size) + 1, -(1 << (size - 1)), 1 << (size - 1), (1 << size) - 1):
            assert (ac == v).any(), v
    assert ((probe[:, 1:63] == 0).all(axis=1) & (probe[:, 63] != 0)).any()                   # ZRL x 3, then a value at 63
    assert ((probe[:, 1:] != 0).all(axis=1)).sum() == 2 and ((probe[:, 1:] == 0).all(axis=1)).any()
    seen, word, span, own, write = set(), 0, 0, 0, 0
    for name, cr in files.items():
        s = cr.sym
        big = name.startswith("b_big")
        nbytes = len(cr.string)
        assert nbytes >= 31 * 1024 if big else nbytes < 2048, (name, nbytes)
        if not big:                                                  # the probe's first symbol sits k bits past the 512 of the filler
            k = int(name[-2:])
            assert s["start"][s["blk"] == 64][0] == 512 + k and len(cr.coef) == 64 + len(probe)
        st, cl, sz, z = s["start"].astype(np.int64), s["clen"].astype(np.int64), s["size"], s["z"]
        o2_far = (st % 32 + cl) >= 32
        for i in np.flatnonzero(sz >= 9):
            seen.add(("dc" if z[i] == 0 else "ac", int(sz[i]), bool(o2_far[i])))
        last = st + cl - 1
        word += int(((st // 32) != (last // 32)).sum())
        span += int(((st // SPAN) != (last // SPAN)).sum())
        own += int(((st < OWN * SPAN) & (last >= OWN * SPAN)).sum())
        write += int(((st < 256 * SPAN) & (last >= 256 * SPAN)).sum())
        # a run of 15 that lands exactly on 63, and three ZRLs in a row
        assert ((s["sym"] >> 4 == 15) & (s["size"] > 0) & (s["z"] == 48)).any()
        zrl = np.flatnonzero(s["sym"] == 0xf0)
        assert any(zrl[i + 2] == zrl[i] + 2 for i in range(len(zrl) - 2))
    want = {(kind, size, far) for kind, sizes in (("dc", (9, 10, 11)), ("ac", (9, 10))) for size in sizes for far in (False, True)}
    assert want <= seen, want - seen
    assert word > 100 and span >= 8 and own >= 1 and write >= 1, (word, span, own, write)


# ------------------------------------------------------------------------------------------------------- (c) second symbols
def _pairs(cr):
    """indices i of AC symbols whose successor is an AC symbol of the same block, and whose two codes and first value lie inside an
    11-bit prefix: the sync tables hold both in one entry"""
    s = cr.sym
    i = np.arange(len(s) - 1)
    both = (s["z"][i] > 0) & (s["z"][i + 1] > 0) & (s["blk"][i] == s["blk"][i + 1])
    fits = (s["clen"][i].astype(int) + s["size"][i] + s["clen"][i + 1]) <= 11
    return i[both & fits]


def test_c_the_pairs_and_the_places_where_the_second_symbol_must_wait():
    files = cs.group_c()
    lut = cs.C_AC.lut()
    eob = zrl = ends_block = at_span_end = 0
    for name, cr in files.items():
        s = cr.sym
        p = _pairs(cr)
        if not cr.rst:
            eob += int((s["sym"][p + 1] == 0).sum())
            zrl += int((s["sym"][p + 1] == 0xf0).sum())
            at_span_end += int((s["start"][p + 1] % SPAN == 0).sum())
            # a value on position 63 ends its block; what follows is the next block's DC code, which the AC table reads as a code
            # of its own inside the same prefix
            last = np.flatnonzero((s["z"] > 0) & (s["size"] > 0) & (s["z"].astype(int) + (s["sym"] >> 4) == 63))
            for i in last:
                e = int(_ends(cr)[i])
                c16 = int.from_bytes(cr.string[e // 8:e // 8 + 3] + b"\0\0\0", "big") >> (48 - 16 - e % 8) & 0xffff
                code = lut[c16]
                if code and int(s["clen"][i]) + int(s["size"][i]) + (code >> 8) <= 11:
                    ends_block += 1
        else:
            assert len(cr.rst) >= 10 and len(p) > 50                # the same streams, where no second symbol may be taken at all
    assert eob >= 4 and zrl >= 4 and ends_block >= 4 and at_span_end >= 1, (eob, zrl, ends_block, at_span_end)
    assert {n + "_rst" for n in files if not n.endswith("_rst")} == {n for n in files if n.endswith("_rst")}


# ------------------------------------------------------------------------------------------------------- (d) minimal blocks
def test_d_two_bits_a_block():
    files = cs.group_d()
    cr = files["d_4096_blocks"]
    assert (cr.w, cr.h) == (512, 512) and cr.nbits == 2 * 4096 == 8 * len(cr.string) and cr.string == bytes(1024)
    cr = files["d_last_byte_padded"]
    assert cr.nbits == 2 * 4093 and len(cr.string) == 1024 and cr.string[:-1] == bytes(1023) and cr.string[-1] == 0x3f
    assert len(cs.d_cut()) == len(files["d_4096_blocks"].data) - 1


# ------------------------------------------------------------------------------------------------------- (e) restart boundaries
def _paddings(cr):
    """per boundary: (bits of padding in front of it, the byte in front of it)"""
    e = _ends(cr)
    out = []
    for r in cr.rst:
        i = int(np.searchsorted(cr.sym["start"], 8 * r)) - 1
        out.append((8 * r - int(e[i]), cr.string[r - 1]))
    return out


def test_e_paddings_and_boundaries():
    files = cs.group_e()
    for name in ("e_grey", "e_410"):
        cr = files[name]
        pads = _paddings(cr)
        assert all(0 <= p <= 7 for p, _ in pads)
        assert {0, 7} <= {p for p, _ in pads}, (name, pads)
        assert any(p > 0 and b == 0xff for p, b in pads), (name, pads)           # a padded byte that is 0xff: stuffed in the file
        assert any(p == 0 and b == 0xff for p, b in pads), (name, pads)          # ... and an unpadded one
        assert cr.data.count(b"\xff\x00\xff") >= 2
    assert files["e_410"].nslots == 10 and files["e_grey"].nslots == 1
    cr = files["e_every_byte"]
    assert cr.rst == list(range(1, 300)) and cr.string == b"\x3f" * 300            # a boundary on a span's start (128, 256) and one byte behind it
    assert 128 in cr.rst and 129 in cr.rst and 256 in cr.rst


# ------------------------------------------------------------------------------------------------------- (f) never in step
def test_f_every_workgroup_but_the_first_ends_the_first_launch_wrong():
    """the issue's arithmetic, by the walker: blocks of 10 bytes whose every byte starts with a 0 bit, so a decoder in ANY state reads
    8-bit symbols; span k starts a block only when 5 divides k, a workgroup's warm-up starts at span 240 g - 16 = 4 (mod 5)"""
    small, big = cs.group_f_small()["f_4wg"], cs.f_big()
    assert (big.w, big.h, len(big.coef), len(big.string)) == (3648, 3648, 207936, 2079360)
    nlanes = (len(big.string) * 8 + SPAN - 1) // SPAN
    assert nlanes == 16245 and (nlanes + OWN - 1) // OWN == 68
    assert np.abs(big.coef[:, 0]).max() <= 1016
    for cr in (small, big):
        assert (np.frombuffer(cr.string[:4000], np.uint8) < 128).all() and len(cr.sym) % 10 == 0
        assert set((cr.sym["clen"].astype(int) + cr.sym["size"]).tolist()) == {8}
    for k in range(12):
        assert (cs.state_at(big, k * SPAN) == (k * SPAN, 0, 0)) == (k % 5 == 0)
    # the 4-workgroup file: the whole first launch of workgroups 1..3, warm-up and own spans, never meets the decoder in step
    nl = len(small.string) * 8 // SPAN
    assert nl == 800
    for g in (1, 2, 3):
        st = ((OWN * g - WARM) * SPAN, 0, 0)
        for stop in (OWN * g, OWN * g + 50, min(OWN * (g + 1), nl) - 1):
            p, z, slot, _ = jc.walk(small, small.string, *st, stop * SPAN)
            assert (p, z, slot) != cs.state_at(small, stop * SPAN) and p == stop * SPAN
            st = (p, z, slot)
    # the large file: every workgroup's warm-up (the rest follows from the period: ten bytes, the same for both decoders)
    for g in range(1, 68):
        p, z, slot, _ = jc.walk(big, big.string, (OWN * g - WARM) * SPAN, 0, 0, OWN * g * SPAN)
        assert (p, z, slot) != cs.state_at(big, OWN * g * SPAN) and p == OWN * g * SPAN
    rst = cs.group_f_small()["f_4wg_rst"]
    assert len(rst.rst) == 204 and rst.rst[0] == 500 and rst.string == small.string


# ------------------------------------------------------------------------------------------------------- (g) damaged
def test_g_the_damage_is_where_the_case_says():
    g = cs.group_g()
    s = g["g_run_past_63"][0].sym
    i = np.flatnonzero(s["sym"] == 0x11)
    assert len(i) == 1 and s["z"][i[0]] == 60                         # the file's DHT calls that code (15, 1): 60 + 15 > 63
    s = g["g_code_outside_table"][0].sym
    i = np.flatnonzero((s["sym"] == 0x0a) & (s["z"] > 0))
    assert len(i) == 1 and s["clen"][i[0]] == 16
    for name, early in (("g_ends_16_early", 16), ("g_ends_3_early", 3)):
        cr, twin = g[name]
        assert cr.rst[0] == twin.rst[0] + early and np.array_equal(cr.coef, twin.coef)
        end_bit = int(_ends(twin)[int(np.searchsorted(twin.sym["start"], 8 * twin.rst[0])) - 1])
        jump = 8 * cr.rst[0] - end_bit
        assert 8 * early <= jump <= 8 * early + 7
        assert end_bit // SPAN == (8 * cr.rst[0]) // SPAN == 0        # the blocks' end and the marker inside one span
        # a decoder that goes by position reads the appended bytes as symbols, and the boundary puts it right
        p, z, slot, blocks = jc.walk(cr, cr.string, 0, 0, 0, 8 * cr.rst[0] + 1, cr.rst)
        assert blocks >= cr.ri_blocks and (z, slot) == (1, 0) and p > 8 * cr.rst[0]
