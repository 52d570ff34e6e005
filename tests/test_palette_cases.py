"""CPU tests of the crafted applyPalette cases (tests/palette_cases.py): the planted index planes are what the numpy restatement
and the oracle compute, the model of the candidate grid reports the list lengths the cases claim, every candidate of a
list_len case is some pixel's only nearest entry (so a dropped slot shows whatever order the slots were filled in), the tied
entry of a rim_tie case sits exactly on the pruning bound, and the model's lists never lose a pixel's nearest entry.

tests/test_palette_cases_gpu.py relies on these conditions: if a generator or a constant of palette.hip drifts, a test fails
here instead of a GPU test quietly turning into one more ordinary image."""
import os
import re

import numpy as np
import pytest

import np_restatement as npr
import palette_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_model_restates_the_kernels_own_lines():
    """what grid_lists and the cases were built from is still palette.hip's.  Two of these lines can change without changing
    a single index (`hi = lo + 8` only lengthens the lists, and any real entry may fill a record's unused slots): they are
    held here, by their text, and nowhere else."""
    text = open(os.path.join(ROOT, "fennec_amd", "csrc", "palette.hip")).read()
    assert re.findall(r"constexpr int PG_BITS = (\d+);", text) == ["5"] and re.findall(r"constexpr int PG_REC = (\d+);", text) == ["32"]
    assert "constexpr int PG_CAP = PG_REC - 1;" in text and pc.CAP == 31 and pc.CELLS == 1 << 15
    assert text.count("const int hi = lo + 7;") == 1
    assert text.count("const int d0 = max(max(below, above), 0);") == 1 and text.count("const int d1 = max(p - lo, hi - p);") == 1
    assert text.count("u = min(u, mx);") == 1 and text.count("if (mn <= u) {") == 1
    assert text.count("if (slot == 0) byte = cnt > static_cast<uint32_t>(PG_CAP) ? 0xffu : cnt;") == 1
    assert text.count("else byte = static_cast<uint32_t>(slot) <= cnt ? s_list[lc][slot] : first;") == 1
    assert text.count("const uint8_t first = s_list[lc][1];") == 1
    assert re.findall(r"ballot_w64\(most > (\d+)u\)", text) == ["3", "7", "15"]
    assert text.count("static_cast<long>(w) * h >= 262144L") == 2                       # both launches choose alike
    assert text.count('"apply_palette_grid_kernel"') == 2 and text.count('"apply_palette_kernel"') == 2


def test_pg_chan_at_the_cubes_faces():
    assert pc.pg_chan(0, 0) == (0, 49) and pc.pg_chan(7, 0) == (0, 49) and pc.pg_chan(8, 0) == (1, 64) and pc.pg_chan(255, 0) == (248 ** 2, 255 ** 2)
    assert pc.pg_chan(255, 248) == (0, 49) and pc.pg_chan(248, 248) == (0, 49) and pc.pg_chan(247, 248) == (1, 64) and pc.pg_chan(0, 248) == (248 ** 2, 255 ** 2)
    assert pc.pg_chan(19, 16) == (0, 16) and pc.pg_chan(20, 16) == (0, 16) and pc.pg_chan(15, 16) == (1, 64)
    # the vectorised model is the scalar one
    pal = pc.random_palette(61, 3)
    cells = [0, pc.CELLS - 1, pc.cell_no(2, 2, 2), pc.cell_no(31, 0, 17), 12345]
    u, cand, tie = pc.grid_arrays(pal, cells)
    for k, cell in enumerate(cells):
        mm = [pc.mind_maxd(p, cell) for p in pal]
        assert u[k] == min(m[1] for m in mm)
        assert cand[k].tolist() == [m[0] <= u[k] for m in mm] and tie[k].tolist() == [m[0] == u[k] for m in mm]


def test_names_and_palette_sizes():
    names = [c.name for c in pc.CASES]
    assert len(set(names)) == len(names)
    for k in pc.LIST_LENS:
        assert f"list_len_{k}" in pc.BY_NAME
    assert pc.LIST_LENS == (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33)
    for k in (4, 8, 16, 32):
        assert f"list_len_{k}_cell0" in pc.BY_NAME and f"list_len_{k}_cell31" in pc.BY_NAME
    assert all(n in pc.BY_NAME for n in pc.PRESENTED)
    sizes = {len(c.palette) for c in pc.CASES}
    assert 256 in sizes and any(n % 8 for n in sizes) and 3 in sizes
    assert all(c.img.shape[0] * c.img.shape[1] <= 32768 for c in pc.CASES)              # the smallest shapes that reach the code


@pytest.mark.parametrize("case", pc.CASES, ids=repr)
def test_planted_plane_is_the_restatements_and_the_oracles(orc, case):
    idx, q = npr.apply_palette(case.img, case.palette)
    assert np.array_equal(idx, case.want), np.argwhere(idx != case.want)[:4]
    oi, oq = orc.apply_palette(case.img, case.palette)
    assert np.array_equal(oi, case.want), np.argwhere(oi != case.want)[:4]
    assert np.array_equal(oq, case.palette[case.want]) and np.array_equal(q, oq) and (oq[..., 3] == 255).all()
    assert np.array_equal(pc.nearest_first(case.palette, case.img), case.want)


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.info["cells"]], ids=repr)
def test_model_reports_the_claimed_list_lengths(case):
    cells = sorted(case.info["cells"])
    for cell, (u, cand, tied) in zip(cells, pc.grid_lists(case.palette, cells)):
        claim = case.info["cells"][cell]
        assert (len(cand) > pc.CAP if claim == pc.MARKED else len(cand) == claim), (case.name, cell, len(cand), claim)
        if "u" in case.info:
            assert u == case.info["u"]
    if case.kind in ("list_len", "rim_tie", "mixed_wave"):                               # the image aims at the cells it names
        assert set(np.unique(pc.cell_of(case.img)).tolist()) == set(cells)


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.kind == "list_len"], ids=repr)
def test_list_len_every_candidate_is_some_pixels_only_nearest(case):
    (cell, k), = case.info["cells"].items()
    (u, cand, tied), = pc.grid_lists(case.palette, [cell])
    assert u == 48 and len(cand) == k and cand == set(case.info["planted"])
    pal = case.palette[:, :3].astype(np.int64)
    px = case.img.reshape(-1, 4)[:, :3].astype(np.int64)
    assert len({tuple(p) for p in px.tolist()}) == 512 and case.img.shape == (2, 256, 4)  # each row one wave, every pixel in the cell
    dist = ((px[:, None, :] - pal[None, :, :]) ** 2).sum(axis=2)
    best = dist.min(axis=1)
    alone = (dist == best[:, None]).sum(axis=1) == 1
    winners = set(dist.argmin(axis=1)[alone].tolist())
    assert winners == cand, (case.name, sorted(cand - winners))
    values = set(case.palette[sorted(cand), :3].reshape(-1).tolist())
    if cell == 0:
        assert 0 in values
    if cell == pc.CELLS - 1:
        assert 255 in values
    if k >= 2:
        assert len(case.palette) - 1 in cand                                             # a candidate at the palette's last index
    assert (k > pc.CAP) == (pc.claimed(k) == pc.MARKED)


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.kind == "rim_tie"], ids=repr)
def test_rim_tie_sits_on_the_pruning_bound(case):
    info = case.info
    (cell, _), = info["cells"].items()
    (u, cand, tied), = pc.grid_lists(case.palette, [cell])
    assert u == info["u"] and info["tied"] in tied and cand == {info["tied"], info["best"]}
    assert pc.mind_maxd(case.palette[info["tied"]], cell)[0] == u == pc.mind_maxd(case.palette[info["best"]], cell)[1]
    px = np.array(info["pixel"])
    d = lambda i: int(((case.palette[i, :3].astype(np.int64) - px) ** 2).sum())
    assert d(info["tied"]) == d(info["best"]) == u
    at = (case.img[..., :3] == px.astype(np.uint8)).all(axis=2)
    assert at.any() and (case.want[at] == min(info["tied"], info["best"])).all() and (case.want[~at] == info["best"]).all()
    assert case.img.shape[1] in (4, 256)


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.kind == "midpoint_tie"], ids=repr)
def test_midpoint_ties_are_ties_and_candidates(case):
    info = case.info
    px = np.array(info["pixel"])
    d = ((case.palette[:, :3].astype(np.int64) - px) ** 2).sum(axis=1)
    pos = info["planted"]
    assert len(set(d[pos].tolist())) == 1 and (np.delete(d, pos) > d[pos[0]]).all()
    (u, cand, tied), = pc.grid_lists(case.palette, [int(pc.cell_of(px))])
    assert set(pos) <= cand
    if "_at" in case.name:
        cells = pc.cell_of(case.palette[pos]).tolist()                                   # the tied entries straddle the border:
        assert len(set(cells)) == {2: 2, 4: 3, 8: 8}[len(pos)] and set(cells) != {int(pc.cell_of(px))}
    else:
        assert set(pc.cell_of(case.palette[pos]).tolist()) == {int(pc.cell_of(px))}


def test_duplicates_lie_far_apart():
    case = pc.BY_NAME["duplicates_pairs"]
    pal = case.palette
    for a, b in ((5, 250), (9, 251)):
        assert np.array_equal(pal[a], pal[b]) and a in case.want and b not in case.want
    assert 255 in case.want
    assert (pc.BY_NAME["duplicates_one_colour"].want == 0).all()
    for name, first in (("duplicates_two_colours_a_first", (0, 100)), ("duplicates_two_colours_b_first", (3, 0))):
        case = pc.BY_NAME[name]
        assert case.info["first"] == first and set(np.unique(case.want).tolist()) == set(first)
        assert len({tuple(p) for p in case.palette.tolist()}) == 2


def test_mixed_wave_interleaves_three_kinds_of_cell():
    for w in pc.MIXED_WIDTHS:
        case = pc.BY_NAME[f"mixed_wave_{w}"]
        assert case.img.shape == (2, w, 4) and len(case.palette) == 256
        cells = pc.cell_of(case.img)
        for x in range(w):
            assert (cells[:, x] == (pc.CROWD_CELL, pc.LONE_CELL, pc.LIST_CELL)[x % 3]).all()
        assert 1 <= (w - 1) % 4 + 1 <= 3 and (w <= 256 or 1 <= w - 256 <= 3)             # a partial last group; 1 or 3 pixels in the next workgroup


def test_alpha_cases_differ_in_alpha_only():
    for name in ("list_len_5", "mixed_wave_255"):
        a, b = pc.BY_NAME[name], pc.BY_NAME["alpha_ignored_" + name]
        assert np.array_equal(a.img[..., :3], b.img[..., :3]) and np.array_equal(a.want, b.want) and a.palette is b.palette
        assert len(np.unique(b.img[..., 3])) > 100 and (b.img[..., 3] < 255).any()


def test_every_cell_reads_every_record():
    img = pc.every_cell_image()
    assert img.shape == (128, 256, 4)
    assert np.array_equal(pc.cell_of(img).reshape(-1), np.arange(pc.CELLS))
    offs = {tuple(v) for v in (img.reshape(-1, 4)[:, :3] & 7).tolist()}
    assert len(offs) == 512                                                              # every offset inside a cell occurs


@pytest.mark.parametrize("kind,seed", [("random", 1), ("random", 2), ("clustered", 3)])
def test_no_argmin_leaves_its_cells_candidates(kind, seed):
    """over all 32768 cells: the nearest entry (first minimum) of every_cell's pixel is in its cell's candidate set, and so
    is every entry tied with it -- the lists alone decide the same plane as the whole palette"""
    pal = pc.random_palette(256, seed) if kind == "random" else pc.clustered_palette(256, seed)
    img = pc.every_cell_image()
    want = pc.nearest_first(pal, img).reshape(-1)
    u, cand, tie = pc.grid_arrays(pal, np.arange(pc.CELLS))
    assert cand[np.arange(pc.CELLS), want].all()
    assert cand.any(axis=1).all() and tie.sum() >= 0 and (u >= 48).all()
    # the plane decided among the candidates only is the plane
    px = img.reshape(-1, 4)[:, :3].astype(np.int64)
    p = pal[:, :3].astype(np.int64)
    dist = np.zeros((pc.CELLS, 256), dtype=np.int64)
    for c in range(3):
        dist += (px[:, c:c + 1] - p[None, :, c]) ** 2
    key = np.where(cand, dist * 256 + np.arange(256)[None, :], np.iinfo(np.int64).max)
    assert np.array_equal((key.min(axis=1) & 255).astype(np.uint8), want)
    lens = cand.sum(axis=1)
    print(f"\n{kind} palette {seed}: lists of {lens.min()}..{lens.max()} candidates, mean {lens.mean():.1f}, {(lens > pc.CAP).sum()} marked cells")
