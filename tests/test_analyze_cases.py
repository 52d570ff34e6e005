"""CPU tests of the crafted Analyze cases (tests/analyze_cases.py): that they reach what they claim -- shown from the exact
classifier alone --, that the oracle and the numpy restatement both meet every planted value, and that the constants the cases
were built from are still analyze.hip's.

tests/test_analyze_cases_gpu.py relies on these conditions: if a generator or a constant of the kernel drifts, a test fails
here instead of a GPU test quietly turning into one more ordinary image.  The counts the cases were measured at are printed
(pytest -s) and asserted."""
import math
import os
import random
import re
from fractions import Fraction

import numpy as np
import pytest

import analyze_cases as ac
import np_restatement as npr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def words_of(img):
    return np.ascontiguousarray(img).view("<u4").reshape(-1).tolist()


# ------------------------------------------------------------------ the kernel's constants
def test_constants_are_the_kernels_own():
    text = open(os.path.join(ROOT, "fennec_amd", "csrc", "analyze.hip")).read()
    api = open(os.path.join(ROOT, "fennec_amd", "csrc", "api.cpp")).read()
    assert re.findall(r"^constexpr int AN_HASH_CAP = 1 << (\d+);", text, flags=re.M) == [str(ac.HASH_BITS)]
    # the slot function, once per route
    assert re.findall(r"uint32_t slot = \(\w+ \* (\d+)u\) >> \(32 - (\d+)\);", text) == [(str(ac.HASH_MULT), str(ac.HASH_BITS))] * 2
    assert text.count("slot = (slot + 1) & (AN_HASH_CAP - 1);") == 2
    assert text.count("const unsigned long long key = (1ull << 32) | p") == 2      # pixel 0 is a key, not the empty slot
    assert re.findall(r"constexpr int FIRST_COLOR_BLOCKS = (\d+);", text) == [str(ac.FIRST_COLOR_BLOCKS)]
    assert "static_cast<long long>(b) * %d + tid" % ac.COLOR_BLOCK in text
    assert "a.colors_only && r->unique_colors >= %d" % ac.COLOR_CAP in text
    assert "if (a[i].unique_colors > %d) a[i].unique_colors = %d;" % (ac.COLOR_CAP, ac.COLOR_CAP) in api
    # the three grids, once per route
    assert re.findall(r"color_step = total > (\d+) \? total / (\d+) : 1;", text) == [(str(ac.COLOR_SAMPLES),) * 2] * 2
    assert re.findall(r"cstep_[xy] = static_cast<int>\(std::fmax\(1\.0, std::ceil\(static_cast<double>\([wh]\) / (\d+)\)\)\);", text) == [str(ac.CONTRAST_DIV)] * 4
    assert re.findall(r"estep_[xy] = static_cast<int>\(std::fmax\(1\.0, static_cast<double>\([wh]\) / (\d+)\)\);", text) == [str(ac.EDGE_DIV)] * 4
    assert text.count("edge = sqrt(gx * gx + gy * gy) > 30.0;") == 2
    assert text.count("return static_cast<int>(lum + 0.5);") == 1
    # what keeps lum601 and the Sobel sum uncontracted
    mk = open(os.path.join(ROOT, "fennec_amd", "csrc", "Makefile")).read()
    assert re.search(r"^CXXFLAGS = .*-ffp-contract=off", mk, flags=re.M)
    assert ac.HASH_CAP == 1 << ac.HASH_BITS and ac.FIRST_SAMPLES == 2048
    assert (ac.HASH_MULT * ac.HASH_INV) % (1 << 32) == 1


def test_rn_is_ieee_round_to_nearest_even():
    rnd = random.Random(7)
    for _ in range(20000):
        x = Fraction(rnd.getrandbits(90) - (1 << 89), rnd.getrandbits(rnd.randrange(1, 70)) + 1)
        assert ac.rn(x) == Fraction(float(x)), x
    for x in (Fraction(3, 2) + Fraction(1, 1 << 53), Fraction(1) + Fraction(1, 1 << 53), Fraction(1) + Fraction(3, 1 << 53)):
        assert ac.rn(x) == Fraction(float(x))                                       # ties go to the even neighbour
    f32 = lambda x: Fraction(float(np.float32(float(x))))
    for _ in range(2000):                                                           # fp32: doubles of few bits round once
        x = Fraction(rnd.getrandbits(40), 1 << rnd.randrange(0, 30))
        assert ac.rn(x, 24) == f32(x), x
    assert math.sqrt(900.0) == 30.0 and math.sqrt(math.nextafter(900.0, math.inf)) > 30.0 and math.sqrt(math.nextafter(900.0, 0.0)) <= 30.0


# ------------------------------------------------------------------ lum_ties
TIES = 16782
MOVED = {"fma_all": 2965, "fma_inner": 1750, "reassoc": 2756, "fp32": 3712, "int_half_up": 3464}


def test_lum_ties_reach_every_tie_and_every_variant_moves_a_thousand():
    t = ac.tie_triples()
    assert len(t) == TIES and len({tuple(v) for v in t.tolist()}) == TIES
    moved, (up, down) = ac.lum_tie_sensitivity()
    print(f"\nlum ties: {len(t)}; the reference's chain rounds {up} up, {down} down; bins moved per variant: {moved}")
    assert (up, down) == (13318, 3464)
    assert all(n >= 1000 for n in moved.values()), moved
    assert moved == MOVED
    for name in ("lum_ties_mixed", "lum_ties_opaque", "lum_ties_sorted"):
        case = ac.BY_NAME[name]
        img, hist = case.img, case.expect["histogram"]
        assert img.shape == (ac.TIES_H, ac.TIES_W, 4) and int(hist.sum()) == ac.TIES_W * ac.TIES_H
        px = {tuple(v) for v in img.reshape(-1, 4)[:, :3].tolist()}
        assert px == {tuple(v) for v in t.tolist()} | {ac.PAD_COLOUR}
        for v in ac.VARIANTS:                                                       # ... and no variant's moves cancel in the histogram
            other = ac.lum_ties_histogram_under(v)                                  # (moves up and down do cancel in part)
            assert int((other != hist).sum()) >= 100, v                             # ... but not in a hundred bins of the 256
    a = ac.BY_NAME["lum_ties_mixed"].img[..., 3]
    assert (a == 255).any() and (a < 255).any() and (ac.BY_NAME["lum_ties_opaque"].img[..., 3] == 255).all()
    # in the spread order the four pixels of a 16-byte unit rarely share a bin, in the sorted order they mostly do (an_count2's two branches)
    def same_pairs(name):
        img = ac.BY_NAME[name].img.reshape(-1, 4)[:TIES - TIES % 2, :3].tolist()
        b = [ac.lum_bin(*c) for c in img]
        return sum(1 for i in range(0, len(b), 2) if b[i] == b[i + 1])
    assert same_pairs("lum_ties_sorted") >= 2000 and same_pairs("lum_ties_mixed") <= 500


# ------------------------------------------------------------------ sobel_ties
def test_sobel_ties_hold_contraction_flips():
    members, seen = ac.flip_members()
    assert len(members) >= 8
    flips = [ac.member_flips(*m) for m in members]
    assert all(ref != cx for ref, cx, _ in flips) and len({ref for ref, _, _ in flips}) == 1       # one direction: they cannot cancel
    print(f"\nsobel ties: {len(members)} centres flip under fma(gx, gx, gy*gy) among {seen} members examined (1 in {seen // len(members)})")
    for m in members:                                                               # each is a member: magnitude 30 in integers
        (bg, right, below) = m
        a, b = ac.milli(*right) - ac.milli(*bg), ac.milli(*below) - ac.milli(*bg)
        assert (2 * a) ** 2 + (2 * b) ** 2 == ac.M30


@pytest.mark.parametrize("name", ["sobel_ties", "sobel_ties_b", "sobel_ties_129x131"])
def test_sobel_ties_images(name):
    case = ac.BY_NAME[name]
    h, w = case.img.shape[:2]
    cl = case.info
    assert max(w, h) <= 399 and ac.edge_axis(w).step == 1 and ac.edge_axis(h).step == 1
    assert cl.total == (w - 2) * (h - 2) == case.expect["edge_total"]
    cells = (w // ac.CELL) * (h // ac.CELL)
    centres = [(ac.CELL * i + 2, ac.CELL * j + 2) for j in range(h // ac.CELL) for i in range(w // ac.CELL)]
    assert all(c in cl.near for c in centres)                                       # every member's centre is rounding's to decide
    a = case.img.astype(np.int64)
    L = ac.milli(a[..., 0], a[..., 1], a[..., 2])
    exact30 = 0
    for (x, y) in cl.near:
        gx = L[y - 1, x + 1] - L[y - 1, x - 1] + 2 * L[y, x + 1] - 2 * L[y, x - 1] + L[y + 1, x + 1] - L[y + 1, x - 1]
        gy = L[y + 1, x - 1] - L[y - 1, x - 1] + 2 * L[y + 1, x] - 2 * L[y - 1, x] + L[y + 1, x + 1] - L[y - 1, x + 1]
        exact30 += int(gx * gx + gy * gy == ac.M30)
    assert exact30 >= 2 * cells                                                     # (the window one down and right of a centre is a tie as well)
    edges_of_ties = sum(1 for g in cl.near.values() if ac.is_edge(ac.sobel_m(*g)))
    share = edges_of_ties / len(cl.near)
    assert 0.25 <= share <= 0.55, share                                             # the fp64 chain calls some 40 % of them edges; integers none
    ref, cx, cy = cl.count(), cl.count("x"), cl.count("y")
    print(f"\n{name}: {w} x {h}, {cells} members, {len(cl.near)} samples within 1e-3 of the threshold ({exact30} exactly on it), "
          f"{edges_of_ties} of them edges; edge_count {ref}, {cx} under fma(gx, gx, .), {cy} under fma(gy, gy, .), {cl.far_edges} with all ties taken for no edge")
    assert ref == case.expect["edge_count"]
    assert ref - cl.far_edges >= 100                                                # an integer evaluation (no tie is an edge) is far off
    if name != "sobel_ties_b":
        assert abs(ref - cx) >= 8, (ref, cx)


# ------------------------------------------------------------------ colour_grid
WALKS = {50000: (1, 50000, 49999), 50001: (1, 50001, 50000), 99999: (1, 99999, 99998), 100000: (2, 50000, 99998),
         100001: (2, 50001, 100000), 149999: (2, 75000, 149998), 150000: (3, 50000, 149997)}
DIMS = {50000: (125, 400), 50001: (21, 2381), 99999: (271, 369), 100000: (250, 400), 100001: (11, 9091), 149999: (61, 2459), 150000: (375, 400)}


def test_colour_walk_arithmetic():
    assert set(WALKS) == set(ac.TOTALS)
    for total, want in WALKS.items():
        assert ac.colour_walk(total) == want
        w, h = ac.grid_dims(total)
        assert (w, h) == DIMS[total] and w * h == total and w % 4
        step, n, last = want
        assert last == (n - 1) * step < total <= n * step                           # one more sample would leave the image


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.kind == "colour_grid"], ids=repr)
def test_colour_grid_plants_what_it_says(case):
    info, words = case.info, words_of(case.img)
    total, step, n, last = len(words), info["step"], info["samples"], info["last"]
    truth = info["truth"]
    sampled = words[::step]
    assert len(sampled) == n and len(set(sampled)) == truth and case.expect["unique_colors"] == min(truth, 1024)
    assert words[last] != ac.BACKGROUND and words.count(words[last]) == 1           # the last sample carries a colour of its own:
    assert len(set(sampled[:-1])) == truth - 1                                      # a walk one sample short counts one less
    if "late" in case.name:
        assert len(set(sampled[:ac.FIRST_SAMPLES])) == 1
    elif "split" in case.name:
        assert len(set(sampled[:ac.FIRST_SAMPLES])) == 1023 and len(set(sampled[:ac.FIRST_SAMPLES - 1])) == 1022
        assert truth - 1023 in (1, 2)
    else:
        assert words[0] != ac.BACKGROUND and words.count(words[0]) == 1
    if step > 1:                                                                    # decoys: any other step, or an offset walk, counts more
        assert info["decoys"] >= 100 and len(set(words)) == truth + info["decoys"]
        if truth >= 1023:
            for other in (step - 1, step + 1):
                assert len(set(words[::other])) != truth
        assert len(set(words[1::step])) >= 100                                      # a walk that starts one pixel late sees them
        assert last + 1 >= total or words[last + 1] != ac.BACKGROUND
    else:
        assert info["decoys"] == 0 and len(set(words)) == truth


# ------------------------------------------------------------------ colliding_colours
@pytest.mark.parametrize("truth", list(ac.COLLIDING))
def test_colliding_colours_make_one_chain_through_slot_zero(truth):
    img, expect, words = ac.colliding_colours(truth)
    n_last, n_prev, n_zero = ac.COLLIDING[truth]
    assert img.shape[0] * img.shape[1] <= ac.COLOR_SAMPLES and set(words_of(img)) == set(words) and len(words) == truth
    homes = [ac.home_slot(p) for p in words]
    assert (homes.count(ac.HASH_CAP - 1), homes.count(ac.HASH_CAP - 2), homes.count(0)) == (n_last, n_prev, n_zero)
    assert 0 in words and expect["unique_colors"] == min(truth, 1024)
    for order in (words, words[::-1], words_of(img)):
        entries, longest, wrapped, slots = ac.simulate_probe(order)
        assert entries == truth
        # one run of occupied slots: from the home before the last slot, over the table's end, through slot 0
        assert slots == sorted(list(range(0, truth - 2)) + [ac.HASH_CAP - 2, ac.HASH_CAP - 1])
        assert wrapped >= n_last - 1 and longest >= n_last - 1
    entries, longest, wrapped, _ = ac.simulate_probe(words)
    print(f"\ncolliding colours, truth {truth}: homes {n_last} / {n_prev} / {n_zero} at slots {ac.HASH_CAP - 1} / {ac.HASH_CAP - 2} / 0; "
          f"inserted in order: longest probe {longest}, {wrapped} inserts wrapped from the last slot to slot 0")


# ------------------------------------------------------------------ contrast_grid, edge_grid
CONTRAST_COUNTS = {99: 99, 100: 100, 101: 51, 200: 100, 201: 67, 301: 76}
EDGE_COUNTS = {3: 1, 4: 2, 5: 3, 399: 397, 400: 199, 401: 200, 402: 200, 599: 299, 600: 200, 601: 200}


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.kind == "contrast_grid"], ids=repr)
def test_contrast_grid_puts_outliers_on_and_off_the_grid(case):
    h, w = case.img.shape[:2]
    info = case.info
    assert case.expect["sample_count"] == CONTRAST_COUNTS.get(w, w) * CONTRAST_COUNTS.get(h, h)
    xs, ys = info["xs"], info["ys"]
    assert (xs[-1], ys[-1]) in info["on"] and xs[-1] + xs.step >= w and ys[-1] + ys.step >= h
    assert any(x == xs[-1] for x, _ in info["on"]) and any(y == ys[-1] for _, y in info["on"])
    if max(w, h) > 100:
        assert len(info["off"]) >= 3
        assert any(abs(x - xs[-1]) == 1 or abs(y - ys[-1]) == 1 for x, y in info["off"])   # beside the last grid line
    px = lambda x, y: int(case.img[y, x, 0])
    assert all(px(x, y) in (0, 255) for x, y in info["on"] + info["off"])
    assert {px(x, y) for x, y in info["on"]} == {0, 255}
    assert info["teeth"] > 1e-6, float(info["teeth"])
    assert float(info["teeth"]) > 1e-3                                              # (in fact: each outlier is worth percents of the sum)


@pytest.mark.parametrize("case", [c for c in ac.CASES if c.kind == "edge_grid"], ids=repr)
def test_edge_grid_counts_turn_on_the_last_centre(case):
    h, w = case.img.shape[:2]
    info = case.info
    xs, ys, white = info["xs"], info["ys"], info["white"]
    assert case.expect["edge_total"] == EDGE_COUNTS.get(w, 5) * EDGE_COUNTS.get(h, 5) == len(xs) * len(ys)
    assert xs[-1] + xs.step > w - 2 and ys[-1] + ys.step > h - 2
    assert all(max(abs(a[0] - b[0]), abs(a[1] - b[1])) >= 4 for i, a in enumerate(white) for b in white[:i])
    assert int((case.img[..., 0] == 255).sum()) == len(white) >= 2

    def count(cxs, cys):
        return sum(1 for x, y in white for cx in cxs for cy in cys if max(abs(cx - x), abs(cy - y)) == 1)
    assert count(xs, ys) == case.expect["edge_count"] > 0
    # a grid one centre short along either axis counts fewer edges (one centre long: its window would leave the image, and
    # edge_total, an integer of the result, is one row or column off)
    for cxs, cys in ((xs[:-1], ys), (xs, ys[:-1])):
        assert count(cxs, cys) != case.expect["edge_count"], (case.name, list(cxs)[-2:], list(cys)[-2:])


# ------------------------------------------------------------------ the reference meets every planted value by itself
@pytest.mark.parametrize("case", ac.CASES, ids=repr)
def test_oracle_and_restatement_agree_with_the_classifier(orc, case):
    img = case.img
    for name, got in (("oracle", orc.analyze(img)), ("np_restatement", npr.analyze(img))):
        for key, want in case.expect.items():
            if key == "histogram":
                assert np.array_equal(np.asarray(got[key], dtype=np.float64), want.astype(np.float64)), (name, key)
            elif key == "unique_colors":
                assert min(got[key], 1024) == want, (name, key, got[key])
            else:
                assert got[key] == want, (name, key, got[key], want)
        if case.kind == "contrast_grid":
            var = case.info["variance"]
            assert abs(Fraction(got["variance_sum"]) - var) <= Fraction(1, 10 ** 9) * var, name


def test_batches_hold_equal_sizes_and_one_repeat():
    for group, names in ac.BATCHES.items():
        assert len({ac.BY_NAME[n].img.shape for n in names}) == 1, group
        for n in (3, 5):
            picked = ac.batch_names(group, n)
            assert len(picked) == n and len(set(picked)) == min(len(names), n - 1)
    kinds = [ac.BY_NAME[n].kind for n in ac.PRESENTED]
    assert sorted(kinds) == sorted({c.kind for c in ac.CASES})
    assert all(ac.BY_NAME[n].img.shape[1] % 4 for n in ac.PRESENTED)
    assert all(c.img.shape[0] * c.img.shape[1] <= 160000 for c in ac.CASES)
