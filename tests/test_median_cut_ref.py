"""The numpy restatement of medianCut under the library's tie rule (tests/median_cut_ref.py) pinned without a GPU: against a
second transliteration of targetsize.go:422-486 with ANOTHER tie order where the reference's answer is unique, and by the
properties that make each of its splits one the reference can produce under some tie order."""
from __future__ import annotations

import numpy as np
import pytest

import median_cut_ref as ref


def test_tie_free_input_has_one_answer_under_both_tie_orders():
    img = ref.tie_free_16x16()
    pals, straddles = ref.median_cut(img, ref.LEVELS)
    assert straddles == 0
    assert [len(p) for p in pals] == [16, 32, 64, 128, 256]
    for level, p in zip(ref.LEVELS, pals):
        assert np.array_equal(p, ref.median_cut_other_ties(img, level)), level


def test_other_tie_order_changes_the_noise_palette():
    """64 x 64 noise: 75 splits straddle a tie and the other order gives another palette -- this case holds the rule"""
    img, _ = ref.CASES["noise_64x64"]
    pals, straddles = ref.want("noise_64x64")
    assert straddles == 75
    assert not np.array_equal(pals[-1], ref.median_cut_other_ties(img, 256))


@pytest.mark.parametrize("name", ["5x2_random", "two_colours_64x64", "tie_free_16x16", "noise_64x64", "noise_317x317"])
def test_prefix_property(name):
    img, levels = ref.CASES[name]
    pals, _ = ref.want(name)
    for level, p in zip(levels, pals):
        one, _ = ref.median_cut(img, [level])
        assert np.array_equal(one[0], p), (name, level)


@pytest.mark.parametrize("name", ["median_tie_3x2", "flat_16x16", "two_colours_64x64", "noise_64x64", "noise_448x447"])
def test_every_split_is_one_the_reference_can_produce(name):
    img, levels = ref.CASES[name]
    trace = []
    ref.median_cut(img, levels, trace=trace)
    assert trace
    for axis, left, right, count in trace:
        assert len(left) == count // 2 and len(left) + len(right) == count
        assert left.max() <= right.min()


def test_scores_leave_32_bits():
    img, _ = ref.CASES["noise_64x64"]
    px = ref.samples(img).astype(np.int64)
    rng = px.max(axis=0) - px.min(axis=0) + 1
    assert int(rng[0]) * int(rng[1]) * int(rng[2]) * len(px) > 2 ** 32


@pytest.mark.parametrize("w,h,step,count", [(447, 447, 1, 199809), (448, 447, 2, 100128), (317, 317, 1, 100489), (316, 316, 1, 99856),
                                            (3840, 2160, 82, 101152)])
def test_sample_counts_and_flat_offsets(w, h, step, count):
    assert ref.sample_step(w, h) == step
    img = np.zeros((h, w, 4), dtype=np.uint8)
    flat = img.reshape(-1, 4)
    flat[:, 0] = np.arange(w * h) & 255
    flat[:, 1] = (np.arange(w * h) >> 8) & 255
    flat[:, 2] = (np.arange(w * h) >> 16) & 255
    s = ref.samples(img).astype(np.int64)
    assert len(s) == count
    at = s[:, 0] | (s[:, 1] << 8) | (s[:, 2] << 16)
    assert np.array_equal(at, np.arange(count) * step)              # sample j is the flat group j step, rows ignored
    assert (count - 1) * step < w * h <= count * step


def test_small_cases_by_hand():
    pals, _ = ref.want("score_tie_8x1")                              # two boxes tie on score 44: the FIRST splits
    assert pals[0][:, 0].tolist() == [5, 105] and pals[1][:, 0].tolist() == [0, 105, 10]
    pals, _ = ref.want("range_tie_2x2")                              # R and G ranges tie: R is the axis
    assert pals[0][0].tolist() == [0, 5, 0, 255]
    pals, s = ref.want("median_tie_3x2")                             # four samples tie on R = 5 across the median: j decides
    assert s == 1 and pals[0].tolist() == [[3, 4, 1, 255], [6, 4, 7, 255]]   # left: j = 4, 0, 1
    pals, _ = ref.want("5x2_random")
    assert [len(p) for p in pals] == [10] * 5
    pals, _ = ref.want("1x1")
    assert all(p.tolist() == [[9, 8, 7, 255]] for p in pals)
    pals, _ = ref.want("flat_16x16")
    assert len(pals[-1]) == 256 and (pals[-1] == np.array([37, 99, 200, 255], np.uint8)).all()
    pals, _ = ref.want("two_colours_64x64")
    assert len(pals[-1]) == 256 and len(np.unique(pals[-1], axis=0)) == 2
    a, _ = ref.want("noise_alpha0_40x30")
    img = ref.CASES["noise_alpha0_40x30"][0].copy()
    img[:, :, 3] = 255
    b, _ = ref.median_cut(img, ref.LEVELS)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))           # alpha is not looked at
    assert ref.median_cut(np.zeros((0, 5, 4), np.uint8), (2, 3))[0][1].tolist() == [[0, 0, 0, 255]]
