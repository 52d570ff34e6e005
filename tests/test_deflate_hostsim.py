"""deflate.hip's own source on the CPU (tools/deflate_hostsim: the two kernels compiled against stand-in headers, a workgroup
as 256 threads), built with AddressSanitizer and UndefinedBehaviorSanitizer as a stand-alone program and run in a child
process.  The streams go through the same contract and the same certificates as the device's
(test_deflate_structure_gpu.py), so the branches those inputs are built for are known to be reached without a GPU; and
since the program also hands out the parse, the chunks that took the stored form are judged too."""
from __future__ import annotations

import numpy as np
import pytest

import deflate_contract as dc
import deflate_hostsim as hs
import inflate_probe as ip
from deflate_contract import CH, S
from test_deflate_gpu import CONTENTS, RATIO_CASES, ROW


@pytest.fixture(scope="module")
def sim(tmp_path_factory):
    work = tmp_path_factory.mktemp("deflate_hostsim")
    exe = hs.build(str(work / "build"))

    def run(x, row=0, label="", src_offset=0, dst_offset=0):
        stream, tokens = hs.run(exe, str(work), x, row, src_offset, dst_offset)
        return stream, dc.contract(stream, x.tobytes(), lambda c: tokens[c], label)[1]
    return run


def test_the_15_bit_limit(sim):
    x = dc.limit15()
    dc.certify_limit15(sim(x, 0, "limit15")[1], 0)
    dc.certify_limit15(sim(dc.behind_noise(x), 0, "limit15 as the second chunk")[1], 1)


def test_ties_go_to_the_leaf(sim):
    x = dc.ties()
    stream, info = sim(x, 0, "ties")
    dc.certify_ties(info, 0, ip.probe(stream).blocks[0].ll_lengths)


def test_the_7_bit_limit_of_the_code_length_code(sim):
    x = dc.limit7()
    dc.certify_limit7(sim(x, 0, "limit7")[1], 0)
    dc.certify_limit7(sim(dc.behind_noise(x), 0, "limit7 as the second chunk")[1], 1)


@pytest.mark.parametrize("name", sorted(dc.FAR))
def test_far_matches(sim, name):
    dc.certify_far(sim(dc.far_match(name), 0, f"far {name}")[1], name)


@pytest.mark.parametrize("dist", [4096, 4097])
def test_three_byte_match_rule(sim, dist):
    x, site = dc.three_bytes(dist)
    dc.certify_three_bytes(sim(x, 0, f"three bytes {dist} back")[1], dist, site)


def test_forms_side_by_side(sim):
    dc.certify_forms(sim(dc.forms(), 0, "forms")[1])


def test_largest_adler_sums(sim):
    sim(np.full(3 * CH + 1, 0xFF, np.uint8), 0, "0xff")


@pytest.mark.parametrize("n", [1, 5, S + 3, CH + 777])
def test_pointers_that_are_not_dword_aligned(sim, n):
    """every misaligned load and store is in front of the sanitizers here, and the program itself checks the fences around the stream"""
    x = CONTENTS["pair_and_noise"][0](n)
    want = sim(x, 0, f"aligned n={n}")[0]
    for soff, doff in [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (3, 1), (1, 2)]:
        assert sim(x, 0, f"n={n} source +{soff} destination +{doff}", soff, doff)[0] == want


@pytest.mark.parametrize("name", sorted(CONTENTS))
def test_contract_on_the_round_trip_contents(sim, name):
    gen = CONTENTS[name][0]
    for n, row in ((3, 0), (259, ROW), (S + 1, 0), (CH + 1, ROW)):
        info = sim(gen(n), row, f"{name} n={n} row={row}")[1]
        if name == "noise" and n > CH:
            assert info[0]["btype"] == ip.STORED


# DESIGN.md section 5.7's size table: the encoder is integer arithmetic, so the CPU run gives the device's sizes
TABLE = {"smooth_rgb": (393472, 202694), "smooth_rgba": (524544, 270746), "stripes": (131328, 2623)}


@pytest.mark.parametrize("name", sorted(RATIO_CASES))
def test_the_size_table(sim, name):
    stream = RATIO_CASES[name]()[0]
    flat = np.ascontiguousarray(stream).reshape(-1)
    out = sim(flat, stream.shape[1], name)[0]
    assert (flat.size, len(out)) == TABLE[name]
