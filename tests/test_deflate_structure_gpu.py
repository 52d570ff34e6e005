"""fnx_deflate's streams read block by block.  zlib.decompress (test_deflate_gpu.py) says that a stream inflates to its
input; this file reads the stream with inflate_probe and holds every block against what DESIGN.md section 5.7 promises
(deflate_contract.contract: layout, match rules, code rules, the choice of form), over the contents of test_deflate_gpu.py
and over inputs that reach what those never do: the 15-bit and the 7-bit length limit, the distance symbols 26 .. 29, the
three-byte rule at 4096 / 4097, the three block forms in one stream, more than 256 chunks, and device pointers that are not
dword aligned.  What an input reaches is certified from the device's own stream."""
from __future__ import annotations

import numpy as np
import pytest

import deflate_contract as dc
import fennec_amd
import inflate_probe as ip
from deflate_contract import CH, S
from test_deflate_gpu import CONTENTS, LENGTHS, ROW, dev, round_trip

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    return fennec_amd.Context(0)


def checked(ctx, x, row=0, label=""):
    """x through the host and the device space (identical bytes, zlib reads them back), then the contract -> per-chunk records"""
    return dc.contract(round_trip(ctx, x, row), x.tobytes(), None, label)[1]


@pytest.mark.parametrize("name", sorted(CONTENTS))
def test_contract_on_the_round_trip_contents(ctx, name):
    gen = CONTENTS[name][0]
    for n in LENGTHS:
        x = gen(n)
        for row in (ROW, 0):                                          # with the row hint and with none
            dc.contract(ctx.deflate(x, row), x.tobytes(), None, f"{name} n={n} row={row}")


def test_the_15_bit_limit(ctx):
    x = dc.limit15()
    dc.certify_limit15(checked(ctx, x, 0, "limit15"), 0)
    dc.certify_limit15(checked(ctx, dc.behind_noise(x), 0, "limit15 as the second chunk"), 1)


def test_ties_go_to_the_leaf(ctx):
    """ties in the merge go to the leaf: the tree of least depth, which needs no limit here, at the Huffman optimum"""
    x = dc.ties()
    p, info = dc.contract(round_trip(ctx, x), x.tobytes(), None, "ties")
    dc.certify_ties(info, 0, p.blocks[0].ll_lengths)


def test_the_7_bit_limit_of_the_code_length_code(ctx):
    x = dc.limit7()
    dc.certify_limit7(checked(ctx, x, 0, "limit7"), 0)
    dc.certify_limit7(checked(ctx, dc.behind_noise(x), 0, "limit7 as the second chunk"), 1)


@pytest.mark.parametrize("name", sorted(dc.FAR))
def test_far_matches(ctx, name):
    """distance symbols 26, 27, 28, 29 (12 and 13 extra bits)"""
    dc.certify_far(checked(ctx, dc.far_match(name), 0, f"far {name}"), name)


@pytest.mark.parametrize("dist", [4096, 4097])
def test_three_byte_match_rule(ctx, dist):
    """a match of three bytes is taken 4096 back and left to its literals 4097 back"""
    x, site = dc.three_bytes(dist)
    dc.certify_three_bytes(checked(ctx, x, 0, f"three bytes {dist} back"), dist, site)


def test_forms_side_by_side(ctx):
    dc.certify_forms(checked(ctx, dc.forms(), 0, "forms"))


def test_more_than_256_chunks(ctx):
    """the gather's loops over the chunks (the prefix sum of the sizes, the Adler-32 combination) make a second trip"""
    x = dc.many_chunks()
    assert len(x) == 257 * CH + 5
    info = checked(ctx, x, ROW, "258 chunks")
    assert [c for c, r in enumerate(info) if r["btype"] == ip.STORED] == [0, 255, 256]


def test_largest_adler_sums(ctx):
    checked(ctx, np.full(3 * CH + 1, 0xFF, np.uint8), 0, "0xff")


@pytest.mark.parametrize("n", [1, 5, S + 3, CH + 777])
def test_pointers_that_are_not_dword_aligned(ctx, n):
    """the chunk kernel's byte-wise load and the gather's head bytes and shifted dwords: the same bytes as the aligned call, and
    nothing outside the stream is written"""
    import torch
    x = CONTENTS["pair_and_noise"][0](n)
    want = round_trip(ctx, x)
    dc.contract(want, x.tobytes(), None, f"aligned n={n}")
    cap = fennec_amd.deflate_bound(n)
    aligned_src = dev(x)
    for soff, doff in [(1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (3, 1), (1, 2)]:
        flat = torch.zeros(n + 8, dtype=torch.uint8, device="cuda")
        flat[soff:soff + n] = aligned_src
        src = flat[soff:soff + n]
        buf = torch.full((cap + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        out = buf[doff:doff + cap]
        assert src.data_ptr() % 4 == soff and out.data_ptr() % 4 == doff
        got = ctx.deflate(src, 0, out=out)
        ctx.sync()
        assert got.cpu().numpy().tobytes() == want, (n, soff, doff)
        host = buf.cpu().numpy()
        assert host[doff:doff + len(want)].tobytes() == want
        assert (host[:doff] == 0xAB).all() and (host[doff + len(want):] == 0xAB).all(), f"bytes outside the stream were written {(n, soff, doff)}"
