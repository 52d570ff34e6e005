"""What DESIGN.md section 5.7 promises of a stream of deflate.hip's, as one function over the stream's bytes (contract), and
the inputs that reach the branches ordinary content does not: both length limits, the far distance symbols, the three-byte
rule, the three block forms side by side, more than 256 chunks.  Shared by the GPU test (test_deflate_structure_gpu.py) and
the CPU run of the kernels' source (test_deflate_hostsim.py); the reader is inflate_probe, which knows nothing of the encoder.

Every input is built from a fixed seed, and what it is meant to reach is certified from the stream it gave (the certify_*
functions), never from figures recorded here."""
from __future__ import annotations

import functools
from collections import Counter

import numpy as np

import inflate_probe as ip
from fennec_amd import FNX_DEFLATE_CHUNK as CH, FNX_DEFLATE_SUB as S

ROW = 1 + 3 * 67                                                      # test_deflate_gpu.ROW: the row of a 67-pixel RGB stream


def is_match(t) -> bool:
    return isinstance(t, tuple)


def _check_code(name, hist, lengths, limit, notes, allow_extra=()):
    """one Huffman code of a dynamic block against the histogram of what the block sent in it -> the histogram's Huffman depth"""
    lengths = list(lengths) + [0] * (len(hist) - len(lengths))
    assert max(lengths) <= limit, f"{name}: a code of {max(lengths)} bits"
    for s, c in enumerate(hist):
        assert c == 0 or lengths[s] > 0, f"{name}: symbol {s} is sent and has no code"
        assert c > 0 or lengths[s] == 0 or s in allow_extra, f"{name}: symbol {s} has a code and is never sent"
    used = sum(1 for c in hist if c)
    depth, optimum = ip.huffman(hist)
    cost = ip.code_cost(hist, lengths)
    if used >= 2:
        have, full = ip.kraft(lengths)
        assert have == full, f"{name}: Kraft sum {have} / {full}: the code is not complete"
    if depth <= limit:
        assert cost == optimum, f"{name}: {cost} bits, the Huffman optimum is {optimum} (depth {depth} fits {limit})"
    else:
        best = ip.limited_cost(hist, limit)
        assert cost >= best, f"{name}: {cost} bits is below the optimum {best} under the limit: the helper is wrong"
        assert max(lengths) == limit
        notes.append(f"{name}: Huffman depth {depth} > {limit}; {cost} bits against package-merge's {best} ({100 * (cost / best - 1):+.2f} %), "
                     f"unlimited {optimum}")
    return depth


def contract(stream: bytes, data: bytes, stored_tokens=None, label: str = ""):
    """Asserts the layout, the match rules, the code rules and the choice of form on a device stream of `data`.
    stored_tokens(c) -> the parse's tokens of chunk c, for chunks that took the stored form (None: those are not judged).
    -> (the probe, one dict per chunk: btype, tokens, and for dynamic blocks the Huffman depth of each histogram)"""
    p = ip.probe(stream)
    n = len(data)
    assert p.out == data, f"{label}: the stream does not inflate to its input"
    assert stream[:2] == b"\x78\x01"
    nch = -(-n // CH)
    # ---- layout
    assert len(p.blocks) == 2 * nch - 1, f"{label}: {len(p.blocks)} blocks for {nch} chunks"
    assert p.tail_pad == 0, "padding bits in front of the check"
    assert len(stream) == (p.blocks[-1].bit_end + 7) // 8 + 4
    notes, info = [], []
    for c in range(nch):
        b = p.blocks[2 * c]
        where = f"{label} chunk {c}"
        assert b.bit_start % 8 == 0, f"{where} does not start on a byte"
        assert b.out_start == c * CH and b.out == data[c * CH:(c + 1) * CH], f"{where}: not the chunk's own bytes"
        assert b.bfinal == (1 if c == nch - 1 else 0), f"{where}: BFINAL {b.bfinal}"
        assert b.pad == 0
        if c < nch - 1:
            e = p.blocks[2 * c + 1]
            assert (e.btype, e.bfinal, len(e.out), e.pad) == (ip.STORED, 0, 0, 0), f"{where}: no empty stored block behind it"
            assert e.bit_start == b.bit_end and e.bit_end % 8 == 0 and e.bit_end - e.bit_start == 3 + -(e.bit_start + 3) % 8 + 32
        rec = {"btype": b.btype, "tokens": b.tokens}
        info.append(rec)
        tokens, bits = b.tokens, b.bit_end - b.bit_start
        if b.btype == ip.STORED:
            assert bits == 8 * (5 + len(b.out))
            if stored_tokens is None:
                continue
            # the parse the block did not use: the match rules hold for it all the same, and the fixed form, whose size
            # follows from the tokens alone, must not have been smaller
            tokens = stored_tokens(c)
            assert ip.expand(tokens, data[:c * CH]) == b.out, f"{where}: the unused parse is not the chunk"
            assert ip.fixed_cost(tokens) >= bits, f"{where}: stored ({bits} bits) although fixed takes {ip.fixed_cost(tokens)}"
            rec["tokens"] = tokens
        # ---- matches
        at = c * CH
        for t in tokens:
            if is_match(t):
                length, dist, start = t
                q = start - c * CH
                assert start == at
                assert dist <= q, f"{where}: a match at {q} reaches {dist} back, behind the chunk's start"
                assert 3 <= length <= 258 and q % S + length <= S, f"{where}: a match of {length} at {q} crosses a multiple of {S}"
                assert length > 3 or dist <= 4096, f"{where}: a 3-byte match {dist} back"
                at += length
            else:
                at += 1
        assert at == c * CH + len(b.out)
        if b.btype == ip.STORED:
            continue
        # ---- form
        fixed = ip.fixed_cost(tokens)
        assert bits <= fixed, f"{where}: {bits} bits, the fixed codes take {fixed}"
        assert bits < 8 * (5 + len(b.out)), f"{where}: {bits} bits, stored takes {8 * (5 + len(b.out))}"
        if b.btype == ip.FIXED:
            assert bits == fixed
            continue
        # ---- codes
        ll, d = ip.histograms(tokens)
        cl = [0] * 19
        for s, _ in b.cl_seq:
            cl[s] += 1
        assert b.hlit == 257 or b.ll_lengths[-1] != 0, f"{where}: HLIT {b.hlit} is not trimmed"
        assert b.hdist == 1 or b.d_lengths[-1] != 0, f"{where}: HDIST {b.hdist} is not trimmed"
        assert b.hclen == 4 or b.cl_lengths[ip.CLORD[b.hclen - 1]] != 0, f"{where}: HCLEN {b.hclen} is not trimmed"
        rec["ll_depth"] = _check_code(f"{where} literal/length", ll, b.ll_lengths, 15, notes)
        if sum(d):
            rec["d_depth"] = _check_code(f"{where} distance", d, b.d_lengths, 15, notes)
        else:
            assert b.d_lengths == (1,), f"{where}: no match, and the distance lengths are {b.d_lengths}"
        # a code-length code of one symbol is sent with a second, unused code so that it is complete
        single = sum(1 for c_ in cl if c_) == 1
        spare = (1 if cl[0] else 0,) if single else ()
        rec["cl_depth"] = _check_code(f"{where} code-length", cl, b.cl_lengths, 7, notes, allow_extra=spare)
        if single:
            assert sorted(l for l in b.cl_lengths if l) == [1, 1]
        rec["cl_hist"] = cl
    for line in notes:
        print(line)
    return p, info


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def distinct_windows(x: np.ndarray, seed: int, max_rounds: int = 400) -> np.ndarray:
    """x with bytes swapped at random until all of its 3-byte windows are distinct (no position has a match then).  A swap is
    kept when it does not add repeated windows."""
    rng = np.random.default_rng(seed)
    x = [int(v) for v in x]
    n = len(x)
    cnt: Counter = Counter((x[i], x[i + 1], x[i + 2]) for i in range(n - 2))
    extra = sum(c - 1 for c in cnt.values())

    def windows(a, b):
        return sorted({i for q in (a, b) for i in range(max(0, q - 2), min(n - 3, q) + 1)})

    for _ in range(max_rounds):
        if extra == 0:
            return np.array(x, dtype=np.uint8)
        repeated = [i for i in range(n - 2) if cnt[(x[i], x[i + 1], x[i + 2])] > 1]
        picks = rng.integers(0, 3, size=len(repeated))
        others = rng.integers(0, n, size=len(repeated))
        for i, k, b in zip(repeated, picks, others):
            a, b = i + int(k), int(b)
            if cnt[(x[i], x[i + 1], x[i + 2])] < 2 or x[a] == x[b]:
                continue
            ws = windows(a, b)
            before = extra
            for w in ws:
                key = (x[w], x[w + 1], x[w + 2])
                cnt[key] -= 1
                extra -= 1 if cnt[key] >= 1 else 0
            x[a], x[b] = x[b], x[a]
            for w in ws:
                key = (x[w], x[w + 1], x[w + 2])
                extra += 1 if cnt[key] >= 1 else 0
                cnt[key] += 1
            if extra > before:                                        # undo
                for w in ws:
                    key = (x[w], x[w + 1], x[w + 2])
                    cnt[key] -= 1
                    extra -= 1 if cnt[key] >= 1 else 0
                x[a], x[b] = x[b], x[a]
                for w in ws:
                    key = (x[w], x[w + 1], x[w + 2])
                    extra += 1 if cnt[key] >= 1 else 0
                    cnt[key] += 1
    raise AssertionError(f"{extra} repeated windows left after {max_rounds} rounds")


@functools.lru_cache(maxsize=None)
def limit15() -> np.ndarray:
    """32768 bytes without a match whose literal/length histogram needs the 15-bit limit: byte values 64 .. 76 have the counts
    1, 2, 3, 5, ... 377, which with the end-of-block's 1 in front are a Fibonacci chain 13 deep; the values 0 .. 63 share
    the other 31782 bytes evenly and put about 6 more levels on top."""
    chain = [1, 2]
    while len(chain) < 13:
        chain.append(chain[-1] + chain[-2])
    assert chain[-1] == 377
    rest = CH - sum(chain)
    counts = [rest // 64 + (1 if v < rest % 64 else 0) for v in range(64)] + chain
    x = np.repeat(np.arange(77, dtype=np.uint8), counts)
    assert len(x) == CH == 32768
    np.random.default_rng(15).shuffle(x)
    return distinct_windows(x, 1515)


@functools.lru_cache(maxsize=None)
def ties() -> np.ndarray:
    """32768 bytes without a match whose literal/length histogram is full of ties between a leaf and an internal node: the
    end-of-block's 1 and the byte values 64 .. 75 with counts 1, 2, 2, 4, 6, 10, 16, 26, 42, 68, 110, 178 (from 4, 6 on each the sum
    of the two before it, which is also what the nodes below it weigh), the values 0 .. 63 sharing the rest.  The merge that
    sends ties to the leaf builds the Huffman tree of least depth, 14 deep here: no limit is needed and the cost is the
    optimum.  Ties to the internal node give a tree 19 deep at the same cost, which the 15-bit limit then makes dearer."""
    chain = [1, 2, 2, 4, 6]
    while len(chain) < 12:
        chain.append(chain[-1] + chain[-2])
    rest = CH - sum(chain)
    counts = [rest // 64 + (1 if v < rest % 64 else 0) for v in range(64)] + chain
    x = np.repeat(np.arange(64 + len(chain), dtype=np.uint8), counts)
    assert len(x) == CH == 32768
    np.random.default_rng(16).shuffle(x)
    return distinct_windows(x, 1616)


@functools.lru_cache(maxsize=None)
def limit7() -> np.ndarray:
    """1023 bytes without a match over the byte values 0 .. 137 whose counts are powers of two (3 x 128, 1 x 64, 5 x 32, 7 x 16,
    12 x 8, 21 x 4, 34 x 2, 55 x 1): with the end-of-block the code lengths are 3 .. 10 exactly, and the lengths 1, 3 .. 10 and
    the one run of zeros are sent 1, 3, 1, 5, 7, 12, 21, 34, 56 and 1 times -- a histogram 9 deep for a code of at most 7 bits.
    No four neighbouring values share a count, so the sequence has no use for symbol 16."""
    left = {128: 3, 64: 1, 32: 5, 16: 7, 8: 12, 4: 21, 2: 34, 1: 55}
    dealt: list = []
    while len(dealt) < 138:                                           # the count most in hand, unless it was dealt three times running
        order = sorted(left, key=lambda c: (-left[c], c))
        pick = next(c for c in order if left[c] and not (len(dealt) >= 3 and dealt[-3:] == [c] * 3))
        dealt.append(pick)
        left[pick] -= 1
    assert not any(left.values())
    x = np.repeat(np.arange(138, dtype=np.uint8), dealt)
    assert len(x) == 1023
    np.random.default_rng(7).shuffle(x)
    return distinct_windows(x, 77, max_rounds=4000)


def behind_noise(x: np.ndarray) -> np.ndarray:
    """x as the second chunk, behind a chunk of noise"""
    return np.concatenate([np.random.default_rng(2).integers(0, 256, size=CH, dtype=np.uint8), x])


# name: first site, distance, word length, distance symbol.  The first four are their symbols' smallest distances, whose extra
# bits are all zero; the others set extra bits, 10941 some of the twelve, 16384 and 24576 all twelve / thirteen.
FAR = {"8193": (5, 8193, 40, 26), "12289": (5, 12289, 40, 27), "16385": (5, 16385, 40, 28), "24577": (5, 24577, 40, 29),
       "32764": (0, 32764, 4, 29), "10941": (5, 10941, 40, 26), "16384": (5, 16384, 40, 27), "24576": (5, 24576, 40, 28)}


def far_match(name: str) -> np.ndarray:
    """a chunk of zeros with one noise word (no zero byte in it) at two sites"""
    at, dist, wlen, _ = FAR[name]
    x = np.zeros(CH, np.uint8)
    word = np.random.default_rng(dist).integers(1, 256, size=wlen, dtype=np.uint8)
    x[at:at + wlen] = word
    x[at + dist:at + dist + wlen] = word
    return x


def three_bytes(dist: int) -> tuple:
    """a chunk of zeros with the word 11 22 33 at two sites `dist` apart, followed by 01 at the first and 02 at the second: a
    match of exactly three bytes -> (the chunk, the second site)"""
    x = np.zeros(CH, np.uint8)
    a = 200
    x[a:a + 4] = [0x11, 0x22, 0x33, 0x01]
    x[a + dist:a + dist + 4] = [0x11, 0x22, 0x33, 0x02]
    return x, a + dist


def forms() -> np.ndarray:
    return np.concatenate([np.random.default_rng(3).integers(0, 256, size=CH, dtype=np.uint8), np.full(CH, 0x5A, np.uint8),
                           np.array([1, 2, 3], np.uint8)])


def many_chunks() -> np.ndarray:
    """257 chunks and 5 bytes: the chunks 0, 255 and 256 noise, the rest a period of ROW bytes"""
    n = 257 * CH + 5
    x = np.resize((np.arange(ROW) * 37 + 11).astype(np.uint8), n)
    for c in (0, 255, 256):
        x[c * CH:(c + 1) * CH] = np.random.default_rng(100 + c).integers(0, 256, size=CH, dtype=np.uint8)
    return x


# ---- certificates: what an input reached, from its stream ---------------------------------------------------------------------
def certify_limit15(info, c: int):
    rec = info[c]
    assert rec["btype"] == ip.DYNAMIC and not any(is_match(t) for t in rec["tokens"]), "one dynamic block without a match"
    assert rec["ll_depth"] > 15, f"the literal/length histogram is only {rec['ll_depth']} deep: the limit was not needed"
    print(f"literal/length histogram {rec['ll_depth']} deep, longest code 15")   # contract has asserted max(lengths) == 15


def certify_ties(info, c: int, lengths):
    """the least-depth tree fits the limit (contract has then asserted the Huffman optimum) and it is the tree that was sent"""
    rec = info[c]
    assert rec["btype"] == ip.DYNAMIC and not any(is_match(t) for t in rec["tokens"]), "one dynamic block without a match"
    assert rec["ll_depth"] == max(lengths) <= 15, (rec["ll_depth"], max(lengths))
    print(f"literal/length histogram with ties: least depth {rec['ll_depth']}, longest code {max(lengths)}")


def certify_limit7(info, c: int):
    rec = info[c]
    assert rec["btype"] == ip.DYNAMIC and not any(is_match(t) for t in rec["tokens"]), "one dynamic block without a match"
    assert rec["cl_depth"] > 7, f"the code-length histogram {rec['cl_hist']} is only {rec['cl_depth']} deep: the limit was not needed"
    print(f"code-length histogram {rec['cl_hist']}, {rec['cl_depth']} deep, longest code 7")


def certify_far(info, name: str):
    at, dist, wlen, sym = FAR[name]
    assert ip.distance_symbol(dist) == sym
    # the zeros behind the word match too: the token is as long as the sub-chunk lets it be
    found = [t for t in info[0]["tokens"] if is_match(t) and t[1:] == (dist, at + dist)]
    assert found and found[0][0] >= wlen, f"no match of at least {wlen} bytes {dist} back at {at + dist}"


def certify_three_bytes(info, dist: int, site: int):
    tokens = info[0]["tokens"]
    if dist <= 4096:
        assert (3, dist, site) in tokens, f"no 3-byte match {dist} back at {site}"
    else:
        at, i = 0, 0
        while at < site:
            at += tokens[i][0] if is_match(tokens[i]) else 1
            i += 1
        assert at == site and tokens[i:i + 4] == [0x11, 0x22, 0x33, 0x02], f"at {site}: {tokens[i:i + 4]}, not the word's literals"


def certify_forms(info):
    assert [r["btype"] for r in info] == [ip.STORED, ip.DYNAMIC, ip.FIXED]
