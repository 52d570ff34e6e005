"""What fnx_ctx_set_deflate_level(FNX_DEFLATE_LEVEL_DENSE) promises of a stream (fennec_hip.h above that entry, DESIGN.md section
5.12) as one function over the stream's bytes (contract_dense), and the inputs that show what the dense parse adds: uncut
matches, the window's edge 32768 back, the lazy step, the chain's depth.  Shared by the CPU run of the kernels' source
(test_deflate_dense_hostsim.py) and the GPU test (test_deflate_dense_gpu.py); the reader is inflate_probe.

The layout, form and code checks are deflate_contract.contract's; the match checks are the dense level's, with positions in the
STREAM.  Every certificate is established from the stream the encoder gave, never from figures recorded here."""
from __future__ import annotations

import functools

import numpy as np

import deflate_contract as dc
import inflate_probe as ip
from deflate_contract import is_match
from fennec_amd import FNX_DEFLATE_CHUNK as CH, FNX_DEFLATE_DENSE_DEPTH as DEPTH, FNX_DEFLATE_SUB as S

WINDOW = 32768


def contract_dense(stream: bytes, data: bytes, stored_tokens=None, label: str = ""):
    """Asserts the layout, the dense match rules, the code rules and the choice of form on a dense device stream of `data`.
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
    assert len(stream) <= n + 10 * max(1, nch) + 6, f"{label}: longer than the stored bound"
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
            tokens = stored_tokens(c)
            assert ip.expand(tokens, data[:c * CH]) == b.out, f"{where}: the unused parse is not the chunk"
            assert ip.fixed_cost(tokens) >= bits, f"{where}: stored ({bits} bits) although fixed takes {ip.fixed_cost(tokens)}"
            rec["tokens"] = tokens
        # ---- matches: positions in the stream
        at, end = c * CH, c * CH + len(b.out)
        for t in tokens:
            if is_match(t):
                length, dist, start = t
                assert start == at
                assert 3 <= length <= 258, f"{where}: a match of {length} bytes"
                assert start + length <= end, f"{where}: a match at {start} of {length} bytes runs past the chunk's end {end}"
                assert 1 <= dist <= min(start, WINDOW), f"{where}: a match at stream position {start} reaches {dist} back"
                assert length > 3 or dist <= 4096, f"{where}: a 3-byte match {dist} back"
                at += length
            else:
                at += 1
        assert at == end
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
        rec["ll_depth"] = dc._check_code(f"{where} literal/length", ll, b.ll_lengths, 15, notes)
        if sum(d):
            rec["d_depth"] = dc._check_code(f"{where} distance", d, b.d_lengths, 15, notes)
        else:
            assert b.d_lengths == (1,), f"{where}: no match, and the distance lengths are {b.d_lengths}"
        single = sum(1 for c_ in cl if c_) == 1
        spare = (1 if cl[0] else 0,) if single else ()
        rec["cl_depth"] = dc._check_code(f"{where} code-length", cl, b.cl_lengths, 7, notes, allow_extra=spare)
        if single:
            assert sorted(l for l in b.cl_lengths if l) == [1, 1]
        rec["cl_hist"] = cl
    for line in notes:
        print(line)
    return p, info


def token_at(tokens, site: int, first: int = 0):
    """-> the index of the token that starts at stream offset `site` (tokens of a chunk whose first byte is at `first`)"""
    at = first
    for i, t in enumerate(tokens):
        if at == site:
            return i
        assert at < site, f"no token starts at {site}: one covers it from {at - (t[0] if is_match(t) else 1)}"
        at += t[0] if is_match(t) else 1
    raise AssertionError(f"no token starts at {site}")


def dense_hash(b0: int, b1: int, b2: int) -> int:
    """the hash of three bytes as fennec_hip.h states it"""
    return (((b0 | b1 << 8 | b2 << 16) * 0x9e3779b1) & 0xffffffff) >> 20


def lazy_replay(table, first: int):
    """the serial walk of the lazy rule over one chunk's (L, D) table -> tokens in inflate_probe's form; `first`: the stream
    offset of the chunk's first byte.  Literals are returned as None (the table does not hold the bytes)."""
    n, p, out = len(table), 0, []
    while p < n:
        l = table[p][0]
        if l >= 3 and p + 1 < n and table[p + 1][0] > l:
            out.append(None)
            p += 1
        elif l >= 3:
            out.append((l, table[p][1], first + p))
            p += l
        else:
            out.append(None)
            p += 1
    return out


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def noise(seed: int, n: int = CH) -> np.ndarray:
    return np.random.default_rng(seed).integers(0, 256, size=n, dtype=np.uint8)


SEED_A, SEED_B = 41, 42


def edge_exact() -> np.ndarray:
    """A ++ A: chunk 1 repeats chunk 0 exactly 32768 back"""
    a = noise(SEED_A)
    return np.concatenate([a, a])


def edge_beyond() -> np.ndarray:
    """A ++ one byte ++ A[:CH - 1]: the repeat is 32769 back, one past the window"""
    a = noise(SEED_A)
    return np.concatenate([a, np.array([a[0] ^ 0x55], np.uint8), a[:CH - 1]])


def edge_two_back() -> np.ndarray:
    """A ++ B ++ A: the repeat is two chunks back"""
    a = noise(SEED_A)
    return np.concatenate([a, noise(SEED_B), a])


@functools.lru_cache(maxsize=None)
def _filler(n: int, seed: int) -> np.ndarray:
    return dc.distinct_windows(np.random.default_rng(seed).integers(0, 200, size=n, dtype=np.uint8), seed + 1000)


SPACING = 600
LAZY_SITES = (SPACING, 2 * SPACING, 3 * SPACING)


@functools.lru_cache(maxsize=None)
def lazy_input() -> np.ndarray:
    """filler without a repeated 3-byte window (values below 200) and, 600 bytes apart, `abc?`, `bcdefghij`, `abcdefghij` (values
    from 200 on): at the third site `abc` is a match of 3, one byte on `bcdefghij` one of 9"""
    x = _filler(4 * SPACING, 21).copy()
    a = list(range(200, 210))                                         # a .. j
    for site, word in zip(LAZY_SITES, ([a[0], a[1], a[2], 250], a[1:], a)):
        x[site:site + len(word)] = word
    return x


def certify_lazy(info):
    tokens = info[0]["tokens"]
    s2, s3 = LAZY_SITES[1], LAZY_SITES[2]
    i = token_at(tokens, s3)
    assert tokens[i:i + 2] == [200, (9, s3 + 1 - s2, s3 + 1)], f"at the third site: {tokens[i:i + 3]}, not the literal and the 9-byte match"


CHAIN_SITES = [SPACING * (k + 1) for k in range(DEPTH + 1)]


@functools.lru_cache(maxsize=None)
def chain_input() -> np.ndarray:
    """the same kind of filler; 600 bytes apart `pqrstuvw`, DEPTH - 1 decoys `pqr` + a byte of their own, `pqrstuvw`: the first
    site is candidate number DEPTH of the last one's chain.  p, q, r are picked so that, of all the input's 3-byte windows, only
    the sites' hash like `pqr` (dense_hash: the header states the function) -- no foreign position takes a place in the chain."""
    base = _filler(SPACING * (DEPTH + 2), 22)
    tail = [200, 201, 202, 203, 204]                                  # s t u v w
    decoy = list(range(205, 205 + DEPTH - 1))
    assert decoy[-1] < 240
    for p in range(240, 256):
        for q in range(240, 256):
            for r in range(240, 256):
                if len({p, q, r}) < 3:
                    continue
                x = base.copy()
                for k, site in enumerate(CHAIN_SITES):
                    word = [p, q, r] + (tail if k in (0, DEPTH) else [decoy[k - 1]])
                    x[site:site + len(word)] = word
                v = x.astype(np.uint64)
                h = ((((v[:-2] | v[1:-1] << np.uint64(8) | v[2:] << np.uint64(16)) * np.uint64(0x9e3779b1)) & np.uint64(0xffffffff)) >> np.uint64(20))
                if np.flatnonzero(h == dense_hash(p, q, r)).tolist() == CHAIN_SITES:
                    return x
    raise AssertionError("no p, q, r whose hash only the sites have")


def certify_chain(info):
    tokens = info[0]["tokens"]
    first, last = CHAIN_SITES[0], CHAIN_SITES[-1]
    i = token_at(tokens, last)
    assert tokens[i] == (8, last - first, last), f"at the last site: {tokens[i]}, not one match of 8 bytes to the first site"


def certify_uncut(info):
    """one chunk of a constant byte: matches as long as the format lets them be, across the lanes' sub-chunks"""
    tokens = info[0]["tokens"]
    assert len(tokens) <= -(-CH // 258) + 3, f"{len(tokens)} tokens"
    assert any(is_match(t) and t[2] // S != (t[2] + t[0] - 1) // S for t in tokens), f"no match crosses a multiple of {S}"


def certify_edge_exact(info):
    """every token of chunk 1 is a match exactly 32768 back -- up to the chunk's last CH mod 258 = 2 bytes, which the serial walk
    reaches with less than a match's three bytes left and must send as literals"""
    tokens = info[1]["tokens"]
    full, rest = divmod(CH, 258)
    assert rest < 3
    want = [(258, WINDOW, CH + 258 * k) for k in range(full)]
    assert tokens[:full] == want, f"chunk 1 does not start with {full} matches of 258 bytes 32768 back: {[t for t, w in zip(tokens, want) if t != w][:1]}"
    assert len(tokens) == full + rest and not any(is_match(t) for t in tokens[full:]), f"chunk 1 ends with {tokens[full:]}"


def certify_edge_beyond(info):
    assert info[1]["btype"] == ip.STORED, "chunk 1 repeats nothing inside the window and is noise: stored"
    # (where the parse is known although the block is stored: the repeat 32769 back is not used -- what matches there are, are
    # noise's chance repeats of three or four bytes, inside the window)
    for t in info[1]["tokens"]:
        assert not is_match(t) or (t[0] <= 4 and t[1] <= WINDOW), f"chunk 1: the match {t}"


def certify_edge_two_back(info):
    assert info[2]["btype"] == ip.STORED, "chunk 2 repeats a chunk two back: out of reach, stored"
