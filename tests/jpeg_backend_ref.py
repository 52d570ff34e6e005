"""What image/jpeg does with a baseline scan's coefficients once they are entropy-decoded, restated in numpy int64 with Go's int32
semantics made explicit: the judge of the device decoder's back half (jpeg_dc_gather_kernel, the DC prefix sum, dec_idct_body and
jpeg_idct.hpp) and of the oracle's (orc_jpeg_decode_planes, orc_jpeg_idct) where their C arithmetic overflows.  Written from
T.81, the Chen-Wang flow graph as idct.go publishes it, and Go's language rules for int32: + - * << wrap to two's complement,
>> is arithmetic.  Here every operation goes through Ops.w, which wraps its int64 result to 32 bits and notes where that changed
the value -- so a case can PROVE that it reaches the overflow it is about.  Every intermediate fits int64: the largest product is
a constant below 2^12 times a value below 2^31.  Test infrastructure only."""
from __future__ import annotations

import numpy as np

ZIG = [0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49, 56,
       57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63]

# image.YCbCrSubsampleRatio by the luminance factors (hy, vy); -1: image.Gray
RATIO = {(1, 1): 0, (2, 1): 1, (2, 2): 2, (1, 2): 3, (4, 1): 4, (4, 2): 5}

# w_k = 2048 sqrt(2) cos(k pi / 16), and 256 / sqrt(2)
W1, W2, W3, W5, W6, W7, R2 = 2841, 2676, 2408, 1609, 1108, 565, 181


def wrap32(x):
    return ((np.asarray(x, np.int64) + 2**31) & 0xffffffff) - 2**31


class Ops:
    """int32 arithmetic on int64 arrays; hit: where a result did not fit (same shape as the operands)"""

    def __init__(self, shape):
        self.hit = np.zeros(shape, bool)

    def w(self, x):
        r = wrap32(x)
        self.hit |= r != x
        return r

    def add(self, a, b):
        return self.w(a + b)

    def sub(self, a, b):
        return self.w(a - b)

    def mul(self, k, a):
        return self.w(k * a)

    def shl(self, a, n):
        return self.w(a * (1 << n))

    def shr(self, a, n):
        return self.w(a >> n)                      # (numpy's >> of a negative int64 is arithmetic; nothing to wrap, kept uniform)


def _row_pass(o, s):
    """the 8-point pass along rows of s = [s0 .. s7], each of some shape S; o: Ops of shape S"""
    a0 = o.add(o.shl(s[0], 11), 128)
    a1 = o.shl(s[4], 11)
    a2, a3, a4, a5, a6, a7 = s[6], s[2], s[1], s[7], s[5], s[3]
    # odd part, first rotations
    t = o.mul(W7, o.add(a4, a5))
    a4 = o.add(t, o.mul(W1 - W7, a4))
    a5 = o.sub(t, o.mul(W1 + W7, a5))
    t = o.mul(W3, o.add(a6, a7))
    a6 = o.sub(t, o.mul(W3 - W5, a6))
    a7 = o.sub(t, o.mul(W3 + W5, a7))
    # even part
    t = o.add(a0, a1)
    a0 = o.sub(a0, a1)
    a1 = o.mul(W6, o.add(a3, a2))
    a2 = o.sub(a1, o.mul(W2 + W6, a2))
    a3 = o.add(a1, o.mul(W2 - W6, a3))
    a1 = o.add(a4, a6)
    a4 = o.sub(a4, a6)
    a6 = o.add(a5, a7)
    a5 = o.sub(a5, a7)
    # third stage
    a7 = o.add(t, a3)
    t = o.sub(t, a3)
    a3 = o.add(a0, a2)
    a0 = o.sub(a0, a2)
    a2 = o.shr(o.add(o.mul(R2, o.add(a4, a5)), 128), 8)
    a4 = o.shr(o.add(o.mul(R2, o.sub(a4, a5)), 128), 8)
    return [o.shr(o.add(a7, a1), 8), o.shr(o.add(a3, a2), 8), o.shr(o.add(a0, a4), 8), o.shr(o.add(t, a6), 8),
            o.shr(o.sub(t, a6), 8), o.shr(o.sub(a0, a4), 8), o.shr(o.sub(a3, a2), 8), o.shr(o.sub(a7, a1), 8)]


def _col_pass(o, s):
    """... along columns: three more bits of precision carried through the rotations, 14 bits dropped at the end"""
    a0 = o.add(o.shl(s[0], 8), 8192)
    a1 = o.shl(s[4], 8)
    a2, a3, a4, a5, a6, a7 = s[6], s[2], s[1], s[7], s[5], s[3]
    t = o.add(o.mul(W7, o.add(a4, a5)), 4)
    a4 = o.shr(o.add(t, o.mul(W1 - W7, a4)), 3)
    a5 = o.shr(o.sub(t, o.mul(W1 + W7, a5)), 3)
    t = o.add(o.mul(W3, o.add(a6, a7)), 4)
    a6 = o.shr(o.sub(t, o.mul(W3 - W5, a6)), 3)
    a7 = o.shr(o.sub(t, o.mul(W3 + W5, a7)), 3)
    t = o.add(a0, a1)
    a0 = o.sub(a0, a1)
    a1 = o.add(o.mul(W6, o.add(a3, a2)), 4)
    a2 = o.shr(o.sub(a1, o.mul(W2 + W6, a2)), 3)
    a3 = o.shr(o.add(a1, o.mul(W2 - W6, a3)), 3)
    a1 = o.add(a4, a6)
    a4 = o.sub(a4, a6)
    a6 = o.add(a5, a7)
    a5 = o.sub(a5, a7)
    a7 = o.add(t, a3)
    t = o.sub(t, a3)
    a3 = o.add(a0, a2)
    a0 = o.sub(a0, a2)
    a2 = o.shr(o.add(o.mul(R2, o.add(a4, a5)), 128), 8)
    a4 = o.shr(o.add(o.mul(R2, o.sub(a4, a5)), 128), 8)
    return [o.shr(o.add(a7, a1), 14), o.shr(o.add(a3, a2), 14), o.shr(o.add(a0, a4), 14), o.shr(o.add(t, a6), 14),
            o.shr(o.sub(t, a6), 14), o.shr(o.sub(a0, a4), 14), o.shr(o.sub(a3, a2), 14), o.shr(o.sub(a7, a1), 14)]


def idct(blocks, row_shortcut=True):
    """blocks: (n, 64) dequantised coefficients in natural order, inside int32 -> ((n, 64) samples before the level shift,
    (n,) whether any operation of the block wrapped).  row_shortcut: a row whose seven AC entries are zero becomes dc << 3
    without going through the flow graph (idct.go does so; False: what the block would be without)."""
    b = np.asarray(blocks, np.int64).reshape(-1, 8, 8)
    assert (wrap32(b) == b).all()
    n = b.shape[0]
    full = Ops((n, 8))
    rows = np.stack(_row_pass(full, [b[:, :, k] for k in range(8)]), axis=2)
    hit = full.hit
    if row_shortcut:
        short = Ops((n, 8))
        dc = short.shl(b[:, :, 0], 3)
        plain = (b[:, :, 1:] == 0).all(axis=2)
        rows = np.where(plain[:, :, None], dc[:, :, None], rows)
        hit = np.where(plain, short.hit, full.hit)
    co = Ops((n, 8))
    out = np.stack(_col_pass(co, [rows[:, k, :] for k in range(8)]), axis=1)
    return out.reshape(n, 64), hit.any(axis=1) | co.hit.any(axis=1)


def level_shift(samples):
    """reader.go: below -128 -> 0, above 127 -> 255, else + 128"""
    s = np.asarray(samples, np.int64)
    return np.where(s < -128, 0, np.where(s > 127, 255, s + 128)).astype(np.uint8)


class Decoded:
    """y, cb, cr: the MCU-padded planes (cb = cr = None: one component); ratio; per block in scan order: dc (the int32 predictor's
    value), dequant ((n, 64), natural order), pre ((n, 64) samples before the level shift), pix (after it), wrapped (any operation
    of the block: the DC sum, a product with the quantiser, the IDCT), wrapped_dequant (the products alone), comp"""


def decode(zz, qtabs, w, h, sampling=None, restart=0, row_shortcut=True):
    """zz: (blocks, 64) as a baseline scan codes them -- zig-zag order, blocks in scan order, position 0 the DC DIFFERENCE.
    qtabs: one or two lists of 64 in zig-zag order (the first for Y, the last for Cb and Cr).  sampling: None (one component)
    or the luminance factors (hy, vy).  restart: MCUs per interval, 0: none."""
    zz = np.asarray(zz, np.int64)
    ncomp = 1 if sampling is None else 3
    hy, vy = (1, 1) if sampling is None else sampling
    mx, my = (w + 8 * hy - 1) // (8 * hy), (h + 8 * vy - 1) // (8 * vy)
    ny = hy * vy
    per = ny + ncomp - 1
    n = mx * my * per
    assert zz.shape == (n, 64), (zz.shape, n)
    comp = np.array([0] * ny + [1, 2][:ncomp - 1], np.int64)[np.arange(n) % per]
    mcu = np.arange(n) // per

    # the predictors: an int32 per component, zero at the start of the scan and of every restart interval
    dc = np.zeros(n, np.int64)
    dc_hit = np.zeros(n, bool)
    for c in range(ncomp):
        idx = np.flatnonzero(comp == c)
        pred, interval = 0, 0
        for i in idx.tolist():
            k = int(mcu[i]) // restart if restart else 0
            if k != interval:
                pred, interval = 0, k
            s = pred + int(zz[i, 0])
            pred = int(wrap32(s))
            dc_hit[i] = pred != s
            dc[i] = pred

    q = np.array([list(qtabs[0]), list(qtabs[-1]), list(qtabs[-1])], np.int64)[comp]       # (n, 64) zig-zag
    coef = zz.copy()
    coef[:, 0] = dc
    mo = Ops((n, 64))
    prod = mo.w(coef * q)
    deq = np.zeros_like(prod)
    deq[:, ZIG] = prod
    pre, idct_hit = idct(deq, row_shortcut)
    pix = level_shift(pre)

    out = Decoded()
    out.ratio = -1 if ncomp == 1 else RATIO[(hy, vy)]
    out.y = np.zeros((8 * vy * my, 8 * hy * mx), np.uint8)
    out.cb = out.cr = None
    if ncomp == 3:
        out.cb, out.cr = np.zeros((8 * my, 8 * mx), np.uint8), np.zeros((8 * my, 8 * mx), np.uint8)
    for i in range(n):
        m, j = divmod(i, per)
        my0, mx0 = divmod(m, mx)
        tile = pix[i].reshape(8, 8)
        if j < ny:                                  # the MCU's Y blocks: hy across, vy down, row by row
            py, px = 8 * (vy * my0 + j // hy), 8 * (hy * mx0 + j % hy)
            out.y[py:py + 8, px:px + 8] = tile
        else:
            (out.cb if j == ny else out.cr)[8 * my0:8 * my0 + 8, 8 * mx0:8 * mx0 + 8] = tile
    out.dc, out.dequant, out.pre, out.pix, out.comp = dc, deq, pre, pix, comp
    out.wrapped_dequant = mo.hit.any(axis=1)
    out.wrapped = dc_hit | out.wrapped_dequant | idct_hit
    out.w, out.h = w, h
    return out


def unsaturated(pix):
    """per block: how many of its 64 samples lie strictly inside 1 .. 254"""
    p = np.asarray(pix).reshape(-1, 64)
    return ((p >= 1) & (p <= 254)).sum(axis=1)
