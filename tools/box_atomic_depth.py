#!/usr/bin/env python3
"""How deep do the box atomics of blur_mfma_kernel<SCORE> serialise?  A CPU model of ONE ds_add_u32 wave instruction.

A step of the kernel issues, per side and wave, four ds_add_u32: instruction k adds, from lane (r, g) = (lane & 15, lane >> 4),
the sum of row 16 j + 4 g + k of the lane's indicator column r = 3 slot + channel into the box table at rowoff[row] + coln
(blur_mfma.hip: mf_box_add4).  Lanes that hit one dword serialise, and so do lanes that hit different dwords of one of the 64
LDS banks.  This tool rebuilds the launch geometry as blur_plan.cpp does (build_score_geom, score_mfma_tables: box_edge, nbx, nby,
the five slots of a wave's 16 px, the row offsets of every segment) and reports, over every 16-row block of every segment and
every wave of every tile column of the blurred side, the mean over instructions of

  * the deepest same-dword chain and the deepest same-bank chain with ALL 64 lanes issuing (the kernel up to r8),
  * the same with only the LIVE lanes issuing (r < 15, the wave has a boxed pixel, the slot holds one of its 16 px),
  * the share of lanes that are not live, and
  * the live lanes' depths at the table row pitch choose_pitch() would pick: the smallest multiple of 16 bytes >= 16 (nbx + 1)
    whose same-bank depth equals the same-dword depth, while the tables still leave three workgroups per CU their LDS.  The
    kernel's pitch IS 16 (nbx + 1): a padded pitch was built, measured and not merged (CHANGELOG, "box atomics only from live
    lanes"), so this line says what a geometry would gain, not what it gets.

    python tools/box_atomic_depth.py 3840 2160 [seg]
"""
import collections
import math
import sys

import numpy as np

BANKS = 64
LDS_PER_CU = 163840
STATIC_LDS = 35648          # blur_mfma_kernel<SCORE, .>: ring, stages, row tables
WORKGROUPS = 3


def ssim_fast_dims(w, h):
    """api.cpp: ssim_fast_dims (ssim.go:52-56)"""
    if w <= 512 and h <= 512:
        return w, h
    scale = 512.0 / max(float(w), float(h))
    rnd = lambda v: int(math.floor(v + 0.5))
    return max(8, rnd(w * scale)), max(8, rnd(h * scale))


def box_edge(d, ratio, n):
    """devutil.hpp: box_edge"""
    s0, s1 = int(float(d) * ratio), int(float(d + 1) * ratio)
    s1 = min(s1, n)
    if s0 >= s1:
        s0 = s1 - 1
    return max(s0, 0), s1


def box_map(n, dst):
    m = [-1] * n
    ratio = float(n) / float(dst)
    for d in range(dst):
        s0, s1 = box_edge(d, ratio, n)
        for x in range(s0, s1):
            m[x] = d
    return m


def span(m, lo, hi):
    v = [b for b in m[lo:hi] if b >= 0]
    return v[-1] - v[0] + 1 if v else 0


class Geometry:
    """blur_plan.cpp: build_score_geom with th_fixed = seg, then score_mfma_tables"""

    def __init__(self, w, h, seg=272):
        self.w, self.h, self.seg = w, h, seg
        self.dstW, self.dstH = ssim_fast_dims(w, h)
        self.bx, self.by = box_map(w, self.dstW), box_map(h, self.dstH)
        self.nbx = max([1] + [span(self.bx, x0, min(w, x0 + 64)) for x0 in range(0, w, 64)])
        self.nby = max([1] + [span(self.by, y0, min(h, y0 + seg)) for y0 in range(0, h, seg)])
        self.tiles_x, self.segs = (w + 63) // 64, (h + seg - 1) // seg

    def min_pitch(self):
        return 16 * (self.nbx + 1)

    def columns(self):
        """Counter of (coln[64], live[64]) over (tile column, wave)"""
        out = collections.Counter()
        for tx in range(self.tiles_x):
            x0 = 64 * tx
            b0 = self.bx[x0]
            colbox = []
            for i in range(64):
                v = self.bx[x0 + i] if x0 + i < self.w else -1
                colbox.append(v - b0 if v >= 0 and b0 >= 0 else 255)
            for wave in range(4):
                px = colbox[16 * wave:16 * wave + 16]
                first = min(px)
                coln, live = [], []
                for lane in range(64):
                    r = lane & 15
                    slot, ch = divmod(r, 3)
                    cnt = sum(1 for c in px if r < 15 and c == first + slot)
                    lv = r < 15 and first != 255 and cnt > 0
                    coln.append(16 * (first + slot if lv else self.nbx) + 4 * (ch if r < 15 else 3))
                    live.append(lv)
                out[(tuple(coln), tuple(live))] += 1
        return out

    def rows(self):
        """Counter of the box-row indices (spare: nby) of lane groups g = 0..3 of one instruction, blurred side:
        row 16 j + 4 g + k of every segment, set j and k"""
        out = collections.Counter()
        for ty in range(self.segs):
            y0 = ty * self.seg
            b0 = self.by[y0]
            nj = (min(self.seg, ((self.h - y0 + 15) >> 4) << 4)) >> 4

            def boxrow(t):
                v = self.by[y0 + t] if 0 <= t < self.seg and y0 + t < self.h else -1
                return v - b0 if v >= 0 and b0 >= 0 else self.nby
            for j in range(nj):
                for k in range(4):
                    out[tuple(boxrow(16 * j + 4 * g + k) for g in range(4))] += 1
        return out


def _depth(key, active):
    """key, active: [..., 64]; deepest chain of active lanes with equal keys, per leading index"""
    eq = (key[..., :, None] == key[..., None, :]) & active[..., :, None] & active[..., None, :]
    return eq.sum(-1).max(-1)


def depths(geo, pitch=None, live_only=False):
    """(mean same-dword depth, mean same-bank depth, dead-lane share) over all box atomic instructions of a launch"""
    pitch = pitch or geo.min_pitch()
    cols, rows = geo.columns(), geo.rows()
    C = np.array([c for c, _ in cols], dtype=np.int64)
    L = np.array([l for _, l in cols], dtype=bool)
    cw = np.array(list(cols.values()), dtype=np.float64)
    R = np.array(list(rows), dtype=np.int64) * pitch
    rw = np.array(list(rows.values()), dtype=np.float64)
    grp = np.arange(64) >> 4
    act = L if live_only else np.ones_like(L)
    sd = sb = 0.0
    for i in range(len(R)):
        addr = R[i][grp][None, :] + C
        dw = addr >> 2
        sd += rw[i] * float((_depth(dw, act) * cw).sum())
        sb += rw[i] * float((_depth(dw % BANKS, act) * cw).sum())
    n = rw.sum() * cw.sum()
    dead = float(((~L).sum(-1) * cw).sum()) / (64.0 * cw.sum())
    return sd / n, sb / n, dead


def lds_budget():
    return LDS_PER_CU // WORKGROUPS - STATIC_LDS


def choose_pitch(geo):
    """smallest pitch (bytes, multiple of 16, >= 16 (nbx + 1)) at which the live lanes' bank depth is their dword depth and the
    two tables fit beside three workgroups' static LDS; None: no pitch fits"""
    p = geo.min_pitch()
    while 2 * p * (geo.nby + 1) <= lds_budget():
        d, b, _ = depths(geo, p, live_only=True)
        if b <= d + 1e-9:
            return p
        p += 16
    return None


def report(w, h, seg=272):
    geo = Geometry(w, h, seg)
    d_all, b_all, dead = depths(geo)
    d_live, b_live, _ = depths(geo, live_only=True)
    pitch = choose_pitch(geo)
    res = {"w": w, "h": h, "seg": seg, "nbx": geo.nbx, "nby": geo.nby, "pitch_min": geo.min_pitch(),
           "all": (d_all, b_all), "live": (d_live, b_live), "dead": dead, "pitch": pitch, "live_at_pitch": None}
    if pitch is not None:
        d, b, _ = depths(geo, pitch, live_only=True)
        res["live_at_pitch"] = (d, b)
    return res


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    w, h = int(argv[1]), int(argv[2])
    seg = int(argv[3]) if len(argv) > 3 else 272
    r = report(w, h, seg)
    print(f"{w}x{h} seg {seg}: nbx {r['nbx']} nby {r['nby']}, table row pitch {r['pitch_min']} B, "
          f"tables {2 * r['pitch_min'] * (r['nby'] + 1)} B of {lds_budget()} B")
    print(f"  all lanes : same dword {r['all'][0]:.2f}  same bank {r['all'][1]:.2f}")
    print(f"  live lanes: same dword {r['live'][0]:.2f}  same bank {r['live'][1]:.2f}   dead lanes {100 * r['dead']:.0f} %")
    if r["pitch"] is None:
        print("  no row pitch within the LDS budget of three workgroups per CU brings the bank depth down to the dword depth")
    else:
        print(f"  live lanes at a pitch of {r['pitch']} B: same dword {r['live_at_pitch'][0]:.2f}  same bank {r['live_at_pitch'][1]:.2f}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
