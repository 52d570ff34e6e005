"""hitTargetSize's PNG legs (targetsize.go:39-43, 51-90, 180-206, 285-347) restated for the tests of fnx_png_target_size and
fnx_hit_target_size.  The control flow is the reference's; the pixel steps are the CPU oracle's and median_cut_ref's
(box_downsample, lanczos_resize, apply_palette, ssim_fast: bit-exact integer steps, plus SSIM); a size is the length of the
file the already-pinned single route writes on the SAME context (Context.png_encode, Context.png_reduce) -- the library's
"fits" is stated over its own files under the context's deflate level."""
from __future__ import annotations

import median_cut_ref as mc
from fennec_amd import (FNX_PNG_NRGBA, FNX_PNG_PALETTED, FNX_TS_FALLBACK_PNG, FNX_TS_QUANTIZE, FNX_TS_SCALE_PNG)
from oracle import oracle as orc

LEVELS = (16, 32, 64, 128, 256)


def empty():
    return dict(strategy=0, quality=0, final_w=0, final_h=0, steps=0, nbytes=0, ssim=0.0)


def better_fit(c, b, t):
    """betterFit (targetsize.go:92-115)."""
    cu, bu = c["nbytes"] <= t, b["nbytes"] <= t
    if cu and not bu:
        return True
    if not cu and bu:
        return False
    if cu and bu:
        if c["ssim"] != b["ssim"]:
            return c["ssim"] > b["ssim"]
        return c["quality"] > b["quality"]
    return c["nbytes"] < b["nbytes"]


def ssim_nrgba(src, img):
    """computeSSIMNRGBA (targetsize.go:563-568)."""
    h, w = src.shape[:2]
    if img.shape[:2] != (h, w):
        img = orc.lanczos_resize(img, w, h)
    return orc.ssim_fast(src, img)


class PngLegs:
    """The three legs over one source on one context; every image and every file is made once and kept."""

    def __init__(self, ctx, src):
        self.ctx, self.src = ctx, src
        self._palettes = None
        self._level, self._box, self._lanczos, self._fallback = {}, {}, {}, None

    # ---- what the legs are built from
    def palettes(self):
        if self._palettes is None:
            self._palettes = mc.median_cut(self.src, LEVELS)[0]
        return self._palettes

    def level(self, l):
        """-> (palette, quantized image, the paletted file) of LEVELS[l]"""
        if l not in self._level:
            pal = self.palettes()[l]
            idx, quant = orc.apply_palette(self.src, pal)
            self._level[l] = (pal, quant, self.ctx.png_encode(idx, FNX_PNG_PALETTED, len(pal), -1, pal))
        return self._level[l]

    def level_sizes(self):
        """s16 .. s256, in LEVELS' order"""
        return [len(self.level(l)[2]) for l in range(5)]

    def box(self, nw, nh):
        if (nw, nh) not in self._box:
            self._box[nw, nh] = len(self.ctx.png_encode(orc.box_downsample(self.src, nw, nh), FNX_PNG_NRGBA))
        return self._box[nw, nh]

    def lanczos(self, fw, fh):
        if (fw, fh) not in self._lanczos:
            img = orc.lanczos_resize(self.src, fw, fh)
            self._lanczos[fw, fh] = (img, self.ctx.png_encode(img, FNX_PNG_NRGBA))
        return self._lanczos[fw, fh]

    def fallback(self):
        if self._fallback is None:
            kind, pal, plane = self.ctx.png_reduce(self.src)
            self._fallback = self.ctx.png_encode(self.src if kind == FNX_PNG_NRGBA else plane, kind, len(pal), -1,
                                                 pal if kind == FNX_PNG_PALETTED else None)
        return self._fallback

    # ---- the legs
    def quantize(self, target):
        """quantizeStrategy (targetsize.go:180-206) -> (candidate, image, file)"""
        h, w = self.src.shape[:2]
        c = empty()
        pals = self.palettes()
        for l in (4, 3, 2, 1, 0):
            if l == 4 or len(pals[l]) != len(pals[l + 1]):               # else the palette before it once more: no new query
                c["steps"] += 1
            pal, quant, file = self.level(l)
            if len(file) <= target:
                c.update(strategy=FNX_TS_QUANTIZE, final_w=w, final_h=h, nbytes=len(file), ssim=ssim_nrgba(self.src, quant))
                return c, quant, file
        return c, None, None

    def scale(self, target, cancelled=False):
        """scaleSearch with format PNG (targetsize.go:285-347)"""
        h, w = self.src.shape[:2]
        c = empty()
        lo, hi, best = 0.05, 1.0, 0.0
        for _ in range(12):
            if cancelled:
                break
            mid = (lo + hi) / 2
            nw, nh = int(float(w) * mid), int(float(h) * mid)
            if nw < 1 or nh < 1:
                lo = mid
                continue
            c["steps"] += 1
            if self.box(nw, nh) <= target:
                best, lo = mid, mid
            else:
                hi = mid
        if best == 0.0:
            return c, None, None
        fw, fh = int(float(w) * best), int(float(h) * best)
        img, file = self.lanczos(fw, fh)
        c["steps"] += 1
        c.update(strategy=FNX_TS_SCALE_PNG, final_w=fw, final_h=fh, nbytes=len(file), ssim=ssim_nrgba(self.src, img))
        return c, img, file

    def fall(self):
        """fallbackTargetSizeEncode's PNG branch (targetsize.go:86-89)"""
        h, w = self.src.shape[:2]
        c = empty()
        file = self.fallback()
        c.update(strategy=FNX_TS_FALLBACK_PNG, final_w=w, final_h=h, steps=1, nbytes=len(file), ssim=1.0)
        return c, self.src, file


def restate(legs: PngLegs, target, strategies, cancelled=False):
    """fnx_png_target_size's answer -> (three candidates, winner index or None, the winner's image, the winner's file)"""
    cands, made = [empty() for _ in range(3)], [None, None, None]
    if strategies & FNX_TS_QUANTIZE and not cancelled:
        cands[0], *made[0] = legs.quantize(target)
    none = not cands[0]["strategy"]
    if strategies & FNX_TS_SCALE_PNG and none and not cancelled:
        cands[1], *made[1] = legs.scale(target)
    if strategies & FNX_TS_FALLBACK_PNG and not any(c["strategy"] for c in cands):
        cands[2], *made[2] = legs.fall()
    win = None
    for i, c in enumerate(cands):
        if c["strategy"] and (win is None or better_fit(c, cands[win], target)):
            win = i
    if win is None:
        return cands, None, None, None
    return cands, win, made[win][0], made[win][1]
