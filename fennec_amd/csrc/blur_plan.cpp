// The host plan of GaussianBlur's launches (blur_plan.hpp): the fixed-point weights and digit tables of the matrix kernels, the
// tile and segment arithmetic, the one-pass form's box geometry, and on top of them plan_blur and plan_blur_scored, the one place
// where a call's kernel family is decided.  Plain C++17, no HIP: built into the library and alone by tools/blur_plan_host.cpp.
#include "blur_plan.hpp"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "box_edge.hpp"
#include "dev_env.hpp"

namespace fnx {

bool mfma_quantise(const double *kernel, int radius, MfmaWeights *q, int rmax)
{
    if (radius < 1 || radius > rmax) return false;
    const int nt = 2 * radius + 1;
    double sum = 0;
    for (int i = 0; i < nt; i++) {
        if (!(kernel[i] >= 0) || !(kernel[i] < 0.49)) return false;   // three signed digits reach 127 * 65793 = 0.498 * 2^24
        sum += kernel[i];
    }
    if (!(std::fabs(sum - 1.0) <= 1e-6)) return false;
    long long tot = 0;
    for (int i = 0; i < nt; i++) {
        q->wq[i] = std::llround(kernel[i] * 16777216.0);
        tot += q->wq[i];
    }
    q->wq[radius] += 16777216 - tot;
    if (q->wq[radius] < 0 || q->wq[radius] > 8355711) return false;
    // S - (exact sum) 2^24 = sum_k (wq[k] - w[k] 2^24) p[k] with 0 <= p[k] <= 255: between -255 (sum of the negative
    // differences) and +255 (sum of the positive ones) -- half of 255 sum |.| when the differences cancel, as they nearly do
    long double ep = 0, en = 0;
    for (int i = 0; i < nt; i++) {
        const long double d = static_cast<long double>(q->wq[i]) - static_cast<long double>(kernel[i]) * 16777216.0L;
        if (d > 0) ep += d; else en -= d;
    }
    q->err255 = static_cast<double>(255.0L * std::max(ep, en));
    return true;
}
static void mfma_digits(long long v, int d[3])
{
    for (int i = 0; i < 3; i++) {
        long long lo = ((v % 256) + 256) % 256;
        if (lo >= 128) lo -= 256;
        d[i] = static_cast<int>(lo);
        v = (v - lo) / 256;
    }
}

// The digit matrices of a matrix kernel whose H window is NKH chunks of 64 bytes around frame radius RF and whose V window is NKV
// chunks of VB rows per lane: BH[NKH][3][64] x 16 bytes (digits hi, mid, lo) | BV[NKV][3][64] x VB bytes.  blur_mfma_kernel is
// (1, 1, MF_RMAX, 8), blur_mfma_wide_kernel<NKH> (NKH, NKV, RF, 16).
static void mfma_build_table(const MfmaWeights &q, int radius, int NKH, int NKV, int RF, int VB, uint32_t *tab)
{
    int8_t *bh = reinterpret_cast<int8_t *>(tab);
    int8_t *bv = bh + 3 * NKH * 64 * 16;
    const int nt = 2 * radius + 1, off = RF - radius;
    for (int lane = 0; lane < 64; lane++) {
        const int nn = lane & 15, kc = lane >> 4;
        for (int kk = 0; kk < NKH; kk++)
            for (int b = 0; b < 16; b++) {   // H: K index 64 kk + 16 kc + b = byte of the window; output byte nn = 4 px + channel
                const int px = 16 * kk + 4 * kc + b / 4, ch = b % 4, c = nn % 4, pj = nn / 4;
                const int t = px - pj - off;
                int d[3] = {0, 0, 0};
                if (ch == c && c < 3 && t >= 0 && t < nt) mfma_digits(q.wq[t], d);
                if (ch == c && c == 3 && px == pj + RF) d[0] = 1;   // alpha column: the centre pixel's alpha as it is (effects.go:189)
                for (int l = 0; l < 3; l++) bh[((3 * kk + (2 - l)) * 64 + lane) * 16 + b] = static_cast<int8_t>(d[l]);
            }
        for (int c = 0; c < NKV; c++)
            for (int b = 0; b < VB; b++) {   // V: K index 4 VB c + VB kc + b = staged row of the set's window; output row nn
                const int t = 4 * VB * c + VB * kc + b - nn - off;
                int d[3] = {0, 0, 0};
                if (t >= 0 && t < nt) mfma_digits(q.wq[t], d);
                for (int l = 0; l < 3; l++) bv[((3 * c + (2 - l)) * 64 + lane) * VB + b] = static_cast<int8_t>(d[l]);
            }
    }
}
std::vector<uint32_t> mfma_table(const BlurPlan &p, const double *kernel)
{
    const bool wide = p.family == BLUR_MFMA_WIDE;
    const int rf = wide ? mf_wide_rf(p.nkh) : MF_RMAX;
    std::vector<uint32_t> tab(wide ? mf_wide_tab_all(p.nkh) : MF_TAB_ALL, 0u);
    if (wide) mfma_build_table(p.q, p.radius, p.nkh, mf_wide_nkv(p.nkh), rf, 16, tab.data());
    else mfma_build_table(p.q, p.radius, 1, 1, rf, 8, tab.data());
    // the caller's fp64 weights behind them, centred in the frame with zeros around
    memcpy(reinterpret_cast<double *>(tab.data() + (wide ? mf_wide_tab_words(p.nkh) : MF_TAB_WORDS)) + (rf - p.radius), kernel, sizeof(double) * (2 * p.radius + 1));
    return tab;
}

// Rows per workgroup.  A workgroup of NJ 16-row sets runs NJ + 4 steps (the pipeline's fill and drain); the grid runs in
// rounds of occ workgroups per CU.  The segment count that minimises rounds x steps: long segments for batches (the halo
// is 22 staged rows per segment), one full round of short ones for a single image (4K alone: 17 segments of 128 rows,
// 18 us against 23 with "at least eight workgroups per CU").
static int blur_mfma_segment(int num_cus, int n, int w, int h, int cap, int occ)
{
    const long tiles_x = (w + 63) / 64, slots = static_cast<long>(occ) * num_cus;
    const int sets = (h + 15) / 16;
    int best_seg = 16, first = 1;
    double best = 0;
    for (int nseg = std::max(1, (h + cap - 1) / cap); nseg <= std::max(1, sets / 2); nseg++) {
        const int nj = (sets + nseg - 1) / nseg, seg = 16 * nj;
        if (seg > cap) continue;
        const long segs = (h + seg - 1) / seg, wgs = tiles_x * segs * n;
        const double cost = static_cast<double>((wgs + slots - 1) / slots) * (nj + 4);
        if (first || cost < best * 0.98) { best = cost; best_seg = seg; first = 0; }   // ties go to the longer segment
    }
    return best_seg;
}

// Two tile shapes (measured on MI355X, 4K: 23.6 vs 22.9 us; 1080p: 5.6 vs 6.0 us per image):
//   128 lanes x 64 intermediate rows  (TH = 52 at R=6, H-pass row halo 1.23x)
//   256 lanes x (2*TH+2R) rows         (TH = 104,      halo 1.12x) -- wins when the image height
//     does not leave a mostly empty last tile row and there are enough tiles to fill the chip.
// Cost model: H work ~ staged rows, V work ~ output rows (about 55 : 45 of the instructions).
static int direct_tile_rows(int R, bool tall)
{
    if (R > SCORE_RMAX && R <= FUSED_RMAX) return ((WIDE_IH - 2 * R) / 8) * 8;
    const int th0 = R >= 1 && R <= SCORE_RMAX ? ((64 - 2 * R) / 4) * 4 : 4;   // never 0: callers divide by it
    return tall ? 2 * th0 : th0;
}
static bool direct_tall(int num_cus, int R, int n, int w, int h)
{
    if (R > SCORE_RMAX) return true;                            // one tile shape for the wide radii
    const int TH0 = direct_tile_rows(R, false), TH1 = direct_tile_rows(R, true);
    const long ty0 = (h + TH0 - 1) / TH0, ty1 = (h + TH1 - 1) / TH1;
    const double cost0 = ty0 * (0.55 * (TH0 + 2 * R) + 0.45 * TH0);
    const double cost1 = ty1 * (0.55 * (TH1 + 2 * R) + 0.45 * TH1);
    const long tiles1 = ty1 * ((w + 63) / 64) * n;
    return cost1 < 0.95 * cost0 && tiles1 >= 4L * num_cus;
}

// The guarded kernel's error bound assumes what GaussianBlur's own kernel guarantees (effects.go:155-165):
// weights >= 0 that sum to 1, so accumulators stay below 256.
static bool guard_kernel_ok(const double *kernel, int radius)
{
    double sum = 0;
    for (int i = 0; i < 2 * radius + 1; i++) {
        if (!(kernel[i] >= 0)) return false;
        sum += kernel[i];
    }
    return sum <= 1.0 + 1e-9;
}

// blur_mfma_kernel<SCORE, .>'s set-up, which depends on the geometry alone, as two tables at the end of the blob (r7: every
// workgroup used to work this out from bx / by through LDS, ~300 vector instructions per wave before its first row set):
//  * per (tile column, wave, lane) one word: coln | cnt << 20 | in[0..3] << 25 | channel << 29 | live << 31 -- the lane's
//    indicator-matrix column (box column first + slot of the wave's 16 px, channel ch; lane n = 3 slot + ch, n = 15: nothing), how
//    many of the 16 px lie in it (the seed 128 cnt undoes the A operands' - 128) and its byte offset in a table row (spare
//    column: none).  live: the column is a box column, somebody reads its sums -- the other lanes (lane 15, slots past the
//    wave's last box column, a wave with no boxed pixel) issue no box atomics at all (4K: 28 lanes of 64)
//  * per segment the byte offset, in a box table, of the box row of each of its seg + 16 staged rows (tile rows -6 ..), then of
//    its seg output rows; rows outside the segment or the image go to the spare row nby
// Written as the device code it replaces was, value for value, the corner cases included (a tile or a wave with no boxed column:
// first = 255 matches every column of slot 0, so cnt = 16 there; its lanes point at the spare column and are not live).
static void score_mfma_tables(ScoreGeom &g, int w, int h)
{
    const int seg = g.th, nbx = g.nbx, nby = g.nby;
    const int tiles_x = (w + 63) / 64, segs = (h + seg - 1) / seg;
    const size_t ref_words = 4 * (static_cast<size_t>(g.dstW) + g.dstH);
    const size_t base = (NHEAD + ref_words + static_cast<size_t>(w) + h + 3) & ~size_t(3);   // 16-byte chunks
    g.coltab = base;
    g.rowtab = base + 256 * static_cast<size_t>(tiles_x);
    g.map.resize(g.rowtab + static_cast<size_t>(segs) * (2 * seg + 16), 0);
    const int32_t *bx = g.map.data() + NHEAD + ref_words, *by = bx + w;
    uint32_t *col = reinterpret_cast<uint32_t *>(g.map.data()) + g.coltab, *row = reinterpret_cast<uint32_t *>(g.map.data()) + g.rowtab;
    for (int tx = 0; tx < tiles_x; tx++) {
        const int x0 = 64 * tx;
        uint32_t colbox[64];
        const int b0x = bx[x0];
        for (int i = 0; i < 64; i++) {
            const int v = x0 + i < w ? bx[x0 + i] : -1;
            colbox[i] = (v >= 0 && b0x >= 0) ? static_cast<uint32_t>(v - b0x) : 255u;
        }
        for (int wave = 0; wave < 4; wave++) {
            uint32_t first = 255u;
            for (int i = 0; i < 16; i++) first = std::min(first, colbox[16 * wave + i]);
            for (int lane = 0; lane < 64; lane++) {
                const int r = lane & 15, gq = lane >> 4;
                const int slot = r / 3, ch = r - 3 * slot;
                uint32_t cnt = 0, in = 0;
                for (int i = 0; i < 16; i++) cnt += (r < 15 && colbox[16 * wave + i] == first + slot) ? 1 : 0;
                for (int e = 0; e < 4; e++)
                    if (r < 15 && first != 255u && colbox[16 * wave + 4 * gq + e] == first + slot) in |= 1u << e;
                const bool live = r < 15 && first != 255u && cnt > 0;
                const uint32_t bc = live ? first + slot : static_cast<uint32_t>(nbx);
                const uint32_t coln = 16u * bc + 4u * (r < 15 ? ch : 3);
                col[(4 * tx + wave) * 64 + lane] = coln | cnt << 20 | in << 25 | static_cast<uint32_t>(ch) << 29 | (live ? 1u << 31 : 0u);
            }
        }
    }
    const int rowbytes = 16 * (nbx + 1);
    for (int ty = 0; ty < segs; ty++) {
        const int y0 = ty * seg, b0y = by[y0];
        uint32_t *rh = row + static_cast<size_t>(ty) * (2 * seg + 16), *rv = rh + seg + 16;
        auto off = [&](int t) {
            const int v = (t >= 0 && t < seg && y0 + t < h) ? by[y0 + t] : -1;
            return static_cast<uint32_t>(rowbytes * ((v >= 0 && b0y >= 0) ? v - b0y : nby));
        };
        for (int u = 0; u < seg + 16; u++) rh[u] = off(u - 6);
        for (int t = 0; t < seg; t++) rv[t] = off(t);
    }
}
static bool build_score_geom(ScoreGeom &g, int w, int h, int radius, int dstW, int dstH, int th_fixed = 0)
{
    // (th_fixed: the matrix-pipe kernels' tile, whose rows do not depend on the radius -- radii up to 24 since r5)
    if (radius < 1 || radius > (th_fixed ? mf_wide_rf(MF_SCORE_NKH) : SCORE_RMAX) || w < dstW || h < dstH || dstW <= 0 || dstH <= 0 || w >= (1 << 24) ||
        h >= (1 << 24))
        return false;
    const double xr = static_cast<double>(w) / static_cast<double>(dstW);   // ssim.go:251-252
    const double yr = static_cast<double>(h) / static_cast<double>(dstH);
    // Where the one-pass kernel wins (measured at steady clocks, tools/time_onepass.py, us per image
    // one-pass / two-call): ratio 3.1 (1600x1200) 10.1 / 9.6, 3.75 (1080p) 9.1 / 9.3, 4.3 (2200 px)
    // 11.5 / 12.1, 5 (1440p) 13.8 / 15.2, 7.5 (4K) 26.9 / 31.9, 15 (8K) 98.3 / 120.1.  Small boxes mean
    // many table entries per tile to zero, store and (no room for copies) contend on; below 3.6 the
    // two ops run back to back.  Upwards the limit is the 16-bit sum fields (boxes of <= 256 px).
    if (std::fmin(xr, yr) < 3.6) return false;
    // source column / row -> box index (boxes of a downscale are disjoint and ascending)
    // one table blob: magic[c], tiedown[c][8] (box_mean_u8) | BoxRef per output column, per output row |
    // box index of every source column, every source row
    const size_t ref_words = 4 * (static_cast<size_t>(dstW) + dstH);
    std::vector<int32_t> &map = g.map;
    map.assign(NHEAD + ref_words + static_cast<size_t>(w) + h, -1);
    {
        uint32_t *magic = reinterpret_cast<uint32_t *>(map.data()), *tiedown = magic + 260;
        std::fill(magic, magic + NHEAD, 0u);
        for (uint32_t c = 1; c <= 256; c++) {
            magic[c] = static_cast<uint32_t>((1ull << 32) / (2ull * c)) + 1u;
            if (c & 1u) continue;                                    // odd counts have no ties
            const double inv = 1.0 / static_cast<double>(c);         // inv := 1.0 / count (ssim.go:301)
            for (uint32_t k = 0; k < 256; k++) {
                const double n = static_cast<double>(c / 2) * static_cast<double>(2 * k + 1);   // n / c == k + 0.5
                if (n > 255.0 * c) break;
                if (n * inv < static_cast<double>(k) + 0.5) tiedown[8 * c + (k >> 5)] |= 1u << (k & 31);
            }
        }
    }
    BoxRef *xref = reinterpret_cast<BoxRef *>(map.data() + NHEAD), *yref = xref + dstW;
    int32_t *bx = map.data() + NHEAD + ref_words, *by = bx + w;
    int maxbw = 0, maxbh = 0;
    for (int d = 0; d < dstW; d++) {
        int s0, s1;
        box_edge(d, xr, w, s0, s1);
        if (d + 1 < dstW) { int n0, n1; box_edge(d + 1, xr, w, n0, n1); if (n0 < s1) return false; }
        for (int x = s0; x < s1; x++) bx[x] = d;
        if (s1 - s0 > maxbw) maxbw = s1 - s0;
    }
    for (int d = 0; d < dstH; d++) {
        int s0, s1;
        box_edge(d, yr, h, s0, s1);
        if (d + 1 < dstH) { int n0, n1; box_edge(d + 1, yr, h, n0, n1); if (n0 < s1) return false; }
        for (int y = s0; y < s1; y++) by[y] = d;
        if (s1 - s0 > maxbh) maxbh = s1 - s0;
    }
    if (static_cast<long>(maxbw) * maxbh > 256) return false;   // 16-bit sum fields
    // most boxes a tile touches, for the preferred tile shape and then the other one
    bool tall = g.tall_pref;
    int th = 0, nbx = 0, nby = 0;
    for (int attempt = 0; attempt < (th_fixed ? 1 : 2); attempt++, tall = !tall) {
        th = th_fixed ? th_fixed : direct_tile_rows(radius, tall);
        nbx = nby = 1;
        auto span = [](const int32_t *m, int lo, int hi) {   // boxes touched by [lo, hi)
            int first = -1, last = -1;
            for (int i = lo; i < hi; i++)
                if (m[i] >= 0) { if (first < 0) first = m[i]; last = m[i]; }
            return first < 0 ? 0 : last - first + 1;
        };
        for (int x0 = 0; x0 < w; x0 += 64) nbx = std::max(nbx, span(bx, x0, std::min(w, x0 + 64)));
        for (int y0 = 0; y0 < h; y0 += th) nby = std::max(nby, span(by, y0, std::min(h, y0 + th)));
        if ((nbx + 1) * (nby + 1) <= (th_fixed > 272 ? 2 * SCORE_NBOX : SCORE_NBOX)) break;   // (th_fixed > 272: the wide matrix kernel's long segments)
        th = 0;
    }
    if (!th) return false;
    tall = th == direct_tile_rows(radius, true);
    if (th_fixed) {
        // blur_mfma_kernel's indicator matrix has five box columns per 16-px group of a tile
        for (int x0 = 0; x0 < w; x0 += 16) {
            int first = -1, last = -1;
            for (int x = x0; x < std::min(w, x0 + 16); x++)
                if (bx[x] >= 0) { if (first < 0) first = bx[x]; last = bx[x]; }
            if (first >= 0 && last - first > 4) return false;
        }
    }
    // a tile whose first column / row is in no box must not hold boxed pixels (kernel uses bx[x0])
    for (int x0 = 0; x0 < w; x0 += 64)
        if (bx[x0] < 0) for (int x = x0; x < std::min(w, x0 + 64); x++) if (bx[x] >= 0) return false;
    for (int y0 = 0; y0 < h; y0 += th)
        if (by[y0] < 0) for (int y = y0; y < std::min(h, y0 + th); y++) if (by[y] >= 0) return false;

    const int slabn = (nbx + 1) * (nby + 1);
    const int tiles_x = (w + 63) / 64, tiles = tiles_x * ((h + th - 1) / th);
    if (static_cast<size_t>(tiles) * 2 * slabn >= (1u << 30)) return false;   // 32-bit slab offsets
    for (int d = 0; d < dstW; d++) {
        int s0, s1;
        box_edge(d, xr, w, s0, s1);
        const int t0 = s0 >> 6, t1 = (s1 - 1) >> 6;
        if (t1 > t0 + 1) return false;
        xref[d].part0 = t0 * 2 * slabn + (d - bx[t0 << 6]);
        xref[d].part1 = t1 > t0 ? t1 * 2 * slabn + (d - bx[t1 << 6]) : -1;
        xref[d].len = s1 - s0; xref[d].pad = 0;
    }
    for (int d = 0; d < dstH; d++) {
        int s0, s1;
        box_edge(d, yr, h, s0, s1);
        const int t0 = s0 / th, t1 = (s1 - 1) / th;
        if (t1 > t0 + 1) return false;
        yref[d].part0 = t0 * tiles_x * 2 * slabn + (d - by[t0 * th]) * (nbx + 1);
        yref[d].part1 = t1 > t0 ? t1 * tiles_x * 2 * slabn + (d - by[t1 * th]) * (nbx + 1) : -1;
        yref[d].len = s1 - s0; yref[d].pad = 0;
    }

    g.th = th; g.nbx = nbx; g.nby = nby; g.tall = tall;
    g.coltab = g.rowtab = 0;
    if (th_fixed && th_fixed <= 272 && radius <= 6) score_mfma_tables(g, w, h);
    return true;
}

// ------------------------------------------------------------------------------------
// who decides the route
// ------------------------------------------------------------------------------------
// FNX_BLUR_EXACT takes the matrix kernels too (FNX_BLUR_MFMA_EXACT=0: blur.hip's guarded fp32 kernel, kept for A/B runs):
// 4K plain 18.7 us against 23.8, one-pass 26.4 against 29.2 per image
static bool plan_matrix(BlurPlan &p, int num_cus, int n, int w, int h, const double *kernel)
{
    static const bool off = [] { const char *e = dev_env("FNX_BLUR_MFMA"); return e && e[0] == '0'; }();
    static const bool exact_on = [] { const char *e = dev_env("FNX_BLUR_MFMA_EXACT"); return !(e && e[0] == '0'); }();
    static const int cap = [] { const char *e = dev_env("FNX_MFMA_SEG"); return e ? atoi(e) : MF_SEG; }();   // development: rows per workgroup
    if (off || (p.exact && !exact_on) || n > 65535 || w < 64 || h < 32 || !mfma_quantise(kernel, p.radius, &p.q, MF_RWIDE)) return false;
    // G (units of 2^-24): the fixed-point error bound, the reference's own fp64 chain error (13 roundings below 256:
    // < 4e-13 = 7e-6 units) and one unit for the bound's own arithmetic
    p.gq = p.exact ? static_cast<long long>(std::ceil(p.q.err255)) + 2 : 0;
    if (p.gq > (1 << 20)) return false;
    p.seed_h = static_cast<int>((1u << 23) + static_cast<uint32_t>(p.gq));                 // staged bytes come out as (value ^ 0x80)
    p.seed_v = static_cast<int>((1u << 23) + (1u << 31) + static_cast<uint32_t>(p.gq));    // plain bytes
    p.thr = static_cast<int>(2 * p.gq);
    if (p.radius <= MF_RMAX) {
        p.family = BLUR_MFMA;
        p.seg = blur_mfma_segment(num_cus, n, w, h, cap, p.exact ? 3 : 4);
    } else {                 // radius 7 .. 62: NKH chunks of 64 bytes in the H window, the V window in one, two or three
        p.family = BLUR_MFMA_WIDE;
        for (p.nkh = 2; p.radius > mf_wide_rf(p.nkh); p.nkh++) {}
        p.seg = blur_mfma_segment(num_cus, n, w, h, MF_SEG, 3);
    }
    return true;
}

BlurPlan plan_blur(int num_cus, int n, int w, int h, const double *kernel, int radius, bool exact)
{
    BlurPlan p;
    p.num_cus = num_cus; p.n = n; p.w = w; p.h = h; p.radius = radius;
    p.exact = exact;
    // non-negative weights under 0.49 that sum to 1, an image of 64 x 32 or more: both passes on the matrix pipe, fast or exact
    if (plan_matrix(p, num_cus, n, w, h, kernel)) return p;
    // what the matrix kernels leave (images under 64 x 32, radii past 62, a weight >= 0.49)
    if (radius < 1 || radius > FUSED_RMAX) {
        // An fp32 accumulator's rounding grows with the tap count -- tools/fuzz_blur.py, seed 71: 0.4 % of the samples one LSB off
        // at 127 taps, past the fast mode's 0.1 % -- so beyond 53 taps the fast mode takes the fp64 passes as well (the
        // reference's own arithmetic, 28 % slower)
        p.family = exact || radius > 26 ? BLUR_GENERIC_F64 : BLUR_GENERIC_F32;
    } else if (!exact || guard_kernel_ok(kernel, radius)) {
        p.family = BLUR_DIRECT;
        p.tall = direct_tall(num_cus, radius, n, w, h);
        p.wdp = exact && radius > SCORE_RMAX;
    } else {
        // any caller-supplied table the guarded kernel's bound does not cover takes the fp64 kernel, which is built for R <= 8
        p.family = radius > SCORE_RMAX ? BLUR_GENERIC_F64 : BLUR_EXACT;
    }
    return p;
}

const char *blur_route(const BlurPlan &p, bool score)
{
    static const char *const names[3][4] = {
        {"blur_mfma_kernel", "blur_mfma_kernel<GUARD>", "blur_mfma_kernel<SCORE>", "blur_mfma_kernel<SCORE, GUARD>"},
        {"blur_mfma_wide_kernel", "blur_mfma_wide_kernel<GUARD>", "blur_mfma_wide_kernel<SCORE>", "blur_mfma_wide_kernel<SCORE, GUARD>"},
        {"blur_direct_kernel", "blur_direct_kernel<GUARD>", "blur_direct_kernel<SCORE>", "blur_direct_kernel<SCORE, GUARD>"}};
    if (p.family <= BLUR_DIRECT) return names[p.family][(score ? 2 : 0) + (p.exact ? 1 : 0)];
    return p.family == BLUR_EXACT ? "blur_exact_kernel" : (p.family == BLUR_GENERIC_F64 ? "blur_pass_kernel<double> x 2" : "blur_pass_kernel<float> x 2");
}

bool plan_blur_scored(const BlurPlan &p, int dstW, int dstH, ScoreGeom &g)
{
    const int num_cus = p.num_cus, n = p.n, w = p.w, h = p.h;
    static const int wide_cap = [] { const char *e = dev_env("FNX_MFMA_WIDE_SEG"); return e ? atoi(e) : MF_SEG_SCORE_WIDE; }();   // development: rows per workgroup
    if (n > 65535) return false;   // grid.z
    // the family's SCORE form: the narrow matrix kernel's, the wide one's up to NKH = 4, the direct kernel's up to radius 8; a
    // matrix tile is 64 px x seg rows whatever the radius, the direct kernel's follows its tile shape
    int seg = 0;
    bool tall_pref = false;
    switch (p.family) {
    case BLUR_MFMA: seg = blur_mfma_segment(num_cus, n, w, h, MF_SEG_SCORE, 3); break;
    case BLUR_MFMA_WIDE:
        if (p.nkh > MF_SCORE_NKH) return false;
        seg = blur_mfma_segment(num_cus, n, w, h, wide_cap, 2);
        break;
    case BLUR_DIRECT:
        if (p.radius > SCORE_RMAX) return false;
        tall_pref = p.tall;
        break;
    default: return false;
    }
    const int radius = p.radius;
    if (!(g.w == w && g.h == h && g.dstW == dstW && g.dstH == dstH && g.radius == radius && g.tall_pref == tall_pref && g.seg == seg)) {
        g.w = w; g.h = h; g.dstW = dstW; g.dstH = dstH; g.radius = radius; g.tall_pref = tall_pref; g.seg = seg;
        // where GaussianBlur alone runs on the matrix pipe but its one-pass geometry does not fit (boxes under 4 px: long side
        // 1843..2047) there is no one-pass form: the direct kernel's fast-mode bytes are not the matrix kernels'
        // (tools/fuzz_blur.py: 72 such shapes in 6 528)
        g.mfma = seg > 0 && build_score_geom(g, w, h, radius, dstW, dstH, seg);
        g.ok = seg > 0 ? g.mfma : build_score_geom(g, w, h, radius, dstW, dstH);
    }
    return g.ok && g.th <= (p.family == BLUR_MFMA ? MF_SEG_SCORE : MF_SEG_SCORE_WIDE);
}

}  // namespace fnx
