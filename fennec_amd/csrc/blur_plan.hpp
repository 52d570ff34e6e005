// The host plan of GaussianBlur's launches (blur_plan.cpp): which kernel family a call gets, with which weights, guard values
// and rows per workgroup, and -- for the one-pass blur + SSIMFast form -- that family's box geometry or none.  Pure functions of
// their arguments in plain C++ -- no HIP call, no ctx --, so that the file builds alone (tools/blur_plan_host.cpp runs it under
// the sanitizers).  blur.hip and blur_mfma.hip launch what a plan says and decide nothing themselves.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace fnx {

// ---- the shapes the kernels are built for (blur_mfma.hip, blur.hip) ----
constexpr int MF_RMAX = 6;           // 4 output px + 2 R <= 16 px = the 64-byte K of one H instruction
constexpr int MF_RWIDE = 62;         // blur_mfma_wide_kernel: 16 + 2 R <= the 64 NKV rows of its V window (NKH = 8: RF = 62)
constexpr int MF_SEG_SCORE = 272;    // most rows per workgroup with SCORE (row tables and box tables in LDS)
constexpr int MF_SEG_SCORE_WIDE = 544;   // ... of blur_mfma_wide_kernel<2, ., SCORE>: two workgroups per CU either way (its ring and stages are 43 KB)
constexpr int MF_SEG = 544;          // ... of a plain launch, narrow or wide
// blur_mfma_wide_kernel<NKH>: 64-row chunks of the V window, and the frame radius the taps sit centred in (14, 22, 24, 38, 46,
// 54, 62 for NKH = 2 .. 8)
constexpr int mf_wide_nkv(int nkh) { return nkh <= 4 ? 1 : (nkh <= 7 ? 2 : 3); }
constexpr int mf_wide_rf(int nkh) { return 8 * nkh - 2 < 32 * mf_wide_nkv(nkh) - 8 ? 8 * nkh - 2 : 32 * mf_wide_nkv(nkh) - 8; }
constexpr int MF_SCORE_NKH = 4;      // the wide kernel's one-pass form: NKH = 2 .. 4 (radius <= 24)
constexpr int FUSED_RMAX = 16;    // radius <= 16 (sigma <= 5.33): the tile kernel; r3: 9..16 added (the H window streams through, see WIDE)
constexpr int SCORE_RMAX = 8;     // the one-pass GaussianBlur + SSIMFast form and the 128-lane tile stop here
constexpr int WIDE_IH = 128;      // staged rows of the R > 8 tile (256 lanes): TH = the multiple of 8 below 128 - 2R
// most entries of a per-tile box table, (nbx+1) * (nby+1): the two tables live in dynamic LDS sized
// per launch (4K: 2 x 176 x 8 B = 2.8 KB); the cap keeps the kernel at >= 3 workgroups per CU
constexpr int SCORE_NBOX = 512;
constexpr int NHEAD = 260 + 257 * 8;   // uint32 words at the head of the table blob: magic[c] (c <= 256, padded to 260), tiedown[8 c + w]
struct BoxRef {           // where one output column (or row) finds its partial sums
    int32_t part0, part1; // slab offsets of the (at most two) tiles the box spans; part1 < 0: one tile
    int32_t len, pad;     // box width (height) in source px
};

// ---- the matrix kernels' weights ----
// Fixed-point form of a blur kernel: wq[k] = round(w[k] 2^24), the centre takes what is left of 2^24.
struct MfmaWeights {
    long long wq[2 * MF_RWIDE + 1];
    double err255;                // 255 * max(sum of the positive, sum of the negative wq[k] - w[k] 2^24): bound of |S - exact sum * 2^24|
};
// false: the table is outside what the three-digit form or the error bound covers
bool mfma_quantise(const double *kernel, int radius, MfmaWeights *q, int rmax = MF_RMAX);
// blur_mfma_kernel's table: BH[3][64] x 16 bytes (digits hi, mid, lo) | BV[3][64] x 8 | 13 fp64 weights, centred, padded to 16
// with zeros (mf_exact_u's two s_load_dwordx16)
constexpr size_t MF_TAB_WORDS = 3 * 64 * 4 + 3 * 64 * 2;
constexpr size_t MF_TAB_ALL = MF_TAB_WORDS + 2 * 16;
// blur_mfma_wide_kernel<NKH>'s: BH[NKH][3][64] x 16 bytes | BV[NKV][3][64] x 16 bytes | 2 RF + 1 fp64 weights, centred (padded to
// whole s_load_dwordx16's)
constexpr size_t mf_wide_tab_words(int nkh) { return (3 * nkh + 3 * mf_wide_nkv(nkh)) * 64 * 4; }
constexpr size_t mf_wide_tab_all(int nkh) { return mf_wide_tab_words(nkh) + 2 * ((2 * mf_wide_rf(nkh) + 1 + 7) / 8 * 8); }

// ---- the plan of one call ----
enum BlurFamily {
    BLUR_MFMA = 0,       // blur_mfma_kernel
    BLUR_MFMA_WIDE,      // blur_mfma_wide_kernel<nkh>
    BLUR_DIRECT,         // blur_direct_kernel<radius>: the 256-lane tile when `tall`, GUARD when `exact`
    BLUR_EXACT,          // blur_exact_kernel<radius>
    BLUR_GENERIC_F32,    // blur_pass_kernel<float> x 2
    BLUR_GENERIC_F64     // blur_pass_kernel<double> x 2
};
struct BlurPlan {
    BlurFamily family = BLUR_GENERIC_F64;
    int num_cus = 0, n = 0, w = 0, h = 0, radius = 0;   // the call
    bool exact = false;         // FNX_BLUR_EXACT: the matrix and direct kernels run their GUARD form
    int nkh = 0;                // BLUR_MFMA_WIDE
    bool tall = false;          // BLUR_DIRECT
    bool wdp = false;           // BLUR_DIRECT: the fp64 weights go to a device table (GUARD, radius > 8)
    int seg = 0;                // matrix kernels: output rows per workgroup (a multiple of 16)
    MfmaWeights q = {};         // matrix kernels
    long long gq = 0;           // ... the guard distance G in units of 2^-24 (0: fast mode)
    int seed_h = 0, seed_v = 0, thr = 0;   // ... rounding seeds (+ G), 2 G
};

// Cached geometry of the one-pass blur + SSIMFast launch (plan_blur_scored)
struct ScoreGeom {
    int w = 0, h = 0, dstW = 0, dstH = 0, radius = 0;
    bool tall_pref = false, tall = false, ok = false;
    bool mfma = false;          // the geometry is a matrix kernel's (tile = 64 px x seg rows)
    int seg = 0;
    int th = 0, nbx = 0, nby = 0;
    std::vector<int32_t> map;   // the table blob uploaded to SLOT_BOXMAP
    // blur_mfma_kernel<SCORE, .>'s set-up tables at the blob's end (word offsets, 0: none): one packed word per
    // (tile column, wave, lane); per segment the table offsets of its seg + 16 staged rows, then of its seg output rows
    size_t coltab = 0, rowtab = 0;
};

// what GaussianBlur of n w x h images with this table launches (w, h, n > 0)
BlurPlan plan_blur(int num_cus, int n, int w, int h, const double *kernel, int radius, bool exact);
// The one-pass form of plan `p` with dstW x dstH box planes: false when there is none (the caller runs the two ops back to
// back), else g holds the geometry, the form's rows per workgroup (g.th) and tile shape (g.tall) included.  It starts from p.family
// and has no other kernel to offer, so the one-pass images are the plain call's by construction.  g is the ctx's cache: rebuilt
// only when its key changes.
bool plan_blur_scored(const BlurPlan &p, int dstW, int dstH, ScoreGeom &g);
// the name of the plan's kernel as note_route gets it (score: of its one-pass form)
const char *blur_route(const BlurPlan &p, bool score);
// the matrix kernels' device table of a plan (SLOT_TABLE_MFMA): the digit matrices and the caller's fp64 weights
std::vector<uint32_t> mfma_table(const BlurPlan &p, const double *kernel);

}  // namespace fnx
