// What png.Encoder{CompressionLevel: BestCompression} does to every row before zlib sees a byte (compress.go:94-107,
// targetsize.go:189, 342), on gfx950: pack the row, run the five PNG filters against the row above, keep the one with the
// smallest sum of |residual| -- the rule is stated in include/fennec_hip.h above fnx_png_filter.  Integers only.
//
//  * png_filter_kernel<MODE> (RGB: NRGBA with alpha dropped, bpp 3; RGBA: NRGBA as stored, bpp 4; GRAY: a byte plane,
//    bpp 1): a workgroup owns whole rows, rows b, b + G, ...  The row above is RAW data (never a filtered row), so rows are
//    independent; the neighbouring workgroup has just read it as its own row: expect it from L2.
//    Pass 1, per row: a lane takes units of four raw dwords (three for RGB: four pixels either way), forms the five
//    residuals four bytes at a time and adds their costs into five 32-bit sums (n <= 262 140 bytes of at most 128 each);
//    the sums go down the wave by shuffles, across the four waves through 20 words of LDS, and every lane reads the
//    totals and makes the same choice.  Integer sums are exact in any association: the bytes depend neither on the grid
//    nor on timing.  Pass 2 forms the chosen filter again (the row and the row above were read a moment ago: L1 / L2) and
//    stores it.  Keeping a row's residuals between the passes would take a row of registers or LDS per filter (a row is up to
//    256 KiB); reading twice from cache costs no HBM traffic.
//  * Packed bytes: a - b mod 256 per byte is the carry-free form sub8(); (a + b) >> 1 in 9 bits is avg8(); the cost
//    abs8(d) = min(d, 256 - d) of four residuals is ONE v_sad_u8: |(d ^ 0x80) - 0x80| per byte is |d as int8| with
//    abs8(128) = 128.  (It is a SAD against the constant, not of the filter's operands: |cur - pred| as integers is NOT
//    abs8((cur - pred) mod 256).)  Paeth's predictor compares three 9-bit distances per byte and is done a byte at a time.
//  * Stores: output rows are 1 + n bytes, so a row starts at every alignment.  A lane's unit is shifted by the row's
//    misalignment with v_alignbyte against the previous lane's last dword (one shuffle) and stored as aligned dwords; what
//    is left over -- the head of a wave's first unit, the tail of its last, a row's partial last unit, the type byte -- goes
//    out as byte stores.  No store touches a byte outside its row.
//  * png_pack_kernel<DEPTH>: the paletted form, filter type 0 and the indices as they are (8 bits) or packed MSB first
//    (4, 2, 1 bits; a row's last byte filled with zero bits), through the same store path.
//  * png_alpha_kernel: image.NRGBA.Opaque() -- visible pixels only -- for callers that do not state opacity.
//
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): no scratch in any kernel;
// VGPRs: png_filter_kernel RGB 49, RGBA 46, GRAY 52; png_pack_kernel 8-bit 26, 4-bit 21, 2-bit 29, 1-bit 45;
// png_alpha_kernel 17.  LDS: 160 bytes (png_filter_kernel), 256 (png_alpha_kernel's block-wide OR).  8 waves per SIMD.
//
//  * png_filter_batch_kernel<MODE>, png_pack_batch_kernel<DEPTH> (fnx_png_compress_batch): the same bodies (png_filter_rows.inc,
//    png_pack_rows.inc, included into both kernels) with a workgroup per unit {image, first row, end row} of any image of the
//    chunk that takes the form, the image's record read through the scalar cache.  No scratch; VGPRs: filter RGB 49, RGBA 46,
//    GRAY 50; pack 8-bit 26, 4-bit 22, 2-bit 30, 1-bit 46; LDS as the single kernels'.
#include "common.hpp"
#include "devutil.hpp"

#include <algorithm>
#include <cstddef>

namespace fnx {

constexpr int PF_T = 256;                // lanes per workgroup
constexpr uint32_t PF_H8 = 0x80808080u;

__host__ __device__ constexpr int pf_k(int mode) { return mode == PNG_ROW_RGB ? 3 : 4; }       // raw dwords per unit
__host__ __device__ constexpr int pf_bpp(int mode) { return mode == PNG_ROW_RGB ? 3 : (mode == PNG_ROW_RGBA ? 4 : 1); }

// four bytes at once: a - b mod 256, floor((a + b) / 2), and the running sum of abs8 over a dword of residuals
__device__ __forceinline__ uint32_t sub8(uint32_t a, uint32_t b) { return ((a | PF_H8) - (b & ~PF_H8)) ^ ((a ^ ~b) & PF_H8); }
__device__ __forceinline__ uint32_t avg8(uint32_t a, uint32_t b) { return (a & b) + (((a ^ b) & 0xfefefefeu) >> 1); }
__device__ __forceinline__ uint32_t cost8(uint32_t d, uint32_t acc) { return __builtin_amdgcn_sad_u8(d ^ PF_H8, PF_H8, acc); }

// Paeth's predictor of four bytes: a left, b above, c above-left
__device__ __forceinline__ uint32_t paeth8(uint32_t a4, uint32_t b4, uint32_t c4)
{
    uint32_t r = 0;
#pragma unroll
    for (int k = 0; k < 32; k += 8) {
        const int a = (a4 >> k) & 0xff, b = (b4 >> k) & 0xff, c = (c4 >> k) & 0xff;
        const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
        const int p = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
        r |= static_cast<uint32_t>(p) << k;
    }
    return r;
}

// the dword of left neighbours of raw dword `cur`: raw bytes 4j - bpp .. 4j - bpp + 3, `before` being raw dword j - 1
template <int BPP>
__device__ __forceinline__ uint32_t left_of(uint32_t before, uint32_t cur)
{
    return BPP == 4 ? before : __builtin_amdgcn_alignbyte(cur, before, 4 - BPP);
}

// Unit u of a row as raw dwords: R[1 .. K] the unit (zeros behind the row's end), R[0] the raw dword in front of it (only its
// top bpp bytes are used; zero for u == 0).  Returns the unit's raw bytes inside the row.  al4: row 4-byte aligned.
template <int MODE>
__device__ __forceinline__ int pf_load(const uint8_t *row, uint32_t u, int w, bool al4, uint32_t R[5])
{
    if (MODE == PNG_ROW_GRAY) {
        const int x0 = 16 * static_cast<int>(u), cnt = min(16, w - x0);
        if (al4 && cnt == 16) {
            const u32x4 q = *(g_u32x4 *)(row + x0);
            R[1] = q.x; R[2] = q.y; R[3] = q.z; R[4] = q.w;
            R[0] = u ? *(g_u32 *)(row + x0 - 4) : 0u;
        } else {
            R[0] = u ? static_cast<uint32_t>(row[x0 - 1]) << 24 : 0u;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    if (4 * j + k < cnt) v |= static_cast<uint32_t>(row[x0 + 4 * j + k]) << (8 * k);
                }
                R[1 + j] = v;
            }
        }
        return cnt;
    }
    const int x0 = 4 * static_cast<int>(u), cnt = min(4, w - x0);
    uint32_t p[5];
    p[0] = u ? ld_px(row, x0 - 1) : 0u;
    if (cnt == 4) {
        const u32x4 q = *(g_u32x4 *)(row + 4 * static_cast<size_t>(x0));
        p[1] = q.x; p[2] = q.y; p[3] = q.z; p[4] = q.w;
    } else {
#pragma unroll
        for (int e = 0; e < 4; e++) p[1 + e] = e < cnt ? ld_px(row, x0 + e) : 0u;
    }
    if (MODE == PNG_ROW_RGBA) {
#pragma unroll
        for (int e = 0; e < 5; e++) R[e] = p[e];
        return 4 * cnt;
    }
    R[0] = p[0] << 8;                                                // r, g, b of the pixel in front: raw bytes -3 .. -1
    R[1] = (p[1] & 0xffffffu) | (p[2] << 24);
    R[2] = ((p[2] >> 8) & 0xffffu) | (p[3] << 16);
    R[3] = ((p[3] >> 16) & 0xffu) | (p[4] << 8);
    R[4] = 0;
    return 3 * cnt;
}

// Store a wave's units of K dwords: lane `lane` holds raw bytes i0 .. i0 + nvalid of the row whose raw byte 0 lives at
// `raw0` (any alignment).  Every lane of the wave calls it (the shuffle); only `active` ones store.  next_full: the unit
// behind this one exists and is a full one, so its lane stores this unit's last (raw0 & 3) bytes with its first dword.
template <int K>
__device__ __forceinline__ void pf_store(uint8_t *raw0, uint32_t i0, const uint32_t D[K], int nvalid, bool active, bool next_full, int lane)
{
    const uint32_t before = __shfl_up(D[K - 1], 1, 64);
    if (!active) return;
    uint8_t *a0 = raw0 + i0;
    if (nvalid < 4 * K) {                                            // a row's partial last unit
#pragma unroll
        for (int k = 0; k < 4 * K; k++) {
            if (k < nvalid) a0[k] = static_cast<uint8_t>(D[k >> 2] >> (8 * (k & 3)));
        }
        return;
    }
    const int s = static_cast<int>(reinterpret_cast<uintptr_t>(raw0) & 3u);   // i0 is a multiple of 4
    if (s == 0) {
#pragma unroll
        for (int j = 0; j < K; j++) *(g_u32w *)(a0 + 4 * j) = D[j];
        return;
    }
    // the aligned dword at a0 - s: s bytes of the unit in front, 4 - s bytes of this one
    if (lane > 0) {
        *(g_u32w *)(a0 - s) = __builtin_amdgcn_alignbyte(D[0], before, 4 - s);
    } else {
        for (int k = 0; k < 4 - s; k++) a0[k] = static_cast<uint8_t>(D[0] >> (8 * k));
    }
#pragma unroll
    for (int j = 1; j < K; j++) *(g_u32w *)(a0 - s + 4 * j) = __builtin_amdgcn_alignbyte(D[j], D[j - 1], 4 - s);
    if (lane == 63 || !next_full) {
        for (int k = 4 - s; k < 4; k++) a0[4 * (K - 1) + k] = static_cast<uint8_t>(D[K - 1] >> (8 * k));
    }
}

struct PngFilterArgs {
    const uint8_t *src;
    int sstride, w, h;
    int n;                               // raw bytes per row
    int al4;                             // src and sstride are multiples of 4 (always, for NRGBA)
    uint8_t *out;                        // h rows of 1 + n bytes
};

template <int MODE>
__global__ __launch_bounds__(PF_T) void png_filter_kernel(PngFilterArgs a)
{
#define PF_FIRST_ROW blockIdx.x
#define PF_ROW_STEP gridDim.x
#include "png_filter_rows.inc"
#undef PF_FIRST_ROW
#undef PF_ROW_STEP
}

// The compress batch: a workgroup per unit -- rows [first, end) of one image of the chunk whose rows take this form.  The unit
// and the image's record come through the scalar cache; the rows are the single kernel's rows (a row's bytes depend on the row
// and the one above alone).
template <int MODE>
__global__ __launch_bounds__(PF_T) void png_filter_batch_kernel(const PngCbUnit *__restrict__ work, const PngFilterArgs *__restrict__ images)
{
    const PngCbUnit u = work[blockIdx.x];
    PngFilterArgs a = images[u.image];
    a.h = static_cast<int>(u.end);                                   // the rows below it are other units'
#define PF_FIRST_ROW static_cast<int>(u.first)
#define PF_ROW_STEP 1
#include "png_filter_rows.inc"
#undef PF_FIRST_ROW
#undef PF_ROW_STEP
}

struct PngPackArgs {
    const uint8_t *src;                  // the index plane
    int sstride, w, h;
    int n;
    int al4;
    uint8_t *out;
};

template <int DEPTH>
__global__ __launch_bounds__(PF_T) void png_pack_kernel(PngPackArgs a)
{
#define PF_FIRST_ROW blockIdx.x
#define PF_ROW_STEP gridDim.x
#include "png_pack_rows.inc"
#undef PF_FIRST_ROW
#undef PF_ROW_STEP
}

template <int DEPTH>
__global__ __launch_bounds__(PF_T) void png_pack_batch_kernel(const PngCbUnit *__restrict__ work, const PngPackArgs *__restrict__ images)
{
    const PngCbUnit u = work[blockIdx.x];
    PngPackArgs a = images[u.image];
    a.h = static_cast<int>(u.end);
#define PF_FIRST_ROW static_cast<int>(u.first)
#define PF_ROW_STEP 1
#include "png_pack_rows.inc"
#undef PF_FIRST_ROW
#undef PF_ROW_STEP
}

// image.NRGBA.Opaque(): *flag (zero before the launch) becomes 1 when a VISIBLE pixel has alpha != 255
__global__ __launch_bounds__(PF_T) void png_alpha_kernel(const uint8_t *src, int sstride, int w, int h, uint32_t *flag)
{
    uint32_t all = 0xff000000u;
    for (int y = blockIdx.x; y < h; y += gridDim.x) {
        const uint8_t *row = src + static_cast<size_t>(y) * sstride;
        for (int x = threadIdx.x; x < w; x += PF_T) all &= ld_px(row, x);
    }
    const int translucent = __syncthreads_or((all >> 24) != 0xffu ? 1 : 0);
    if (translucent && threadIdx.x == 0) *flag = 1u;                 // every writer stores the same word
}

namespace {

int pf_grid(const fnx_ctx *ctx, int h) { return std::max(1, std::min(h, 8 * ctx->num_cus)); }

int pf_al4(const uint8_t *src, int sstride) { return ((reinterpret_cast<uintptr_t>(src) | static_cast<uintptr_t>(sstride)) & 3u) == 0 ? 1 : 0; }

}  // namespace

int png_row_bytes(int form, int w, int depth)
{
    if (form == PNG_ROW_RGB) return 3 * w;
    if (form == PNG_ROW_RGBA) return 4 * w;
    if (form == PNG_ROW_GRAY) return w;
    return static_cast<int>((static_cast<long long>(w) * depth + 7) / 8);
}

int launch_png_alpha(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, uint32_t *d_flag)
{
    FNX_HIP(hipMemsetAsync(d_flag, 0, sizeof(uint32_t), ctx->stream));
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(png_alpha_kernel, dim3(pf_grid(ctx, h)), dim3(PF_T), 0, ctx->stream, src, sstride, w, h, d_flag);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    return FNX_OK;
}

int launch_png_filter(fnx_ctx *ctx, int form, const uint8_t *src, int sstride, int w, int h, int depth, uint8_t *d_out)
{
    const dim3 grid(pf_grid(ctx, h)), block(PF_T);
    if (form == PNG_ROW_PALETTED) {
        PngPackArgs pa{};
        pa.src = src; pa.sstride = sstride; pa.w = w; pa.h = h; pa.n = png_row_bytes(form, w, depth);
        pa.al4 = pf_al4(src, sstride); pa.out = d_out;
        note_route(ctx, FNX_PROF_MAIN, "png_pack_kernel");
        FNX_TRY(prof_begin(ctx));
        switch (depth) {
        case 8: hipLaunchKernelGGL(png_pack_kernel<8>, grid, block, 0, ctx->stream, pa); break;
        case 4: hipLaunchKernelGGL(png_pack_kernel<4>, grid, block, 0, ctx->stream, pa); break;
        case 2: hipLaunchKernelGGL(png_pack_kernel<2>, grid, block, 0, ctx->stream, pa); break;
        default: hipLaunchKernelGGL(png_pack_kernel<1>, grid, block, 0, ctx->stream, pa); break;
        }
        FNX_HIP(hipGetLastError());
        FNX_TRY(prof_end(ctx));
        return FNX_OK;
    }
    PngFilterArgs fa{};
    fa.src = src; fa.sstride = sstride; fa.w = w; fa.h = h; fa.n = png_row_bytes(form, w, 8);
    fa.al4 = pf_al4(src, sstride); fa.out = d_out;
    note_route(ctx, FNX_PROF_MAIN, "png_filter_kernel");
    FNX_TRY(prof_begin(ctx));
    switch (form) {
    case PNG_ROW_RGB: hipLaunchKernelGGL(png_filter_kernel<PNG_ROW_RGB>, grid, block, 0, ctx->stream, fa); break;
    case PNG_ROW_RGBA: hipLaunchKernelGGL(png_filter_kernel<PNG_ROW_RGBA>, grid, block, 0, ctx->stream, fa); break;
    default: hipLaunchKernelGGL(png_filter_kernel<PNG_ROW_GRAY>, grid, block, 0, ctx->stream, fa); break;
    }
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    return FNX_OK;
}

// The row stage of a chunk of the compress batch: per form present one launch over that form's units.  d_units: the units of
// forms 0, 1, ... back to back (nunits[k] of form k); d_rows: m records (DEVICE; a record is PngFilterArgs and PngPackArgs alike).
#define PF_SAME_FIELD(f) \
    static_assert(offsetof(PngCbRows, f) == offsetof(PngFilterArgs, f) && offsetof(PngCbRows, f) == offsetof(PngPackArgs, f) && \
                  sizeof(PngCbRows::f) == sizeof(PngFilterArgs::f) && sizeof(PngCbRows::f) == sizeof(PngPackArgs::f), "one record for both kernels: " #f)
PF_SAME_FIELD(src);
PF_SAME_FIELD(sstride);
PF_SAME_FIELD(w);
PF_SAME_FIELD(h);
PF_SAME_FIELD(n);
PF_SAME_FIELD(al4);
PF_SAME_FIELD(out);
#undef PF_SAME_FIELD
static_assert(sizeof(PngCbRows) == sizeof(PngFilterArgs) && sizeof(PngCbRows) == sizeof(PngPackArgs), "one record for both kernels");

int png_cb_al4(const uint8_t *src, int sstride) { return pf_al4(src, sstride); }

int launch_png_rows_batch(fnx_ctx *ctx, const PngCbUnit *d_units, const int nunits[PNG_CB_FORMS], const PngCbRows *d_rows)
{
    const dim3 block(PF_T);
    const PngCbUnit *u = d_units;
    const PngFilterArgs *fa = reinterpret_cast<const PngFilterArgs *>(d_rows);
    const PngPackArgs *pa = reinterpret_cast<const PngPackArgs *>(d_rows);
    for (int k = 0; k < PNG_CB_FORMS; k++) {
        if (nunits[k] == 0) continue;
        const dim3 grid(nunits[k]);
        FNX_TRY(prof_begin(ctx));
        switch (k) {
        case PNG_CB_RGB: hipLaunchKernelGGL(png_filter_batch_kernel<PNG_ROW_RGB>, grid, block, 0, ctx->stream, u, fa); break;
        case PNG_CB_RGBA: hipLaunchKernelGGL(png_filter_batch_kernel<PNG_ROW_RGBA>, grid, block, 0, ctx->stream, u, fa); break;
        case PNG_CB_GRAY: hipLaunchKernelGGL(png_filter_batch_kernel<PNG_ROW_GRAY>, grid, block, 0, ctx->stream, u, fa); break;
        case PNG_CB_PACK8: hipLaunchKernelGGL(png_pack_batch_kernel<8>, grid, block, 0, ctx->stream, u, pa); break;
        case PNG_CB_PACK4: hipLaunchKernelGGL(png_pack_batch_kernel<4>, grid, block, 0, ctx->stream, u, pa); break;
        case PNG_CB_PACK2: hipLaunchKernelGGL(png_pack_batch_kernel<2>, grid, block, 0, ctx->stream, u, pa); break;
        default: hipLaunchKernelGGL(png_pack_batch_kernel<1>, grid, block, 0, ctx->stream, u, pa); break;
        }
        FNX_HIP(hipGetLastError());
        FNX_TRY(prof_end(ctx));
        u += nunits[k];
    }
    return FNX_OK;
}

}  // namespace fnx
