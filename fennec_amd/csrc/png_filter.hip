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
#include "common.hpp"
#include "devutil.hpp"

#include <algorithm>

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
    constexpr int K = pf_k(MODE), BPP = pf_bpp(MODE);
    __shared__ uint32_t s_sum[2][PF_T / 64][5];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t n = static_cast<uint32_t>(a.n);
    const uint32_t units = (n + 4 * K - 1) / (4 * K);
    const bool al4 = a.al4 != 0;
    int parity = 0;
    for (int y = blockIdx.x; y < a.h; y += gridDim.x, parity ^= 1) {
        const uint8_t *cur = a.src + static_cast<size_t>(y) * a.sstride;
        const uint8_t *prev = cur - a.sstride;                       // read for y > 0 only
        // ---- pass 1: the five sums, in the order of the type numbers: None, Sub, Up, Average, Paeth
        uint32_t sum[5] = {0, 0, 0, 0, 0};
        for (uint32_t u = tid; u < units; u += PF_T) {
            uint32_t C[5], P[5] = {0, 0, 0, 0, 0};
            const int nvalid = pf_load<MODE>(cur, u, a.w, al4, C);
            if (y > 0) pf_load<MODE>(prev, u, a.w, al4, P);
#pragma unroll
            for (int j = 0; j < K; j++) {
                // a residual behind the row's end is not part of the sum (Sub, Average and Paeth see a left neighbour there)
                const int v = nvalid - 4 * j;
                const uint32_t m = v >= 4 ? 0xffffffffu : (v <= 0 ? 0u : (1u << (8 * v)) - 1u);
                const uint32_t c = C[1 + j], up = P[1 + j];
                const uint32_t l = left_of<BPP>(C[j], c), ul = left_of<BPP>(P[j], up);
                sum[0] = cost8(c, sum[0]);
                sum[1] = cost8(sub8(c, l) & m, sum[1]);
                sum[2] = cost8(sub8(c, up), sum[2]);
                sum[3] = cost8(sub8(c, avg8(l, up)) & m, sum[3]);
                sum[4] = cost8(sub8(c, paeth8(l, up, ul)) & m, sum[4]);
            }
        }
#pragma unroll
        for (int f = 0; f < 5; f++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum[f] += __shfl_xor(sum[f], off, 64);
        }
        // two sets of words, by the parity of the workgroup's row count: a wave can be at most one barrier ahead of another
        if (lane == 0) {
#pragma unroll
            for (int f = 0; f < 5; f++) s_sum[parity][wave][f] = sum[f];
        }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < 5; f++) sum[f] = s_sum[parity][0][f] + s_sum[parity][1][f] + s_sum[parity][2][f] + s_sum[parity][3][f];
        // tried in the order Up, Paeth, None, Sub, Average; a later one wins only when strictly smaller
        int ft = 2;
        uint32_t best = sum[2];
        if (sum[4] < best) { best = sum[4]; ft = 4; }
        if (sum[0] < best) { best = sum[0]; ft = 0; }
        if (sum[1] < best) { best = sum[1]; ft = 1; }
        if (sum[3] < best) { best = sum[3]; ft = 3; }

        // ---- pass 2: the chosen filter, stored
        uint8_t *orow = a.out + static_cast<size_t>(y) * (static_cast<size_t>(n) + 1);
        if (tid == 0) orow[0] = static_cast<uint8_t>(ft);
        const bool need_prev = ft >= 2 && y > 0;
        for (uint32_t base = wave * 64; base < units; base += PF_T) {
            const uint32_t u = base + lane;
            const bool active = u < units;
            uint32_t C[5] = {0, 0, 0, 0, 0}, P[5] = {0, 0, 0, 0, 0}, D[K];
            int nvalid = 0;
            if (active) {
                nvalid = pf_load<MODE>(cur, u, a.w, al4, C);
                if (need_prev) pf_load<MODE>(prev, u, a.w, al4, P);
            }
#pragma unroll
            for (int j = 0; j < K; j++) {
                const uint32_t c = C[1 + j], up = P[1 + j];
                const uint32_t l = left_of<BPP>(C[j], c), ul = left_of<BPP>(P[j], up);
                uint32_t d = c;
                if (ft == 1) d = sub8(c, l);
                else if (ft == 2) d = sub8(c, up);
                else if (ft == 3) d = sub8(c, avg8(l, up));
                else if (ft == 4) d = sub8(c, paeth8(l, up, ul));
                D[j] = d;
            }
            const uint32_t i0 = 4u * K * u;
            pf_store<K>(orow + 1, i0, D, nvalid, active, i0 + 8u * K <= n, lane);
        }
    }
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
    constexpr int K = DEPTH == 8 ? 4 : 1, PPB = 8 / DEPTH;           // raw dwords per unit, pixels per raw byte
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t n = static_cast<uint32_t>(a.n);
    const uint32_t units = (n + 4 * K - 1) / (4 * K);
    for (int y = blockIdx.x; y < a.h; y += gridDim.x) {
        const uint8_t *row = a.src + static_cast<size_t>(y) * a.sstride;
        uint8_t *orow = a.out + static_cast<size_t>(y) * (static_cast<size_t>(n) + 1);
        if (tid == 0) orow[0] = 0;                                   // paletted rows are never filtered
        for (uint32_t base = wave * 64; base < units; base += PF_T) {
            const uint32_t u = base + lane;
            const bool active = u < units;
            uint32_t D[K];
            int nvalid = 0;
            if (DEPTH == 8) {
                uint32_t R[5] = {0, 0, 0, 0, 0};
                if (active) nvalid = pf_load<PNG_ROW_GRAY>(row, u, a.w, a.al4 != 0, R);
#pragma unroll
                for (int j = 0; j < K; j++) D[j] = R[1 + j];
            } else {
                D[0] = 0;
                if (active) {
                    nvalid = min(4, static_cast<int>(n - 4u * u));
                    const int x0 = 4 * PPB * static_cast<int>(u);    // 4 raw bytes of PPB pixels each
                    if (a.al4 && x0 + 4 * PPB <= a.w) {
#pragma unroll
                        for (int q = 0; q < PPB; q++) {              // source dword q: pixels 4q .. 4q + 3, raw byte 4q / PPB
                            const uint32_t v = *(g_u32 *)(row + x0 + 4 * q);
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                const int px = 4 * q + e, k = px / PPB, slot = PPB - 1 - px % PPB;
                                D[0] |= (((v >> (8 * e)) & 0xffu) << (DEPTH * slot) & 0xffu) << (8 * k);
                            }
                        }
                    } else {
#pragma unroll
                        for (int px = 0; px < 4 * PPB; px++) {
                            const int k = px / PPB, slot = PPB - 1 - px % PPB;
                            const uint32_t v = x0 + px < a.w ? row[x0 + px] : 0u;
                            D[0] |= ((v << (DEPTH * slot)) & 0xffu) << (8 * k);
                        }
                    }
                }
            }
            const uint32_t i0 = 4u * K * u;
            pf_store<K>(orow + 1, i0, D, nvalid, active, i0 + 8u * K <= n, lane);
        }
    }
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

}  // namespace fnx
