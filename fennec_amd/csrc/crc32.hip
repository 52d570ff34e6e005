// CRC-32 (ISO 3309 / PNG / zlib: reflected polynomial 0xedb88320, register from all ones, inverted at the end) of bytes that
// are already on the device -- the gathered zlib stream of deflate.hip above all, whose IDAT chunk's CRC was the last pass
// over the stream the host made (fnx_ctx_set_png_crc), and any resident or uploaded bytes through fnx_crc32.  The lane and
// workgroup bodies, with the arithmetic they rest on, are crc32_piece.inc (tools/crc32_hostsim runs the same text on the CPU).
//
// crc32_pieces_kernel: one workgroup of 256 lanes per piece of FNX_CRC_PIECE = 16 KiB, a lane a run of FNX_CRC_RUN = 64 bytes:
//  slice-by-4 from four 256-word tables the workgroup builds in LDS (8 shift steps a lane, then three look-ups), aligned dwords
//  in the middle of a run, single bytes at a misaligned head or tail; the 256 remainders folded in eight log-steps, each one
//  32-step GF(2) multiplication by the constant x^(8 RUN 2^k); a short piece stands at the end of its runs (crc32_piece.inc), so
//  no step needs another factor.  One word R(piece) per piece.  The length is an argument, or -- the PNG routes, where the host
//  does not know it when it enqueues -- the word deflate_gather_kernel wrote, read on the device and held to the grid's bytes
//  (fnx_deflate_bound); a workgroup whose piece lies wholly behind the stream's end writes a zero word and leaves.  Nothing
//  outside [src, src + length) is read.
// crc32_fold_kernel: one workgroup per stream: a lane shifts piece j's word by the bytes behind piece j (square-and-multiply
//  over x^(8 2^k), k = 0..31), one lane the seed register by the stream's length; the workgroup xors the terms and writes the
//  inverted result as one word.
// crc32_pieces_batch_kernel, crc32_fold_batch_kernel (fnx_png_compress_batch): the same bodies over the streams
//  deflate_gather_batch_kernel laid back to back: a unit {stream, piece} per 16 KiB of a stream's BOUND, the stream's start the
//  sum of the size words in front of it and its length its own size word, both read on the device (each held to its bound, so
//  every read stays inside the area of the bounds' sum).
// No workgroup waits for another: no flags, no spinning, no atomics on global memory; the result is a function of the bytes.
//
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): no scratch in any kernel;
//   crc32_pieces_kernel and crc32_pieces_batch_kernel 37 VGPRs, crc32_fold_kernel and crc32_fold_batch_kernel 12;
//   LDS 5120 bytes (the four tables, the 256 words of the fold), the batched pieces kernel 5152 (its prefix sum's 4 words).
// The table-free form (a carry-less multiplication a dword) was not measured: DESIGN.md section 5.17.
#include "common.hpp"
#include "devutil.hpp"

#include <algorithm>

namespace fnx {

#define CRC_FN __device__ __forceinline__
#define CRC_CONST __device__ const
#define CRC_UNROLL _Pragma("unroll")
#define CRC_LD32(p) (*(g_u32 *)(p))
#define CRC_PHASE(call) { call; } __syncthreads();
#define CRC_RUN_PARAMS , CrcLane &ln, const int lane
#include "crc32_piece.inc"
#undef CRC_RUN_PARAMS
#undef CRC_PHASE
#undef CRC_LD32
#undef CRC_UNROLL
#undef CRC_CONST
#undef CRC_FN

struct CrcArgs {
    const uint8_t *src;
    unsigned long long n_max;            // the bytes the grid covers
    const unsigned long long *d_n;       // the length, at most n_max; nullptr: n_max
    uint32_t *words;                     // R(piece) per piece of the grid
    uint32_t seed;                       // the register the stream starts from
    uint32_t *crc;
};

__device__ __forceinline__ unsigned long long crc_length(const CrcArgs &a)
{
    if (!a.d_n) return a.n_max;
    const unsigned long long n = *a.d_n;
    return n < a.n_max ? n : a.n_max;
}

__global__ __launch_bounds__(CRC_LANES) void crc32_pieces_kernel(CrcArgs a)
{
    __shared__ CrcShared s;
    const int lane = threadIdx.x;
    const unsigned long long n = crc_length(a), off = static_cast<unsigned long long>(blockIdx.x) * CRC_PIECE;
    if (off >= n) {
        if (lane == 0) a.words[blockIdx.x] = 0;
        return;
    }
    const uint32_t plen = static_cast<uint32_t>(n - off < CRC_PIECE ? n - off : CRC_PIECE);
    CrcLane ln{0};
    const uint32_t r = crc_piece(a.src + off, plen, s, ln, lane);
    if (lane == 0) a.words[blockIdx.x] = r;
}

__global__ __launch_bounds__(CRC_LANES) void crc32_fold_kernel(CrcArgs a)
{
    __shared__ CrcShared s;
    const int lane = threadIdx.x;
    CrcLane ln{0};
    const uint32_t crc = crc_stream(a.words, crc_length(a), a.seed, s, ln, lane);
    if (lane == 0) *a.crc = crc;
}

// ---- the streams of a compress batch ----
struct CrcBatchUnit {
    uint32_t image, piece;
};
struct CrcBatchImage {
    unsigned long long bound;            // deflate_bound of the stream: what its size word is held to
    uint32_t word0, npieces;             // its pieces' words: [word0, word0 + npieces), npieces = the bound's
};
struct CrcBatchArgs {
    const CrcBatchUnit *units;
    const CrcBatchImage *images;
    const uint8_t *out;                  // the streams back to back at their true sizes (deflate_gather_batch_kernel)
    const unsigned long long *sizes;     // per stream
    uint32_t *words;
    uint32_t seed;
    uint32_t *crcs;                      // per stream
};

__device__ __forceinline__ unsigned long long crc_batch_size(const CrcBatchArgs &a, uint32_t i)
{
    const unsigned long long n = a.sizes[i], b = a.images[i].bound;
    return n < b ? n : b;
}

__global__ __launch_bounds__(CRC_LANES) void crc32_pieces_batch_kernel(CrcBatchArgs a)
{
    __shared__ CrcShared s;
    __shared__ unsigned long long s_sum[4];
    const int lane = threadIdx.x;
    const CrcBatchUnit u = a.units[blockIdx.x];
    unsigned long long start = 0;                                    // the sizes in front of the stream
    for (uint32_t k = lane; k < u.image; k += CRC_LANES) start += crc_batch_size(a, k);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) start += __shfl_xor(start, off, 64);
    if ((lane & 63) == 0) s_sum[lane >> 6] = start;
    __syncthreads();
    start = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
    const unsigned long long n = crc_batch_size(a, u.image), off = static_cast<unsigned long long>(u.piece) * CRC_PIECE;
    const uint32_t w = a.images[u.image].word0 + u.piece;
    if (off >= n) {
        if (lane == 0) a.words[w] = 0;
        return;
    }
    const uint32_t plen = static_cast<uint32_t>(n - off < CRC_PIECE ? n - off : CRC_PIECE);
    CrcLane ln{0};
    const uint32_t r = crc_piece(a.out + start + off, plen, s, ln, lane);
    if (lane == 0) a.words[w] = r;
}

__global__ __launch_bounds__(CRC_LANES) void crc32_fold_batch_kernel(CrcBatchArgs a)
{
    __shared__ CrcShared s;
    const int lane = threadIdx.x;
    CrcLane ln{0};
    const uint32_t crc = crc_stream(a.words + a.images[blockIdx.x].word0, crc_batch_size(a, blockIdx.x), a.seed, s, ln, lane);
    if (lane == 0) a.crcs[blockIdx.x] = crc;
}

static int crc_grid(unsigned long long pieces, uint32_t *grid)
{
    if (pieces > 0x7fffffffull) {
        set_error("invalid argument: a CRC over more than 2^31 - 1 pieces of %d bytes", CRC_PIECE);
        return FNX_ERR_INVALID;
    }
    *grid = static_cast<uint32_t>(pieces);
    return FNX_OK;
}

int launch_crc32(fnx_ctx *ctx, const uint8_t *d_src, size_t n_max, const unsigned long long *d_n, uint32_t seed, uint32_t *d_crc)
{
    uint32_t grid = 0;
    FNX_TRY(crc_grid((static_cast<unsigned long long>(n_max) + CRC_PIECE - 1) / CRC_PIECE, &grid));
    void *dw = nullptr;
    FNX_TRY(scratch(ctx, SLOT_CRC, sizeof(uint32_t) * (static_cast<size_t>(grid) + 4), &dw));
    CrcArgs a{};
    a.src = d_src; a.n_max = n_max; a.d_n = d_n; a.words = static_cast<uint32_t *>(dw); a.seed = seed; a.crc = d_crc;
    if (grid) {                                                      // (no byte: the fold's seed term alone)
        FNX_TRY(prof_begin(ctx));
        hipLaunchKernelGGL(crc32_pieces_kernel, dim3(grid), dim3(CRC_LANES), 0, ctx->stream, a);
        FNX_HIP(hipGetLastError());
        FNX_TRY(prof_end(ctx));
    }
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(crc32_fold_kernel, dim3(1), dim3(CRC_LANES), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    return FNX_OK;
}

int launch_crc32_batch(fnx_ctx *ctx, const uint8_t *d_out, const unsigned long long *d_sizes, const size_t *bounds, uint32_t m, uint32_t seed,
                       uint32_t *d_crcs)
{
    std::vector<CrcBatchImage> images(m);
    std::vector<CrcBatchUnit> units;
    unsigned long long total = 0;
    for (uint32_t i = 0; i < m; i++) {
        const unsigned long long np = (static_cast<unsigned long long>(bounds[i]) + CRC_PIECE - 1) / CRC_PIECE;
        uint32_t grid = 0;
        FNX_TRY(crc_grid(total + np, &grid));
        images[i] = CrcBatchImage{bounds[i], static_cast<uint32_t>(total), static_cast<uint32_t>(np)};
        for (uint32_t j = 0; j < np; j++) units.push_back(CrcBatchUnit{i, j});
        total += np;
    }
    void *dw = nullptr;
    FNX_TRY(scratch(ctx, SLOT_CRC, sizeof(uint32_t) * (static_cast<size_t>(total) + 4), &dw));
    const void *hosts[2] = {units.data(), images.data()};
    const size_t sizes[2] = {sizeof(CrcBatchUnit) * units.size(), sizeof(CrcBatchImage) * images.size()};
    void *dp[2];
    FNX_TRY(upload_tables(ctx, SLOT_CRC_TAB, hosts, sizes, 2, dp));
    CrcBatchArgs a{};
    a.units = static_cast<const CrcBatchUnit *>(dp[0]); a.images = static_cast<const CrcBatchImage *>(dp[1]);
    a.out = d_out; a.sizes = d_sizes; a.words = static_cast<uint32_t *>(dw); a.seed = seed; a.crcs = d_crcs;
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(crc32_pieces_batch_kernel, dim3(static_cast<uint32_t>(total)), dim3(CRC_LANES), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(crc32_fold_batch_kernel, dim3(m), dim3(CRC_LANES), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    return FNX_OK;
}

}  // namespace fnx
