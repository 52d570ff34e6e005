// medianCut (targetsize.go:422-486) on gfx950: the palettes of quantizeStrategy (targetsize.go:180-206) without the image
// leaving the device.  The five palette sizes the strategy asks for are five prefixes of ONE greedy run -- the split sequence
// does not depend on maxColors -- so one launch answers all of them.
//
// One workgroup of 512 lanes owns the whole run (median_cut_split.inc, which tools/median_cut_hostsim runs on the CPU): up to
// 255 dependent splits, no kernel boundary and no other workgroup to wait for between them.  The samples (<= 199 999 packed
// words, 800 KB, L2-resident) live in a ping-pong pair of global buffers; every box is a contiguous run in ascending sample
// number, and a split is a 256-bin LDS histogram of the axis byte, a prefix over the bins for the median value, and ONE stable
// partition pass that also gathers both halves' minima, maxima and sums.  Tied samples keep the order they were taken in: that
// is the library's tie rule (the reference's is whatever pdqsort leaves), and it makes every split a function of sets, so the
// launch geometry cannot reach the bytes.  Integers only.
//
// median_cut_gather_kernel takes the samples from a resident image (FNX_DEVICE); a host image's samples are gathered by the
// host and uploaded alone (<= 800 KB instead of the image).
#include "common.hpp"
#include "devutil.hpp"

namespace fnx {

#define MC_FN __device__ __forceinline__
#define MC_PHASE(call) { call; } __syncthreads();
#define MC_ATOMIC_ADD(p, v) atomicAdd(p, v)
#define MC_ATOMIC_MAX64(p, v) atomicMax(p, v)
#define MC_LOAD4(p) mc_load4(p)
#define MC_UNIFORM(x) static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(x)))
#define MC_RUN_PARAMS , McLane &ln, int tid

struct McVec4;
__device__ __forceinline__ McVec4 mc_load4(const uint32_t *p);
#include "median_cut_split.inc"

__device__ __forceinline__ McVec4 mc_load4(const uint32_t *p)
{
    const u32x4 v = *reinterpret_cast<const u32x4 *>(p);
    return McVec4{v.x, v.y, v.z, v.w};
}

static_assert(sizeof(McShared) <= 64 * 1024, "the run's LDS fits a workgroup's 64 KB");

__global__ __launch_bounds__(MC_LANES) void median_cut_kernel(McArgs a)
{
    __shared__ McShared s;
    McLane ln;
    mc_run(a, s, ln, static_cast<int>(threadIdx.x));
}

// sample j = the R, G, B of the flat 4-byte group at byte 4 j step (targetsize.go:436-440)
__global__ __launch_bounds__(256) void median_cut_gather_kernel(const uint8_t *src, unsigned long long step, uint32_t ns, uint32_t *out)
{
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < ns) out[j] = *(g_u32 *)(src + 4ull * j * step) & 0x00ffffffu;
}

void median_cut_samples(long long n, long long *step, long long *ns)
{
    *step = n > 100000 ? n / 100000 : 1;
    *ns = (n + *step - 1) / *step;
}

// src: a tight w x h image, w h >= 1, in `space`; max_colors: nlevels strictly ascending sizes within 1 .. 256 (checked by the
// caller).  *d_out (device): [nlevels][256] entries r | g << 8 | b << 16 | 255 << 24, then ncolors[nlevels].  Nothing is waited for.
int launch_median_cut(fnx_ctx *ctx, int space, const uint8_t *src, int w, int h, int nlevels, const int *max_colors, const uint32_t **d_out)
{
    long long step = 1, ns = 0;
    median_cut_samples(static_cast<long long>(w) * h, &step, &ns);
    FNX_REQUIRE(ns >= 1 && ns <= MC_MAX_SAMPLES, "median cut: sample count");
    const size_t cap = ((static_cast<size_t>(ns) + 3) & ~size_t(3)) + 4;
    void *d = nullptr;
    FNX_TRY(scratch(ctx, SLOT_MEDIAN_CUT, sizeof(uint32_t) * (2 * cap + static_cast<size_t>(nlevels) * 257), &d));
    McArgs a{};
    a.buf[0] = static_cast<uint32_t *>(d);
    a.buf[1] = a.buf[0] + cap;
    a.out = a.buf[1] + cap;
    a.n = static_cast<uint32_t>(ns);
    a.nlevels = static_cast<uint32_t>(nlevels);
    for (int l = 0; l < nlevels; l++) a.level_mask[(max_colors[l] - 1) >> 5] |= 1u << ((max_colors[l] - 1) & 31);
    if (space == FNX_HOST) {
        void *pin = nullptr;
        FNX_TRY(pinned_alloc(ctx, sizeof(uint32_t) * static_cast<size_t>(ns), &pin));
        uint32_t *hs = static_cast<uint32_t *>(pin);
        for (long long j = 0; j < ns; j++) {
            const uint8_t *p = src + 4 * j * step;
            hs[j] = p[0] | (static_cast<uint32_t>(p[1]) << 8) | (static_cast<uint32_t>(p[2]) << 16);
        }
        FNX_HIP(hipMemcpyAsync(a.buf[0], hs, sizeof(uint32_t) * static_cast<size_t>(ns), hipMemcpyHostToDevice, ctx->stream));
    } else {
        hipLaunchKernelGGL(median_cut_gather_kernel, dim3(static_cast<unsigned>((ns + 255) / 256)), dim3(256), 0, ctx->stream, src,
                           static_cast<unsigned long long>(step), a.n, a.buf[0]);
    }
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(median_cut_kernel, dim3(1), dim3(MC_LANES), 0, ctx->stream, a);
    FNX_TRY(prof_end(ctx));
    FNX_HIP(hipGetLastError());
    note_route(ctx, FNX_PROF_MAIN, "median_cut_kernel");
    *d_out = a.out;
    return FNX_OK;
}

}  // namespace fnx
