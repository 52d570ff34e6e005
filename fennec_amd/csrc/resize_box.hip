// boxDownsample(lanczosResize(src, midW, midH), dstW, dstH) (resize.go:37-53, then ssim.go:244-309) in one pass on gfx950:
// the midW x midH image is never stored.  That pair is what computeSSIMNRGBA (targetsize.go:563-568) does to its second
// image before SSIMFast's windows see it: an upscale back to the source's size, consumed only as <= 512 px of box sums.
//
// One workgroup owns an RB_TW x RB_TH tile of the midW x midH image:
//   1. H pass, global -> LDS: the rows of the reference's uint8 intermediate (midW x srcH, resize.go:51) that the tile's
//      V taps read, as NRGBA words -- the zero pixel where al <= 0.5 (resize.go:107-113);
//   2. V pass, LDS -> registers: a wave walks down its RB_TH / 4 rows, a lane per column;
//   3. each pixel's bytes are added to its lane's sums of the current box row (packed 2 x 16 bit: <= 8 rows x 255), and
//      when the box row ends the wave adds the columns of each box together (lane shuffles: no LDS, no barrier);
//   4. the first lane of every box adds the wave's part to the image-wide integer sums with two 64-bit vector atomics.
// Integer sums do not depend on the order of the additions, so the result is bit-reproducible.  box_finish_sums_kernel
// then turns sums into bytes as averageBoxPixel does (devutil.hpp: box_finish).
//
// Arithmetic of both passes: resize_tap in tap order, fp64, unfused (-ffp-contract=off), clampF_dev -- resize_pass_kernel's,
// hence fnx_lanczos_resize's bytes whatever kernel that call takes.  No rounding guard, no plan, no state between calls (the
// table slot skips an upload of bytes it already holds, like every table slot).
//
// Domain (launch_resize_box checks it; everything else is composed from the resize and the box kernels by the caller):
//   * both tables have contiguous, in-range tap indices, at most RB_TAPS taps per output, and first / last indices that
//     do not decrease from one output to the next -- every table precomputeWeights makes for an upscale (<= 7 taps);
//   * an RB_TH-row band of outputs reads at most RB_ROWS intermediate rows (an upscale: <= RB_TH + 6);
//   * dst <= mid on both axes, the boxes do not overlap (box_edge with a ratio >= 1), and a box is at most RB_BOXW wide
//     (mid / dst <= 31: far beyond 8192 px / 512).
#include "common.hpp"
#include "devutil.hpp"

#include <algorithm>
#include <vector>

namespace fnx {

constexpr int RB_TW = 64, RB_TH = 32;   // tile of the mid image: a wave is one row of 64 columns
constexpr int RB_ROWS = 40;             // intermediate rows in LDS (10 KiB)
constexpr int RB_TAPS = 8;              // H taps held in registers
constexpr int RB_BOXW = 32;             // 32 columns x 8 rows x 255 < 65536: the packed 16-bit fields cannot overflow

struct ResizeBoxArgs {
    const uint8_t *src;
    int sstride, srcW, srcH;
    int midW, midH, dstW, dstH;
    const int32_t *offH, *idxH, *offV, *idxV;
    const double *wH, *wV;
    const int32_t *bx, *by;           // box index of mid column x / row y, -1: in no box
    unsigned long long *sums;         // [dstH][dstW][2]: R | G << 32, B | A << 32 (zero before the launch)
    int maxbw;                        // widest box, in columns
};

__global__ __launch_bounds__(256) void resize_box_kernel(ResizeBoxArgs a)
{
    __shared__ uint32_t s_tile[RB_ROWS * RB_TW];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int x = blockIdx.x * RB_TW + lane;
    const int y0 = blockIdx.y * RB_TH;
    const int y1 = min(y0 + RB_TH, a.midH);
    const bool live = x < a.midW;
    // intermediate rows [r0, r1) feed the tile (first / last tap indices do not decrease with y: table_covered)
    const int r0 = a.idxV[a.offV[y0]];
    const int r1 = a.idxV[a.offV[y1] - 1] + 1;

    // ---- 1. H pass: column x's taps in registers, rows r0 + wave, + 4, ...
    {
        double w[RB_TAPS] = {};
        int n = 0, s0 = 0;
        if (live) {
            const int t0 = a.offH[x];
            n = a.offH[x + 1] - t0;
            s0 = n > 0 ? a.idxH[t0] : 0;
#pragma unroll
            for (int k = 0; k < RB_TAPS; k++) w[k] = k < n ? a.wH[t0 + k] : 0.0;
        }
        for (int r = r0 + wave; r < r1; r += 4) {
            uint32_t o = 0;
            if (live) {
                const uint8_t *row = a.src + static_cast<size_t>(r) * a.sstride;
                double rr = 0, g = 0, b = 0, al = 0;
#pragma unroll
                for (int k = 0; k < RB_TAPS; k++)
                    if (k < n) resize_tap(ld_px(row, s0 + k), w[k], rr, g, b, al);
                if (al > 0.5) {                                 // resize.go:107-113
                    const double inv = 1.0 / al;
                    o = clampF_dev(rr * inv) | (clampF_dev(g * inv) << 8) | (clampF_dev(b * inv) << 16) | (clampF_dev(al) << 24);
                }
            }
            s_tile[(r - r0) * RB_TW + lane] = o;
        }
    }
    __syncthreads();

    // ---- 2.-4. V pass down the wave's rows, box sums as the rows go by
    const int d = live ? a.bx[x] : -1;
    const int d_left = __shfl_up(d, 1, 64);
    const bool leader = d >= 0 && (lane == 0 || d_left != d);
    uint32_t lo = 0, hi = 0;          // (R, B) and (G, A) of this column within the current box row
    int cur = -1;                     // the current box row (wave-uniform)
    auto flush = [&]() {
        if (cur >= 0) {
            uint32_t slo = lo, shi = hi;
            for (int k = 1; k < a.maxbw; k++) {
                const int dk = __shfl_down(d, k, 64);
                const uint32_t vlo = __shfl_down(lo, k, 64), vhi = __shfl_down(hi, k, 64);
                if (lane + k < 64 && dk == d) { slo += vlo; shi += vhi; }
            }
            if (leader) {
                unsigned long long *p = a.sums + (static_cast<size_t>(cur) * a.dstW + d) * 2;
                atomicAdd(p, static_cast<unsigned long long>(slo & 0xffffu) | (static_cast<unsigned long long>(shi & 0xffffu) << 32));
                atomicAdd(p + 1, static_cast<unsigned long long>(slo >> 16) | (static_cast<unsigned long long>(shi >> 16) << 32));
            }
        }
        lo = hi = 0;
    };
    const int ya = y0 + wave * (RB_TH / 4), yb = min(ya + RB_TH / 4, y1);
    for (int y = ya; y < yb; y++) {
        const int brow = a.by[y];
        if (brow != cur) {
            flush();
            cur = brow;
        }
        if (brow < 0) continue;
        const int t0 = a.offV[y], n = a.offV[y + 1] - t0;
        const int s0 = (n > 0 ? a.idxV[t0] : r0) - r0;
        double rr = 0, g = 0, b = 0, al = 0;
        for (int k = 0; k < n; k++) resize_tap(s_tile[(s0 + k) * RB_TW + lane], a.wV[t0 + k], rr, g, b, al);
        if (al > 0.5) {
            const double inv = 1.0 / al;
            lo += clampF_dev(rr * inv) | (clampF_dev(b * inv) << 16);
            hi += clampF_dev(g * inv) | (clampF_dev(al) << 16);
        }
    }
    flush();
}

struct BoxFinishArgs {
    const unsigned long long *sums;
    uint8_t *dst;
    int dstride, dstW, dstH, srcW, srcH;
    double xRatio, yRatio;
};

// sums -> averageBoxPixel's bytes (ssim.go:280-309); the counts are box_edge's, as in every other box kernel
__global__ __launch_bounds__(256) void box_finish_sums_kernel(BoxFinishArgs a)
{
    const int dx = blockIdx.x * 64 + (threadIdx.x & 63);
    const int dy = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (dx >= a.dstW || dy >= a.dstH) return;
    int sx0, sx1, sy0, sy1;
    box_edge(dx, a.xRatio, a.srcW, sx0, sx1);
    box_edge(dy, a.yRatio, a.srcH, sy0, sy1);
    const int count = (sy1 - sy0) * (sx1 - sx0);
    const unsigned long long *p = a.sums + (static_cast<size_t>(dy) * a.dstW + dx) * 2;
    const unsigned long long rg = p[0], ba = p[1];
    uint32_t o = 0;
    if (count > 0)
        o = box_finish(static_cast<uint32_t>(rg), static_cast<uint32_t>(rg >> 32), static_cast<uint32_t>(ba), static_cast<uint32_t>(ba >> 32), count);
    *(g_u32w *)(a.dst + static_cast<size_t>(dy) * a.dstride + 4 * static_cast<size_t>(dx)) = o;
}

// One pass's table inside the kernel's reach?  (see the head of this file)
static bool table_covered(const TapTable &t, int srcN, int band)
{
    int prev_first = 0, prev_last = 0;
    for (int d = 0; d < t.nout; d++) {
        const int t0 = t.off[d], n = t.off[d + 1] - t0;
        if (t0 < 0 || n < 1 || n > RB_TAPS) return false;
        const int first = t.idx[t0], last = first + n - 1;
        if (first < 0 || last >= srcN) return false;
        for (int k = 1; k < n; k++)
            if (t.idx[t0 + k] != first + k) return false;
        if (d > 0 && (first < prev_first || last < prev_last)) return false;
        prev_first = first;
        prev_last = last;
    }
    if (band > 0)
        for (int d0 = 0; d0 < t.nout; d0 += band) {
            const int d1 = std::min(d0 + band, t.nout) - 1;
            const int span = t.idx[t.off[d1 + 1] - 1] + 1 - t.idx[t.off[d0]];
            if (span > RB_ROWS) return false;
        }
    return true;
}

// box index of every mid column (row); false when boxes overlap or one is wider than the packed sums allow
static bool box_map(int midN, int dstN, int32_t *map, int *maxb)
{
    const double ratio = static_cast<double>(midN) / static_cast<double>(dstN);
    for (int i = 0; i < midN; i++) map[i] = -1;
    int prev_end = 0;
    *maxb = 0;
    for (int d = 0; d < dstN; d++) {
        int s0, s1;
        box_edge(d, ratio, midN, s0, s1);
        if (s0 < prev_end || s1 - s0 > RB_BOXW) return false;
        for (int i = s0; i < s1; i++) map[i] = d;
        if (s1 - s0 > *maxb) *maxb = s1 - s0;
        prev_end = s1;
    }
    return true;
}

// Is the pair inside resize_box_kernel's domain (the head of this file)?  Host arithmetic only.  map (optional) receives the box
// index of every mid column, then of every mid row; *maxbw the widest box.
bool resize_box_covers(const TapTable &th, const TapTable &tv, int srcW, int srcH, int midW, int midH, int dstW, int dstH,
                       std::vector<int32_t> *map, int *maxbw)
{
    if (srcW < 1 || srcH < 1 || dstW < 1 || dstH < 1 || dstW > midW || dstH > midH || th.nout != midW || tv.nout != midH) return false;
    if (!th.off || !th.idx || !th.wt || !tv.off || !tv.idx || !tv.wt) return false;
    if (!table_covered(th, srcW, 0) || !table_covered(tv, srcH, RB_TH)) return false;
    std::vector<int32_t> own;
    std::vector<int32_t> &m = map ? *map : own;
    m.assign(static_cast<size_t>(midW) + midH, -1);
    int bw = 0, bh = 0;
    if (!box_map(midW, dstW, m.data(), &bw) || !box_map(midH, dstH, m.data() + midW, &bh)) return false;
    if (maxbw) *maxbw = bw;
    return true;
}

// dst (device, dstW x dstH) = boxDownsample(lanczosResize(src, midW, midH), dstW, dstH), src on the device.
// FNX_NOOP (nothing launched) outside the kernel's domain.
int launch_resize_box(fnx_ctx *ctx, const uint8_t *src, int sstride, int srcW, int srcH, const TapTable &th, const TapTable &tv,
                      int midW, int midH, uint8_t *dst, int dstride, int dstW, int dstH)
{
    std::vector<int32_t> map;
    int maxbw = 0;
    if (!resize_box_covers(th, tv, srcW, srcH, midW, midH, dstW, dstH, &map, &maxbw)) return FNX_NOOP;
    const void *hosts[7] = {th.off, th.idx, th.wt, tv.off, tv.idx, tv.wt, map.data()};
    const size_t sizes[7] = {sizeof(int32_t) * (static_cast<size_t>(midW) + 1), sizeof(int32_t) * th.off[midW], sizeof(double) * th.off[midW],
                             sizeof(int32_t) * (static_cast<size_t>(midH) + 1), sizeof(int32_t) * tv.off[midH], sizeof(double) * tv.off[midH],
                             sizeof(int32_t) * map.size()};
    void *dp[7];
    FNX_TRY(upload_tables(ctx, SLOT_RZBOX_TABLES, hosts, sizes, 7, dp));   // (skipped when the slot already holds these bytes)
    const size_t sum_bytes = sizeof(unsigned long long) * 2 * static_cast<size_t>(dstW) * dstH;
    void *sums = nullptr;
    FNX_TRY(scratch(ctx, SLOT_RZBOX_SUMS, sum_bytes, &sums));
    FNX_TRY(prof_begin(ctx, FNX_PROF_RESIZE));          // the route's whole device time: the zeroing, the kernel, the finish
    FNX_HIP(hipMemsetAsync(sums, 0, sum_bytes, ctx->stream));

    ResizeBoxArgs a{};
    a.src = src; a.sstride = sstride; a.srcW = srcW; a.srcH = srcH;
    a.midW = midW; a.midH = midH; a.dstW = dstW; a.dstH = dstH;
    a.offH = static_cast<const int32_t *>(dp[0]); a.idxH = static_cast<const int32_t *>(dp[1]); a.wH = static_cast<const double *>(dp[2]);
    a.offV = static_cast<const int32_t *>(dp[3]); a.idxV = static_cast<const int32_t *>(dp[4]); a.wV = static_cast<const double *>(dp[5]);
    a.bx = static_cast<const int32_t *>(dp[6]); a.by = a.bx + midW;
    a.sums = static_cast<unsigned long long *>(sums);
    a.maxbw = maxbw;
    hipLaunchKernelGGL(resize_box_kernel, dim3((midW + RB_TW - 1) / RB_TW, (midH + RB_TH - 1) / RB_TH), dim3(256), 0, ctx->stream, a);
    BoxFinishArgs f{};
    f.sums = a.sums; f.dst = dst; f.dstride = dstride; f.dstW = dstW; f.dstH = dstH; f.srcW = midW; f.srcH = midH;
    f.xRatio = static_cast<double>(midW) / static_cast<double>(dstW);
    f.yRatio = static_cast<double>(midH) / static_cast<double>(dstH);
    hipLaunchKernelGGL(box_finish_sums_kernel, dim3((dstW + 63) / 64, (dstH + 3) / 4), dim3(256), 0, ctx->stream, f);
    FNX_TRY(prof_end(ctx));
    FNX_HIP(hipGetLastError());
    note_route(ctx, FNX_PROF_RESIZE, "resize_box_kernel");
    return FNX_OK;
}

}  // namespace fnx
