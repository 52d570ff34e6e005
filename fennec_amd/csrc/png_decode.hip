// fnx_png_decode's device side: the inflated stream of a PNG file (h rows of 1 + rowbytes bytes: the filter type, the
// filtered row) -> the reconstructed rows (png_unfilter_kernel) -> image.Decode's pixels through toNRGBA (png_expand_kernel).
// The rule both kernels follow is restated above fnx_png_decode in include/fennec_hip.h.  fnx_png_decode_batch runs the same
// two bodies over a chunk of files at once: png_unfilter_batch_kernel, png_expand_batch_kernel (per-file descriptors in device
// memory instead of kernel arguments; one workgroup per unit of any file, 256 pixels of a row of any file).  An Adam7 file
// (fnx_ctx_set_png_adam7) is seven small images to png_unfilter_batch_kernel -- a descriptor per present pass, every pass's
// units in one launch -- and png_expand_adam7_kernel gathers the passes' pixels into the image (below).
//
// png_unfilter_kernel.  Average and Paeth need the pixel to the left and the row above, so a chain of dependent rows is
// walked as a skewed wavefront: a lane owns a row and trails the lane that owns the row above by one pixel (one step), so at
// step s thread t reconstructs pixel s - lag(t) of its row.  A step handles one whole pixel -- bpp <= 8 bytes in a 64-bit
// register pair -- and per step a lane gets b (the pixel above) from the lane below it by one cross-lane move of the
// neighbour's last result; the b of the step before is its c, its own last result its a.  The filter type is a per-lane
// constant: the four predictors are computed and one is selected, no branch.
//   * A workgroup is PNG_DEC_ROWS lanes = 16 waves = one BAND of rows in flight (four waves a SIMD: one chain is one
//     workgroup, so its latencies can only hide behind its own other waves).  Lane 63 of a wave leaves its pixels in an LDS
//     ring, lane 0 of the next wave takes them from there.  A wave lags the wave above by UF_C extra steps and the
//     workgroup meets at a barrier every UF_C steps: the entry lane 0 reads was written UF_C + 1 steps earlier, so a barrier
//     lies between the write and the read, and between two barriers the waves drift apart by less than UF_C steps, so a
//     ring of 2 UF_C + 1 entries is never overwritten early (UF_RING = 128).
//   * A unit (png_row_plan: whole chain segments) longer than a band is marched band by band by the SAME workgroup; row 0
//     of the next band reads the band's last row back from the reconstructed plane behind a barrier.  No workgroup ever
//     waits for another one.
//   * Each lane streams its own row: 16-byte aligned loads into a 24-byte shift queue the pixels are taken from, and a
//     16-byte store whenever the output queue holds that much.  The reconstructed rows go to a second plane whose rows
//     start on 16-byte boundaries, so no two lanes ever write into one 16-byte word (in place, neighbouring rows of
//     the tight stream would).  Chosen over staging tiles through LDS because the skew makes a wave's 64 rows need 64
//     different column windows at any time: a staged tile would be a parallelogram of 64 short row pieces, one load
//     instruction each, which is what the per-lane stream issues anyway -- without the LDS round trip.
#include "common.hpp"

#include <type_traits>

namespace fnx {

namespace {

constexpr int UF_T = PNG_DEC_ROWS;           // lanes = rows in flight
constexpr int UF_WAVES = UF_T / 64;
constexpr int UF_C = 32;                     // steps between barriers = a wave's extra lag behind the wave above
constexpr int UF_RING = 128;                 // >= 2 UF_C + 1, a power of two
static_assert(UF_T % 64 == 0 && UF_RING >= 2 * UF_C + 1 && (UF_RING & (UF_RING - 1)) == 0, "png_unfilter_kernel geometry");

typedef unsigned long long u64;

// a row's bytes in order, BPP at a time, from 16-byte aligned loads.  Bits of the queue above 8 * avail are zero.
struct RowReader {
    u64 q0 = 0, q1 = 0, q2 = 0;
    int avail = 0;
    const ulonglong2 *next = nullptr;
    const uint8_t *end = nullptr;

    __device__ void init(const uint8_t *p, const uint8_t *e)
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        next = reinterpret_cast<const ulonglong2 *>(a & ~uintptr_t(15));
        end = e;
        const int skip = static_cast<int>(a & 15);
        const ulonglong2 w = *next++;
        if (skip >= 8) {
            q0 = w.y >> (8 * (skip - 8));
            q1 = 0;
        } else if (skip == 0) {
            q0 = w.x;
            q1 = w.y;
        } else {
            q0 = (w.x >> (8 * skip)) | (w.y << (64 - 8 * skip));
            q1 = w.y >> (8 * skip);
        }
        q2 = 0;
        avail = 16 - skip;
    }

    template <int BPP>
    __device__ u64 take()
    {
        if (avail < 8 && reinterpret_cast<const uint8_t *>(next) < end) {
            const ulonglong2 w = *next++;
            if (avail == 0) {
                q0 = w.x;
                q1 = w.y;
                q2 = 0;
            } else {
                const int sh = 8 * avail;
                q0 |= w.x << sh;
                q1 = (w.x >> (64 - sh)) | (w.y << sh);
                q2 = w.y >> (64 - sh);
            }
            avail += 16;
        }
        u64 px;
        if constexpr (BPP == 8) {
            px = q0;
            q0 = q1;
            q1 = q2;
            q2 = 0;
        } else {
            constexpr int s = 8 * BPP;
            px = q0 & ((u64(1) << s) - 1);
            q0 = (q0 >> s) | (q1 << (64 - s));
            q1 = (q1 >> s) | (q2 << (64 - s));
            q2 >>= s;
        }
        avail -= BPP;
        return px;
    }
};

// a row's bytes out, BPP at a time, as 16-byte stores to a 16-byte aligned row
struct RowWriter {
    u64 o0 = 0, o1 = 0, o2 = 0;
    int cnt = 0;
    ulonglong2 *dst = nullptr;

    template <int BPP>
    __device__ void push(u64 px)
    {
        // px at byte cnt (0 .. 15) of the 24-byte queue: values are selected, never registers (an indexed queue goes to scratch)
        const int s = (8 * cnt) & 63;
        const u64 lo = px << s, hi = s ? px >> (64 - s) : 0;
        const bool upper = cnt >= 8;
        o0 |= upper ? 0 : lo;
        o1 |= upper ? lo : hi;
        o2 |= upper ? hi : 0;
        cnt += BPP;
        if (cnt >= 16) {
            *dst++ = make_ulonglong2(o0, o1);
            o0 = o2;
            o1 = 0;
            o2 = 0;
            cnt -= 16;
        }
    }
    __device__ void flush()
    {
        if (cnt > 0) *dst++ = make_ulonglong2(o0, o1);
        cnt = 0;
    }
};

// one pixel: f + predictor(a, b, c) per byte, mod 256
template <int BPP>
__device__ u64 reconstruct(u64 f, u64 a, u64 b, u64 c, int ftype)
{
    u64 x = 0;
#pragma unroll
    for (int j = 0; j < BPP; j++) {
        const int ff = static_cast<int>((f >> (8 * j)) & 255), aa = static_cast<int>((a >> (8 * j)) & 255);
        const int bb = static_cast<int>((b >> (8 * j)) & 255), cc = static_cast<int>((c >> (8 * j)) & 255);
        const int pa = abs(bb - cc), pb = abs(aa - cc), pc = abs(aa + bb - 2 * cc);
        const int paeth = (pa <= pb && pa <= pc) ? aa : (pb <= pc ? bb : cc);
        int pred = 0;
        pred = ftype == 1 ? aa : pred;
        pred = ftype == 2 ? bb : pred;
        pred = ftype == 3 ? (aa + bb) >> 1 : pred;
        pred = ftype == 4 ? paeth : pred;
        x |= static_cast<u64>((ff + pred) & 255) << (8 * j);
    }
    return x;
}

struct UnfilterArgs {
    const uint8_t *stream;       // h rows of spitch = 1 + rowbytes bytes
    size_t spitch;
    int rowbytes, npix;          // npix = rowbytes / BPP
    const uint32_t *units;       // [first row, end row) per workgroup
    uint8_t *rows;               // the reconstructed rows, ppitch (a multiple of 16) apart
    size_t ppitch;
};

// the rows [r0, r1) of one unit, band by band: the body of both unfilter kernels.  A, r0 and r1 are the same in every lane
template <int BPP>
__device__ __forceinline__ void unfilter_unit(const UnfilterArgs &A, const uint32_t r0, const uint32_t r1, u64 (*ring)[UF_RING])
{
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int lag = t + wv * UF_C;
    for (uint32_t band = r0; band < r1; band += UF_T) {
        // the band's last row finishes its last pixel at step npix - 1 + its lane's lag: a short unit does not pay for idle lanes
        const int tl = static_cast<int>(r1 - band < static_cast<uint32_t>(UF_T) ? r1 - band : static_cast<uint32_t>(UF_T)) - 1;
        const int nsteps = A.npix + tl + (tl >> 6) * UF_C;
        const uint32_t y = band + t;
        const bool live = y < r1;
        const bool from_plane = t == 0 && band > r0;                      // the row above is the band before's last row
        int ftype = 0;
        RowReader in, up;
        RowWriter out;
        if (live) {
            const uint8_t *rp = A.stream + static_cast<size_t>(y) * A.spitch;
            ftype = rp[0];
            in.init(rp + 1, rp + 1 + A.rowbytes);
            out.dst = reinterpret_cast<ulonglong2 *>(A.rows + static_cast<size_t>(y) * A.ppitch);
        }
        if (from_plane) {
            const uint8_t *ap = A.rows + static_cast<size_t>(y - 1) * A.ppitch;
            up.init(ap, ap + A.rowbytes);
        }
        u64 a = 0, c = 0, last = 0;
        for (int s = 0; s < nsteps; s++) {
            if ((s % UF_C) == 0) __syncthreads();
            const int p = s - lag;
            const bool act = live && p >= 0 && p < A.npix;
            u64 b = __shfl_up(last, 1);                                    // what the lane above made one step ago: pixel p of its row
            if (lane == 0) {
                b = 0;
                if (act && wv > 0) b = ring[wv - 1][p & (UF_RING - 1)];
                if (act && from_plane) b = up.take<BPP>();
            }
            if (act) {
                if (p == 0) a = c = 0;
                const u64 f = in.take<BPP>();
                const u64 x = reconstruct<BPP>(f, a, b, c, ftype);
                out.push<BPP>(x);
                a = x;
                c = b;
                last = x;
                if (lane == 63 && wv < UF_WAVES - 1) ring[wv][p & (UF_RING - 1)] = x;
                if (p == A.npix - 1) out.flush();
            }
        }
        __syncthreads();                                                   // the band's rows are in the plane before the next band reads its last one
    }
}

template <int BPP>
__global__ __launch_bounds__(UF_T) void png_unfilter_kernel(UnfilterArgs A)
{
    __shared__ u64 ring[UF_WAVES - 1][UF_RING];
    unfilter_unit<BPP>(A, A.units[2 * blockIdx.x], A.units[2 * blockIdx.x + 1], ring);
}

// fnx_png_decode_batch: the units of all files of a chunk whose pixels are BPP bytes, one workgroup each.  The unit and its
// file's descriptor are indexed by blockIdx.x alone -- uniform, so they are read once through the scalar cache and stay in
// scalar registers --, and from there the workgroup is png_unfilter_kernel's
template <int BPP>
__global__ __launch_bounds__(UF_T) void png_unfilter_batch_kernel(const PngBatchUnit *__restrict__ units, const PngBatchFile *__restrict__ files)
{
    __shared__ u64 ring[UF_WAVES - 1][UF_RING];
    const PngBatchUnit u = units[blockIdx.x];
    const PngBatchFile &f = files[u.file];
    UnfilterArgs A;
    A.stream = f.stream;
    A.spitch = f.spitch;
    A.rowbytes = f.rowbytes;
    A.npix = f.npix;
    A.units = nullptr;
    A.rows = f.rows;
    A.ppitch = f.ppitch;
    unfilter_unit<BPP>(A, u.r0, u.r1, ring);
}

// ---- png_expand_kernel: one thread per pixel ------------------------------------------------------------------------------
struct ExpandArgs {
    const uint8_t *rows;
    size_t ppitch;
    PngExpand e;
    const uint32_t *table;       // colour type 3: the 256 pixel values
    uint8_t *dst;
    int dstride;
};

__device__ inline uint32_t pack(uint32_t r, uint32_t g, uint32_t b, uint32_t a) { return r | (g << 8) | (b << 16) | (a << 24); }

// convertToNRGBA (convert.go:34-64) of a color.NRGBA64: premultiply, un-premultiply, high bytes -- exact in uint32
__device__ inline uint32_t nrgba64_pixel(uint32_t R, uint32_t G, uint32_t B, uint32_t A)
{
    if (A == 0) return 0;
    if (A == 0xffffu) return pack(R >> 8, G >> 8, B >> 8, 255);
    const uint32_t r = (R * A / 0xffffu) * 0xffffu / A, g = (G * A / 0xffffu) * 0xffffu / A, b = (B * A / 0xffffu) * 0xffffu / A;
    return pack(r >> 8, g >> 8, b >> 8, A >> 8);
}

// pixel x of the reconstructed row r
__device__ __forceinline__ uint32_t expand_pixel(const PngExpand &e, const uint32_t *table, const uint8_t *r, const int x)
{
    uint32_t out = 0;
    if (e.depth < 8) {                                   // colour types 0 and 3: samples packed MSB first
        const int bit = x * e.depth;
        const uint32_t v = (static_cast<uint32_t>(r[bit >> 3]) >> (8 - e.depth - (bit & 7))) & ((1u << e.depth) - 1u);
        if (e.color_type == 3) {
            out = table[v];
        } else {
            const uint32_t g = v * (e.depth == 1 ? 0xffu : e.depth == 2 ? 0x55u : 0x11u);
            out = pack(g, g, g, (e.has_trns && v == (e.key[0] & 0xffu)) ? 0 : 255);
        }
    } else if (e.depth == 8) {
        switch (e.color_type) {
        case 0: {
            const uint32_t g = r[x];
            out = pack(g, g, g, (e.has_trns && g == (e.key[0] & 0xffu)) ? 0 : 255);
            break;
        }
        case 2: {
            const uint32_t cr = r[3 * x], cg = r[3 * x + 1], cb = r[3 * x + 2];
            const bool hit = e.has_trns && cr == (e.key[0] & 0xffu) && cg == (e.key[1] & 0xffu) && cb == (e.key[2] & 0xffu);
            out = pack(cr, cg, cb, hit ? 0 : 255);
            break;
        }
        case 3: out = table[r[x]]; break;
        case 4: out = pack(r[2 * x], r[2 * x], r[2 * x], r[2 * x + 1]); break;
        default: out = pack(r[4 * x], r[4 * x + 1], r[4 * x + 2], r[4 * x + 3]); break;
        }
    } else {                                             // 16-bit samples, big-endian
        const int ch = e.color_type == 0 ? 1 : e.color_type == 4 ? 2 : e.color_type == 2 ? 3 : 4;
        const uint8_t *p = r + static_cast<size_t>(x) * ch * 2;
        uint32_t s[4] = {0, 0, 0, 0};
        for (int k = 0; k < ch; k++) s[k] = (static_cast<uint32_t>(p[2 * k]) << 8) | p[2 * k + 1];
        uint32_t R, G, B, Al;
        bool alpha = true;
        if (e.color_type == 0) {
            R = G = B = s[0];
            alpha = e.has_trns;
            Al = (e.has_trns && s[0] == e.key[0]) ? 0 : 0xffffu;
        } else if (e.color_type == 2) {
            R = s[0]; G = s[1]; B = s[2];
            alpha = e.has_trns;
            Al = (e.has_trns && s[0] == e.key[0] && s[1] == e.key[1] && s[2] == e.key[2]) ? 0 : 0xffffu;
        } else if (e.color_type == 4) {
            R = G = B = s[0];
            Al = s[1];
        } else {
            R = s[0]; G = s[1]; B = s[2];
            Al = s[3];
        }
        out = alpha ? nrgba64_pixel(R, G, B, Al) : pack(R >> 8, G >> 8, B >> 8, 255);     // Gray16 / RGBA64: the high bytes
    }
    return out;
}

__global__ __launch_bounds__(256) void png_expand_kernel(ExpandArgs A)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= A.e.w) return;
    const uint32_t out = expand_pixel(A.e, A.table, A.rows + static_cast<size_t>(y) * A.ppitch, x);
    *reinterpret_cast<uint32_t *>(A.dst + static_cast<size_t>(y) * A.dstride + 4 * static_cast<size_t>(x)) = out;
}

// fnx_png_decode_batch: the pixels of all files of a chunk in one launch.  A workgroup is 256 pixels of one row of one file;
// the files' workgroups lie back to back (tile0: a file's first one, files[m].tile0 would be the grid), so the file is found
// by a search over at most FNX_PNG_DECODE_CHUNK descriptors that is the same in every lane.  A chunk's rows do not fit a grid
// dimension the way one file's h <= 65535 does.
__global__ __launch_bounds__(256) void png_expand_batch_kernel(const PngBatchFile *__restrict__ files, const int m)
{
    int lo = 0, hi = m - 1;                              // the last file whose tile0 <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (files[mid].tile0 <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const PngBatchFile &f = files[lo];
    const uint32_t tile = blockIdx.x - f.tile0, tiles_x = (static_cast<uint32_t>(f.e.w) + 255u) / 256u;
    const uint32_t y = tile / tiles_x;
    const int x = static_cast<int>((tile - y * tiles_x) * 256u + threadIdx.x);
    if (x >= f.e.w || y >= static_cast<uint32_t>(f.e.h)) return;
    const uint32_t out = expand_pixel(f.e, f.table, f.rows + static_cast<size_t>(y) * f.ppitch, x);
    *reinterpret_cast<uint32_t *>(f.dst + static_cast<size_t>(y) * f.dstride + 4 * static_cast<size_t>(x)) = out;
}

// ---- Adam7: the passes' planes -> the image ----------------------------------------------------------------------------------
// The gather form: a thread per OUTPUT pixel, a workgroup 256 pixels of one output row, so every lane's store is the 4 bytes
// next to its neighbour's.  (x & 7, y & 7) names the pass in Adam7's 8 x 8 map; the row y is the workgroup's, so which passes
// a row draws from is uniform: an odd row reads pass 7 alone, rows 2 and 6 of the eight passes 5 and 6, row 4 passes 3, 4 and
// 6, row 0 passes 1, 2, 4 and 6.  Pass p starts at (x0, y0) < (dx, dy) and dx, dy are powers of two, so the pixel's place in
// its pass is (x >> log2 dx, y >> log2 dy).  The seven plane pointers and pitches are kernel arguments (the batch form: a
// descriptor indexed by blockIdx.x alone), scalar registers the lane's own pair is SELECTED from -- an indexed read would make
// them a per-lane load.  The reads of one pass are a lane in 2, 4 or 8 apart over densely packed pass rows: neighbouring lanes of
// the same pass read neighbouring pass pixels.
__device__ __forceinline__ uint32_t adam7_pixel(const PngAdam7File &f, const int x, const uint32_t y)
{
    const uint32_t yc = y & 7u;
    int p;                                               // 0-based pass
    if (yc & 1u) p = 6;
    else if (yc & 2u) p = (x & 1) ? 5 : 4;
    else if (yc & 4u) p = (x & 1) ? 5 : ((x & 2) ? 3 : 2);
    else p = (x & 1) ? 5 : ((x & 2) ? 3 : ((x & 4) ? 1 : 0));
    const int xs = 3 - (p >> 1);                         // log2 dx: 3 3 2 2 1 1 0
    const int ys = 3 - ((p > 0 ? p - 1 : 0) >> 1);       // log2 dy: 3 3 3 2 2 1 1
    const uint8_t *plane = f.plane[0];
    uint32_t pitch = f.ppitch[0];
#pragma unroll
    for (int k = 1; k < 7; k++) {
        plane = p == k ? f.plane[k] : plane;
        pitch = p == k ? f.ppitch[k] : pitch;
    }
    return expand_pixel(f.e, f.table, plane + static_cast<size_t>(y >> ys) * pitch, x >> xs);
}

__global__ __launch_bounds__(256) void png_expand_adam7_kernel(PngAdam7File A)
{
    const int x = blockIdx.x * 256 + threadIdx.x;
    const uint32_t y = blockIdx.y;
    if (x >= A.e.w) return;
    *reinterpret_cast<uint32_t *>(A.dst + static_cast<size_t>(y) * A.dstride + 4 * static_cast<size_t>(x)) = adam7_pixel(A, x, y);
}

// the Adam7 files of a chunk in one launch: png_expand_batch_kernel's tiling and search over descriptors of their own
__global__ __launch_bounds__(256) void png_expand_adam7_batch_kernel(const PngAdam7File *__restrict__ files, const int m)
{
    int lo = 0, hi = m - 1;                              // the last file whose tile0 <= blockIdx.x
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (files[mid].tile0 <= blockIdx.x) lo = mid;
        else hi = mid - 1;
    }
    const PngAdam7File &f = files[lo];
    const uint32_t tile = blockIdx.x - f.tile0, tiles_x = (static_cast<uint32_t>(f.e.w) + 255u) / 256u;
    const uint32_t y = tile / tiles_x;
    const int x = static_cast<int>((tile - y * tiles_x) * 256u + threadIdx.x);
    if (x >= f.e.w || y >= static_cast<uint32_t>(f.e.h)) return;
    *reinterpret_cast<uint32_t *>(f.dst + static_cast<size_t>(y) * f.dstride + 4 * static_cast<size_t>(x)) = adam7_pixel(f, x, y);
}

// launch(std::integral_constant<int, BPP>()) for the unfilter kernels' six pixel distances; false: bpp is none of them
template <typename Launch> bool with_bpp(int bpp, Launch launch)
{
    switch (bpp) {
    case 1: launch(std::integral_constant<int, 1>()); return true;
    case 2: launch(std::integral_constant<int, 2>()); return true;
    case 3: launch(std::integral_constant<int, 3>()); return true;
    case 4: launch(std::integral_constant<int, 4>()); return true;
    case 6: launch(std::integral_constant<int, 6>()); return true;
    case 8: launch(std::integral_constant<int, 8>()); return true;
    default: return false;
    }
}

int launch_unfilter_batch(fnx_ctx *ctx, int bpp, const PngBatchUnit *u, int nunits, const PngBatchFile *d_files)
{
    const dim3 grid(nunits), block(UF_T);
    FNX_TRY(prof_begin(ctx));
    if (!with_bpp(bpp, [&](auto b) { hipLaunchKernelGGL(png_unfilter_batch_kernel<b()>, grid, block, 0, ctx->stream, u, d_files); })) {
        set_error("internal: png_unfilter_batch_kernel has no form for bpp %d", bpp);
        return FNX_ERR_INVALID;
    }
    FNX_HIP(hipGetLastError());
    return prof_end(ctx);
}

}  // namespace

size_t png_plane_pitch(const PngFile &f) { return (f.rowbytes + 15) & ~size_t(15); }

int launch_png_unfilter(fnx_ctx *ctx, const uint8_t *d_stream, const PngFile &f, const uint32_t *d_units, int nunits, uint8_t *d_rows)
{
    UnfilterArgs a;
    a.stream = d_stream;
    a.spitch = 1 + f.rowbytes;
    a.rowbytes = static_cast<int>(f.rowbytes);
    a.npix = static_cast<int>(f.rowbytes / f.bpp);
    a.units = d_units;
    a.rows = d_rows;
    a.ppitch = png_plane_pitch(f);
    const dim3 grid(nunits), block(UF_T);
    FNX_TRY(prof_begin(ctx));
    if (!with_bpp(f.bpp, [&](auto b) { hipLaunchKernelGGL(png_unfilter_kernel<b()>, grid, block, 0, ctx->stream, a); })) {
        set_error("internal: png_unfilter_kernel has no form for bpp %d", f.bpp);
        return FNX_ERR_INVALID;
    }
    FNX_HIP(hipGetLastError());
    return prof_end(ctx);
}

int launch_png_expand(fnx_ctx *ctx, const uint8_t *d_rows, const PngFile &f, const uint32_t *d_table, uint8_t *dst, int dstride)
{
    ExpandArgs a;
    a.rows = d_rows;
    a.ppitch = png_plane_pitch(f);
    a.e = png_expand_of(f);
    a.table = d_table;
    a.dst = dst;
    a.dstride = dstride;
    note_route(ctx, FNX_PROF_MAIN, "png_unfilter_kernel, png_expand_kernel");
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(png_expand_kernel, dim3((f.w + 255) / 256, f.h), dim3(256), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    return prof_end(ctx);
}

int launch_png_decode_chunk(fnx_ctx *ctx, const PngBatchUnit *d_units, const int nunits[6], const PngBatchFile *d_files, int m, uint32_t tiles,
                            const PngAdam7File *d_adam7, int ma, uint32_t atiles)
{
    note_route(ctx, FNX_PROF_MAIN, ma ? "png_unfilter_batch_kernel, png_expand_batch_kernel, png_expand_adam7_batch_kernel"
                                      : "png_unfilter_batch_kernel, png_expand_batch_kernel");
    const PngBatchUnit *u = d_units;
    for (int k = 0; k < 6; k++) {
        if (nunits[k] == 0) continue;
        FNX_TRY(launch_unfilter_batch(ctx, PNG_BPPS[k], u, nunits[k], d_files));
        u += nunits[k];
    }
    if (m > 0) {                                         // (a chunk of Adam7 files alone has no workgroup for this kernel)
        FNX_TRY(prof_begin(ctx));
        hipLaunchKernelGGL(png_expand_batch_kernel, dim3(tiles), dim3(256), 0, ctx->stream, d_files, m);
        FNX_HIP(hipGetLastError());
        FNX_TRY(prof_end(ctx));
    }
    if (ma > 0) {
        FNX_TRY(prof_begin(ctx));
        hipLaunchKernelGGL(png_expand_adam7_batch_kernel, dim3(atiles), dim3(256), 0, ctx->stream, d_adam7, ma);
        FNX_HIP(hipGetLastError());
        FNX_TRY(prof_end(ctx));
    }
    return FNX_OK;
}

int launch_png_adam7(fnx_ctx *ctx, int bpp, const PngBatchUnit *d_units, int nunits, const PngBatchFile *d_passes, const PngAdam7File &a)
{
    note_route(ctx, FNX_PROF_MAIN, "png_unfilter_batch_kernel, png_expand_adam7_kernel");
    FNX_TRY(launch_unfilter_batch(ctx, bpp, d_units, nunits, d_passes));
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(png_expand_adam7_kernel, dim3((a.e.w + 255) / 256, a.e.h), dim3(256), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    return prof_end(ctx);
}

}  // namespace fnx
