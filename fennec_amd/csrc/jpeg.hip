// The JPEG quantisation round trip on the device -- SURVEY 8(f)2, first slice.
//
// compressJPEGOptimal (compress.go:21-87) encodes the source at a candidate quality, decodes the bytes again and
// scores the decoded image with SSIMFast, up to seven times per image: the host codec is ~99 % of CompressBatch.
// For the SEARCH only the decoded pixels matter, and they are a function of the quantised DCT coefficients alone --
// Huffman coding is lossless.  These kernels therefore do, per candidate quality, what Go's image/jpeg does to the
// pixels and nothing else: RGB -> YCbCr (color.RGBToYCbCr, 16.16 fixed point; non-opaque pixels premultiplied as
// color.NRGBA.RGBA() does), 4:2:0 with edge replication and (sum + 2) >> 2 chroma averaging (writer.go), the IJG
// integer FDCT (fdct.go), division by 8 q rounded half away from zero, multiplication by q (reader.go), the Chen-Wang
// integer IDCT (idct.go), level shift + clamp -- into the planes an *image.YCbCr would hold; convert.hip then makes
// the NRGBA image toNRGBARef would and ssim.hip scores it.  The winning quality is encoded ONCE by the real codec on
// the host.  All integer arithmetic: bit-exact against the CPU restatement the tests check it with,
// which -- like this file -- restates Go's standard library from the published algorithms it implements (the source
// is not under /root/reference): parity with Go is unpinned twice over.
#include <vector>
#include "common.hpp"
#include "devutil.hpp"
#include "jpeg_idct.hpp"
#include "jpeg_layout.hpp"

namespace fnx {

struct YccArgs {
    const uint8_t *src;
    int sstride, w, h;
    uint8_t *yp, *cbp, *crp;     // Y: ys x 16 my; Cb, Cr: cs x 8 my
    int ys, cs, my;
    // r3: the source as a DECODED JPEG's planes (dy != nullptr): a pixel is toNRGBARef's (devutil.hpp's ycc_nrgba_px of
    // its samples), computed here instead of read from an image that fnx_jpeg_recompress would write only for this kernel
    // and the reference plane's box sums
    const uint8_t *dy, *dcb, *dcr;
    int dys, dcs, dxs, dysh;
};

// color.RGBToYCbCr on a (possibly premultiplied) pixel: Y | Cb << 8 | Cr << 16
__device__ __forceinline__ uint32_t rgb_to_ycc(uint32_t p)
{
    int32_t r = p & 0xffu, g = (p >> 8) & 0xffu, b = (p >> 16) & 0xffu;
    const uint32_t a = p >> 24;
    if (a != 0xffu) {                                  // color.NRGBA.RGBA(): c * 0x101 * A / 0xff, high byte kept
        r = static_cast<int32_t>((static_cast<uint32_t>(r) * 0x101u * a / 0xffu) >> 8);
        g = static_cast<int32_t>((static_cast<uint32_t>(g) * 0x101u * a / 0xffu) >> 8);
        b = static_cast<int32_t>((static_cast<uint32_t>(b) * 0x101u * a / 0xffu) >> 8);
    }
    const int32_t yy = (19595 * r + 38470 * g + 7471 * b + (1 << 15)) >> 16;
    int32_t cb = -11056 * r - 21712 * g + 32768 * b + (257 << 15);
    cb = ((static_cast<uint32_t>(cb) & 0xff000000u) == 0) ? cb >> 16 : ~(cb >> 31);
    int32_t cr = 32768 * r - 27440 * g - 5328 * b + (257 << 15);
    cr = ((static_cast<uint32_t>(cr) & 0xff000000u) == 0) ? cr >> 16 : ~(cr >> 31);
    return static_cast<uint32_t>(yy) | ((static_cast<uint32_t>(cb) & 0xffu) << 8) | ((static_cast<uint32_t>(cr) & 0xffu) << 16);
}

// a lane converts a 4 x 2 pixel patch of the MCU-padded image: 8 luma samples, 2 chroma pairs
// (workgroup (bx, by) of one image: jpeg_ycc_kernel's and jpeg_ycc_batch_kernel's)
__device__ __forceinline__ void jpeg_ycc_body(const YccArgs &a, int bx, int by)
{
    const int px = (bx * 64 + (threadIdx.x & 63)) * 4;
    const int py = (by * 4 + (threadIdx.x >> 6)) * 2;
    if (px >= a.ys || py >= 16 * a.my) return;
    uint32_t ycc[2][4];
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int yy = min(py + j, a.h - 1);                                                     // toYCbCr clamps to the last row / column
        if (a.dy) {
            const uint8_t *yr = a.dy + static_cast<size_t>(yy) * a.dys;
            const size_t co = static_cast<size_t>(yy >> a.dysh) * a.dcs;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int xx = min(px + i, a.w - 1);
                ycc[j][i] = rgb_to_ycc(ycc_nrgba_px(yr[xx], a.dcb[co + (xx >> a.dxs)], a.dcr[co + (xx >> a.dxs)]));
            }
        } else {
            const uint8_t *row = a.src + static_cast<size_t>(yy) * a.sstride;
#pragma unroll
            for (int i = 0; i < 4; i++) ycc[j][i] = rgb_to_ycc(ld_px(row, min(px + i, a.w - 1)));
        }
    }
#pragma unroll
    for (int j = 0; j < 2; j++)
        *reinterpret_cast<uint32_t *>(a.yp + static_cast<size_t>(py + j) * a.ys + px) =
            (ycc[j][0] & 0xffu) | ((ycc[j][1] & 0xffu) << 8) | ((ycc[j][2] & 0xffu) << 16) | ((ycc[j][3] & 0xffu) << 24);
    // writer.go scale(): (c00 + c01 + c10 + c11 + 2) >> 2
    uint32_t cb2 = 0, cr2 = 0;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        const uint32_t sb = ((ycc[0][2 * i] >> 8) & 0xffu) + ((ycc[0][2 * i + 1] >> 8) & 0xffu) + ((ycc[1][2 * i] >> 8) & 0xffu) + ((ycc[1][2 * i + 1] >> 8) & 0xffu);
        const uint32_t sr = ((ycc[0][2 * i] >> 16) & 0xffu) + ((ycc[0][2 * i + 1] >> 16) & 0xffu) + ((ycc[1][2 * i] >> 16) & 0xffu) + ((ycc[1][2 * i + 1] >> 16) & 0xffu);
        cb2 |= ((sb + 2) >> 2) << (8 * i);
        cr2 |= ((sr + 2) >> 2) << (8 * i);
    }
    *reinterpret_cast<uint16_t *>(a.cbp + static_cast<size_t>(py / 2) * a.cs + px / 2) = static_cast<uint16_t>(cb2);
    *reinterpret_cast<uint16_t *>(a.crp + static_cast<size_t>(py / 2) * a.cs + px / 2) = static_cast<uint16_t>(cr2);
}

__global__ __launch_bounds__(256) void jpeg_ycc_kernel(YccArgs a)
{
    jpeg_ycc_body(a, blockIdx.x, blockIdx.y);
}

// 4:4:4 (fnx_ctx_set_jpeg_subsampling, jpeg_layout.hpp): three planes of one size, ps x ph (multiples of 8), no scale().  A lane's
// 4 x 2 patch gives 8 samples to each plane: two 32-bit stores per plane (ps and the lane's column are multiples of 4, the
// plane bases jpeg_planes': 4-byte aligned)
struct Ycc444Args {
    const uint8_t *src;
    int sstride, w, h;
    uint8_t *yp, *cbp, *crp;
    int ps, ph;
};

__global__ __launch_bounds__(256) void jpeg_ycc444_kernel(Ycc444Args a)
{
    const int px = (blockIdx.x * 64 + (threadIdx.x & 63)) * 4;
    const int py = (blockIdx.y * 4 + (threadIdx.x >> 6)) * 2;
    if (px >= a.ps || py >= a.ph) return;
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const uint8_t *row = a.src + static_cast<size_t>(min(py + j, a.h - 1)) * a.sstride;     // toYCbCr clamps to the last row / column
        uint32_t y4 = 0, cb4 = 0, cr4 = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const uint32_t ycc = rgb_to_ycc(ld_px(row, min(px + i, a.w - 1)));
            y4 |= (ycc & 0xffu) << (8 * i);
            cb4 |= ((ycc >> 8) & 0xffu) << (8 * i);
            cr4 |= ((ycc >> 16) & 0xffu) << (8 * i);
        }
        const size_t o = static_cast<size_t>(py + j) * a.ps + px;
        *reinterpret_cast<uint32_t *>(a.yp + o) = y4;
        *reinterpret_cast<uint32_t *>(a.cbp + o) = cb4;
        *reinterpret_cast<uint32_t *>(a.crp + o) = cr4;
    }
}

// fnx_jpeg_compress_batch: the unquantised planes of n sources of one geometry.  Image = blockIdx.x / gx (images in x: the
// grid's y stays the one image's row count); image i's planes at planes + i * plane_bytes (Y | Cb | Cr, jpeg_planes' layout)
struct YccBatchArgs {
    YccArgs one;                  // geometry (src and plane pointers unused)
    const uint8_t *const *srcs;   // [n] device
    uint8_t *planes;
    size_t plane_bytes, cb_off, cr_off;
    int gx;
};

__global__ __launch_bounds__(256) void jpeg_ycc_batch_kernel(YccBatchArgs b)
{
    const int img = blockIdx.x / b.gx;
    YccArgs a = b.one;
    a.src = b.srcs[img];
    a.yp = b.planes + static_cast<size_t>(img) * b.plane_bytes;
    a.cbp = a.yp + b.cb_off;
    a.crp = a.yp + b.cr_off;
    jpeg_ycc_body(a, blockIdx.x - img * b.gx, blockIdx.y);
}

// ------------------------------------------------------------------------------------
// jpeg_ycc_kernel's planes of boxDownsample(src, dw, dh) (ssim.go:244-309) without the downsampled image: the target-size
// searches (targetsize.go:210-357) ask for the file size of up to 26 scaled copies of one source, and every copy would
// otherwise be written as NRGBA only to be read back by the colour conversion.  Workgroup = one chroma row (two padded
// output rows) x a segment of padded output columns.  Per output row: box_tiled_body's column sums (16-byte loads, packed
// 2 x 16-bit per source column, <= 257 box rows) into LDS, then one lane per output column adds its box's columns and
// finishes with the one fp64 multiply by 1 / count -- the same integers and the same clampF as box_tiled_kernel /
// box_generic_kernel.  Shapes the column sums do not cover (an upscale, boxes over 256 px) take box_generic_kernel's
// per-pixel sums (GENERIC).  The two rows' pixels then go through rgb_to_ycc and writer.go's chroma averaging exactly as
// in jpeg_ycc_kernel; padded positions take the box pixel at min(x, dw - 1) / min(y, dh - 1).
// ------------------------------------------------------------------------------------
constexpr int JB_CHUNKS = 256;            // 16-byte chunks (4 px) of the source a workgroup row covers
constexpr int JB_MAXROWS = 257;           // 257 * 255 < 65536: the packed column sums cannot overflow
constexpr int JB_SEG = 240;               // most box columns per workgroup: + 15 padding columns <= 256 lanes

struct BoxYccJob {
    const uint8_t *src;
    int sstride, srcW, srcH;
    int dw, dh;
    double xRatio, yRatio;
    int seg, vec_in;
    uint8_t *yp, *cbp, *crp;
    int ys, cs;
};

template <bool GENERIC>
__global__ __launch_bounds__(256) void jpeg_box_ycc_kernel(BoxYccJob a)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_col[JB_CHUNKS * 4 * 2];
    __shared__ uint32_t s_px[2][256];
    const int tid = threadIdx.x;
    const int py = 2 * blockIdx.y;                                  // first padded output row of the chroma row
    const int dx_lo = blockIdx.x * a.seg;
    const int dx_hi = min(dx_lo + a.seg, a.dw);                     // box columns of this segment
    const int dx_end = dx_hi == a.dw ? a.ys : dx_hi;                // ... plus the MCU padding in the last one
    const int ncol = dx_end - dx_lo;
    const int bxc = min(dx_lo + tid, a.dw - 1);                     // this lane's box column (padding: the last one)
    int sx0, sx1;
    box_edge(bxc, a.xRatio, a.srcW, sx0, sx1);
    int c0 = 0, nchunk = 0;
    if (!GENERIC) {
        int sxa, t1, t0, sxb;
        box_edge(dx_lo, a.xRatio, a.srcW, sxa, t1);
        box_edge(dx_hi - 1, a.xRatio, a.srcW, t0, sxb);
        c0 = sxa >> 2;
        nchunk = ((sxb + 3) >> 2) - c0;                             // <= JB_CHUNKS by the choice of seg
    }
    const int nrow = min(py + 1, a.dh - 1) == min(py, a.dh - 1) ? 1 : 2;   // padding rows repeat row dh - 1
    for (int j = 0; j < nrow; j++) {
        const int ry = min(py + j, a.dh - 1);
        int sy0, sy1;
        box_edge(ry, a.yRatio, a.srcH, sy0, sy1);
        uint32_t px = 0;
        if (GENERIC) {
            if (tid < ncol) {
                unsigned long long r = 0, g = 0, b = 0, al = 0;
                for (int sy = sy0; sy < sy1; sy++) {
                    const uint8_t *row = a.src + static_cast<size_t>(sy) * a.sstride;
                    for (int sx = sx0; sx < sx1; sx++) {
                        const uint32_t p = ld_px(row, sx);
                        r += p & 0xffu; g += (p >> 8) & 0xffu; b += (p >> 16) & 0xffu; al += p >> 24;
                    }
                }
                const long long count = static_cast<long long>(sy1 - sy0) * (sx1 - sx0);
                if (count > 0) {                                    // count == 0 (an upscale's sx1 == 0): the zero pixel
                    const double inv = 1.0 / static_cast<double>(count);
                    px = clampF_dev(static_cast<double>(r) * inv) | (clampF_dev(static_cast<double>(g) * inv) << 8) |
                         (clampF_dev(static_cast<double>(b) * inv) << 16) | (clampF_dev(static_cast<double>(al) * inv) << 24);
                }
            }
        } else {
            if (tid < nchunk) {
                const int x = 4 * (c0 + tid);
                uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
                const uint8_t *p = a.src + static_cast<size_t>(sy0) * a.sstride;
                if (a.vec_in && x + 3 < a.srcW) {
                    // four rows of 16-byte loads in flight per trip; a short last trip re-reads the box's last row and adds
                    // nothing for it
                    const uint8_t *q = p + 4 * static_cast<size_t>(x);
                    for (int sy = sy0; sy < sy1; sy += 4) {
                        u32x4 v[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) v[u] = ld16_stream(q + static_cast<size_t>(min(sy + u, sy1 - 1) - sy0) * a.sstride);
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            if (sy + u < sy1) {                     // uniform across the workgroup: one box row
#pragma unroll
                                for (int e = 0; e < 4; e++) {
                                    lo[e] += v[u][e] & 0x00ff00ffu;
                                    hi[e] += (v[u][e] >> 8) & 0x00ff00ffu;
                                }
                            }
                        }
                    }
                } else {
                    // an unaligned source, or the chunk that sticks out of the row: pixel by pixel, clamped (the surplus
                    // columns belong to no box)
                    for (int sy = sy0; sy < sy1; sy++, p += a.sstride) {
#pragma unroll
                        for (int e = 0; e < 4; e++) {
                            const uint32_t q = ld_px(p, min(x + e, a.srcW - 1));
                            lo[e] += q & 0x00ff00ffu;
                            hi[e] += (q >> 8) & 0x00ff00ffu;
                        }
                    }
                }
                uint4 *sp = reinterpret_cast<uint4 *>(s_col + tid * 8);
                sp[0] = make_uint4(lo[0], hi[0], lo[1], hi[1]);
                sp[1] = make_uint4(lo[2], hi[2], lo[3], hi[3]);
            }
            __syncthreads();
            if (tid < ncol) {
                uint32_t r = 0, g = 0, b = 0, al = 0;
                for (int sx = sx0; sx < sx1; sx++) {
                    const uint2 c = *reinterpret_cast<const uint2 *>(s_col + (sx - 4 * c0) * 2);
                    r += c.x & 0xffffu; b += c.x >> 16;
                    g += c.y & 0xffffu; al += c.y >> 16;
                }
                px = box_finish(r, g, b, al, (sy1 - sy0) * (sx1 - sx0));   // a downscale: every box is non-empty
            }
        }
        if (tid < ncol) s_px[j][tid] = px;
        __syncthreads();                                            // s_col is refilled by the next row
    }
    // lane = a pair of padded columns: 2 x 2 pixels -> 4 luma samples and one (Cb, Cr) pair, as jpeg_ycc_kernel
    if (2 * tid < ncol) {
        uint32_t ycc[2][2];
#pragma unroll
        for (int j = 0; j < 2; j++)
#pragma unroll
            for (int i = 0; i < 2; i++) ycc[j][i] = rgb_to_ycc(s_px[j < nrow ? j : 0][2 * tid + i]);
        const int dx = dx_lo + 2 * tid;
#pragma unroll
        for (int j = 0; j < 2; j++)
            *reinterpret_cast<uint16_t *>(a.yp + static_cast<size_t>(py + j) * a.ys + dx) =
                static_cast<uint16_t>((ycc[j][0] & 0xffu) | ((ycc[j][1] & 0xffu) << 8));
        const uint32_t sb = ((ycc[0][0] >> 8) & 0xffu) + ((ycc[0][1] >> 8) & 0xffu) + ((ycc[1][0] >> 8) & 0xffu) + ((ycc[1][1] >> 8) & 0xffu);
        const uint32_t sr = ((ycc[0][0] >> 16) & 0xffu) + ((ycc[0][1] >> 16) & 0xffu) + ((ycc[1][0] >> 16) & 0xffu) + ((ycc[1][1] >> 16) & 0xffu);
        a.cbp[static_cast<size_t>(py / 2) * a.cs + dx / 2] = static_cast<uint8_t>((sb + 2) >> 2);
        a.crp[static_cast<size_t>(py / 2) * a.cs + dx / 2] = static_cast<uint8_t>((sr + 2) >> 2);
    }
}

// ---- fdct.go (jfdctint.c's algorithm, 13-bit constants) and idct.go (Chen-Wang) on 8 values in registers ----
template <int PASS>
__device__ __forceinline__ void fdct8(int32_t &x0, int32_t &x1, int32_t &x2, int32_t &x3, int32_t &x4, int32_t &x5, int32_t &x6, int32_t &x7)
{
    constexpr int CB = 13, P1 = 2, SH = PASS == 1 ? CB - P1 : CB + P1;
    int32_t tmp0 = x0 + x7, tmp1 = x1 + x6, tmp2 = x2 + x5, tmp3 = x3 + x4;
    int32_t tmp10 = tmp0 + tmp3, tmp12 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp13 = tmp1 - tmp2;
    tmp0 = x0 - x7; tmp1 = x1 - x6; tmp2 = x2 - x5; tmp3 = x3 - x4;
    if (PASS == 1) {
        x0 = (tmp10 + tmp11 - 8 * 128) << P1;
        x4 = (tmp10 - tmp11) << P1;
    } else {
        tmp10 += 1 << (P1 - 1);
        x0 = (tmp10 + tmp11) >> P1;
        x4 = (tmp10 - tmp11) >> P1;
    }
    int32_t z1 = (tmp12 + tmp13) * 4433;
    z1 += 1 << (SH - 1);
    x2 = (z1 + tmp12 * 6270) >> SH;
    x6 = (z1 - tmp13 * 15137) >> SH;
    tmp10 = tmp0 + tmp3; tmp11 = tmp1 + tmp2; tmp12 = tmp0 + tmp2; tmp13 = tmp1 + tmp3;
    z1 = (tmp12 + tmp13) * 9633;
    z1 += 1 << (SH - 1);
    tmp0 *= 12299; tmp1 *= 25172; tmp2 *= 16819; tmp3 *= 2446;
    tmp10 *= -7373; tmp11 *= -20995; tmp12 *= -3196; tmp13 *= -16069;
    tmp12 += z1; tmp13 += z1;
    x1 = (tmp0 + tmp10 + tmp12) >> SH;
    x3 = (tmp1 + tmp11 + tmp13) >> SH;
    x5 = (tmp2 + tmp11 + tmp12) >> SH;
    x7 = (tmp3 + tmp10 + tmp13) >> SH;
}

struct BlockArgs {
    const uint8_t *in[3];     // Y, Cb, Cr planes before quantisation
    uint8_t *out[3];          // ... after the round trip
    int stride[3], nbx[3], nblocks[3];
    uint32_t q[2][64];        // quantiser steps, natural order: [0] luminance, [1] chrominance
    uint32_t magic[2][64];    // floor(2^32 / 8q) + 1: (|c| + 4q) / 8q by one v_mul_hi_u32 (|c| + 4q < 2^18, 8q <= 2040)
};

// one 8 x 8 block's round trip, all 64 samples in registers: no LDS, no transposes, no barriers.  q / magic: the plane's
// table (kernel arguments in jpeg_block_kernel, the per-ctx quality table in jpeg_block_batch_kernel)
template <typename QT>
__device__ __forceinline__ void jpeg_block_body(const uint8_t *ip, uint8_t *op, int stride, const QT *q_tab, const QT *magic_tab)
{
    int32_t b[64];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const u32x2 v = *reinterpret_cast<const u32x2 *>(ip + static_cast<size_t>(r) * stride);
#pragma unroll
        for (int c = 0; c < 8; c++) b[8 * r + c] = static_cast<int32_t>(((c < 4 ? v.x : v.y) >> (8 * (c & 3))) & 0xffu);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) fdct8<1>(b[8 * r], b[8 * r + 1], b[8 * r + 2], b[8 * r + 3], b[8 * r + 4], b[8 * r + 5], b[8 * r + 6], b[8 * r + 7]);
#pragma unroll
    for (int c = 0; c < 8; c++) fdct8<2>(b[c], b[8 + c], b[16 + c], b[24 + c], b[32 + c], b[40 + c], b[48 + c], b[56 + c]);
    // writer.go div(b, 8 * q) -- nearest, halves away from zero -- then reader.go's multiplication by q
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const int32_t q = static_cast<int32_t>(q_tab[k]);
        const uint32_t mag = static_cast<uint32_t>(b[k] < 0 ? -b[k] : b[k]) + 4u * static_cast<uint32_t>(q);
        const int32_t quot = static_cast<int32_t>(__umulhi(mag, magic_tab[k]));
        b[k] = (b[k] < 0 ? -quot : quot) * q;
    }
#pragma unroll
    for (int r = 0; r < 8; r++) idct8_row(b[8 * r], b[8 * r + 1], b[8 * r + 2], b[8 * r + 3], b[8 * r + 4], b[8 * r + 5], b[8 * r + 6], b[8 * r + 7]);
#pragma unroll
    for (int c = 0; c < 8; c++) idct8_col(b[c], b[8 + c], b[16 + c], b[24 + c], b[32 + c], b[40 + c], b[48 + c], b[56 + c]);
#pragma unroll
    for (int r = 0; r < 8; r++) {
        u32x2 v = {0, 0};
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int32_t s = b[8 * r + c];
            const uint32_t u = s < -128 ? 0u : (s > 127 ? 255u : static_cast<uint32_t>(s + 128));      // reader.go: level shift, clip
            if (c < 4) v.x |= u << (8 * c); else v.y |= u << (8 * (c - 4));
        }
        *reinterpret_cast<u32x2 *>(op + static_cast<size_t>(r) * stride) = v;
    }
}

// one lane = one 8 x 8 block
__global__ __launch_bounds__(256) void jpeg_block_kernel(BlockArgs a)
{
    const int plane = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nblocks[plane]) return;
    const int t = plane ? 1 : 0;
    const int by = i / a.nbx[plane], bx = i - by * a.nbx[plane];
    const int stride = a.stride[plane];
    const size_t o = static_cast<size_t>(8 * by) * stride + 8 * bx;
    jpeg_block_body(a.in[plane] + o, a.out[plane] + o, stride, a.q[t], a.magic[t]);
}

// The per-ctx quality table of the batched forms: for quality 1..100, [q][t][0][k] = the quantiser step, [q][t][1][k] = its
// magic -- exactly what launch_jpeg_blocks / quant_tables compute for one quality (JPEG_QTAB_WORDS, common.hpp)

// fnx_jpeg_compress_batch's search step: the candidate planes of every item still searching, each at its own quality.
// Job j = (image, quality): reads image's unquantised planes (orig + image * plane_bytes), writes job j's planes
// (work + j * plane_bytes).  Job = blockIdx.x / gx (jobs in x), plane = blockIdx.y.
struct BlockBatchArgs {
    const uint8_t *orig;
    uint8_t *work;
    size_t plane_bytes;
    size_t off[3];
    int stride[3], nbx[3], nblocks[3];
    const int2 *jobs;                 // [njobs] (image, quality)
    const uint32_t *qtab;             // JPEG_QTAB_WORDS
    int gx;
};

__global__ __launch_bounds__(256) void jpeg_block_batch_kernel(BlockBatchArgs a)
{
    const int plane = blockIdx.y;
    const int job = blockIdx.x / a.gx;
    const int i = (blockIdx.x - job * a.gx) * 256 + threadIdx.x;
    if (i >= a.nblocks[plane]) return;
    const int t = plane ? 1 : 0;
    const int2 jb = a.jobs[job];
    const int by = i / a.nbx[plane], bx = i - by * a.nbx[plane];
    const int stride = a.stride[plane];
    const size_t o = a.off[plane] + static_cast<size_t>(8 * by) * stride + 8 * bx;
    const uint32_t *qt = a.qtab + (static_cast<size_t>(jb.y) * 2 + t) * 128;
    jpeg_block_body(a.orig + static_cast<size_t>(jb.x) * a.plane_bytes + o, a.work + static_cast<size_t>(job) * a.plane_bytes + o, stride,
                    qt, qt + 64);
}

// writer.go, Encode: quality in [1, 100], scale = 5000 / q below 50, 200 - 2 q from 50, x = (x * scale + 50) / 100 in [1, 255]
static const uint8_t K1[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                               14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                               49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
static const uint8_t K2[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                               47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                               99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

void jpeg_plane_dims(int w, int h, int *ys, int *yh, int *cs, int *chh, int mode)
{
    int mx, my;
    jpeg_layout_dims(mode, w, h, ys, yh, cs, chh, &mx, &my);
}

// src (device NRGBA) -> the unquantised planes (quality-independent: once per source)
int launch_jpeg_ycc(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, uint8_t *yp, uint8_t *cbp, uint8_t *crp, int mode)
{
    if (mode == JPEG_444) {
        Ycc444Args b{};
        int cs, chh;
        jpeg_plane_dims(w, h, &b.ps, &b.ph, &cs, &chh, mode);
        b.src = src; b.sstride = sstride; b.w = w; b.h = h; b.yp = yp; b.cbp = cbp; b.crp = crp;
        hipLaunchKernelGGL(jpeg_ycc444_kernel, dim3((b.ps / 4 + 63) / 64, (b.ph / 2 + 3) / 4), dim3(256), 0, ctx->stream, b);
        FNX_HIP(hipGetLastError());
        note_route(ctx, FNX_PROF_JPEG, "jpeg_ycc444_kernel");
        return FNX_OK;
    }
    YccArgs a{};
    int yh, chh;
    jpeg_plane_dims(w, h, &a.ys, &yh, &a.cs, &chh);
    a.src = src; a.sstride = sstride; a.w = w; a.h = h; a.yp = yp; a.cbp = cbp; a.crp = crp; a.my = yh / 16;
    hipLaunchKernelGGL(jpeg_ycc_kernel, dim3((a.ys / 4 + 63) / 64, (yh / 2 + 3) / 4), dim3(256), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    return FNX_OK;
}

// the same from a decoded JPEG's planes (ratio: image.YCbCrSubsampleRatio), the NRGBA image in between never written
int launch_jpeg_ycc_planes(fnx_ctx *ctx, const uint8_t *dy, int dys, const uint8_t *dcb, const uint8_t *dcr, int dcs, int ratio, int w, int h,
                           uint8_t *yp, uint8_t *cbp, uint8_t *crp)
{
    static const int xs[6] = {0, 1, 1, 0, 2, 2}, ysh[6] = {0, 0, 1, 1, 0, 1};
    YccArgs a{};
    int yh, chh;
    jpeg_plane_dims(w, h, &a.ys, &yh, &a.cs, &chh);
    a.w = w; a.h = h; a.yp = yp; a.cbp = cbp; a.crp = crp; a.my = yh / 16;
    a.dy = dy; a.dcb = dcb; a.dcr = dcr; a.dys = dys; a.dcs = dcs; a.dxs = xs[ratio]; a.dysh = ysh[ratio];
    hipLaunchKernelGGL(jpeg_ycc_kernel, dim3((a.ys / 4 + 63) / 64, (yh / 2 + 3) / 4), dim3(256), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    return FNX_OK;
}

// src (device NRGBA, w x h) -> the unquantised planes of boxDownsample(src, dw, dh) (jpeg_box_ycc_kernel)
int launch_jpeg_box_ycc(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, int dw, int dh, uint8_t *yp, uint8_t *cbp,
                        uint8_t *crp)
{
    if (w <= 0 || h <= 0 || dw <= 0 || dh <= 0) {
        set_error("invalid argument: box-downsampled planes of a %d x %d image at %d x %d", w, h, dw, dh);
        return FNX_ERR_INVALID;
    }
    BoxYccJob a{};
    int yh, chh;
    jpeg_plane_dims(dw, dh, &a.ys, &yh, &a.cs, &chh);
    a.src = src; a.sstride = sstride; a.srcW = w; a.srcH = h; a.dw = dw; a.dh = dh;
    a.xRatio = static_cast<double>(w) / static_cast<double>(dw);   // ssim.go:251-252
    a.yRatio = static_cast<double>(h) / static_cast<double>(dh);
    a.yp = yp; a.cbp = cbp; a.crp = crp;
    a.vec_in = aligned16(src, sstride);
    // launch_box_downsample_pair's test for the column sums: boxes tile the source, fit 16-bit sums and one LDS row
    const bool tiled = w >= dw && h >= dh && a.yRatio + 1.0 < JB_MAXROWS && a.xRatio + 1.0 < JB_MAXROWS &&
                       a.xRatio * 2 + 8 < 4 * JB_CHUNKS;
    int seg = tiled ? static_cast<int>((4 * JB_CHUNKS - 8) / a.xRatio) : JB_SEG;
    seg = seg > JB_SEG ? JB_SEG : seg;
    seg &= ~1;                                                     // chroma pairs never straddle two workgroups
    a.seg = seg < 2 ? 2 : seg;
    const dim3 grid((dw + a.seg - 1) / a.seg, yh / 2);
    if (tiled) hipLaunchKernelGGL(jpeg_box_ycc_kernel<false>, grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(jpeg_box_ycc_kernel<true>, grid, dim3(256), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    return FNX_OK;
}

// the planes at `quality`: fdct, quantise, dequantise, idct of every block (in -> out; in == out is allowed)
int launch_jpeg_blocks(fnx_ctx *ctx, int w, int h, int quality, const uint8_t *const in[3], uint8_t *const out[3], int mode)
{
    BlockArgs a{};
    int ys, yh, cs, chh;
    jpeg_plane_dims(w, h, &ys, &yh, &cs, &chh, mode);
    if (quality < 1) quality = 1;
    if (quality > 100) quality = 100;
    const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 64; k++) {
            int x = (static_cast<int>(t ? K2[k] : K1[k]) * scale + 50) / 100;
            x = x < 1 ? 1 : (x > 255 ? 255 : x);
            a.q[t][k] = static_cast<uint32_t>(x);
            a.magic[t][k] = static_cast<uint32_t>((1ull << 32) / (8ull * x)) + 1u;
        }
    for (int p = 0; p < 3; p++) {
        a.in[p] = in[p]; a.out[p] = out[p];
        a.stride[p] = p ? cs : ys;
        a.nbx[p] = (p ? cs : ys) / 8;
        a.nblocks[p] = a.nbx[p] * ((p ? chh : yh) / 8);
    }
    FNX_TRY(prof_begin(ctx, FNX_PROF_JPEG));
    hipLaunchKernelGGL(jpeg_block_kernel, dim3((a.nblocks[0] + 255) / 256, 3), dim3(256), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    return prof_end(ctx);
}


// ------------------------------------------------------------------------------------
// Baseline entropy coding on the device -- SURVEY 8(f)2, second slice: jpeg.Encode's FILE (io.go:157-169) from a
// device-resident NRGBA image, so that CompressBatch needs the host codec only to decode its source.
//
// What writer.go does after the quantiser: zig-zag order, DC differences per component, (run, size) symbols with the
// typical Huffman tables of ITU T.81 Annex K.3.3 (writer.go's theHuffmanSpec), value bits, 0xff stuffing, 1-padding of
// the last byte, and the header segments in writer.go's order (SOI, one DQT with both tables, SOF0, one DHT with four
// tables, SOS; no APP0).  A JPEG scan is one long bit string, but a block's code depends on the rest of the image only
// through the previous block's DC and through its own position in the string:
//   1. jpeg_coef_kernel   lane = block: FDCT + quantiser, coefficients in zig-zag order, coefficient-major
//   2. jpeg_code_kernel   lane = block: the block's bits into a staging strip (<= 52 words), its bit count
//   3. prefix sum         of the bit counts (two launches) = every block's position in the string
//   4. jpeg_pack_kernel   lane = block: the strip shifted into place (atomicOr into zeroed words, MSB first)
//   5. stuffing           0xff bytes per word, prefix sum, every byte to its final place with 0x00 behind each 0xff
// The host writes the header (589 bytes) and the EOI marker.  All integer work: byte-for-byte against the CPU
// restatement the tests hold, which is itself checked against libjpeg-turbo where it can be and is
// otherwise -- like the quantiser path -- unpinned against Go.
// ------------------------------------------------------------------------------------
__device__ __constant__ uint8_t c_zigpos[64] = {          // zig-zag position of natural index k
    0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30, 41, 43, 9,  11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};
static const uint8_t UNZIG[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct CoefArgs {
    const uint8_t *in[3];     // Y, Cb, Cr planes (jpeg_ycc_kernel)
    int stride[3], nbx[3], nblocks[3];
    uint32_t q[2][64], magic[2][64];     // as BlockArgs
    int16_t *coef;            // [64][nblk]: coefficient zig of scan-order block b at zig * nblk + b
    int mx, nblk;
};

// lane = block (plane-major, so that loads coalesce); stores go to the block's place in SCAN order:
// MCU-major, Y0 Y1 Y2 Y3 Cb Cr (4:4:4: Y Cb Cr) inside an MCU (writer.go writeSOS; jpeg_layout.hpp).  in: the image's planes;
// base: its first block in the coefficient array (0 for one image)
template <int MODE>
__device__ __forceinline__ void jpeg_coef_body(const CoefArgs &a, const uint8_t *const in[3], int plane, int i, const uint32_t *q_tab,
                                               const uint32_t *magic_tab, int base)
{
    const int by = i / a.nbx[plane], bx = i - by * a.nbx[plane];
    const int stride = a.stride[plane];
    const uint8_t *ip = in[plane] + static_cast<size_t>(8 * by) * stride + 8 * bx;
    int32_t b[64];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const u32x2 v = *reinterpret_cast<const u32x2 *>(ip + static_cast<size_t>(r) * stride);
#pragma unroll
        for (int c = 0; c < 8; c++) b[8 * r + c] = static_cast<int32_t>(((c < 4 ? v.x : v.y) >> (8 * (c & 3))) & 0xffu);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) fdct8<1>(b[8 * r], b[8 * r + 1], b[8 * r + 2], b[8 * r + 3], b[8 * r + 4], b[8 * r + 5], b[8 * r + 6], b[8 * r + 7]);
#pragma unroll
    for (int c = 0; c < 8; c++) fdct8<2>(b[c], b[8 + c], b[16 + c], b[24 + c], b[32 + c], b[40 + c], b[48 + c], b[56 + c]);
    const int sb = base + jpeg_scan_index(MODE, a.mx, plane, bx, by);
#pragma unroll
    for (int k = 0; k < 64; k++) {
        const int32_t q = static_cast<int32_t>(q_tab[k]);
        const uint32_t mag = static_cast<uint32_t>(b[k] < 0 ? -b[k] : b[k]) + 4u * static_cast<uint32_t>(q);
        const int32_t quot = static_cast<int32_t>(__umulhi(mag, magic_tab[k]));     // writer.go div(b, 8 * q)
        a.coef[static_cast<size_t>(c_zigpos[k]) * a.nblk + sb] = static_cast<int16_t>(b[k] < 0 ? -quot : quot);
    }
}

template <int MODE>
__global__ __launch_bounds__(256) void jpeg_coef_kernel(CoefArgs a)
{
    const int plane = blockIdx.y;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nblocks[plane]) return;
    const int t = plane ? 1 : 0;
    jpeg_coef_body<MODE>(a, a.in, plane, i, a.q[t], a.magic[t], 0);
}

// the winners of fnx_jpeg_compress_batch: image = blockIdx.x / gx, its planes at planes + image * plane_bytes, its blocks at
// image * seg of ONE coefficient array (a.nblk = n * seg), its quality quality[image] (the per-ctx table)
struct CoefBatchArgs {
    CoefArgs one;                 // geometry, coef, nblk = all images' blocks (in / q / magic unused)
    const uint8_t *planes;
    size_t plane_bytes, off[3];
    const int *quality;           // [n]
    const uint32_t *qtab;         // JPEG_QTAB_WORDS
    int seg, gx;
};

__global__ __launch_bounds__(256) void jpeg_coef_batch_kernel(CoefBatchArgs b)
{
    const int plane = blockIdx.y;
    const int img = blockIdx.x / b.gx;
    const int i = (blockIdx.x - img * b.gx) * 256 + threadIdx.x;
    if (i >= b.one.nblocks[plane]) return;
    const int t = plane ? 1 : 0;
    const uint8_t *base = b.planes + static_cast<size_t>(img) * b.plane_bytes;
    const uint8_t *const in[3] = {base + b.off[0], base + b.off[1], base + b.off[2]};
    const uint32_t *qt = b.qtab + (static_cast<size_t>(b.quality[img]) * 2 + t) * 128;
    jpeg_coef_body<JPEG_420>(b.one, in, plane, i, qt, qt + 64, img * b.seg);
}

constexpr int JPEG_STRIP = 52;            // words per block's staging strip: 20 + 63 * 26 bits at most

struct CodeArgs {
    const int16_t *coef;
    const uint32_t *lut;      // [4][256] length << 24 | code: luminance DC, luminance AC, chrominance DC, chrominance AC
    uint32_t *strip;          // [JPEG_STRIP][nblk]
    uint32_t *nbits;          // [nblk]
    int nblk;
    int seg;                  // blocks per image, whole MCUs: the batched form's images lie back to back (one image: seg = nblk)
};

// PER_IMAGE: a.lut holds four tables for every image ([nblk / seg][4][256], jpeg_hufftab_kernel's), and a workgroup's blocks
// may belong to two images: each lane reads its own image's tables where they are
template <bool PER_IMAGE, int MODE>
__global__ __launch_bounds__(256) void jpeg_code_kernel(CodeArgs a)
{
    __shared__ uint32_t s_lut[PER_IMAGE ? 1 : 4 * 256];
    if (!PER_IMAGE) {
        for (int i = threadIdx.x; i < 4 * 256; i += 256) s_lut[i] = a.lut[i];
        __syncthreads();
    }
    const int blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= a.nblk) return;
    const int j = blk % jpeg_mcu_blocks(MODE);             // the block's place in its MCU (seg is a multiple of the MCU's blocks)
    const uint32_t *luts = PER_IMAGE ? a.lut + static_cast<size_t>(blk / a.seg) * (4 * 256) : s_lut;
    const uint32_t *dc_lut = luts + (jpeg_slot_class(MODE, j) ? 512 : 0), *ac_lut = dc_lut + 256;
    // the component's previous block in scan order
    const int prev = blk - jpeg_slot_prev(MODE, j);
    const int first = blk - blk % a.seg;                   // the image's first block
    const int32_t dc = a.coef[blk];
    const int32_t pd = prev >= first ? static_cast<int32_t>(a.coef[prev]) : 0;
    unsigned long long acc = 0;      // MSB-first bit accumulator: the low `nacc` bits are pending
    int nacc = 0, nw = 0;
    auto emit = [&](uint32_t bits, int n) {                // n <= 27
        acc = (acc << n) | bits;
        nacc += n;
        if (nacc >= 32) {
            a.strip[static_cast<size_t>(nw) * a.nblk + blk] = static_cast<uint32_t>(acc >> (nacc - 32));
            nw++;
            nacc -= 32;
        }
    };
    // emitHuffRLE: the (run, size) code, then `size` low bits of the value (value - 1 for negatives)
    auto rle = [&](const uint32_t *lut, int run, int32_t v) {
        const int32_t av = v < 0 ? -v : v, bv = v < 0 ? v - 1 : v;
        const int nb = 32 - __clz(av);                     // 0 for 0
        const uint32_t x = lut[(run << 4) | nb];
        const int len = static_cast<int>(x >> 24);
        emit(((x & 0x00ffffffu) << nb) | (static_cast<uint32_t>(bv) & ((1u << nb) - 1u)), len + nb);
    };
    rle(dc_lut, 0, dc - pd);
    int run = 0;
    for (int zig = 1; zig < 64; zig++) {
        const int32_t ac = a.coef[static_cast<size_t>(zig) * a.nblk + blk];
        if (ac == 0) {
            run++;
        } else {
            while (run > 15) {
                const uint32_t x = ac_lut[0xf0];
                emit(x & 0x00ffffffu, static_cast<int>(x >> 24));
                run -= 16;
            }
            rle(ac_lut, run, ac);
            run = 0;
        }
    }
    if (run > 0) {
        const uint32_t x = ac_lut[0x00];
        emit(x & 0x00ffffffu, static_cast<int>(x >> 24));
    }
    if (nacc > 0) a.strip[static_cast<size_t>(nw) * a.nblk + blk] = static_cast<uint32_t>(acc << (32 - nacc));   // left-aligned, zero tail
    a.nbits[blk] = static_cast<uint32_t>(32 * nw + nacc);
}

// ------------------------------------------------------------------------------------
// Optimised Huffman tables (fnx_ctx_set_jpeg_huffman(ctx, FNX_JPEG_HUFFMAN_OPTIMIZED)): the four tables of
// a file built from the symbols its own scan codes (T.81 Annex K.2), between the coefficient kernel and the code kernel,
// without the host:
//   jpeg_symhist_kernel   lane = block: the symbols jpeg_code_kernel will emit for it, counted into the workgroup's LDS
//                         histogram [4][256] (luminance DC, luminance AC, chrominance DC, chrominance AC), the non-zero bins
//                         added to the image's histogram (zeroed on the stream before)
//   jpeg_hufftab_kernel   one wave per (image, table): jpeg_hufftab.inc -- the code look-up words jpeg_code_kernel reads, and
//                         the table's record (counts and values of its DHT body, "standard table taken") for the host's header
// ------------------------------------------------------------------------------------
struct SymHistArgs {
    const int16_t *coef;      // jpeg_coef_kernel's
    uint32_t *hist;           // [images][4][256], zero
    int nblk;                 // blocks of all images
    int seg;                  // blocks per image (whole MCUs)
    int gx;                   // workgroups per image: image = blockIdx.x / gx
};

template <int MODE>
__global__ __launch_bounds__(256) void jpeg_symhist_kernel(SymHistArgs a)
{
    __shared__ uint32_t s_h[4 * 256];
    for (int i = threadIdx.x; i < 4 * 256; i += 256) s_h[i] = 0;
    __syncthreads();
    const int img = blockIdx.x / a.gx;
    const int i = (blockIdx.x - img * a.gx) * 256 + threadIdx.x;        // the block inside its image
    if (i < a.seg) {
        const int first = img * a.seg, blk = first + i;
        const int j = i % jpeg_mcu_blocks(MODE);
        uint32_t *dc_h = s_h + (jpeg_slot_class(MODE, j) ? 512 : 0), *ac_h = dc_h + 256;
        const int prev = blk - jpeg_slot_prev(MODE, j);                   // as jpeg_code_kernel
        const int32_t dc = a.coef[blk];
        const int32_t pd = prev >= first ? static_cast<int32_t>(a.coef[prev]) : 0;
        const int32_t d = dc - pd;
        atomicAdd(&dc_h[(32 - __clz(d < 0 ? -d : d)) & 255], 1u);
        int run = 0;
        for (int zig = 1; zig < 64; zig++) {
            const int32_t ac = a.coef[static_cast<size_t>(zig) * a.nblk + blk];
            if (ac == 0) {
                run++;
            } else {
                if (run > 15) {
                    atomicAdd(&ac_h[0xf0], static_cast<uint32_t>(run >> 4));
                    run &= 15;
                }
                atomicAdd(&ac_h[((run << 4) | (32 - __clz(ac < 0 ? -ac : ac))) & 255], 1u);
                run = 0;
            }
        }
        if (run > 0) atomicAdd(&ac_h[0x00], 1u);
    }
    __syncthreads();
    uint32_t *out = a.hist + static_cast<size_t>(img) * (4 * 256);
    for (int k = threadIdx.x; k < 4 * 256; k += 256) {
        const uint32_t v = s_h[k];
        if (v) atomicAdd(&out[k], v);
    }
}

// the wave's two smallest keys out of every lane's two (k1 <= k2): after the butterfly all 64 lanes hold them.  The lane sets
// that meet in a step are disjoint, so no key is counted twice; ~0 ("none") loses every comparison
__device__ __forceinline__ void ht_wave_min2(unsigned long long &k1, unsigned long long &k2)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o1 = __shfl_xor(k1, off, 64), o2 = __shfl_xor(k2, off, 64);
        const unsigned long long lo = k1 < o1 ? k1 : o1, hi = k1 < o1 ? o1 : k1;
        const unsigned long long m2 = k2 < o2 ? k2 : o2;
        k1 = lo;
        k2 = hi < m2 ? hi : m2;
    }
}

#define HT_FN __device__ __forceinline__
#define HT_UNROLL _Pragma("unroll")
#define HT_PHASE(call) { call; } __syncthreads();
#define HT_MIN2 ht_wave_min2(ln.k1, ln.k2)
#define HT_LANE0(field) ln.field
#define HT_ATOMIC_ADD(p, v) atomicAdd(p, v)
#define HT_ATOMIC_OR(p, v) atomicOr(p, v)
#define HT_RUN_PARAMS , HtLane &ln, int lane
#include "jpeg_hufftab.inc"

struct HuffTabArgs {
    const uint32_t *hist;     // [units][256]: unit = image * 4 + table
    uint32_t *lut;            // [units][256]
    uint32_t *rec;            // [units][HT_REC_WORDS] (host-mapped)
    const uint32_t *std_lut;  // [4][256] huffman_luts()
    const uint32_t *std_rec;  // [4][HT_REC_WORDS] huffman_std_recs()
};

__global__ __launch_bounds__(64) void jpeg_hufftab_kernel(HuffTabArgs a)
{
    __shared__ HtShared s;
    HtLane ln;
    const int u = blockIdx.x, t = u & 3;
    ht_run(a.hist + static_cast<size_t>(u) * 256, a.lut + static_cast<size_t>(u) * 256, a.rec + static_cast<size_t>(u) * HT_REC_WORDS,
           a.std_lut + t * 256, a.std_rec + t * HT_REC_WORDS, s, ln, static_cast<int>(threadIdx.x));
}

// ---- exclusive prefix sum of n uint32 into uint64: 2048 per workgroup, then the workgroups' totals ----
constexpr int SCAN_PER_WG = 2048;

__global__ __launch_bounds__(256) void scan_local_kernel(const uint32_t *in, unsigned long long *out, unsigned long long *totals, int n)
{
    __shared__ unsigned long long s_w[4];
    const int base = blockIdx.x * SCAN_PER_WG + threadIdx.x * 8;
    uint32_t v[8];
    unsigned long long sum = 0;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        v[e] = base + e < n ? in[base + e] : 0u;
        sum += v[e];
    }
    unsigned long long inc = sum;                           // inclusive scan of the lanes' sums inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long o = __shfl_up(inc, off, 64);
        if ((threadIdx.x & 63) >= off) inc += o;
    }
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = inc;
    __syncthreads();
    unsigned long long woff = 0;
    for (int w = 0; w < static_cast<int>(threadIdx.x >> 6); w++) woff += s_w[w];
    unsigned long long run = woff + inc - sum;
#pragma unroll
    for (int e = 0; e < 8; e++) {
        if (base + e < n) out[base + e] = run;
        run += v[e];
    }
    if (threadIdx.x == 255) totals[blockIdx.x] = woff + inc;
}

// out[i] += sum of the totals of the workgroups before i's; grand[0] = the sum of everything
__global__ __launch_bounds__(256) void scan_add_kernel(unsigned long long *out, const unsigned long long *totals, int n, unsigned long long *grand)
{
    // the totals before this workgroup's, summed by all 256 lanes (one lane walking up to ~100 of them was a chain of
    // dependent loads: 16 us per launch, four launches per JPEG item); integer sums, any order
    __shared__ unsigned long long s_part[4];
    unsigned long long mine = 0;
    for (int w = threadIdx.x; w < static_cast<int>(blockIdx.x); w += 256) mine += totals[w];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = mine;
    __syncthreads();
    const unsigned long long o = (s_part[0] + s_part[1]) + (s_part[2] + s_part[3]);
    if (threadIdx.x == 0 && blockIdx.x == gridDim.x - 1 && grand) grand[0] = o + totals[blockIdx.x];
    const int base = blockIdx.x * SCAN_PER_WG;
    for (int i = threadIdx.x; i < SCAN_PER_WG && base + i < n; i += 256) out[base + i] += o;
}

int launch_scan(fnx_ctx *ctx, const uint32_t *in, unsigned long long *out, unsigned long long *totals, int n, unsigned long long *grand)
{
    const int nwg = (n + SCAN_PER_WG - 1) / SCAN_PER_WG;
    hipLaunchKernelGGL(scan_local_kernel, dim3(nwg), dim3(256), 0, ctx->stream, in, out, totals, n);
    hipLaunchKernelGGL(scan_add_kernel, dim3(nwg), dim3(256), 0, ctx->stream, out, totals, n, grand);
    FNX_HIP(hipGetLastError());
    return FNX_OK;
}

struct PackArgs {
    const uint32_t *strip, *nbits;
    const unsigned long long *pos;     // bit position of every block
    uint32_t *bits;                    // the scan's bit string, 32 bits per word, MSB first; zeroed
    int nblk;
};

__global__ __launch_bounds__(256) void jpeg_pack_kernel(PackArgs a)
{
    const int blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= a.nblk) return;
    const unsigned long long p0 = a.pos[blk];
    const int nw = static_cast<int>((a.nbits[blk] + 31u) >> 5);
    const int s = static_cast<int>(p0 & 31u);
    size_t d = static_cast<size_t>(p0 >> 5);
    for (int k = 0; k < nw; k++, d++) {
        const uint32_t w = a.strip[static_cast<size_t>(k) * a.nblk + blk];
        atomicOr(&a.bits[d], w >> s);
        if (s) atomicOr(&a.bits[d + 1], w << (32 - s));
    }
}

struct StuffArgs {
    uint32_t *bits;                       // in: the bit string; the padding 1s are added here
    const unsigned long long *total;      // its length in bits
    uint32_t *ffcount;                    // [nwords] 0xff bytes per word (bytes past the end do not count)
    const unsigned long long *ffbefore;   // exclusive prefix sum of ffcount (second pass)
    uint8_t *out;                         // the entropy-coded segment
    int nwords;
};

__device__ __forceinline__ uint32_t padded_word(const StuffArgs &a, int i, unsigned long long tbits, int *nbytes)
{
    // writer.go: emit(0x7f, 7) -- the last byte's free bits become 1s; a byte-aligned string gets nothing
    const unsigned long long tb = (tbits + 7) >> 3;                   // bytes of the string
    uint32_t w = a.bits[i];
    const unsigned long long lo = static_cast<unsigned long long>(i) * 32;
    if (tbits > lo && tbits < lo + 32 && (tbits & 7u)) {
        const int used = static_cast<int>(tbits - lo);                // bits of this word that belong to the string
        const int upto = (used + 7) & ~7;                             // ... rounded up to the byte
        w |= (0xffffffffu >> used) & ~(upto == 32 ? 0u : (0xffffffffu >> upto));
    }
    const long long left = static_cast<long long>(tb) - static_cast<long long>(i) * 4;
    *nbytes = left >= 4 ? 4 : (left > 0 ? static_cast<int>(left) : 0);
    return w;
}

__global__ __launch_bounds__(256) void jpeg_ffcount_kernel(StuffArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nwords) return;
    int nb;
    const uint32_t w = padded_word(a, i, a.total[0], &nb);
    uint32_t c = 0;
    for (int k = 0; k < nb; k++) c += ((w >> (24 - 8 * k)) & 0xffu) == 0xffu ? 1u : 0u;
    a.ffcount[i] = c;
}

__global__ __launch_bounds__(256) void jpeg_stuff_kernel(StuffArgs a)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.nwords) return;
    int nb;
    const uint32_t w = padded_word(a, i, a.total[0], &nb);
    uint8_t *o = a.out + static_cast<size_t>(i) * 4 + a.ffbefore[i];
    for (int k = 0; k < nb; k++) {
        const uint8_t b = static_cast<uint8_t>(w >> (24 - 8 * k));
        *o++ = b;
        if (b == 0xffu) *o++ = 0x00;
    }
}

#include "jpeg_huffman_std.inc"

static void quant_tables(int quality, uint32_t (&q)[2][64], uint32_t (&magic)[2][64])
{
    if (quality < 1) quality = 1;
    if (quality > 100) quality = 100;
    const int scale = quality < 50 ? 5000 / quality : 200 - quality * 2;
    for (int t = 0; t < 2; t++)
        for (int k = 0; k < 64; k++) {
            int x = (static_cast<int>(t ? K2[k] : K1[k]) * scale + 50) / 100;
            x = x < 1 ? 1 : (x > 255 ? 255 : x);
            q[t][k] = static_cast<uint32_t>(x);
            magic[t][k] = static_cast<uint32_t>((1ull << 32) / (8ull * x)) + 1u;
        }
}

// the bytes jpeg.Encode writes before the entropy-coded segment.  rec: nullptr -- the four typical tables; else the four
// records jpeg_hufftab_kernel left (JPEG_HUFF_REC_WORDS each): still ONE DHT segment, the tables in the same order, each with
// the counts and the values of its record, 2 + sum(17 + values) bytes
void jpeg_header(int w, int h, int quality, std::vector<uint8_t> &o, const uint32_t *rec, int mode)
{
    uint32_t q[2][64], magic[2][64];
    quant_tables(quality, q, magic);
    auto marker = [&](uint8_t m, int len) { o.push_back(0xff); o.push_back(m); o.push_back(uint8_t(len >> 8)); o.push_back(uint8_t(len & 0xff)); };
    o.push_back(0xff); o.push_back(0xd8);
    marker(0xdb, 2 + 2 * (1 + 64));
    for (int t = 0; t < 2; t++) {
        o.push_back(uint8_t(t));
        for (int zig = 0; zig < 64; zig++) o.push_back(uint8_t(q[t][UNZIG[zig]]));
    }
    marker(0xc0, 8 + 3 * 3);
    o.push_back(8);
    o.push_back(uint8_t(h >> 8)); o.push_back(uint8_t(h & 0xff));
    o.push_back(uint8_t(w >> 8)); o.push_back(uint8_t(w & 0xff));
    o.push_back(3);
    const uint8_t comp[9] = {1, static_cast<uint8_t>(jpeg_y_sampling(mode)), 0, 2, 0x11, 1, 3, 0x11, 1};
    o.insert(o.end(), comp, comp + 9);
    auto nvals = [&](int t) { return !rec ? HNVAL[t] : (rec[t * HT_REC_WORDS] > 256u ? 256 : static_cast<int>(rec[t * HT_REC_WORDS])); };
    int dht = 2;
    for (int t = 0; t < 4; t++) dht += 1 + 16 + nvals(t);
    marker(0xc4, dht);
    const uint8_t tcth[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; t++) {
        o.push_back(tcth[t]);
        if (rec) {
            const uint8_t *body = reinterpret_cast<const uint8_t *>(rec + t * HT_REC_WORDS + 2);    // 16 counts, the values
            o.insert(o.end(), body, body + 16 + nvals(t));
            continue;
        }
        o.insert(o.end(), HCOUNT[t], HCOUNT[t] + 16);
        o.insert(o.end(), HVAL[t], HVAL[t] + HNVAL[t]);
    }
    const uint8_t sos[14] = {0xff, 0xda, 0x00, 0x0c, 0x03, 0x01, 0x00, 0x02, 0x11, 0x03, 0x11, 0x00, 0x3f, 0x00};
    o.insert(o.end(), sos, sos + 14);
}

static void huffman_luts(uint32_t *luts)        // [4][256]: length << 24 | code (canonical codes, T.81 Annex C)
{
    for (int t = 0; t < 4; t++) {
        uint32_t *lut = luts + 256 * t;
        for (int i = 0; i < 256; i++) lut[i] = 0;
        uint32_t code = 0;
        int k = 0;
        for (int len = 1; len <= 16; len++) {
            for (int j = 0; j < HCOUNT[t][len - 1]; j++) lut[HVAL[t][k++]] = (static_cast<uint32_t>(len) << 24) | code++;
            code <<= 1;
        }
    }
}

// The entropy-coded segment of jpeg.Encode(src, quality), in two steps with ONE small read-back between them (the
// length of the bit string decides how much the second step has to touch; sizing it for the worst case would scan
// 52 words per block instead of the ~3 a photograph needs):
//   jpeg_entropy_code   coefficients, per-block codes, their prefix sum; totals[0] (device) = bits of the string
//   jpeg_entropy_pack   (total_bits known on the host) the string packed, stuffed into `ecs`; totals[1] = 0xff bytes in it
// planes: jpeg_ycc_kernel's output.
static_assert(JPEG_HUFF_REC_WORDS == HT_REC_WORDS, "common.hpp's record size is jpeg_hufftab.inc's");

// the four standard tables as jpeg_hufftab_kernel's records (what it hands out for a table that took the standard one)
static void huffman_std_recs(uint32_t *recs)
{
    for (int t = 0; t < 4; t++) {
        uint32_t *rec = recs + t * HT_REC_WORDS;
        std::memset(rec, 0, sizeof(uint32_t) * HT_REC_WORDS);
        rec[0] = static_cast<uint32_t>(HNVAL[t]);
        uint8_t *body = reinterpret_cast<uint8_t *>(rec + 2);
        std::memcpy(body, HCOUNT[t], 16);
        std::memcpy(body + 16, HVAL[t], static_cast<size_t>(HNVAL[t]));
    }
}

// the standard tables on the device, for the tables that take them: [0] huffman_luts(), [1] huffman_std_recs()
static int upload_huffman_std(fnx_ctx *ctx, void **dp)
{
    uint32_t std_lut[4 * 256], std_rec[4 * HT_REC_WORDS];
    huffman_luts(std_lut);
    huffman_std_recs(std_rec);
    const void *hosts[2] = {std_lut, std_rec};
    const size_t sizes[2] = {sizeof(std_lut), sizeof(std_rec)};
    return upload_tables(ctx, SLOT_JPEG_HUFF_STD, hosts, sizes, 2, dp);
}

// jpeg_symhist_kernel over the blocks of `units / 4` images in `coef` (seg blocks each), then jpeg_hufftab_kernel: the tables'
// look-up words -> *d_lut ([units][256], device), their records -> rec (host-mapped, [units][JPEG_HUFF_REC_WORDS])
static int launch_jpeg_hufftabs(fnx_ctx *ctx, const int16_t *coef, int nimg, int seg, uint32_t *rec, const uint32_t **d_lut, int mode = JPEG_420)
{
    const size_t words = static_cast<size_t>(nimg) * 4 * 256;
    void *hs = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_HUFF, 2 * sizeof(uint32_t) * words, &hs));
    uint32_t *hist = static_cast<uint32_t *>(hs), *lut = hist + words;
    void *dp[2];
    FNX_TRY(upload_huffman_std(ctx, dp));
    FNX_HIP(hipMemsetAsync(hist, 0, sizeof(uint32_t) * words, ctx->stream));
    SymHistArgs sa{coef, hist, nimg * seg, seg, (seg + 255) / 256};
    if (mode == JPEG_444) hipLaunchKernelGGL(jpeg_symhist_kernel<JPEG_444>, dim3(sa.gx * nimg), dim3(256), 0, ctx->stream, sa);
    else hipLaunchKernelGGL(jpeg_symhist_kernel<JPEG_420>, dim3(sa.gx * nimg), dim3(256), 0, ctx->stream, sa);
    HuffTabArgs ha{hist, lut, rec, static_cast<const uint32_t *>(dp[0]), static_cast<const uint32_t *>(dp[1])};
    hipLaunchKernelGGL(jpeg_hufftab_kernel, dim3(4 * nimg), dim3(64), 0, ctx->stream, ha);
    FNX_HIP(hipGetLastError());
    *d_lut = lut;
    return FNX_OK;
}

// fnx_jpeg_huffman_tables: jpeg_hufftab_kernel on the caller's four histograms (host) -> lut [4][256], rec [4][JPEG_HUFF_REC_WORDS] (host)
int jpeg_huffman_tables_of(fnx_ctx *ctx, const uint32_t *hist, uint32_t *lut, uint32_t *rec)
{
    void *hs = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_HUFF, 2 * sizeof(uint32_t) * 4 * 256, &hs));
    uint32_t *d_hist = static_cast<uint32_t *>(hs), *d_lut = d_hist + 4 * 256;
    void *dp[2];
    FNX_TRY(upload_huffman_std(ctx, dp));
    void *pin = nullptr;
    FNX_TRY(pinned_alloc(ctx, sizeof(uint32_t) * 4 * (256 + HT_REC_WORDS), &pin));
    uint32_t *p_hist = static_cast<uint32_t *>(pin), *p_rec = p_hist + 4 * 256;
    std::memcpy(p_hist, hist, sizeof(uint32_t) * 4 * 256);
    std::memset(p_rec, 0xff, sizeof(uint32_t) * 4 * HT_REC_WORDS);
    FNX_HIP(hipMemcpyAsync(d_hist, p_hist, sizeof(uint32_t) * 4 * 256, hipMemcpyHostToDevice, ctx->stream));
    HuffTabArgs ha{d_hist, d_lut, p_rec, static_cast<const uint32_t *>(dp[0]), static_cast<const uint32_t *>(dp[1])};
    hipLaunchKernelGGL(jpeg_hufftab_kernel, dim3(4), dim3(64), 0, ctx->stream, ha);
    FNX_HIP(hipGetLastError());
    note_route(ctx, FNX_PROF_JPEG, "jpeg_hufftab_kernel");
    FNX_TRY(fetch_bytes(ctx, d_lut, lut, sizeof(uint32_t) * 4 * 256));
    std::memcpy(rec, p_rec, sizeof(uint32_t) * 4 * HT_REC_WORDS);
    return FNX_OK;
}

static void coef_args(int mode, int w, int h, int quality, const uint8_t *const planes[3], int16_t *coef, CoefArgs *ca)
{
    int ys, yh, cs, chh, mx, my;
    jpeg_layout_dims(mode, w, h, &ys, &yh, &cs, &chh, &mx, &my);
    quant_tables(quality, ca->q, ca->magic);
    for (int pl = 0; pl < 3; pl++) {
        ca->in[pl] = planes[pl];
        ca->stride[pl] = pl ? cs : ys;
        ca->nbx[pl] = (pl ? cs : ys) / 8;
        ca->nblocks[pl] = ca->nbx[pl] * ((pl ? chh : yh) / 8);
    }
    ca->coef = coef; ca->mx = mx; ca->nblk = jpeg_scan_blocks(mode, mx, my);
}

// blocks in the scan of a w x h image
static int scan_blocks(int mode, int w, int h)
{
    int ys, yh, cs, chh, mx, my;
    jpeg_layout_dims(mode, w, h, &ys, &yh, &cs, &chh, &mx, &my);
    return jpeg_scan_blocks(mode, mx, my);
}

static void launch_jpeg_coef(fnx_ctx *ctx, int mode, const CoefArgs &ca)
{
    const dim3 grid((ca.nblocks[0] + 255) / 256, 3);
    if (mode == JPEG_444) hipLaunchKernelGGL(jpeg_coef_kernel<JPEG_444>, grid, dim3(256), 0, ctx->stream, ca);
    else hipLaunchKernelGGL(jpeg_coef_kernel<JPEG_420>, grid, dim3(256), 0, ctx->stream, ca);
}

// fnx_jpeg_symbol_histogram: what jpeg_symhist_kernel counts for the image of `planes` at `quality` -> hist [4][256] (host)
int jpeg_symbol_hist_of(fnx_ctx *ctx, int w, int h, int quality, const uint8_t *const planes[3], uint32_t *hist, int mode)
{
    const int nblk = scan_blocks(mode, w, h);
    void *sc = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_ENC, sizeof(int16_t) * 64 * static_cast<size_t>(nblk) + 256, &sc));
    void *hs = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_HUFF, 2 * sizeof(uint32_t) * 4 * 256, &hs));
    CoefArgs ca{};
    coef_args(mode, w, h, quality, planes, static_cast<int16_t *>(sc), &ca);
    launch_jpeg_coef(ctx, mode, ca);
    FNX_HIP(hipMemsetAsync(hs, 0, sizeof(uint32_t) * 4 * 256, ctx->stream));
    SymHistArgs sa{ca.coef, static_cast<uint32_t *>(hs), nblk, nblk, (nblk + 255) / 256};
    if (mode == JPEG_444) hipLaunchKernelGGL(jpeg_symhist_kernel<JPEG_444>, dim3(sa.gx), dim3(256), 0, ctx->stream, sa);
    else hipLaunchKernelGGL(jpeg_symhist_kernel<JPEG_420>, dim3(sa.gx), dim3(256), 0, ctx->stream, sa);
    FNX_HIP(hipGetLastError());
    note_route(ctx, FNX_PROF_JPEG, "jpeg_symhist_kernel");
    return fetch_bytes(ctx, hs, hist, sizeof(uint32_t) * 4 * 256);
}

// rec: nullptr -- the typical tables (what the library always wrote); else host-mapped room for four records
// (JPEG_HUFF_REC_WORDS each): the tables are built from this image's symbols (launch_jpeg_hufftabs) and the records are there
// when totals[0] is
int jpeg_entropy_code(fnx_ctx *ctx, int w, int h, int quality, const uint8_t *const planes[3], unsigned long long *totals, uint32_t *rec,
                      int mode)
{
    const int nblk = scan_blocks(mode, w, h);
    const size_t strip_words = static_cast<size_t>(nblk) * JPEG_STRIP;
    auto al = [](size_t n) { return (n + 255) & ~size_t(255); };
    const size_t b_coef = al(sizeof(int16_t) * 64 * nblk), b_strip = al(4 * strip_words), b_nbits = al(4 * size_t(nblk)),
                 b_pos = al(8 * size_t(nblk)), b_tot = al(8 * (size_t(nblk) / SCAN_PER_WG + 2));
    void *sc = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_ENC, b_coef + b_strip + b_nbits + b_pos + b_tot, &sc));
    unsigned char *p = static_cast<unsigned char *>(sc);
    int16_t *coef = reinterpret_cast<int16_t *>(p); p += b_coef;
    uint32_t *strip = reinterpret_cast<uint32_t *>(p); p += b_strip;
    uint32_t *nbits = reinterpret_cast<uint32_t *>(p); p += b_nbits;
    unsigned long long *pos = reinterpret_cast<unsigned long long *>(p); p += b_pos;
    unsigned long long *wgt = reinterpret_cast<unsigned long long *>(p);
    void *dlut = nullptr;
    if (!rec) {
        uint32_t hlut[4 * 256];
        huffman_luts(hlut);
        FNX_TRY(upload_table(ctx, SLOT_JPEG_LUT, hlut, sizeof(hlut), &dlut));
    }

    CoefArgs ca{};
    coef_args(mode, w, h, quality, planes, coef, &ca);
    FNX_TRY(prof_begin(ctx, FNX_PROF_JPEG));
    launch_jpeg_coef(ctx, mode, ca);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    const uint32_t *lut = static_cast<const uint32_t *>(dlut);
    if (rec) FNX_TRY(launch_jpeg_hufftabs(ctx, coef, 1, nblk, rec, &lut, mode));
    CodeArgs co{coef, lut, strip, nbits, nblk, nblk};
    if (mode == JPEG_444) hipLaunchKernelGGL((jpeg_code_kernel<false, JPEG_444>), dim3((nblk + 255) / 256), dim3(256), 0, ctx->stream, co);
    else hipLaunchKernelGGL((jpeg_code_kernel<false, JPEG_420>), dim3((nblk + 255) / 256), dim3(256), 0, ctx->stream, co);
    FNX_HIP(hipGetLastError());
    return launch_scan(ctx, nbits, pos, wgt, nblk, totals);
}

size_t jpeg_ecs_capacity(unsigned long long total_bits)
{
    return static_cast<size_t>((total_bits + 7) / 8) * 2 + 64;        // every byte could be 0xff
}

int jpeg_entropy_pack(fnx_ctx *ctx, int w, int h, unsigned long long total_bits, uint8_t *ecs, unsigned long long *totals, int mode)
{
    const int nblk = scan_blocks(mode, w, h);
    const size_t strip_words = static_cast<size_t>(nblk) * JPEG_STRIP;
    auto al = [](size_t n) { return (n + 255) & ~size_t(255); };
    // phase-1 layout again (same slot, same sizes: nothing moves)
    const size_t b_coef = al(sizeof(int16_t) * 64 * nblk), b_strip = al(4 * strip_words), b_nbits = al(4 * size_t(nblk));
    void *sc = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_ENC, b_coef + b_strip + b_nbits + al(8 * size_t(nblk)) + al(8 * (size_t(nblk) / SCAN_PER_WG + 2)), &sc));
    unsigned char *p = static_cast<unsigned char *>(sc) + b_coef;
    const uint32_t *strip = reinterpret_cast<const uint32_t *>(p); p += b_strip;
    const uint32_t *nbits = reinterpret_cast<const uint32_t *>(p); p += b_nbits;
    const unsigned long long *pos = reinterpret_cast<const unsigned long long *>(p);
    const size_t nw = static_cast<size_t>((total_bits + 31) / 32);
    if (nw > strip_words || nw >= (size_t(1) << 31)) {
        set_error("jpeg: bit string of %llu bits does not fit its blocks' strips", total_bits);
        return FNX_ERR_INVALID;
    }
    const int nwords = static_cast<int>(nw);
    const size_t b_bits = al(4 * (nw + 2)), b_ffc = al(4 * nw + 4), b_ffb = al(8 * nw + 8), b_tot = al(8 * (nw / SCAN_PER_WG + 2));
    void *s2 = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_ENC2, b_bits + b_ffc + b_ffb + b_tot, &s2));
    p = static_cast<unsigned char *>(s2);
    uint32_t *bits = reinterpret_cast<uint32_t *>(p); p += b_bits;
    uint32_t *ffc = reinterpret_cast<uint32_t *>(p); p += b_ffc;
    unsigned long long *ffb = reinterpret_cast<unsigned long long *>(p); p += b_ffb;
    unsigned long long *wgt = reinterpret_cast<unsigned long long *>(p);
    FNX_HIP(hipMemsetAsync(bits, 0, 4 * (nw + 2), ctx->stream));
    PackArgs pa{strip, nbits, pos, bits, nblk};
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((nblk + 255) / 256), dim3(256), 0, ctx->stream, pa);
    if (nwords > 0) {
        StuffArgs sa{bits, totals, ffc, ffb, ecs, nwords};
        hipLaunchKernelGGL(jpeg_ffcount_kernel, dim3((nwords + 255) / 256), dim3(256), 0, ctx->stream, sa);
        FNX_TRY(launch_scan(ctx, ffc, ffb, wgt, nwords, totals + 1));
        hipLaunchKernelGGL(jpeg_stuff_kernel, dim3((nwords + 255) / 256), dim3(256), 0, ctx->stream, sa);
    }
    FNX_HIP(hipGetLastError());
    note_route(ctx, FNX_PROF_JPEG, "jpeg_pack_kernel");
    return FNX_OK;
}

// ---- the size of the file without its bytes: the 0xff bytes of the string, counted from the strips ----
// A size query needs (bits + 7) / 8 + the number of stuffed bytes, and the second term can be had without the packed string:
// lane = block counts the bytes whose first bit lies in its block (jpeg_ffcount_strips.inc: the ownership rule), the wave
// adds its lanes' counts up and adds the sum to `total` (integer sums: the order does not matter); jpeg_ffcount_finish_kernel,
// the next launch on the stream, hands the total to the host's pinned slot and puts `total` back to zero for the next query.
// (A hand-over by the workgroup that finishes last needs a device-scope fence per workgroup, and on this part each of them
// writes back the L2 the coder's kernels have just filled: ~45 us of a 4K query, measured.  A launch boundary orders the same
// for ~5 us.)
struct FfStripArgs {
    const uint32_t *strip, *nbits;
    const unsigned long long *pos;
    unsigned long long *total;         // device, zero between queries
    int nblk;
};

__global__ __launch_bounds__(256) void jpeg_ffcount_strips_kernel(FfStripArgs a)
{
    const int blk = blockIdx.x * 256 + threadIdx.x;
    uint32_t count = 0;
    if (blk < a.nblk) {
        const uint32_t *strip = a.strip, *nbits = a.nbits;
        const unsigned long long *pos = a.pos;
        const int nblk = a.nblk;
#include "jpeg_ffcount_strips.inc"
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_down(count, off, 64);
    if ((threadIdx.x & 63) == 0 && count) atomicAdd(a.total, static_cast<unsigned long long>(count));
}

__global__ __launch_bounds__(64) void jpeg_ffcount_finish_kernel(unsigned long long *total, unsigned long long *out)
{
    if (threadIdx.x == 0) out[0] = atomicExch(total, 0ull);
}

int jpeg_entropy_ffcount(fnx_ctx *ctx, int w, int h, unsigned long long *totals, int mode)
{
    const int nblk = scan_blocks(mode, w, h);
    auto al = [](size_t n) { return (n + 255) & ~size_t(255); };
    // jpeg_entropy_code's layout (same slot, same sizes: nothing moves)
    const size_t b_coef = al(sizeof(int16_t) * 64 * nblk), b_strip = al(4 * static_cast<size_t>(nblk) * JPEG_STRIP), b_nbits = al(4 * size_t(nblk));
    void *sc = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_ENC, b_coef + b_strip + b_nbits + al(8 * size_t(nblk)) + al(8 * (size_t(nblk) / SCAN_PER_WG + 2)), &sc));
    unsigned char *p = static_cast<unsigned char *>(sc) + b_coef;
    const uint32_t *strip = reinterpret_cast<const uint32_t *>(p); p += b_strip;
    const uint32_t *nbits = reinterpret_cast<const uint32_t *>(p); p += b_nbits;
    const unsigned long long *pos = reinterpret_cast<const unsigned long long *>(p);
    const void *before = ctx->slot[SLOT_JPEG_FF].p;
    void *ff = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_FF, 16, &ff));
    if (ff != before) FNX_HIP(hipMemsetAsync(ff, 0, 16, ctx->stream));      // first use: the finish kernel keeps it zero from here on
    FfStripArgs fa{strip, nbits, pos, static_cast<unsigned long long *>(ff), nblk};
    hipLaunchKernelGGL(jpeg_ffcount_strips_kernel, dim3((nblk + 255) / 256), dim3(256), 0, ctx->stream, fa);
    hipLaunchKernelGGL(jpeg_ffcount_finish_kernel, dim3(1), dim3(64), 0, ctx->stream, fa.total, totals + 1);
    FNX_HIP(hipGetLastError());
    note_route(ctx, FNX_PROF_JPEG, "jpeg_ffcount_strips_kernel");
    return FNX_OK;
}

// ------------------------------------------------------------------------------------
// Batched forms of the above (fnx_jpeg_compress_batch): n images of ONE geometry.  Every kernel puts the image index in
// x (blockIdx.x = image * gx + workgroup), so no grid dimension is the image count times anything but x; each image's
// arithmetic is the single-image kernel's body.
// ------------------------------------------------------------------------------------
void jpeg_qtab(uint32_t *tab)                     // JPEG_QTAB_WORDS: see jpeg_block_batch_kernel
{
    for (int q = 0; q <= 100; q++) {
        uint32_t qq[2][64], mm[2][64];
        quant_tables(q, qq, mm);
        for (int t = 0; t < 2; t++)
            for (int k = 0; k < 64; k++) {
                tab[(q * 2 + t) * 128 + k] = qq[t][k];
                tab[(q * 2 + t) * 128 + 64 + k] = mm[t][k];
            }
    }
}

// item i's Y | Cb | Cr planes at base + i * jpeg_batch_plane_bytes(): jpeg_planes' layout, 256-byte aligned per item
size_t jpeg_batch_plane_bytes(int w, int h, size_t *cb_off, size_t *cr_off)
{
    int ys, yh, cs, chh;
    jpeg_plane_dims(w, h, &ys, &yh, &cs, &chh);
    const size_t yb = static_cast<size_t>(ys) * yh, cb = static_cast<size_t>(cs) * chh;
    if (cb_off) *cb_off = yb;
    if (cr_off) *cr_off = yb + cb;
    return (yb + 2 * cb + 16 + 255) & ~size_t(255);
}

int launch_jpeg_ycc_batch(fnx_ctx *ctx, int n, const uint8_t *const *d_srcs, int sstride, int w, int h, uint8_t *planes)
{
    YccBatchArgs b{};
    int yh, chh;
    jpeg_plane_dims(w, h, &b.one.ys, &yh, &b.one.cs, &chh);
    b.one.sstride = sstride; b.one.w = w; b.one.h = h; b.one.my = yh / 16;
    b.srcs = d_srcs; b.planes = planes;
    b.plane_bytes = jpeg_batch_plane_bytes(w, h, &b.cb_off, &b.cr_off);
    b.gx = (b.one.ys / 4 + 63) / 64;
    hipLaunchKernelGGL(jpeg_ycc_batch_kernel, dim3(b.gx * n, (yh / 2 + 3) / 4), dim3(256), 0, ctx->stream, b);
    FNX_HIP(hipGetLastError());
    return FNX_OK;
}

// d_jobs: [njobs] (image, quality) device; job j's planes at work + j * plane bytes
int launch_jpeg_blocks_batch(fnx_ctx *ctx, int njobs, int w, int h, const uint8_t *orig, uint8_t *work, const int2 *d_jobs,
                             const uint32_t *d_qtab)
{
    BlockBatchArgs a{};
    int ys, yh, cs, chh;
    jpeg_plane_dims(w, h, &ys, &yh, &cs, &chh);
    a.orig = orig; a.work = work; a.jobs = d_jobs; a.qtab = d_qtab;
    a.plane_bytes = jpeg_batch_plane_bytes(w, h, &a.off[1], &a.off[2]);
    a.off[0] = 0;
    for (int p = 0; p < 3; p++) {
        a.stride[p] = p ? cs : ys;
        a.nbx[p] = (p ? cs : ys) / 8;
        a.nblocks[p] = a.nbx[p] * ((p ? chh : yh) / 8);
    }
    a.gx = (a.nblocks[0] + 255) / 256;
    FNX_TRY(prof_begin(ctx, FNX_PROF_JPEG));
    hipLaunchKernelGGL(jpeg_block_batch_kernel, dim3(a.gx * njobs, 3), dim3(256), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    return prof_end(ctx);
}

// n images' w x h sources -> tight w x h copies at dst + i * dst_bytes (the prepared reference of a search that does not
// downsample: against_device's side `a` is tight).  Workgroup = one row of one image.
__global__ __launch_bounds__(256) void copy_tight_batch_kernel(const uint8_t *const *srcs, int sstride, int w, int h, uint8_t *dst,
                                                               size_t dst_bytes)
{
    const int img = blockIdx.x / h, y = blockIdx.x - img * h;
    const uint8_t *s = srcs[img] + static_cast<size_t>(y) * sstride;
    uint8_t *d = dst + static_cast<size_t>(img) * dst_bytes + static_cast<size_t>(y) * w * 4;
    for (int x = threadIdx.x; x < w; x += 256) *reinterpret_cast<uint32_t *>(d + 4 * static_cast<size_t>(x)) = ld_px(s, x);
}

int launch_copy_tight_batch(fnx_ctx *ctx, int n, const uint8_t *const *d_srcs, int sstride, int w, int h, uint8_t *dst, size_t dst_bytes)
{
    hipLaunchKernelGGL(copy_tight_batch_kernel, dim3(n * h), dim3(256), 0, ctx->stream, d_srcs, sstride, w, h, dst, dst_bytes);
    FNX_HIP(hipGetLastError());
    return FNX_OK;
}

// ---- entropy coding of n winners: the blocks of all images in one array (image i's at i * seg, seg = its block count), ONE
// prefix sum over all of them, each image's positions relative to its first block (a segmented sum by subtraction: integer,
// any order).  The bit strings are per image (word base wbase[i]), stuffed into per-image ranges of one ECS buffer.
struct PackItem {
    unsigned long long wbase;     // first word of the image's bit string (nw + 2 words: the pack kernel's overhang, a zero count)
    unsigned long long ecs;       // first byte of its entropy-coded segment
    unsigned long long tbits;     // bits of its string
    int nw, pad;
};

// out[i] = the bits of image i's string (pos is exclusive: the last block's position + its count - the first block's position)
__global__ __launch_bounds__(256) void seg_bits_kernel(const unsigned long long *pos, const uint32_t *nbits, int seg, int n,
                                                       unsigned long long *out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t last = static_cast<size_t>(i + 1) * seg - 1;
    out[i] = pos[last] + nbits[last] - pos[static_cast<size_t>(i) * seg];
}

struct PackBatchArgs {
    const uint32_t *strip, *nbits;
    const unsigned long long *pos;
    uint32_t *bits;
    const PackItem *item;
    int nblk, seg;
};

__global__ __launch_bounds__(256) void jpeg_pack_batch_kernel(PackBatchArgs a)
{
    const int blk = blockIdx.x * 256 + threadIdx.x;
    if (blk >= a.nblk) return;
    const int img = blk / a.seg;
    const unsigned long long p0 = a.pos[blk] - a.pos[static_cast<size_t>(img) * a.seg];
    const int nw = static_cast<int>((a.nbits[blk] + 31u) >> 5);
    const int s = static_cast<int>(p0 & 31u);
    uint32_t *bits = a.bits + a.item[img].wbase;
    size_t d = static_cast<size_t>(p0 >> 5);
    for (int k = 0; k < nw; k++, d++) {
        const uint32_t w = a.strip[static_cast<size_t>(k) * a.nblk + blk];
        atomicOr(&bits[d], w >> s);
        if (s) atomicOr(&bits[d + 1], w << (32 - s));
    }
}

struct StuffBatchArgs {
    uint32_t *bits;
    const PackItem *item;
    uint32_t *ffcount;                    // one array over every image's words (+ 2 zero words each)
    const unsigned long long *ffbefore;   // its exclusive prefix sum
    uint8_t *ecs;
    unsigned long long *fftot;            // [n] 0xff bytes of image i's string
    int gx;
};

__global__ __launch_bounds__(256) void jpeg_ffcount_batch_kernel(StuffBatchArgs b)
{
    const int img = blockIdx.x / b.gx;
    const int k = (blockIdx.x - img * b.gx) * 256 + threadIdx.x;
    const PackItem it = b.item[img];
    if (k >= it.nw + 2) return;
    uint32_t c = 0;
    if (k < it.nw) {
        StuffArgs a{};
        a.bits = b.bits + it.wbase;
        int nb;
        const uint32_t w = padded_word(a, k, it.tbits, &nb);
        for (int e = 0; e < nb; e++) c += ((w >> (24 - 8 * e)) & 0xffu) == 0xffu ? 1u : 0u;
    }
    b.ffcount[it.wbase + k] = c;
}

__global__ __launch_bounds__(256) void jpeg_stuff_batch_kernel(StuffBatchArgs b)
{
    const int img = blockIdx.x / b.gx;
    const int k = (blockIdx.x - img * b.gx) * 256 + threadIdx.x;
    const PackItem it = b.item[img];
    if (k == 0) b.fftot[img] = b.ffbefore[it.wbase + it.nw] - b.ffbefore[it.wbase];
    if (k >= it.nw) return;
    StuffArgs a{};
    a.bits = b.bits + it.wbase;
    int nb;
    const uint32_t w = padded_word(a, k, it.tbits, &nb);
    uint8_t *o = b.ecs + it.ecs + static_cast<size_t>(k) * 4 + (b.ffbefore[it.wbase + k] - b.ffbefore[it.wbase]);
    for (int e = 0; e < nb; e++) {
        const uint8_t v = static_cast<uint8_t>(w >> (24 - 8 * e));
        *o++ = v;
        if (v == 0xffu) *o++ = 0x00;
    }
}

static void entropy_batch_layout(int n, int w, int h, int *seg, size_t *sizes)
{
    *seg = scan_blocks(JPEG_420, w, h);
    const size_t nblk = static_cast<size_t>(n) * *seg;
    auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
    sizes[0] = al(sizeof(int16_t) * 64 * nblk);
    sizes[1] = al(4 * nblk * JPEG_STRIP);
    sizes[2] = al(4 * nblk);
    sizes[3] = al(8 * nblk);
    sizes[4] = al(8 * (nblk / SCAN_PER_WG + 2));
}

// device bytes per image of phase 1 (fnx_jpeg_compress_batch's chunking)
size_t jpeg_entropy_batch_bytes(int w, int h)
{
    int seg;
    size_t sz[5];
    entropy_batch_layout(1, w, h, &seg, sz);
    return static_cast<size_t>(seg) * (2 * 64 + 4 * JPEG_STRIP + 4 + 8) + 256;
}

// phase 1 of n images: coefficients at quality[i] (device [n]), codes, positions; tot[i] (host-mapped, n) = bits of image i
// rec: nullptr, or host-mapped room for every image's four records ([n][4][JPEG_HUFF_REC_WORDS]): tables per image
int jpeg_entropy_code_batch(fnx_ctx *ctx, int n, int w, int h, const uint8_t *planes, const int *d_quality, const uint32_t *d_qtab,
                            unsigned long long *tot, uint32_t *rec)
{
    int seg;
    size_t sz[5];
    entropy_batch_layout(n, w, h, &seg, sz);
    const long long nblk_ll = static_cast<long long>(n) * seg;
    if (nblk_ll >= (1LL << 31) / JPEG_STRIP) {
        set_error("jpeg batch: %lld blocks in one entropy pass", nblk_ll);
        return FNX_ERR_INVALID;
    }
    const int nblk = static_cast<int>(nblk_ll);
    void *sc = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_ENC, sz[0] + sz[1] + sz[2] + sz[3] + sz[4], &sc));
    unsigned char *p = static_cast<unsigned char *>(sc);
    int16_t *coef = reinterpret_cast<int16_t *>(p); p += sz[0];
    uint32_t *strip = reinterpret_cast<uint32_t *>(p); p += sz[1];
    uint32_t *nbits = reinterpret_cast<uint32_t *>(p); p += sz[2];
    unsigned long long *pos = reinterpret_cast<unsigned long long *>(p); p += sz[3];
    unsigned long long *wgt = reinterpret_cast<unsigned long long *>(p);
    void *dlut = nullptr;
    if (!rec) {
        uint32_t hlut[4 * 256];
        huffman_luts(hlut);
        FNX_TRY(upload_table(ctx, SLOT_JPEG_LUT, hlut, sizeof(hlut), &dlut));
    }

    CoefBatchArgs cb{};
    int ys, yh, cs, chh;
    jpeg_plane_dims(w, h, &ys, &yh, &cs, &chh);
    for (int pl = 0; pl < 3; pl++) {
        cb.one.stride[pl] = pl ? cs : ys;
        cb.one.nbx[pl] = (pl ? cs : ys) / 8;
        cb.one.nblocks[pl] = cb.one.nbx[pl] * ((pl ? chh : yh) / 8);
    }
    cb.one.coef = coef; cb.one.mx = ys / jpeg_mcu_px(JPEG_420); cb.one.nblk = nblk;
    cb.planes = planes;
    cb.plane_bytes = jpeg_batch_plane_bytes(w, h, &cb.off[1], &cb.off[2]);
    cb.off[0] = 0;
    cb.quality = d_quality; cb.qtab = d_qtab; cb.seg = seg;
    cb.gx = (cb.one.nblocks[0] + 255) / 256;
    FNX_TRY(prof_begin(ctx, FNX_PROF_JPEG));
    hipLaunchKernelGGL(jpeg_coef_batch_kernel, dim3(cb.gx * n, 3), dim3(256), 0, ctx->stream, cb);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    const uint32_t *lut = static_cast<const uint32_t *>(dlut);
    if (rec) FNX_TRY(launch_jpeg_hufftabs(ctx, coef, n, seg, rec, &lut));
    CodeArgs co{coef, lut, strip, nbits, nblk, seg};
    if (rec) hipLaunchKernelGGL((jpeg_code_kernel<true, JPEG_420>), dim3((nblk + 255) / 256), dim3(256), 0, ctx->stream, co);
    else hipLaunchKernelGGL((jpeg_code_kernel<false, JPEG_420>), dim3((nblk + 255) / 256), dim3(256), 0, ctx->stream, co);
    FNX_HIP(hipGetLastError());
    FNX_TRY(launch_scan(ctx, nbits, pos, wgt, nblk, nullptr));
    hipLaunchKernelGGL(seg_bits_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, pos, nbits, seg, n, tot);
    FNX_HIP(hipGetLastError());
    return FNX_OK;
}

// phase 2: tbits[i] (host) known; image i's entropy-coded segment goes to *ecs + ecs_off[i] (ecs_off: host, filled here);
// fftot[i] (host-mapped) = its 0xff bytes
int jpeg_entropy_pack_batch(fnx_ctx *ctx, int n, int w, int h, const unsigned long long *tbits, uint8_t **ecs, size_t *ecs_off,
                            unsigned long long *fftot)
{
    int seg;
    size_t sz[5];
    entropy_batch_layout(n, w, h, &seg, sz);
    const int nblk = n * seg;
    void *sc = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_ENC, sz[0] + sz[1] + sz[2] + sz[3] + sz[4], &sc));   // phase 1's layout: nothing moves
    unsigned char *p = static_cast<unsigned char *>(sc) + sz[0];
    const uint32_t *strip = reinterpret_cast<const uint32_t *>(p); p += sz[1];
    const uint32_t *nbits = reinterpret_cast<const uint32_t *>(p); p += sz[2];
    const unsigned long long *pos = reinterpret_cast<const unsigned long long *>(p);
    std::vector<PackItem> items(n);
    size_t words = 0, bytes = 0;
    int maxw = 0;
    for (int i = 0; i < n; i++) {
        const size_t nw = static_cast<size_t>((tbits[i] + 31) / 32);
        if (nw > static_cast<size_t>(seg) * JPEG_STRIP) {
            set_error("jpeg: bit string of %llu bits does not fit its blocks' strips", tbits[i]);
            return FNX_ERR_INVALID;
        }
        items[i].wbase = words;
        items[i].ecs = bytes;
        items[i].tbits = tbits[i];
        items[i].nw = static_cast<int>(nw);
        words += nw + 2;
        bytes += (jpeg_ecs_capacity(tbits[i]) + 15) & ~size_t(15);
        maxw = static_cast<int>(nw) + 2 > maxw ? static_cast<int>(nw) + 2 : maxw;
        ecs_off[i] = items[i].ecs;
    }
    if (words >= (size_t(1) << 31)) {
        set_error("jpeg batch: %zu words of bit strings in one pass", words);
        return FNX_ERR_INVALID;
    }
    void *ditems = nullptr;
    FNX_TRY(upload_table(ctx, SLOT_PTRS, items.data(), sizeof(PackItem) * n, &ditems));
    auto al = [](size_t v) { return (v + 255) & ~size_t(255); };
    const size_t b_bits = al(4 * words), b_ffc = al(4 * words), b_ffb = al(8 * words), b_tot = al(8 * (words / SCAN_PER_WG + 2));
    void *s2 = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_ENC2, b_bits + b_ffc + b_ffb + b_tot, &s2));
    p = static_cast<unsigned char *>(s2);
    uint32_t *bits = reinterpret_cast<uint32_t *>(p); p += b_bits;
    uint32_t *ffc = reinterpret_cast<uint32_t *>(p); p += b_ffc;
    unsigned long long *ffb = reinterpret_cast<unsigned long long *>(p); p += b_ffb;
    unsigned long long *wgt = reinterpret_cast<unsigned long long *>(p);
    void *dec = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_ECS, bytes + 64, &dec));
    *ecs = static_cast<uint8_t *>(dec);
    FNX_HIP(hipMemsetAsync(bits, 0, 4 * words, ctx->stream));
    const PackItem *it = static_cast<const PackItem *>(ditems);
    PackBatchArgs pa{strip, nbits, pos, bits, it, nblk, seg};
    hipLaunchKernelGGL(jpeg_pack_batch_kernel, dim3((nblk + 255) / 256), dim3(256), 0, ctx->stream, pa);
    FNX_HIP(hipGetLastError());
    StuffBatchArgs sb{bits, it, ffc, ffb, *ecs, fftot, (maxw + 255) / 256};
    hipLaunchKernelGGL(jpeg_ffcount_batch_kernel, dim3(sb.gx * n), dim3(256), 0, ctx->stream, sb);
    FNX_HIP(hipGetLastError());
    FNX_TRY(launch_scan(ctx, ffc, ffb, wgt, static_cast<int>(words), nullptr));
    hipLaunchKernelGGL(jpeg_stuff_batch_kernel, dim3(sb.gx * n), dim3(256), 0, ctx->stream, sb);
    FNX_HIP(hipGetLastError());
    return FNX_OK;
}

}  // namespace fnx
