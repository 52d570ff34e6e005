// Baseline JPEG decoding on the device -- SURVEY 8(f)2, third slice: image.Decode of CompressBatch's SOURCE
// (batch.go:88-101 -> io.go:60-95) without the host codec, so that a JPEG crosses PCIe as its file bytes and the
// quality search (jpeg.hip) starts from pixels that never left the GPU.
//
// A scan is one long Huffman-coded bit string: where a symbol starts depends on every symbol before it.  What makes it
// parallel is that Huffman codes SELF-SYNCHRONISE: a decoder started at a wrong bit falls into step with the right one
// after a few symbols, and from there on both produce the same thing.  (The decoder state here is more than the bit
// position -- also the position inside the block and the block's place in the MCU, which picks the tables -- so "in
// step" means all three agree.)  The string is cut into spans of 1024 bits, one per lane:
//   1. jpeg_dsync_kernel<false>  every lane decodes its span from a guessed state (block start, first slot), notes
//                                the state it ends in and the blocks it finished; then a lane whose predecessor ended
//                                somewhere else than the lane assumed decodes again from there -- until nothing in the
//                                workgroup changes.  No values are read, only code lengths.
//   2. jpeg_dsync_kernel<true>   the same across workgroups: a workgroup whose predecessor's last lane ended somewhere
//                                else than its first lane assumed repairs its chain (which stops as soon as a lane
//                                ends where it ended before).  Launched until a round changes nothing.  When that
//                                holds every lane's start state follows from the file's first bit: exact, whatever
//                                the guesses were; content only decides how many rounds it takes.
//   3. prefix sum of the finished-block counts = the block every lane starts in
//   4. jpeg_dwrite_kernel        every lane decodes its span once more, now with the values, into the block-major
//                                coefficient array (natural order; DC still as the difference)
//   5. DC differences -> DC: one prefix sum over the blocks laid out component by component
//   6. jpeg_didct_kernel         lane = block: dequantise, idct.go's IDCT, level shift, clamp, into the planes an
//                                *image.YCbCr holds; convert.hip makes toNRGBARef's image of them
// The host parses the segments, builds the decoding tables and removes the 0x00 stuffed behind every 0xff while it
// copies the scan into pinned memory (one memchr pass).
//
// Handled: what jpeg.Encode, libjpeg and most cameras write -- baseline (SOF0), 8 bit, three components (4:4:4, 4:2:2,
// 4:2:0, 4:4:0, 4:1:1, 4:1:0) or one (image.Gray), one scan, with or without restart intervals.  Anything else is FNX_ERR_UNSUPPORTED (the caller decodes on the
// host); a scan that ends early or holds a code outside its table is FNX_ERR_INVALID.  Restated from ITU T.81 and
// reader.go / scan.go / huffman.go's published behaviour, not from Go's source: bit-exact against the CPU restatement
// the tests hold (which libjpeg-turbo's files and hand-built ones exercise: DESIGN.md 5.13), parity with Go unpinned.
// Steps 5 and 6 are also held by an arithmetic-level reference (tests/jpeg_backend_ref.py: numpy int64 with Go's int32 wrap made
// explicit) where that arithmetic leaves its usual range: DC sums beyond 16 bits, DC x q beyond 2^31, quantisers up to 255 with
// AC sizes up to 15, IDCT operations that wrap, restart intervals across MCU rows for every sampling.
// The span decoder itself -- geometry, arguments, state word, dec_span, the sync tables -- is jpeg_dec_span.inc, which
// tools/jpeg_dec_hostsim includes as well.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "common.hpp"
#include "devutil.hpp"
#include "jpeg_idct.hpp"

namespace fnx {

#include "jpeg_dec_span.inc"

// the 256 spans from span0 on (+ 3 words of look-ahead) into LDS; spans before the string's start or past its end read as zeros
__device__ __forceinline__ void dec_stage(DecShared &sh, const DecArgs &a, long long span0, const void *tab, int tab_bytes)
{
    const long long base = span0 * DEC_WPT;
    for (int i = threadIdx.x; i < DEC_WG_WORDS + 3; i += 256) {
        const long long w = base + i;
        sh.seg[i + i / DEC_WPT] = (w >= 0 && w < a.nwords) ? __builtin_bswap32(a.ecs[w]) : 0u;
    }
    const uint32_t *tw = reinterpret_cast<const uint32_t *>(tab);
    uint32_t *sw = reinterpret_cast<uint32_t *>(&sh.tab);
    for (int i = threadIdx.x; i < tab_bytes / 4; i += 256) sw[i] = tw[i];
    if (threadIdx.x < 64) sh.unzig[threadIdx.x] = c_unzig[threadIdx.x];
}

// <false>: workgroup g owns spans [g OWN, (g + 1) OWN) and decodes the WARM spans before them as well (their results
// are dropped).  <true>: the same ownership, no warm-up -- only a workgroup whose predecessor ended elsewhere runs.
// The body of both launches: g is the workgroup's number INSIDE ITS FILE (a's arrays are that file's), flag the round's word.
template <bool FIX, bool RST>
__device__ __forceinline__ void dec_sync_body(DecShared &sh, const DecArgs &a, const int g, uint32_t *flag)
{
    const int t = threadIdx.x;
    const long long span0 = static_cast<long long>(g) * DEC_OWN - (FIX ? 0 : DEC_WARM);
    const long long gs = span0 + t;
    const bool live = gs >= 0 && gs < a.nlanes && (!FIX || t < DEC_OWN);
    const long long wg_bit = span0 * DEC_SPAN;
    unsigned long long my_in, my_out = 0;
    uint32_t my_cnt = 0;
    bool need;
    if (!FIX) {
        my_in = dec_state(static_cast<unsigned long long>(live ? gs : 0) * DEC_SPAN, 0, 0);
        my_out = my_in;
        need = live;
    } else {
        if (g == 0) return;
        // every lane reads the same two words: the branch is uniform
        const unsigned long long prev = __hip_atomic_load(&a.s_out[span0 - 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (prev == a.s_in[span0]) return;
        my_in = live ? a.s_in[gs] : 0;
        my_out = live ? a.s_out[gs] : 0;
        my_cnt = live ? a.cnt[gs] : 0;
        need = t == 0;
        if (t == 0) my_in = prev;
    }
    dec_stage(sh, a, span0, a.tab_sync, static_cast<int>(sizeof(DecSyncTables)));
    sh.out[t] = my_out;
    __syncthreads();
    const uint32_t end = static_cast<uint32_t>(t + 1) * DEC_SPAN;
    uint32_t passes = 0, decodes = 0;
    for (;;) {
        passes++;
        decodes += need ? 1u : 0u;
        // After the first pass only a few lanes decode again -- one per chain of corrections, anywhere in the workgroup --
        // and a wave with ONE such lane issues the whole span's instructions all the same: PMC counted 45 M VALU
        // wave-instructions per 4K file against 13 M for one full decode (the write pass).  When at most 64 lanes need
        // it, they hand their (span, start state) to the workgroup's first wave, which decodes them side by side; the
        // other three waves wait at the barrier.  Same decodes, same order of passes: the fixed point is untouched.
        bool packed = false;
        int slot_c = 0;
        if (!FIX && passes > 1) {
            const unsigned long long bal = __ballot(need);
            if ((t & 63) == 0) sh.wcnt[t >> 6] = static_cast<uint32_t>(__popcll(bal));
            __syncthreads();
            const uint32_t k0 = sh.wcnt[0], k1 = sh.wcnt[1], k2 = sh.wcnt[2], k3 = sh.wcnt[3];
            const uint32_t total = k0 + k1 + k2 + k3;
            packed = total <= 64u;                                  // workgroup-uniform
            if (packed) {
                const int wv = t >> 6;
                const uint32_t base = (wv > 0 ? k0 : 0u) + (wv > 1 ? k1 : 0u) + (wv > 2 ? k2 : 0u);
                slot_c = static_cast<int>(base) + __popcll(bal & ((1ull << (t & 63)) - 1ull));
                if (need) {
                    sh.todo[slot_c] = static_cast<uint16_t>(t);
                    sh.tin[slot_c] = my_in;
                }
                __syncthreads();
                if (t < static_cast<int>(total)) {
                    const int src = sh.todo[t];
                    const unsigned long long in = sh.tin[t];
                    uint32_t rel = static_cast<uint32_t>(static_cast<long long>(in & 0xffffffffffull) - wg_bit);
                    int z = static_cast<int>((in >> 40) & 0xffu), slot = static_cast<int>(in >> 48);
                    uint32_t bad = 0, cnt = 0;
                    dec_span<false, RST>(sh, a, rel, z, slot, static_cast<uint32_t>(src + 1) * DEC_SPAN, cnt,
                                         src >= DEC_WARM ? span0 + src : -1ll, bad, wg_bit);
                    sh.rout[t] = dec_state(static_cast<unsigned long long>(wg_bit + rel), z, slot);
                    sh.rcnt[t] = cnt;
                }
                __syncthreads();
                if (need) {
                    my_out = sh.rout[slot_c];
                    my_cnt = sh.rcnt[slot_c];
                    sh.out[t] = my_out;
                }
            }
        }
        if (!packed && need) {
            uint32_t rel = static_cast<uint32_t>(static_cast<long long>(my_in & 0xffffffffffull) - wg_bit);
            int z = static_cast<int>((my_in >> 40) & 0xffu), slot = static_cast<int>(my_in >> 48);
            uint32_t bad = 0;
            my_cnt = 0;
            dec_span<false, RST>(sh, a, rel, z, slot, end, my_cnt, (FIX || t >= DEC_WARM) ? gs : -1ll, bad, wg_bit);
            my_out = dec_state(static_cast<unsigned long long>(wg_bit + rel), z, slot);
            sh.out[t] = my_out;
        }
        __syncthreads();
        need = false;
        if (t > 0 && live && gs > 0) {                     // (span 0 starts where the string starts: never corrected)
            const unsigned long long pv = sh.out[t - 1];
            if (pv != my_in) {
                my_in = pv;
                need = true;
            }
        }
        if (!__syncthreads_or(need ? 1 : 0)) break;
    }
    if (live && (FIX || t >= DEC_WARM)) {
        a.s_in[gs] = my_in;
        __hip_atomic_store(&a.s_out[gs], my_out, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        a.cnt[gs] = my_cnt;
    }
    if (FIX && t == 0) flag[0] = 1u;
    if (a.dbg) {
        if (t == 0) {
            atomicMax(&a.dbg[0], passes);
            atomicAdd(&a.dbg[1], passes);
        }
        atomicAdd(&a.dbg[2], decodes);
    }
}

template <bool FIX, bool RST>
__global__ __launch_bounds__(256) void jpeg_dsync_kernel(DecArgs a)
{
    __shared__ DecShared sh;
    dec_sync_body<FIX, RST>(sh, a, blockIdx.x, a.flag);
}

// ---- a chunk of files per launch (fnx_jpeg_decode_batch) ----
// One file's scan is ~215 workgroups at 4K and a handful for a thumbnail: a chunk of files shares every launch.  The files'
// DecArgs sit in a device array, each with ITS slice of the chunk's arrays (its own scan with its own zero look-ahead and
// limits, tables, restart offsets; lanes and blocks laid end to end without gaps), and blockIdx.x finds (file, workgroup in
// the file) in a flattened table -- a grid of "largest file x files" would park a DecShared on workgroups that have nothing
// to do.  The body is the single file's: a workgroup never looks outside its file's slice.
struct DecWg {
    int file, wg;
};

template <bool FIX, bool RST>
__global__ __launch_bounds__(256) void jpeg_dsync_batch_kernel(const DecArgs *__restrict__ files, const DecWg *__restrict__ wgs, uint32_t *flag)
{
    __shared__ DecShared sh;
    const DecWg w = wgs[blockIdx.x];
    const DecArgs a = files[w.file];
    dec_sync_body<FIX, RST>(sh, a, w.wg, flag);
}

// BATCH: first_blk is the file's slice of a prefix sum over the whole chunk's lanes -- a lane's first block is its prefix
// minus the prefix at the file's first lane
template <bool RST, bool BATCH>
__device__ __forceinline__ void dec_write_body(DecShared &sh, const DecArgs &a, const int g)
{
    const int t = threadIdx.x, gt = g * 256 + t;
    dec_stage(sh, a, static_cast<long long>(g) * 256, a.tab, static_cast<int>(sizeof(DecTables)));
    __syncthreads();
    if (gt >= a.nlanes) return;
    const unsigned long long st = a.s_in[gt];
    const unsigned long long fb0 = BATCH ? a.first_blk[0] : 0ull;
    long long blk = static_cast<long long>(a.first_blk[gt] - fb0);
    if (RST && a.nrst > 0) {
        // Block numbers are counted from the restart interval's start, not from the file's: the sync passes go by position and
        // cannot know when an interval's blocks are complete, so the <= 7 bits a DAMAGED interval leaves before its boundary
        // can read as one more complete block there (DC category 0 + EOB is 4 bits) -- a block no decoder that counts MCUs
        // ever sees, and one that would shift every block number behind it (the fuzzer's find, seed 77:
        // tests/golden/damaged_interval_phantom_block.jpg).  With j the last boundary at or before this lane's start:
        // blocks before it = (j + 1) ri_blocks by definition, blocks since = the prefix sums' difference.
        const unsigned long long at = st & 0xffffffffffull;
        int lo_k = 0, hi_k = a.nrst;                               // first boundary AFTER the start
        while (lo_k < hi_k) {
            const int mid = (lo_k + hi_k) >> 1;
            if (8ull * a.rst[mid] <= at) lo_k = mid + 1; else hi_k = mid;
        }
        const int j = lo_k - 1;
        if (j >= 0) {
            const unsigned long long rec = a.rst_rec[j];
            const long long before = static_cast<long long>(a.first_blk[rec >> 32] - fb0) + static_cast<long long>(rec & 0xffffffffull);
            blk = static_cast<long long>(j + 1) * a.ri_blocks + (blk - before);
        }
    }
    if (blk >= a.nblk) return;                                     // padding behind the last block
    const unsigned long long wg_bit = static_cast<unsigned long long>(g) * 256u * DEC_SPAN;
    uint32_t rel = static_cast<uint32_t>((st & 0xffffffffffull) - wg_bit);
    int z = static_cast<int>((st >> 40) & 0xffu), slot = static_cast<int>(st >> 48);
    uint32_t cnt = 0, bad = 0;
    const unsigned long long left = a.nbits - wg_bit;              // (this lane exists: its span starts inside the string)
    dec_span<true, RST>(sh, a, rel, z, slot, static_cast<uint32_t>(t + 1) * DEC_SPAN, cnt, blk, bad, static_cast<long long>(wg_bit),
                        left > 0xfffffff0ull ? 0xfffffff0u : static_cast<uint32_t>(left));
    if (bad) atomicOr(a.err, bad);
}

template <bool RST>
__global__ __launch_bounds__(256) void jpeg_dwrite_kernel(DecArgs a)
{
    __shared__ DecShared sh;
    dec_write_body<RST, false>(sh, a, blockIdx.x);
}

// what the host reads of a file when the chunk is done (the single file's d_flag + 64: err, then the blocks finished)
struct DecResult {
    uint32_t err, pad;
    unsigned long long blocks;
};

template <bool RST>
__global__ __launch_bounds__(256) void jpeg_dwrite_batch_kernel(const DecArgs *__restrict__ files, const DecWg *__restrict__ wgs)
{
    __shared__ DecShared sh;
    const DecWg w = wgs[blockIdx.x];
    const DecArgs a = files[w.file];
    // the blocks finished inside the file's string: the difference of two bases (the prefix sum runs one lane past the chunk's last)
    if (w.wg == 0 && threadIdx.x == 0) reinterpret_cast<DecResult *>(a.err)->blocks = a.first_blk[a.nlanes] - a.first_blk[0];
    dec_write_body<RST, true>(sh, a, w.wg);
}

// ---- DC prediction and the blocks ----
struct DcArgs {
    const int16_t *coef;
    uint32_t *dcb;            // [nblk] DC difference + 2048, component by component (Y in scan order, then Cb, then Cr)
    int nblk, nmcu, ny, nc;   // ny: Y blocks per MCU (1, 2 or 4); nc: chroma components (2 or 0)
};

// scan-order block -> its place in the component-major array
__device__ __forceinline__ int dc_place(int b, int nmcu, int ny, int nc)
{
    const int per = ny + nc, m = b / per, j = b - m * per;
    return j < ny ? m * ny + j : (ny + (j - ny)) * nmcu + m;
}

__device__ __forceinline__ void dc_gather_body(const DcArgs &a, const int b)
{
    if (b >= a.nblk) return;
    a.dcb[dc_place(b, a.nmcu, a.ny, a.nc)] = static_cast<uint32_t>(static_cast<int32_t>(a.coef[static_cast<size_t>(b) * 64]) + 2048);
}

__global__ __launch_bounds__(256) void jpeg_dc_gather_kernel(DcArgs a)
{
    dc_gather_body(a, blockIdx.x * 256 + threadIdx.x);
}

// (coef and dcb: the file's slices of the chunk's arrays)
__global__ __launch_bounds__(256) void jpeg_dc_gather_batch_kernel(const DcArgs *__restrict__ files, const DecWg *__restrict__ wgs)
{
    const DecWg w = wgs[blockIdx.x];
    dc_gather_body(files[w.file], w.wg * 256 + threadIdx.x);
}

struct IdctArgs {
    const int16_t *coef;
    const uint32_t *dcb;
    const unsigned long long *dcsum;     // exclusive prefix sum of dcb
    uint8_t *out[4];
    int stride[4], nbx[4], nblocks[4];
    int mx, nmcu, hy, vy, nc;            // MCUs per row, MCUs, Y blocks per MCU across / down, chroma components
    int ri;                              // MCUs per restart interval (the DC prediction starts over in each); 0: one interval
    int abs_dc;                          // progressive files (jpeg_prog.cpp): coef[0] IS the DC, no prediction to undo
    uint16_t q[4][64];                   // natural order (a fourth plane -- the black of a CMYK file -- only with abs_dc)
};

__device__ __forceinline__ void dec_idct_body(const IdctArgs &a, const int plane, const int i)
{
    if (i >= a.nblocks[plane]) return;
    const int by = i / a.nbx[plane], bx = i - by * a.nbx[plane];
    const int ny = a.hy * a.vy, per = ny + a.nc;
    int sb, place, start;
    if (plane == 0) {
        const int m = (by / a.vy) * a.mx + bx / a.hy, j = (by % a.vy) * a.hy + bx % a.hy;
        sb = m * per + j;
        place = m * ny + j;
        start = a.ri > 0 ? (m / a.ri) * a.ri * ny : 0;
    } else {
        const int m = by * a.mx + bx;
        sb = m * per + ny + plane - 1;
        const int first = (ny + plane - 1) * a.nmcu;
        place = first + m;
        start = first + (a.ri > 0 ? (m / a.ri) * a.ri : 0);
    }
    const int16_t *cp = a.coef + static_cast<size_t>(sb) * 64;
    int32_t b[64];
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const u32x4 v = *reinterpret_cast<const u32x4 *>(cp + 8 * r);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int32_t cv = static_cast<int16_t>((w[c >> 1] >> (16 * (c & 1))) & 0xffffu);
            b[8 * r + c] = cv * static_cast<int32_t>(a.q[plane][8 * r + c]);
        }
    }
    // the block's DC: the sum of its component's differences from the start of its restart interval up to it
    if (!a.abs_dc) {
        const long long dsum = static_cast<long long>(a.dcsum[place] - a.dcsum[start]) + a.dcb[place] - 2048ll * (place - start + 1);
        b[0] = static_cast<int32_t>(dsum) * static_cast<int32_t>(a.q[plane][0]);
    }
#pragma unroll
    for (int r = 0; r < 8; r++) idct8_row(b[8 * r], b[8 * r + 1], b[8 * r + 2], b[8 * r + 3], b[8 * r + 4], b[8 * r + 5], b[8 * r + 6], b[8 * r + 7]);
#pragma unroll
    for (int c = 0; c < 8; c++) idct8_col(b[c], b[8 + c], b[16 + c], b[24 + c], b[32 + c], b[40 + c], b[48 + c], b[56 + c]);
    const int stride = a.stride[plane];
    uint8_t *op = a.out[plane] + static_cast<size_t>(8 * by) * stride + 8 * bx;
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

__global__ __launch_bounds__(256) void jpeg_didct_kernel(IdctArgs a)
{
    dec_idct_body(a, blockIdx.y, blockIdx.x * 256 + threadIdx.x);
}

// coef, dcb and dcsum are the file's slices: the DC is a DIFFERENCE of two prefix sums inside the file's own blocks, so a
// prefix sum over the whole chunk's blocks serves every file.  nblocks[c] = 0 for a plane the file does not have.
__global__ __launch_bounds__(256) void jpeg_didct_batch_kernel(const IdctArgs *__restrict__ files, const DecWg *__restrict__ wgs)
{
    const DecWg w = wgs[blockIdx.x];
    dec_idct_body(files[w.file], blockIdx.y, w.wg * 256 + threadIdx.x);
}

// ---- the host side (segments, tables, the scan without its stuffing: jpeg_parse.cpp) and the launches ----
constexpr int SCAN_PER_WG_D = 2048;

// data (host): the file.  On return the planes (SLOT_JPEG_DEC_PLANES: Y, Cb, Cr back to back, MCU-padded) are
// enqueued and *f describes them; the scan has been validated (one small read-back).
// SOF2: every scan's entropy decoding on the host (jpeg_prog.cpp: why), the coefficients across PCIe at 2 bytes each, then the
// same dequantisation + IDCT launch as a baseline file's
static int jpeg_decode_planes_progressive(fnx_ctx *ctx, const uint8_t *data, size_t n, JpegFile *f, uint8_t *planes[4], int *ystride, int *cstride)
{
    const long long nmcu = static_cast<long long>(f->mx) * f->my;
    const long long nblk_ll = nmcu * f->nslots;
    if (nblk_ll > JPEG_HOST_MAX_BLOCKS) return jpeg_unsupported("a host-decoded file of more than 4 M blocks (FNX_JPEG_HOST_MAX_BLOCKS)");
    // a first DC scan costs every block at least one bit: a header that promises more blocks than the file has bits is refused
    // before anything is sized by it
    if (8ull * n < static_cast<unsigned long long>(nblk_ll)) return jpeg_corrupt("the file is too short for the image's blocks");
    const int nblk = static_cast<int>(nblk_ll);
    const int ys = 8 * f->hy * f->mx, yh = 8 * f->vy * f->my, cs = 8 * f->mx, chh = 8 * f->my;
    const size_t b_coef = sizeof(int16_t) * 64 * static_cast<size_t>(nblk);
    void *pin = nullptr;
    FNX_TRY(pinned_alloc(ctx, b_coef, &pin));
    std::memset(pin, 0, b_coef);
    FNX_TRY(jpeg_progressive_coefficients(data, n, f, static_cast<int16_t *>(pin)));
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    void *sc = nullptr, *pl = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_DEC, al(b_coef), &sc));
    const size_t b_y = al(static_cast<size_t>(ys) * yh), b_c = al(static_cast<size_t>(cs) * chh);
    FNX_TRY(scratch(ctx, SLOT_JPEG_DEC_PLANES, b_y + 3 * b_c, &pl));
    planes[0] = static_cast<uint8_t *>(pl);
    planes[1] = planes[0] + b_y;
    planes[2] = planes[1] + b_c;
    planes[3] = planes[2] + b_c;                  // (four components: all of one geometry, b_c == b_y)
    *ystride = ys; *cstride = cs;
    FNX_HIP(hipMemcpyAsync(sc, pin, b_coef, hipMemcpyHostToDevice, ctx->stream));
    IdctArgs ia{};
    ia.coef = static_cast<const int16_t *>(sc); ia.dcb = nullptr; ia.dcsum = nullptr;
    for (int c = 0; c < 4; c++) {
        ia.out[c] = planes[c];
        ia.stride[c] = c ? cs : ys;
        ia.nbx[c] = (c ? cs : ys) / 8;
        ia.nblocks[c] = ia.nbx[c] * ((c ? chh : yh) / 8);
        for (int k = 0; k < 64; k++) ia.q[c][k] = f->q[c][k];
    }
    ia.mx = f->mx; ia.nmcu = static_cast<int>(nmcu); ia.hy = f->hy; ia.vy = f->vy; ia.nc = f->ncomp - 1; ia.ri = 0; ia.abs_dc = 1;
    FNX_TRY(prof_begin(ctx, FNX_PROF_JPEG));
    hipLaunchKernelGGL(jpeg_didct_kernel, dim3((ia.nblocks[0] + 255) / 256, f->ncomp), dim3(256), 0, ctx->stream, ia);
    FNX_HIP(hipGetLastError());
    note_route(ctx, FNX_PROF_JPEG, "jpeg_didct_kernel behind the host's scans (jpeg_prog.cpp)");
    FNX_TRY(prof_end(ctx));
    f->rounds = 0;
    return FNX_OK;
}

// a baseline file's dequantisation + IDCT launch: coef / dcb / dcsum are its blocks', planes its Y, Cb, Cr (MCU-padded)
static IdctArgs dec_idct_args(const JpegFile &f, const int16_t *coef, const uint32_t *dcb, const unsigned long long *dcsum, uint8_t *const planes[3])
{
    const int ys = 8 * f.hy * f.mx, yh = 8 * f.vy * f.my, cs = 8 * f.mx, chh = 8 * f.my;
    IdctArgs ia{};
    ia.coef = coef; ia.dcb = dcb; ia.dcsum = dcsum;
    for (int c = 0; c < 3; c++) {
        ia.out[c] = planes[c];
        ia.stride[c] = c ? cs : ys;
        ia.nbx[c] = (c ? cs : ys) / 8;
        ia.nblocks[c] = ia.nbx[c] * ((c ? chh : yh) / 8);
        for (int k = 0; k < 64; k++) ia.q[c][k] = f.q[c][k];
    }
    ia.mx = f.mx; ia.nmcu = f.mx * f.my; ia.hy = f.hy; ia.vy = f.vy; ia.nc = f.ncomp - 1; ia.ri = f.ri; ia.abs_dc = 0;
    return ia;
}

// the write pass's complaints and the blocks the scan held, as fnx_jpeg_decode answers them
static int dec_verdict(uint32_t err, unsigned long long blocks, int nblk)
{
    if (blocks < static_cast<unsigned long long>(nblk)) return jpeg_corrupt("the scan ends before the last block");
    if (err & 8u) return jpeg_corrupt("the scan ends before the last block");
    if (err & 16u) return jpeg_corrupt("a restart interval does not hold the blocks it should");
    if (err) return jpeg_corrupt("the scan holds a code outside its Huffman table or a run past the end of a block");
    return FNX_OK;
}

int jpeg_decode_planes(fnx_ctx *ctx, const uint8_t *data, size_t n, JpegFile *f, uint8_t *planes[4], int *ystride, int *cstride)
{
    FNX_TRY(jpeg_parse(data, n, f));
    if (f->progressive) return jpeg_decode_planes_progressive(ctx, data, n, f, planes, ystride, cstride);
    void *pin = nullptr, *tpin = nullptr;
    const size_t cap = (n - f->scan + 64 + 63) & ~size_t(63);           // >= the scan + 4 words of zeros
    const long long nmcu0 = static_cast<long long>(f->mx) * f->my;
    const size_t rst_max = f->ri > 0 ? static_cast<size_t>((nmcu0 + f->ri - 1) / f->ri) : 0;
    FNX_TRY(pinned_alloc(ctx, cap + sizeof(DecTables) + sizeof(DecSyncTables) + 4 * rst_max + 64, &pin));   // one slice: a second request could wrap the ring onto it
    tpin = static_cast<uint8_t *>(pin) + cap;
    size_t nb = 0;
    std::vector<uint32_t> rst;
    FNX_TRY(jpeg_unstuff(data, n, *f, static_cast<uint8_t *>(pin), &nb, &rst));
    uint32_t *rpin = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(tpin) + sizeof(DecTables) + sizeof(DecSyncTables));
    if (!rst.empty()) std::memcpy(rpin, rst.data(), 4 * rst.size());
    const size_t nwords = (nb + 3) / 4 + 4;
    std::memset(static_cast<uint8_t *>(pin) + nb, 0, nwords * 4 - nb);
    const unsigned long long nbits = 8ull * nb;
    const size_t nlanes_z = static_cast<size_t>((nbits + DEC_SPAN - 1) / DEC_SPAN);
    const long long nmcu = static_cast<long long>(f->mx) * f->my;
    const long long nblk_ll = nmcu * f->nslots;
    if (nlanes_z == 0) return jpeg_corrupt("an empty scan");
    if (nlanes_z >= (size_t(1) << 30) || nblk_ll >= (1ll << 30)) return jpeg_unsupported("a file this large");
    // every block costs at least two bits (a DC code and an end of block): a header that promises more blocks than the scan
    // can hold is refused BEFORE anything is sized by it (65 535 x 65 535 in the frame header of a 1 KB file)
    if (nbits < 2ull * static_cast<unsigned long long>(nblk_ll)) return jpeg_corrupt("the scan is too short for the image's blocks");
    const int nlanes = static_cast<int>(nlanes_z), nblk = static_cast<int>(nblk_ll);
    const int nwg = (nlanes + DEC_OWN - 1) / DEC_OWN, nwg_write = (nlanes + 255) / 256;
    const int ys = 8 * f->hy * f->mx, yh = 8 * f->vy * f->my, cs = 8 * f->mx, chh = 8 * f->my;

    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    const size_t lanes_pad = static_cast<size_t>(nwg) * 256;
    const size_t b_ecs = al(nwords * 4 + 64), b_tab = al(sizeof(DecTables) + sizeof(DecSyncTables) + 4 * rst_max + 16), b_state = al(8 * lanes_pad), b_cnt = al(4 * lanes_pad),
                 b_first = al(8 * lanes_pad), b_tot = al(8 * (lanes_pad / SCAN_PER_WG_D + 2)), b_flag = al(4 * 64 + 16),
                 b_coef = al(sizeof(int16_t) * 64 * static_cast<size_t>(nblk)), b_dcb = al(4 * static_cast<size_t>(nblk)),
                 b_dcs = al(8 * static_cast<size_t>(nblk)), b_tot2 = al(8 * (static_cast<size_t>(nblk) / SCAN_PER_WG_D + 2)),
                 b_rec = al(8 * (rst.size() + 1));
    void *sc = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_DEC, b_ecs + b_tab + 2 * b_state + b_cnt + b_first + b_tot + b_flag + b_coef + b_dcb + b_dcs + b_tot2 + b_rec, &sc));
    unsigned char *p = static_cast<unsigned char *>(sc);
    uint32_t *d_ecs = reinterpret_cast<uint32_t *>(p); p += b_ecs;
    DecTables *d_tab = reinterpret_cast<DecTables *>(p); p += b_tab;
    unsigned long long *d_in = reinterpret_cast<unsigned long long *>(p); p += b_state;
    unsigned long long *d_out = reinterpret_cast<unsigned long long *>(p); p += b_state;
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(p); p += b_cnt;
    unsigned long long *d_first = reinterpret_cast<unsigned long long *>(p); p += b_first;
    unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(p); p += b_tot;
    uint32_t *d_flag = reinterpret_cast<uint32_t *>(p); p += b_flag;          // [0..63] rounds, then err, then 2 x u64 totals
    int16_t *d_coef = reinterpret_cast<int16_t *>(p); p += b_coef;
    uint32_t *d_dcb = reinterpret_cast<uint32_t *>(p); p += b_dcb;
    unsigned long long *d_dcs = reinterpret_cast<unsigned long long *>(p); p += b_dcs;
    unsigned long long *d_tot2 = reinterpret_cast<unsigned long long *>(p); p += b_tot2;
    unsigned long long *d_rec = reinterpret_cast<unsigned long long *>(p);
    void *pl = nullptr;
    const size_t b_y = al(static_cast<size_t>(ys) * yh), b_c = al(static_cast<size_t>(cs) * chh);
    FNX_TRY(scratch(ctx, SLOT_JPEG_DEC_PLANES, b_y + 2 * b_c, &pl));
    planes[0] = static_cast<uint8_t *>(pl);
    planes[1] = planes[0] + b_y;
    planes[2] = planes[1] + b_c;
    *ystride = ys; *cstride = cs;

    std::memcpy(tpin, &f->tab, sizeof(DecTables));
    dec_sync_tables(f->tab, reinterpret_cast<DecSyncTables *>(static_cast<uint8_t *>(tpin) + sizeof(DecTables)));
    FNX_HIP(hipMemcpyAsync(d_ecs, pin, nwords * 4, hipMemcpyHostToDevice, ctx->stream));
    FNX_HIP(hipMemcpyAsync(d_tab, tpin, sizeof(DecTables) + sizeof(DecSyncTables) + 4 * rst.size(), hipMemcpyHostToDevice, ctx->stream));
    FNX_HIP(hipMemsetAsync(d_flag, 0, b_flag, ctx->stream));
    FNX_HIP(hipMemsetAsync(d_coef, 0, sizeof(int16_t) * 64 * static_cast<size_t>(nblk), ctx->stream));

    DecArgs a{};
    a.ecs = d_ecs; a.tab = d_tab; a.tab_sync = reinterpret_cast<const DecSyncTables *>(d_tab + 1); a.s_in = d_in; a.s_out = d_out; a.cnt = d_cnt; a.flag = d_flag;
    a.first_blk = d_first; a.coef = d_coef; a.err = d_flag + 64;
    const char *trc = std::getenv("FNX_JPEG_TRACE");
    const bool trace = trc && trc[0] == '1';
    a.dbg = trace ? d_flag + 72 : nullptr;
    a.nwords = static_cast<long long>(nwords); a.nbits = nbits; a.nlanes = nlanes; a.nblk = nblk; a.nslots = f->nslots;
    a.dcpack = f->dcpack; a.acpack = f->acpack;
    a.rst = reinterpret_cast<const uint32_t *>(reinterpret_cast<const uint8_t *>(d_tab) + sizeof(DecTables) + sizeof(DecSyncTables)); a.nrst = static_cast<int>(rst.size());
    a.ri_blocks = f->ri * f->nslots;
    a.rst_rec = d_rec;
    const bool has_rst = !rst.empty();
    if (has_rst) FNX_HIP(hipMemsetAsync(d_rec, 0, 8 * rst.size(), ctx->stream));
    FNX_TRY(prof_begin(ctx, FNX_PROF_JPEG));
    if (has_rst) hipLaunchKernelGGL((jpeg_dsync_kernel<false, true>), dim3(nwg), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL((jpeg_dsync_kernel<false, false>), dim3(nwg), dim3(256), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    note_route(ctx, FNX_PROF_JPEG, "jpeg_dsync_kernel");
    FNX_TRY(prof_end(ctx));
    // rounds across workgroups, two per read-back; a round that changes nothing ends it (at most nwg rounds can change something)
    f->rounds = 0;
    if (nwg > 1) {
        uint32_t flags[64];
        int r = 0, rewound = 0;                  // rounds before the last rewind of the flags
        for (;;) {
            const int r0 = r;
            for (int k = 0; k < 2 && r < 64; k++, r++) {
                a.flag = d_flag + r;
                if (has_rst) hipLaunchKernelGGL((jpeg_dsync_kernel<true, true>), dim3(nwg), dim3(256), 0, ctx->stream, a);
                else hipLaunchKernelGGL((jpeg_dsync_kernel<true, false>), dim3(nwg), dim3(256), 0, ctx->stream, a);
            }
            FNX_HIP(hipGetLastError());
            FNX_TRY(fetch_bytes(ctx, d_flag, flags, sizeof(uint32_t) * static_cast<size_t>(r)));
            bool quiet = false;
            for (int k = r0; k < r; k++) quiet = quiet || flags[k] == 0;
            f->rounds = rewound + r;
            if (quiet) break;
            if (r >= 64) {                       // start the flags over: the pattern that needs this many rounds is contrived, not wrong
                FNX_HIP(hipMemsetAsync(d_flag, 0, 4 * 64, ctx->stream));
                rewound += r;
                r = 0;
            }
        }
    }
    FNX_TRY(launch_scan(ctx, d_cnt, d_first, d_tot, nlanes, reinterpret_cast<unsigned long long *>(d_flag + 66)));
    if (has_rst) hipLaunchKernelGGL(jpeg_dwrite_kernel<true>, dim3(nwg_write), dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(jpeg_dwrite_kernel<false>, dim3(nwg_write), dim3(256), 0, ctx->stream, a);
    DcArgs da{d_coef, d_dcb, nblk, static_cast<int>(nmcu), f->hy * f->vy, f->ncomp - 1};
    hipLaunchKernelGGL(jpeg_dc_gather_kernel, dim3((nblk + 255) / 256), dim3(256), 0, ctx->stream, da);
    FNX_TRY(launch_scan(ctx, d_dcb, d_dcs, d_tot2, nblk, nullptr));
    const IdctArgs ia = dec_idct_args(*f, d_coef, d_dcb, d_dcs, planes);
    hipLaunchKernelGGL(jpeg_didct_kernel, dim3((ia.nblocks[0] + 255) / 256, f->ncomp), dim3(256), 0, ctx->stream, ia);
    FNX_HIP(hipGetLastError());
    // what the scan held: blocks finished inside the string, and the write pass's complaints
    struct { uint32_t err, pad; unsigned long long blocks; } chk;
    FNX_TRY(fetch_bytes(ctx, d_flag + 64, &chk, sizeof(chk)));
    if (trace) {
        uint32_t dbg[3];
        FNX_TRY(fetch_bytes(ctx, d_flag + 72, dbg, sizeof(dbg)));
        std::fprintf(stderr, "[fennec jpeg] %d x %d, %zu scan bytes, %d lanes in %d workgroups: passes max %u avg %.1f, lane-decodes %u (%.2f per lane), "
                             "cross-workgroup rounds %d\n", f->w, f->h, nb, nlanes, nwg, dbg[0], double(dbg[1]) / nwg, dbg[2], double(dbg[2]) / nlanes, f->rounds);
    }
    return dec_verdict(chk.err, chk.blocks, nblk);
}

// ---- a chunk of baseline files in one set of launches (fnx_jpeg_decode_batch) ----
// Device layout of a chunk (SLOT_JPEG_DEC), m files of which the live ones passed the host's refusals:
//   uploaded slice 1   every file's scan without its stuffing (own slice, own four words of zero look-ahead), then every
//                      file's DecTables | DecSyncTables | restart offsets -- ONE pinned slice, one copy
//   uploaded slice 2   DecArgs[m] | DcArgs[m] | IdctArgs[m] | the five workgroup tables -- one copy
//   per lane           s_in, s_out, first_blk: the live files' lanes end to end, NO gaps, one lane more at the end (whose count
//                      is zero: first_blk there is the chunk's total, so every file's blocks are a difference of two bases)
//   zeroed at once     64 round flags | DecResult[m] | cnt (per lane)
//   per block          coef (zeroed), dcb, dcsum: the live files' blocks end to end; rst_rec: their boundaries end to end
// Host waits: one per pair of repair rounds (shared by every file: quiet = no workgroup of ANY file decoded again), one for
// every file's DecResult.  Nothing else -- unless the pinned ring wraps (runtime.cpp), which waits for the stream first.
size_t jpeg_decode_chunk_bytes(const JpegFile &f, size_t n)
{
    const size_t scan = n - f.scan;
    const unsigned long long hdr = static_cast<unsigned long long>(f.mx) * f.my * f.nslots;
    const unsigned long long nblk = hdr < 4ull * scan ? hdr : 4ull * scan;          // (a scan holds at most 4 blocks a byte)
    const size_t lanes = scan * 8 / DEC_SPAN + 2;
    return scan + 4 * (scan / 2 + 1 < hdr ? scan / 2 + 1 : static_cast<size_t>(hdr)) + sizeof(DecTables) + sizeof(DecSyncTables) + sizeof(DecArgs) + sizeof(DcArgs) +
           sizeof(IdctArgs) + 1024 + 28 * lanes + static_cast<size_t>(nblk) * (128 + 4 + 8 + 8 + 64);
}

int jpeg_decode_planes_chunk(fnx_ctx *ctx, int m, JpegBatchItem *it)
{
    auto al = [](size_t x) { return (x + 255) & ~size_t(255); };
    struct Plan {
        size_t o_ecs = 0, o_tab = 0, nb = 0, nwords = 0, nrst = 0;
        size_t lane0 = 0, blk0 = 0, rec0 = 0, o_planes = 0, b_y = 0, b_c = 0;
        int nlanes = 0, nblk = 0;
        bool live = false;
    };
    std::vector<Plan> pl(m);
    // slice 1, sized by the files' bytes (never by a header): scans, then tables + restart offsets
    size_t up = 0;
    for (int i = 0; i < m; i++) {
        pl[i].o_ecs = up;
        up += al((it[i].n - it[i].f.scan + 64 + 63) & ~size_t(63));                // >= the scan + 4 words of zeros
    }
    for (int i = 0; i < m; i++) {
        const JpegFile &f = it[i].f;
        const size_t by_file = (it[i].n - f.scan) / 2 + 1;                          // a restart marker is two bytes
        const unsigned long long by_hdr = f.ri > 0 ? (static_cast<unsigned long long>(f.mx) * f.my + f.ri - 1) / f.ri : 0;
        pl[i].o_tab = up;
        up += al(sizeof(DecTables) + sizeof(DecSyncTables) + 4 * (by_hdr < by_file ? static_cast<size_t>(by_hdr) : by_file) + 16);
    }
    void *pin = nullptr;
    FNX_TRY(pinned_alloc(ctx, up, &pin));
    uint8_t *hp = static_cast<uint8_t *>(pin);
    std::vector<uint32_t> rst;
    size_t L = 0, NB = 0, NR = 0, PB = 0;
    size_t n_sync = 0, n_fix = 0, n_write = 0, n_gather = 0, n_idct = 0;
    bool any_rst = false;
    for (int i = 0; i < m; i++) {
        JpegFile &f = it[i].f;
        Plan &p = pl[i];
        it[i].status = jpeg_unstuff(it[i].data, it[i].n, f, hp + p.o_ecs, &p.nb, &rst);
        if (it[i].status < 0) continue;
        p.nwords = (p.nb + 3) / 4 + 4;
        std::memset(hp + p.o_ecs + p.nb, 0, p.nwords * 4 - p.nb);
        // the single file's refusals (jpeg_decode_planes), before anything is sized by the header
        const unsigned long long nbits = 8ull * p.nb;
        const size_t nlanes_z = static_cast<size_t>((nbits + DEC_SPAN - 1) / DEC_SPAN);
        const long long nblk_ll = static_cast<long long>(f.mx) * f.my * f.nslots;
        if (nlanes_z == 0) it[i].status = jpeg_corrupt("an empty scan");
        else if (nlanes_z >= (size_t(1) << 30) || nblk_ll >= (1ll << 30)) it[i].status = jpeg_unsupported("a file this large");
        else if (nbits < 2ull * static_cast<unsigned long long>(nblk_ll)) it[i].status = jpeg_corrupt("the scan is too short for the image's blocks");
        if (it[i].status < 0) continue;
        uint8_t *tp = hp + p.o_tab;
        std::memcpy(tp, &f.tab, sizeof(DecTables));
        dec_sync_tables(f.tab, reinterpret_cast<DecSyncTables *>(tp + sizeof(DecTables)));
        if (!rst.empty()) std::memcpy(tp + sizeof(DecTables) + sizeof(DecSyncTables), rst.data(), 4 * rst.size());
        p.nrst = rst.size();
        p.nlanes = static_cast<int>(nlanes_z);
        p.nblk = static_cast<int>(nblk_ll);
        p.b_y = al(static_cast<size_t>(8 * f.hy * f.mx) * (8 * f.vy * f.my));
        p.b_c = al(static_cast<size_t>(8 * f.mx) * (8 * f.my));
        p.lane0 = L; L += p.nlanes;
        p.blk0 = NB; NB += p.nblk;
        p.rec0 = NR; NR += p.nrst;
        p.o_planes = PB; PB += p.b_y + 2 * p.b_c;
        const size_t nwg = (p.nlanes + DEC_OWN - 1) / DEC_OWN;
        n_sync += nwg;
        n_fix += nwg - 1;                                                            // (a file's workgroup 0 has no predecessor: never repaired)
        n_write += (p.nlanes + 255) / 256;
        n_gather += (p.nblk + 255) / 256;
        n_idct += (static_cast<size_t>(f.hy * f.mx) * (f.vy * f.my) + 255) / 256;
        any_rst = any_rst || p.nrst > 0;
        p.live = true;
    }
    if (L == 0) return FNX_OK;                                                       // every file refused
    FNX_REQUIRE(L + 1 < (size_t(1) << 30) && NB < (size_t(1) << 30), "decode batch: a chunk of more than 2^30 lanes or blocks");
    const size_t lanes = L + 1;

    const size_t o_args = 0, o_dc = o_args + al(sizeof(DecArgs) * m), o_idct = o_dc + al(sizeof(DcArgs) * m), o_wgs = o_idct + al(sizeof(IdctArgs) * m);
    const size_t n_wgs = n_sync + n_fix + n_write + n_gather + n_idct;
    const size_t up2 = o_wgs + al(sizeof(DecWg) * n_wgs);
    const size_t b_state = al(8 * lanes), b_tot = al(8 * (lanes / SCAN_PER_WG_D + 2)), b_flag = al(4 * 64), b_res = al(sizeof(DecResult) * m), b_cnt = al(4 * lanes),
                 b_coef = al(sizeof(int16_t) * 64 * NB), b_dcb = al(4 * NB), b_dcs = al(8 * NB), b_tot2 = al(8 * (NB / SCAN_PER_WG_D + 2)), b_rec = al(8 * (NR + 1));
    void *sc = nullptr, *plv = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_DEC, up + up2 + 3 * b_state + b_tot + b_flag + b_res + b_cnt + b_coef + b_dcb + b_dcs + b_tot2 + b_rec, &sc));
    FNX_TRY(scratch(ctx, SLOT_JPEG_DEC_PLANES, PB, &plv));
    unsigned char *q = static_cast<unsigned char *>(sc);
    unsigned char *d_up = q; q += up;
    unsigned char *d_up2 = q; q += up2;
    unsigned long long *d_in = reinterpret_cast<unsigned long long *>(q); q += b_state;
    unsigned long long *d_out = reinterpret_cast<unsigned long long *>(q); q += b_state;
    unsigned long long *d_first = reinterpret_cast<unsigned long long *>(q); q += b_state;
    unsigned long long *d_tot = reinterpret_cast<unsigned long long *>(q); q += b_tot;
    uint32_t *d_flag = reinterpret_cast<uint32_t *>(q); q += b_flag;
    DecResult *d_res = reinterpret_cast<DecResult *>(q); q += b_res;
    uint32_t *d_cnt = reinterpret_cast<uint32_t *>(q); q += b_cnt;
    int16_t *d_coef = reinterpret_cast<int16_t *>(q); q += b_coef;
    uint32_t *d_dcb = reinterpret_cast<uint32_t *>(q); q += b_dcb;
    unsigned long long *d_dcs = reinterpret_cast<unsigned long long *>(q); q += b_dcs;
    unsigned long long *d_tot2 = reinterpret_cast<unsigned long long *>(q); q += b_tot2;
    unsigned long long *d_rec = reinterpret_cast<unsigned long long *>(q);
    // slice 1 goes up before slice 2 is asked for: should the ring wrap there, it waits for this copy first
    FNX_HIP(hipMemcpyAsync(d_up, hp, up, hipMemcpyHostToDevice, ctx->stream));
    FNX_HIP(hipMemsetAsync(d_flag, 0, b_flag + b_res + b_cnt, ctx->stream));
    FNX_HIP(hipMemsetAsync(d_coef, 0, sizeof(int16_t) * 64 * NB, ctx->stream));
    if (NR) FNX_HIP(hipMemsetAsync(d_rec, 0, 8 * NR, ctx->stream));

    void *pin2 = nullptr;
    FNX_TRY(pinned_alloc(ctx, up2, &pin2));
    uint8_t *hp2 = static_cast<uint8_t *>(pin2);
    std::memset(hp2, 0, o_wgs);
    DecArgs *h_args = reinterpret_cast<DecArgs *>(hp2 + o_args);
    DcArgs *h_dc = reinterpret_cast<DcArgs *>(hp2 + o_dc);
    IdctArgs *h_idct = reinterpret_cast<IdctArgs *>(hp2 + o_idct);
    DecWg *h_wgs = reinterpret_cast<DecWg *>(hp2 + o_wgs);
    DecWg *w_sync = h_wgs, *w_fix = w_sync + n_sync, *w_write = w_fix + n_fix, *w_gather = w_write + n_write, *w_idct = w_gather + n_gather;
    for (int i = 0; i < m; i++) {
        const Plan &p = pl[i];
        if (!p.live) continue;
        const JpegFile &f = it[i].f;
        DecArgs a{};
        const unsigned char *d_tab = d_up + p.o_tab;
        a.ecs = reinterpret_cast<const uint32_t *>(d_up + p.o_ecs);
        a.tab = reinterpret_cast<const DecTables *>(d_tab);
        a.tab_sync = reinterpret_cast<const DecSyncTables *>(d_tab + sizeof(DecTables));
        a.s_in = d_in + p.lane0; a.s_out = d_out + p.lane0; a.cnt = d_cnt + p.lane0; a.flag = d_flag;
        a.first_blk = d_first + p.lane0; a.coef = d_coef + 64 * p.blk0; a.err = &d_res[i].err; a.dbg = nullptr;
        a.nwords = static_cast<long long>(p.nwords); a.nbits = 8ull * p.nb; a.nlanes = p.nlanes; a.nblk = p.nblk; a.nslots = f.nslots;
        a.dcpack = f.dcpack; a.acpack = f.acpack;
        a.rst = reinterpret_cast<const uint32_t *>(d_tab + sizeof(DecTables) + sizeof(DecSyncTables)); a.nrst = static_cast<int>(p.nrst);
        a.ri_blocks = f.ri * f.nslots;
        a.rst_rec = d_rec + p.rec0;
        h_args[i] = a;
        h_dc[i] = DcArgs{a.coef, d_dcb + p.blk0, p.nblk, f.mx * f.my, f.hy * f.vy, f.ncomp - 1};
        uint8_t *y = static_cast<uint8_t *>(plv) + p.o_planes;
        it[i].planes[0] = y; it[i].planes[1] = y + p.b_y; it[i].planes[2] = y + p.b_y + p.b_c;
        it[i].ystride = 8 * f.hy * f.mx; it[i].cstride = 8 * f.mx;
        h_idct[i] = dec_idct_args(f, a.coef, d_dcb + p.blk0, d_dcs + p.blk0, it[i].planes);
        for (int c = f.ncomp; c < 3; c++) h_idct[i].nblocks[c] = 0;
        const int nwg = (p.nlanes + DEC_OWN - 1) / DEC_OWN, nwg_write = (p.nlanes + 255) / 256, nwg_gather = (p.nblk + 255) / 256,
                  nwg_idct = (h_idct[i].nblocks[0] + 255) / 256;
        for (int g = 0; g < nwg; g++) *w_sync++ = DecWg{i, g};
        for (int g = 1; g < nwg; g++) *w_fix++ = DecWg{i, g};
        for (int g = 0; g < nwg_write; g++) *w_write++ = DecWg{i, g};
        for (int g = 0; g < nwg_gather; g++) *w_gather++ = DecWg{i, g};
        for (int g = 0; g < nwg_idct; g++) *w_idct++ = DecWg{i, g};
    }
    FNX_HIP(hipMemcpyAsync(d_up2, hp2, up2, hipMemcpyHostToDevice, ctx->stream));
    const DecArgs *d_args = reinterpret_cast<const DecArgs *>(d_up2 + o_args);
    const DecWg *d_wsync = reinterpret_cast<const DecWg *>(d_up2 + o_wgs), *d_wfix = d_wsync + n_sync, *d_wwrite = d_wfix + n_fix,
                *d_wgather = d_wwrite + n_write, *d_widct = d_wgather + n_gather;

    // the RST forms when any file of the chunk has intervals (a file without them meets no boundary there: same states, same blocks)
    FNX_TRY(prof_begin(ctx, FNX_PROF_JPEG));
    if (any_rst) hipLaunchKernelGGL((jpeg_dsync_batch_kernel<false, true>), dim3(static_cast<unsigned>(n_sync)), dim3(256), 0, ctx->stream, d_args, d_wsync, d_flag);
    else hipLaunchKernelGGL((jpeg_dsync_batch_kernel<false, false>), dim3(static_cast<unsigned>(n_sync)), dim3(256), 0, ctx->stream, d_args, d_wsync, d_flag);
    FNX_HIP(hipGetLastError());
    note_route(ctx, FNX_PROF_JPEG, "jpeg_dsync_batch_kernel");
    FNX_TRY(prof_end(ctx));
    int rounds = 0;
    if (n_fix > 0) {
        uint32_t flags[64];
        int r = 0, rewound = 0;
        for (;;) {
            const int r0 = r;
            for (int k = 0; k < 2 && r < 64; k++, r++) {
                if (any_rst) hipLaunchKernelGGL((jpeg_dsync_batch_kernel<true, true>), dim3(static_cast<unsigned>(n_fix)), dim3(256), 0, ctx->stream, d_args, d_wfix, d_flag + r);
                else hipLaunchKernelGGL((jpeg_dsync_batch_kernel<true, false>), dim3(static_cast<unsigned>(n_fix)), dim3(256), 0, ctx->stream, d_args, d_wfix, d_flag + r);
            }
            FNX_HIP(hipGetLastError());
            FNX_TRY(fetch_bytes(ctx, d_flag, flags, sizeof(uint32_t) * static_cast<size_t>(r)));
            bool quiet = false;
            for (int k = r0; k < r; k++) quiet = quiet || flags[k] == 0;
            rounds = rewound + r;
            if (quiet) break;
            if (r >= 64) {
                FNX_HIP(hipMemsetAsync(d_flag, 0, 4 * 64, ctx->stream));
                rewound += r;
                r = 0;
            }
        }
    }
    FNX_TRY(launch_scan(ctx, d_cnt, d_first, d_tot, static_cast<int>(lanes), nullptr));
    if (any_rst) hipLaunchKernelGGL(jpeg_dwrite_batch_kernel<true>, dim3(static_cast<unsigned>(n_write)), dim3(256), 0, ctx->stream, d_args, d_wwrite);
    else hipLaunchKernelGGL(jpeg_dwrite_batch_kernel<false>, dim3(static_cast<unsigned>(n_write)), dim3(256), 0, ctx->stream, d_args, d_wwrite);
    hipLaunchKernelGGL(jpeg_dc_gather_batch_kernel, dim3(static_cast<unsigned>(n_gather)), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const DcArgs *>(d_up2 + o_dc), d_wgather);
    FNX_TRY(launch_scan(ctx, d_dcb, d_dcs, d_tot2, static_cast<int>(NB), nullptr));
    hipLaunchKernelGGL(jpeg_didct_batch_kernel, dim3(static_cast<unsigned>(n_idct), 3), dim3(256), 0, ctx->stream,
                       reinterpret_cast<const IdctArgs *>(d_up2 + o_idct), d_widct);
    FNX_HIP(hipGetLastError());
    std::vector<DecResult> res(m);
    FNX_TRY(fetch_bytes(ctx, d_res, res.data(), sizeof(DecResult) * m));
    for (int i = 0; i < m; i++) {
        if (!pl[i].live) continue;
        it[i].f.rounds = rounds;
        it[i].status = dec_verdict(res[i].err, res[i].blocks, pl[i].nblk);
    }
    return FNX_OK;
}

}  // namespace fnx
