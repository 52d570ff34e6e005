// A chunk-parallel deflate for gfx950: a zlib stream (RFC 1950) of deflate blocks (RFC 1951) from bytes that are already on
// the device -- the filtered scanlines of png_filter.hip above all.  No library code; the format, restated:
//
//  * RFC 1950: CMF = 0x78 (deflate, 32 KiB window), FLG = 0x01 (no dictionary, level 0, (CMF * 256 + FLG) % 31 == 0), the
//    deflate blocks, then Adler-32 of the input, big-endian: a = 1 + sum x[i], b = n + sum (n - i) x[i], both mod 65521,
//    b << 16 | a.
//  * RFC 1951: bits are packed from bit 0 of each byte upwards; Huffman codes go in most significant bit first (the code
//    tables below hold them bit-reversed), everything else least significant bit first.  A block starts with BFINAL (1 bit)
//    and BTYPE (2 bits): 00 stored (pad to a byte, LEN, ~LEN as 16-bit little-endian words, LEN bytes), 01 the fixed codes
//    (literal/length lengths 8 for 0..143, 9 for 144..255, 7 for 256..279, 8 for 280..287; distance codes 5 bits), 10
//    dynamic codes: HLIT - 257 (5 bits), HDIST - 1 (5), HCLEN - 4 (4), HCLEN code-length-code lengths of 3 bits in the order
//    16 17 18 0 8 7 9 6 10 5 11 4 12 3 13 2 14 1 15, then the HLIT + HDIST code lengths in that code: 0..15 a length, 16
//    repeat the previous length 3..6 times (2 extra bits), 17 / 18 a run of 3..10 / 11..138 zeros (3 / 7 extra bits).
//    Symbol 256 ends a block.  Length l = 3..258: symbol 257 + (l - 3) below 11; 285 for 258; else with e = msb(l - 3) - 2,
//    265 + 4 (e - 1) + (((l - 3) >> e) & 3) and e extra bits.  Distance d = 1..32768: symbol d - 1 below 5; else with
//    m = msb(d - 1), 2 m + (((d - 1) >> (m - 1)) & 1) and m - 1 extra bits.  Codes are canonical: within a length in symbol
//    order, lengths ascending.
//
// deflate_chunk_kernel: one workgroup of 256 lanes per chunk of FNX_DEFLATE_CHUNK = 32 KiB, the chunk's bytes in LDS.
//  * No match reaches behind its chunk's start; every chunk is ONE block and every chunk but the last ends with an empty
//    stored block (3 header bits, padding, 00 00 ff ff), so each chunk's output is whole bytes and the chunks concatenate by
//    a byte copy.  The last chunk carries BFINAL.
//  * Candidates for position p: the PNG distances 1, 2, 3, 4, 6, 8 and `row` (the stream's row length, 0: none), and one
//    hash candidate.  The hash table (4096 words of LDS, three bytes hashed) is filled segment by segment, 256 positions at
//    a time: every lane looks up, barrier, atomicMax of its own position, barrier -- a lookup sees positions of EARLIER
//    segments only, and the largest of them, so the candidate is a function of the input alone.  The longest match wins,
//    the smaller distance on ties; 3..258 bytes (a 3-byte match further than 4096 back costs more than its literals and
//    is not taken).
//  * Parse: lane t owns the sub-chunk [t S, (t + 1) S), S = FNX_DEFLATE_SUB = 128, and parses it greedily; sub-chunk starts
//    are token boundaries, a match is cut at its sub-chunk's end (it may START before it).  Tokens go to the chunk's region
//    of global scratch, one word each -- the region first holds the hash candidates of the chunk's positions: a lane reads
//    position p's word before it writes token k <= p - t S over a word in front of it.
//  * Codes: both histograms by LDS atomics while parsing; symbols ranked by (count, symbol) in parallel; the Huffman trees by
//    the two-queue merge on one lane each (literal/length on lane 0, distance on lane 64); depths above 15 (7 for the
//    code-length code) are folded into the limit and the Kraft sum repaired by moving one code down a level at a time;
//    lengths are handed out by rank.  A block without a match still sends one distance code (symbol 0, one bit); a code with
//    a single symbol gets one bit (the code-length code, which inflate wants complete, a second unused one).
//    The block takes the smallest of dynamic, fixed and stored; stored is one block (LEN is 16 bits: static_assert below).
//  * Emit: lanes add up their tokens' bits, an exclusive prefix sum over the workgroup gives each lane its bit offset, lanes
//    OR their bits into the LDS words that held the chunk (zeroed; integer OR: any order gives the same bytes), and the
//    words go to the chunk's slot (sized by the stored bound) as dword vector stores.  Each chunk writes its byte count and
//    its Adler-32 partial (a, b, len).
// deflate_gather_kernel: one workgroup per chunk: the sum of the byte counts in front of it (the prefix sum, every
// workgroup for itself), the two header bytes, the byte copy into the caller's buffer (aligned dwords by v_alignbyte), the
// combined Adler-32 behind the last chunk, the total size in a result word.  A total above `cap` writes nothing.
//
// deflate_chunk_batch_kernel, deflate_gather_batch_kernel (fnx_png_compress_batch): the same two bodies over the streams of a
// batch -- a workgroup per 32 KiB of ANY stream, the unit {source, length, row, last-of-stream, stream} read through the scalar
// cache; the gather places a chunk by the prefix over its own stream's units and the stream by the sum over the units in front,
// so the streams lie back to back at their true sizes.  The chunk body is deflate_chunk.inc, included into both chunk kernels.
//
// deflate_dense_chunk_kernel, deflate_dense_chunk_batch_kernel (fnx_ctx_set_deflate_level, FNX_DEFLATE_LEVEL_DENSE): the same
// layout, slots and gather behind another parse -- hash chains, a window that reaches into the previous chunk, uncut matches,
// one lazy step; see the comment in front of them, deflate_dense_chunk.inc and DESIGN.md section 5.12.  The codes / form / emit
// half of a chunk body is deflate_codes.inc, shared by deflate_chunk.inc and deflate_dense_chunk.inc.
//
// deflate_chunk_size_kernel, deflate_dense_chunk_size_kernel, deflate_size_kernel (deflate_size.inc; fnx_png_encoded_size, the PNG legs):
// the SIZE-ONLY forms -- the chunk bodies with DF_SIZE_ONLY 1 end where lane 0 knows the block's form and bit count and write the
// chunk's byte count (what the emitting form writes into meta[0]) and nothing else: no codes, no bits, no slot; one workgroup
// adds the counts and the 6 bytes of framing.  56 / 54 VGPRs, 51568 / 151408 bytes of LDS, no scratch -- DESIGN.md section 5.15.
//
// Resources (hipcc --offload-arch=gfx950 -O3, -Rpass-analysis=kernel-resource-usage): no scratch in any kernel;
// VGPRs: see DESIGN.md section 5.7 (the figures are the compiler's and are restated there with the LDS sizes); the batched
// kernels have their twins' figures: 60 VGPRs / 53296 bytes of LDS (chunk), 34 / 32 (gather) -- DESIGN.md section 5.10; the
// dense chunk kernels 61 VGPRs / 152116 bytes of LDS -- section 5.12.
#include "common.hpp"
#include "devutil.hpp"
#include "deflate_batch.hpp"

#include <algorithm>

namespace fnx {

constexpr int DF_T = 256;                          // lanes per workgroup
constexpr int DF_C = FNX_DEFLATE_CHUNK;
constexpr int DF_S = FNX_DEFLATE_SUB;              // a lane's sub-chunk
constexpr int DF_HBITS = 12;
constexpr int DF_SLOT = DEFLATE_SLOT_BYTES;        // a chunk's output slot: stored bound C + 10, dword reads one past the end
constexpr uint32_t DF_ADLER = 65521u;
constexpr int DF_STORED = 0, DF_FIXED = 1, DF_DYNAMIC = 2;   // BTYPE
constexpr int DF_DENSE_WORDS = 2 * DF_C + DF_C / 2; // the dense level's scratch words per chunk: tokens, the (L, D) table, the previous chunk's links (16 bits each)
static_assert(DF_S * DF_T == DF_C && DF_S >= 64, "equal sub-chunks of at least 64 bytes");
static_assert(DF_C <= 32768, "distances are at most 32768; a stored block's LEN is 16 bits");

__device__ const uint8_t DF_CLORD[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct DeflateArgs {
    const uint8_t *src;
    size_t n;
    int row;
    uint32_t nchunks;
    uint32_t *tok;                       // DF_C words per chunk
    uint8_t *slots;                      // DF_SLOT bytes per chunk, 16-byte aligned
    uint32_t *meta;                      // per chunk: bytes, adler a, adler b, len
};

// one Huffman build's work arrays (LDS: the hash table's words, which are dead by then)
struct HuffWork {
    uint32_t ifreq[288];                 // internal nodes: weight, later depth
    uint16_t iparent[288];
    uint16_t lparent[288];
    uint16_t order[288];                 // symbols with a count, ascending by (count, symbol)
    uint32_t count[16];                  // codes per length
};

// symbol and extra bits of a match length / distance
__device__ __forceinline__ void df_len_sym(int l, int &sym, int &ebits, int &eval)
{
    const int l3 = l - 3;
    if (l3 < 8) { sym = 257 + l3; ebits = 0; eval = 0; return; }
    if (l3 == 255) { sym = 285; ebits = 0; eval = 0; return; }
    const int e = 29 - __clz(l3);
    sym = 261 + 4 * e + ((l3 >> e) & 3);
    ebits = e;
    eval = l3 & ((1 << e) - 1);
}
__device__ __forceinline__ void df_dist_sym(int d, int &sym, int &ebits, int &eval)
{
    const int d1 = d - 1;
    if (d1 < 4) { sym = d1; ebits = 0; eval = 0; return; }
    const int m = 31 - __clz(d1);
    sym = 2 * m + ((d1 >> (m - 1)) & 1);
    ebits = m - 1;
    eval = d1 & ((1 << (m - 1)) - 1);
}
__device__ __forceinline__ int df_len_ebits(int sym) { return sym >= 265 && sym < 285 ? (sym - 261) >> 2 : 0; }
__device__ __forceinline__ int df_dist_ebits(int sym) { return sym >= 4 ? (sym >> 1) - 1 : 0; }
__device__ __forceinline__ int df_fixed_len(int sym) { return sym < 144 ? 8 : (sym < 256 ? 9 : (sym < 280 ? 7 : 8)); }

// a token: a literal byte, or 1 << 31 | (len - 3) << 16 | (dist - 1)
__device__ __forceinline__ uint32_t df_match_tok(int len, int dist) { return 0x80000000u | (static_cast<uint32_t>(len - 3) << 16) | static_cast<uint32_t>(dist - 1); }

// order[r] = the symbol of rank r among those with a count, by (count, symbol); every lane of the workgroup
__device__ __forceinline__ void df_rank(const uint32_t *freq, int n, uint16_t *order, int tid)
{
    for (int s = tid; s < n; s += DF_T) {
        const uint32_t f = freq[s];
        if (!f) continue;
        int r = 0;
        for (int j = 0; j < n; j++) {
            const uint32_t g = freq[j];
            r += (g != 0 && (g < f || (g == f && j < s))) ? 1 : 0;
        }
        order[r] = static_cast<uint16_t>(s);
    }
}

// code lengths of at most maxbits from counts and their ranking; ONE lane
__device__ void df_build_lengths(const uint32_t *freq, int n, int maxbits, uint8_t *lens, HuffWork &w)
{
    int m = 0;
    for (int j = 0; j < n; j++) {
        lens[j] = 0;
        m += freq[j] != 0 ? 1 : 0;
    }
    if (m == 0) return;
    if (m == 1) { lens[w.order[0]] = 1; return; }
    // the two-queue merge: leaves in rank order, internal nodes in the order they are made (their weights never decrease)
    int li = 0, ii = 0;
    for (int k = 0; k < m - 1; k++) {
        uint32_t f = 0;
        for (int t = 0; t < 2; t++) {
            const uint32_t lf = li < m ? freq[w.order[li]] : 0u;
            if (li < m && (ii >= k || lf <= w.ifreq[ii])) { w.lparent[li] = static_cast<uint16_t>(k); f += lf; li++; }
            else { w.iparent[ii] = static_cast<uint16_t>(k); f += w.ifreq[ii]; ii++; }
        }
        w.ifreq[k] = f;
    }
    w.ifreq[m - 2] = 0;                                              // the root's depth; a parent is made after its children
    for (int k = m - 3; k >= 0; k--) w.ifreq[k] = w.ifreq[w.iparent[k]] + 1;
    for (int l = 0; l < 16; l++) w.count[l] = 0;
    for (int i = 0; i < m; i++) {
        const int d = static_cast<int>(w.ifreq[w.lparent[i]]) + 1;
        w.count[min(d, maxbits)]++;                                  // deeper than the limit: folded into it
    }
    uint32_t total = 0;
    for (int l = 1; l <= maxbits; l++) total += w.count[l] << (maxbits - l);
    while (total > (1u << maxbits)) {                                // each round takes 2^-maxbits off the Kraft sum
        w.count[maxbits]--;
        for (int l = maxbits - 1; l > 0; l--) {
            if (w.count[l]) { w.count[l]--; w.count[l + 1] += 2; break; }
        }
        total--;
    }
    int i = m - 1;                                                   // the most frequent symbol takes the shortest code
    for (int l = 1; l <= maxbits; l++) {
        for (uint32_t c = w.count[l]; c > 0; c--) lens[w.order[i--]] = static_cast<uint8_t>(l);
    }
}

// canonical codes, bit-reversed for the stream; every lane of the workgroup
__device__ __forceinline__ void df_assign_codes(const uint8_t *lens, int n, uint16_t *codes, int tid)
{
    for (int s = tid; s < n; s += DF_T) {
        const int L = lens[s];
        uint32_t code = 0;
        if (L) {
            for (int j = 0; j < n; j++) {
                const int lj = lens[j];
                if (lj && lj < L) code += 1u << (L - lj);            // the first code of length L
                else if (lj == L && j < s) code++;
            }
            code = __brev(code) >> (32 - L);
        }
        codes[s] = static_cast<uint16_t>(code);
    }
}

// a lane's bit writer into the workgroup's LDS words
struct DfBits {
    uint32_t *w;
    uint64_t acc;
    int nacc;                            // < 32 between calls
    uint32_t word;
    __device__ __forceinline__ DfBits(uint32_t *words, uint32_t bitpos) : w(words), acc(0), nacc(static_cast<int>(bitpos & 31u)), word(bitpos >> 5) {}
    __device__ __forceinline__ void put(uint32_t v, int n)           // n <= 31
    {
        acc |= static_cast<uint64_t>(v) << nacc;
        nacc += n;
        if (nacc >= 32) {
            atomicOr(&w[word++], static_cast<uint32_t>(acc));
            acc >>= 32;
            nacc -= 32;
        }
    }
    __device__ __forceinline__ uint32_t pos() const { return (word << 5) + static_cast<uint32_t>(nacc); }
    __device__ __forceinline__ void align8() { put(0u, (8 - (nacc & 7)) & 7); }
    __device__ __forceinline__ void flush() { if (nacc > 0) atomicOr(&w[word], static_cast<uint32_t>(acc)); }
};

__global__ __launch_bounds__(DF_T) void deflate_chunk_kernel(DeflateArgs a)
{
#define DF_CHUNK_INDEX blockIdx.x
#define DF_SIZE_ONLY 0
#include "deflate_chunk.inc"
#undef DF_SIZE_ONLY
#undef DF_CHUNK_INDEX
}

// The streams of a batch in one launch each (the PNG compress batch): unit c -- a chunk of any stream -- has token words, slot
// and meta words c; the unit and, in the gather, its stream's record come through the scalar cache.
struct DeflateBatchArgs {
    const DeflateBatchUnit *units;
    const DeflateBatchImage *images;
    uint32_t *tok;                       // DF_C words per unit
    uint8_t *slots;                      // DF_SLOT bytes per unit, 16-byte aligned
    uint32_t *meta;                      // per unit: bytes, adler a, adler b, len
    uint8_t *out;                        // the zlib streams one behind another, stream i at 6 i + the block bytes of the units in front of its first
    unsigned long long *sizes;           // per stream
};

__global__ __launch_bounds__(DF_T) void deflate_chunk_batch_kernel(DeflateBatchArgs b)
{
    const DeflateBatchUnit u = b.units[blockIdx.x];
    DeflateArgs a;                                                   // the unit as chunk 0 of a stream of its own bytes
    a.src = u.src; a.n = u.len; a.row = u.row;
    a.nchunks = u.last ? 1u : 2u;                                    // (a chunk is the last one when none follows)
    a.tok = b.tok + static_cast<size_t>(blockIdx.x) * DF_C;
    a.slots = b.slots + static_cast<size_t>(blockIdx.x) * DF_SLOT;
    a.meta = b.meta + 4 * static_cast<size_t>(blockIdx.x);
#define DF_CHUNK_INDEX 0u
#define DF_SIZE_ONLY 0
#include "deflate_chunk.inc"
#undef DF_SIZE_ONLY
#undef DF_CHUNK_INDEX
}

// ---- the dense level (fnx_ctx_set_deflate_level): the same launches, arguments, slots and gather, another
// parse.  The window is the previous chunk and the own one, 64 KiB of LDS; hash chains FNX_DEFLATE_DENSE_DEPTH deep, uncut
// matches, one step of lazy evaluation -- deflate_dense_chunk.inc.  152 116 bytes of LDS: a workgroup has its CU to itself.

// bytes i .. i + 3 of the window's words (v_alignbyte over two aligned dwords)
__device__ __forceinline__ uint32_t df_ld4(const uint32_t *w, int i) { return __builtin_amdgcn_alignbyte(w[(i >> 2) + 1], w[i >> 2], i & 3); }
// how many of the maxl bytes from a on equal those from b on, a dword at a time (reads up to 7 bytes behind a + maxl)
__device__ __forceinline__ int df_match_len(const uint32_t *w, int a, int b, int maxl)
{
    int l = 0;
    while (l < maxl) {
        const uint32_t x = df_ld4(w, a + l) ^ df_ld4(w, b + l);
        if (x) { l += __builtin_ctz(x) >> 3; break; }
        l += 4;
    }
    return min(l, maxl);
}

__global__ __launch_bounds__(DF_T) void deflate_dense_chunk_kernel(DeflateArgs a)
{
#define DF_CHUNK_INDEX blockIdx.x
#define DF_STREAM_POS base
#define DF_SIZE_ONLY 0
#include "deflate_dense_chunk.inc"
#undef DF_SIZE_ONLY
#undef DF_STREAM_POS
#undef DF_CHUNK_INDEX
}

// unit c as chunk 0 of a stream of its own bytes, as in deflate_chunk_batch_kernel -- but the bytes in front of it are its
// stream's: the unit's place in the stream is its distance from the stream's first unit
__global__ __launch_bounds__(DF_T) void deflate_dense_chunk_batch_kernel(DeflateBatchArgs b)
{
    const DeflateBatchUnit u = b.units[blockIdx.x];
    const uint32_t first = b.images[u.image].chunk0;
    DeflateArgs a;
    a.src = u.src; a.n = u.len; a.row = u.row;
    a.nchunks = u.last ? 1u : 2u;
    a.tok = b.tok + static_cast<size_t>(blockIdx.x) * DF_DENSE_WORDS;
    a.slots = b.slots + static_cast<size_t>(blockIdx.x) * DF_SLOT;
    a.meta = b.meta + 4 * static_cast<size_t>(blockIdx.x);
#define DF_CHUNK_INDEX 0u
#define DF_STREAM_POS (static_cast<size_t>(blockIdx.x - first) * DF_C)
#define DF_SIZE_ONLY 0
#include "deflate_dense_chunk.inc"
#undef DF_SIZE_ONLY
#undef DF_STREAM_POS
#undef DF_CHUNK_INDEX
}

struct GatherArgs {
    const uint8_t *slots;
    const uint32_t *meta;
    uint32_t nchunks;
    size_t n;
    uint8_t *out;
    size_t cap;
    unsigned long long *result;          // the stream's size
};

// the sum of v over the workgroup, in every lane (s_red: 4 words; two barriers)
__device__ __forceinline__ unsigned long long df_block_sum(unsigned long long v, unsigned long long *s_red)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    __syncthreads();                                                 // the previous sum has been read
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// Chunk c of the stream `a` describes, every lane of the workgroup: `before` block bytes of the stream lie in front of the
// chunk's, `all` is the stream's sum.  Both gather kernels are this body behind their own prefix sums.
__device__ __forceinline__ void df_gather(const GatherArgs &a, const uint32_t c, const unsigned long long before, const unsigned long long all,
                                          unsigned long long *s_red)
{
    const int tid = threadIdx.x;
    const unsigned long long size = 2 + all + 4;
    if (c == 0 && tid == 0) *a.result = size;
    if (size > a.cap) return;                                        // the caller is told the size and nothing is written
    if (c == 0 && tid == 0) { a.out[0] = 0x78; a.out[1] = 0x01; }

    const int nb = static_cast<int>(a.meta[4 * static_cast<size_t>(c)]);
    const uint8_t *s = a.slots + static_cast<size_t>(c) * DF_SLOT;
    uint8_t *dst = a.out + 2 + before;
    const int head = min(nb, static_cast<int>((4u - (reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u));
    const int nd = (nb - head) >> 2;
    if (tid < head) dst[tid] = s[tid];
    for (int i = tid; i < nd; i += DF_T) {
        const int j = head + 4 * i;                                  // dst + j is dword aligned; the slot's dwords j >> 2 and the next hold it
        const uint32_t lo = *(g_u32 *)(s + (j & ~3)), hi = *(g_u32 *)(s + (j & ~3) + 4);
        *(g_u32w *)(dst + j) = __builtin_amdgcn_alignbyte(hi, lo, j & 3);
    }
    for (int k = head + 4 * nd + tid; k < nb; k += DF_T) dst[k] = s[k];

    if (c + 1 == a.nchunks) {
        // Adler-32 of the whole: a = 1 + sum a_j, b = n + sum (b_j + (n - end_j) a_j), end_j the input offset behind chunk j
        unsigned long long sa = 0, sb = 0;
        for (uint32_t j = tid; j < a.nchunks; j += DF_T) {
            const uint32_t *m = a.meta + 4 * static_cast<size_t>(j);
            const unsigned long long end = static_cast<unsigned long long>(j) * DF_C + m[3];
            sa += m[1];
            sb += m[2] + ((a.n - end) % DF_ADLER) * m[1];            // below 2^33 a term
        }
        sa = df_block_sum(sa, s_red);
        sb = df_block_sum(sb, s_red);
        if (tid == 0) {
            const uint32_t av = static_cast<uint32_t>((1 + sa) % DF_ADLER);
            const uint32_t bv = static_cast<uint32_t>((a.n % DF_ADLER + sb) % DF_ADLER);
            uint8_t *t = a.out + 2 + all;
            t[0] = static_cast<uint8_t>(bv >> 8); t[1] = static_cast<uint8_t>(bv);
            t[2] = static_cast<uint8_t>(av >> 8); t[3] = static_cast<uint8_t>(av);
        }
    }
}

__global__ __launch_bounds__(DF_T) void deflate_gather_kernel(GatherArgs a)
{
    __shared__ unsigned long long s_red[4];
    const int tid = threadIdx.x;
    const uint32_t c = blockIdx.x;
    unsigned long long before = 0, all = 0;
    for (uint32_t j = tid; j < a.nchunks; j += DF_T) {
        const unsigned long long nb = a.meta[4 * static_cast<size_t>(j)];
        all += nb;
        if (j < c) before += nb;
    }
    before = df_block_sum(before, s_red);
    all = df_block_sum(all, s_red);
    df_gather(a, c, before, all, s_red);
}

#include "deflate_size.inc"

// A workgroup per unit: the prefix over its OWN stream's units places the chunk inside the stream, the sum over the units of
// the streams in front places the stream -- stream i starts at out + 6 i + that sum, so the streams lie back to back at their
// true sizes and one copy of sum(sizes) bytes brings them all down.  Nothing depends on the order the workgroups run in.
__global__ __launch_bounds__(DF_T) void deflate_gather_batch_kernel(DeflateBatchArgs a)
{
    __shared__ unsigned long long s_red[4];
    const int tid = threadIdx.x;
    const uint32_t c = blockIdx.x;
    const uint32_t image = a.units[c].image;
    const DeflateBatchImage im = a.images[image];
    unsigned long long front = 0, before = 0, all = 0;
    for (uint32_t j = tid; j < im.chunk0 + im.nchunks; j += DF_T) {
        const unsigned long long nb = a.meta[4 * static_cast<size_t>(j)];
        if (j < im.chunk0) front += nb;
        else {
            all += nb;
            if (j < c) before += nb;
        }
    }
    front = df_block_sum(front, s_red);
    before = df_block_sum(before, s_red);
    all = df_block_sum(all, s_red);
    GatherArgs g;
    g.slots = a.slots + static_cast<size_t>(im.chunk0) * DF_SLOT;
    g.meta = a.meta + 4 * static_cast<size_t>(im.chunk0);
    g.nchunks = im.nchunks;
    g.n = static_cast<size_t>(im.n);
    g.out = a.out + 6 * static_cast<size_t>(image) + front;
    g.cap = ~size_t(0);                                              // the area holds every stream's bound
    g.result = a.sizes + image;
    df_gather(g, c - im.chunk0, before, all, s_red);
}

int launch_deflate(fnx_ctx *ctx, const uint8_t *d_src, size_t n, int row, uint8_t *d_out, size_t cap, const unsigned long long **d_size)
{
    const size_t nchunks = deflate_chunks(n);
    const bool dense = ctx->deflate_level == FNX_DEFLATE_LEVEL_DENSE;
    void *dt = nullptr, *ds = nullptr;
    FNX_TRY(scratch(ctx, SLOT_DEFLATE_TOK, nchunks * (dense ? DF_DENSE_WORDS : DF_C) * sizeof(uint32_t) + 16, &dt));
    // the result word (16 bytes: the size, and room for the PNG route's CRC word), the chunks' (bytes, a, b, len), the chunks' slots
    const size_t meta_bytes = (16 * nchunks + 16 + 15) & ~size_t(15);
    FNX_TRY(scratch(ctx, SLOT_DEFLATE_SLOTS, meta_bytes + nchunks * DF_SLOT + 16, &ds));
    uint8_t *p = static_cast<uint8_t *>(ds);
    DeflateArgs da{};
    da.src = d_src; da.n = n; da.row = deflate_row_hint(row); da.nchunks = static_cast<uint32_t>(nchunks);
    da.tok = static_cast<uint32_t *>(dt);
    da.meta = reinterpret_cast<uint32_t *>(p + 16);
    da.slots = p + meta_bytes;
    note_route(ctx, FNX_PROF_MAIN, dense ? "deflate_dense_chunk_kernel" : "deflate_chunk_kernel");
    FNX_TRY(prof_begin(ctx));
    if (dense) hipLaunchKernelGGL(deflate_dense_chunk_kernel, dim3(da.nchunks), dim3(DF_T), 0, ctx->stream, da);
    else hipLaunchKernelGGL(deflate_chunk_kernel, dim3(da.nchunks), dim3(DF_T), 0, ctx->stream, da);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    GatherArgs ga{};
    ga.slots = da.slots; ga.meta = da.meta; ga.nchunks = da.nchunks; ga.n = n; ga.out = d_out; ga.cap = cap;
    ga.result = reinterpret_cast<unsigned long long *>(p);
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(deflate_gather_kernel, dim3(da.nchunks), dim3(DF_T), 0, ctx->stream, ga);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    *d_size = ga.result;
    return FNX_OK;
}

// launch_deflate's size: the chunk kernels' size-only forms and deflate_size_kernel.  The token words as launch_deflate asks for
// them (the parse lives there); no slot area and no output -- the result word and the chunks' meta words in a slot of their own
int launch_deflate_size(fnx_ctx *ctx, const uint8_t *d_src, size_t n, int row, const unsigned long long **d_size)
{
    const size_t nchunks = deflate_chunks(n);
    const bool dense = ctx->deflate_level == FNX_DEFLATE_LEVEL_DENSE;
    void *dt = nullptr, *dm = nullptr;
    FNX_TRY(scratch(ctx, SLOT_DEFLATE_TOK, nchunks * (dense ? DF_DENSE_WORDS : DF_C) * sizeof(uint32_t) + 16, &dt));
    FNX_TRY(scratch(ctx, SLOT_DEFLATE_SIZE, 16 + 16 * nchunks, &dm));
    uint8_t *p = static_cast<uint8_t *>(dm);
    DeflateArgs da{};
    da.src = d_src; da.n = n; da.row = deflate_row_hint(row); da.nchunks = static_cast<uint32_t>(nchunks);
    da.tok = static_cast<uint32_t *>(dt);
    da.meta = reinterpret_cast<uint32_t *>(p + 16);
    note_route(ctx, FNX_PROF_MAIN, dense ? "deflate_dense_chunk_size_kernel" : "deflate_chunk_size_kernel");
    FNX_TRY(prof_begin(ctx));
    if (dense) hipLaunchKernelGGL(deflate_dense_chunk_size_kernel, dim3(da.nchunks), dim3(DF_T), 0, ctx->stream, da);
    else hipLaunchKernelGGL(deflate_chunk_size_kernel, dim3(da.nchunks), dim3(DF_T), 0, ctx->stream, da);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    unsigned long long *result = reinterpret_cast<unsigned long long *>(p);
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(deflate_size_kernel, dim3(1), dim3(DF_T), 0, ctx->stream, da.meta, da.nchunks, result);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    *d_size = result;
    return FNX_OK;
}

// d_units / d_images: DEVICE tables of the batch's nunits units (sorted by stream, a stream's units in order) and m streams;
// out_bytes: the sum of the streams' bounds.  *d_out: the streams back to back (see the gather), *d_sizes: their m sizes.
int launch_deflate_batch(fnx_ctx *ctx, const DeflateBatchUnit *d_units, const DeflateBatchImage *d_images, uint32_t nunits, uint32_t m,
                         size_t out_bytes, const uint8_t **d_out, const unsigned long long **d_sizes)
{
    const bool dense = ctx->deflate_level == FNX_DEFLATE_LEVEL_DENSE;
    void *dt = nullptr, *ds = nullptr, *dz = nullptr;
    FNX_TRY(scratch(ctx, SLOT_DEFLATE_TOK, static_cast<size_t>(nunits) * (dense ? DF_DENSE_WORDS : DF_C) * sizeof(uint32_t) + 16, &dt));
    // the streams' sizes (and a word each behind them for crc32.hip's CRCs), the units' (bytes, a, b, len), the units' slots
    const size_t sizes_bytes = (12 * static_cast<size_t>(m) + 15) & ~size_t(15);
    const size_t meta_bytes = 16 * static_cast<size_t>(nunits);
    FNX_TRY(scratch(ctx, SLOT_DEFLATE_SLOTS, sizes_bytes + meta_bytes + static_cast<size_t>(nunits) * DF_SLOT + 16, &ds));
    FNX_TRY(scratch(ctx, SLOT_DEFLATE_OUT, out_bytes + 16, &dz));
    uint8_t *p = static_cast<uint8_t *>(ds);
    DeflateBatchArgs a{};
    a.units = d_units; a.images = d_images;
    a.tok = static_cast<uint32_t *>(dt);
    a.sizes = reinterpret_cast<unsigned long long *>(p);
    a.meta = reinterpret_cast<uint32_t *>(p + sizes_bytes);
    a.slots = p + sizes_bytes + meta_bytes;
    a.out = static_cast<uint8_t *>(dz);
    FNX_TRY(prof_begin(ctx));
    if (dense) hipLaunchKernelGGL(deflate_dense_chunk_batch_kernel, dim3(nunits), dim3(DF_T), 0, ctx->stream, a);
    else hipLaunchKernelGGL(deflate_chunk_batch_kernel, dim3(nunits), dim3(DF_T), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(deflate_gather_batch_kernel, dim3(nunits), dim3(DF_T), 0, ctx->stream, a);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    *d_out = a.out;
    *d_sizes = a.sizes;
    return FNX_OK;
}

}  // namespace fnx
