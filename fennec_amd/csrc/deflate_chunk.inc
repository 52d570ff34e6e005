// The body of deflate.hip's two chunk kernels, included into each: chunk DF_CHUNK_INDEX of the stream `a` (a DeflateArgs)
// describes, every lane of its workgroup -- the parse into the chunk's token words, the block into its slot, its four meta
// words (DF_SIZE_ONLY 1: the parse and the block's byte count alone, deflate_codes.inc).  It is a file and not a __device__
// function because a function, simplified on its own before it is inlined, gives deflate_chunk_kernel other registers than
// the body written into it, and that kernel's figures are pinned (DESIGN.md 5.7).
    __shared__ uint32_t s_w[(DF_C + 64) / 4];                        // the chunk's bytes, later its output bits
    __shared__ uint32_t s_hash[1 << DF_HBITS];                       // position + 1; later three HuffWork
    __shared__ uint32_t s_llf[288], s_df[32], s_clf[20];
    __shared__ uint8_t s_lll[288], s_dl[32], s_cll[20];
    __shared__ uint16_t s_cltok[320];                                // symbol | extra value << 8
    __shared__ uint32_t s_adler[2];
#if !DF_SIZE_ONLY                                                    // the emit's: the codes, the lanes' bit counts, what lane 0 found
    __shared__ uint16_t s_llc[288], s_dc[32], s_clc[20];
    __shared__ uint32_t s_scan[DF_T];
    __shared__ uint32_t s_form, s_hlit, s_hdist, s_hclen, s_ncl, s_hdr_bits, s_nbytes;
#endif
    static_assert(3 * sizeof(HuffWork) <= sizeof(uint32_t) << DF_HBITS, "the Huffman work arrays take the hash table's words");

    const int tid = threadIdx.x;
    const uint32_t c = DF_CHUNK_INDEX;
    const size_t base = static_cast<size_t>(c) * DF_C;
    const int len = static_cast<int>(std::min<size_t>(DF_C, a.n - base));
    const bool last = c + 1 == a.nchunks;
    const uint8_t *src = a.src + base;
    uint8_t *s_b = reinterpret_cast<uint8_t *>(s_w);
    uint32_t *tok = a.tok + static_cast<size_t>(c) * DF_C;
    HuffWork *hw = reinterpret_cast<HuffWork *>(s_hash);

    // ---- the chunk into LDS
    if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0) {
        const int nd = len >> 2;
        for (int i = tid; i < nd; i += DF_T) s_w[i] = *(g_u32 *)(src + 4 * i);
        for (int i = 4 * nd + tid; i < len; i += DF_T) s_b[i] = src[i];
    } else {
        for (int i = tid; i < len; i += DF_T) s_b[i] = src[i];
    }
    for (int i = tid; i < (1 << DF_HBITS); i += DF_T) s_hash[i] = 0;
    for (int i = tid; i < 288; i += DF_T) s_llf[i] = i == 256 ? 1u : 0u;   // one end-of-block
    if (tid < 32) s_df[tid] = 0;
    if (tid < 20) s_clf[tid] = 0;
    if (tid < 2) s_adler[tid] = 0;
    __syncthreads();

    // ---- the hash candidate of every position, segment by segment: tok[p] = its distance, 0 for none
    for (int seg = 0; seg < len; seg += DF_T) {
        const int p = seg + tid;
        const bool hashed = p + 2 < len;
        uint32_t h = 0;
        if (hashed) {
            const uint32_t v = s_b[p] | (static_cast<uint32_t>(s_b[p + 1]) << 8) | (static_cast<uint32_t>(s_b[p + 2]) << 16);
            h = (v * 0x9e3779b1u) >> (32 - DF_HBITS);
            const uint32_t seen = s_hash[h];
            tok[p] = seen ? static_cast<uint32_t>(p) + 1u - seen : 0u;
        } else if (p < len) {
            tok[p] = 0;
        }
        __syncthreads();
        if (hashed) atomicMax(&s_hash[h], static_cast<uint32_t>(p) + 1u);
        __syncthreads();
    }

    // ---- the greedy parse of this lane's sub-chunk
    const int s0 = tid * DF_S, e0 = min(s0 + DF_S, len);
    int ntok = 0;
    {
        uint32_t asum = 0, bsum = 0;
        for (int p = s0; p < e0;) {
            const int maxl = min(258, e0 - p);
            int best = 0, bestd = 0;
            if (maxl >= 3) {
                const int hd = static_cast<int>(tok[p]);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int d = k == 0 ? 1 : k == 1 ? 2 : k == 2 ? 3 : k == 3 ? 4 : k == 4 ? 6 : k == 5 ? 8 : k == 6 ? a.row : hd;
                    if (d <= 0 || d > p) continue;
                    int l = 0;
                    while (l < maxl && s_b[p + l] == s_b[p - d + l]) l++;
                    if (l == 3 && d > 4096) continue;
                    if (l > best || (l == best && d < bestd)) { best = l; bestd = d; }
                }
            }
            if (best >= 3) {
                int sym, eb, ev;
                df_len_sym(best, sym, eb, ev);
                atomicAdd(&s_llf[sym], 1u);
                df_dist_sym(bestd, sym, eb, ev);
                atomicAdd(&s_df[sym], 1u);
                tok[s0 + ntok++] = df_match_tok(best, bestd);
                p += best;
            } else {
                const uint32_t b = s_b[p];
                atomicAdd(&s_llf[b], 1u);
                tok[s0 + ntok++] = b;
                p++;
            }
        }
        // Adler-32's sums of the sub-chunk, b against the CHUNK's end: at most 128 * 255 * 32768 < 2^32
        for (int i = s0; i < e0; i++) {
            const uint32_t x = s_b[i];
            asum += x;
            bsum += x * static_cast<uint32_t>(len - i);
        }
        if (s0 < e0) {
            atomicAdd(&s_adler[0], asum);                            // at most 32768 * 255
            atomicAdd(&s_adler[1], bsum % DF_ADLER);                 // at most 256 * 65520
        }
    }
    __syncthreads();

#include "deflate_codes.inc"
