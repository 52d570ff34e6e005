// The body of deflate.hip's two DENSE chunk kernels (FNX_DEFLATE_LEVEL_DENSE), included into each: chunk DF_CHUNK_INDEX of the
// stream `a` (a DeflateArgs) describes, every lane of its workgroup; DF_STREAM_POS is the position of the chunk's first byte
// in its stream (0: nothing lies in front; else the whole previous chunk does, at src - DF_C).  The stream's rules are stated
// above fnx_ctx_set_deflate_level (fennec_hip.h) and in DESIGN.md section 5.12; the steps:
//  1. the window into LDS: the previous chunk's bytes at [0, DF_C), the own at [DF_C, DF_C + len).
//  2. the chains: the window's positions in segments of 256 as in deflate_chunk.inc (look up, barrier, atomicMax, barrier),
//     then a search inside the segment.  A position's LINK is the distance to the next position of its chain: the next
//     smaller position of its hash in its own segment, from the smallest of them the largest one of the earlier segments --
//     in all, the largest earlier position of the window with its hash.  0: none, or further than 32768.  Own positions'
//     links in LDS, the previous chunk's in the chunk's scratch.
//  3. (L, D) of every own position into the table words of the chunk's scratch: lane t its sub-chunk's 128 positions.
//  4. the lazy walk: every lane walks its sub-chunk from a guessed entry and marks what it visits; a lane's true entry is the
//     lane in front's exit; an entry that is marked leaves the exit as it is, any other is walked again; until no exit moves.
//     Then entry(0) = 0, entry(t) = exit(t - 1), exit(t) = the walk's from entry(t): the serial walk's, by induction on t.
//  5. the tokens of the lane's part of the walk into the token words (NOT the table's: a lane reads the next lane's L), the
//     histograms, Adler-32; then deflate_codes.inc as in the fast kernel.
    __shared__ uint32_t s_win[(2 * DF_C + 64) / 4];                  // the window; its second half later the output bits
    __shared__ uint16_t s_link[DF_C];
    __shared__ uint32_t s_hash[1 << DF_HBITS];                       // position + 1; then the walk's marks; later three HuffWork
    __shared__ uint32_t s_llf[288], s_df[32], s_clf[20];
    __shared__ uint8_t s_lll[288], s_dl[32], s_cll[20];
#if !DF_SIZE_ONLY                                                    // the emit's codes
    __shared__ uint16_t s_llc[288], s_dc[32], s_clc[20];
#endif
    __shared__ uint16_t s_cltok[320];                                // symbol | extra value << 8
    __shared__ uint32_t s_scan[DF_T];                                // the lanes' exits; later their bit counts
    __shared__ uint32_t s_adler[2];
    __shared__ uint32_t s_moved;
    __shared__ uint16_t s_segh[DF_T];                                // the hashes of a segment's positions
#if !DF_SIZE_ONLY                                                    // what lane 0 found, for the emit
    __shared__ uint32_t s_form, s_hlit, s_hdist, s_hclen, s_ncl, s_hdr_bits, s_nbytes;
#endif
    static_assert(3 * sizeof(HuffWork) <= sizeof(uint32_t) << DF_HBITS, "the Huffman work arrays take the hash table's words");
    static_assert(4 * DF_T <= (1 << DF_HBITS) && DF_S == 128, "a lane's marks are four words of the hash table's");

    const int tid = threadIdx.x;
    const uint32_t c = DF_CHUNK_INDEX;
    const size_t base = static_cast<size_t>(c) * DF_C;
    const int len = static_cast<int>(std::min<size_t>(DF_C, a.n - base));
    const bool last = c + 1 == a.nchunks;
    const bool has_prev = (DF_STREAM_POS) != 0;
    const uint8_t *src = a.src + base;
    uint8_t *s_wb = reinterpret_cast<uint8_t *>(s_win);
#if !DF_SIZE_ONLY
    uint32_t *s_w = s_win + DF_C / 4;                                // the own chunk's words
#endif
    uint8_t *s_b = s_wb + DF_C;
    uint32_t *tok = a.tok + static_cast<size_t>(c) * DF_DENSE_WORDS;
    uint32_t *tab = tok + DF_C;                                      // L << 16 | D - 1 of every own position, 0: no match
    uint16_t *plink = reinterpret_cast<uint16_t *>(tab + DF_C);      // the previous chunk's links
    HuffWork *hw = reinterpret_cast<HuffWork *>(s_hash);
    uint32_t *mark = s_hash + 4 * tid;

    // ---- the window into LDS
    const int w0 = has_prev ? 0 : DF_C, wend = DF_C + len;
    if ((reinterpret_cast<uintptr_t>(src) & 3u) == 0) {
        for (int i = (w0 >> 2) + tid; i < (wend >> 2); i += DF_T) s_win[i] = *(g_u32 *)(src + (4 * i - DF_C));
        for (int i = (wend & ~3) + tid; i < wend; i += DF_T) s_wb[i] = src[i - DF_C];
    } else {
        for (int i = w0 + tid; i < wend; i += DF_T) s_wb[i] = src[i - DF_C];
    }
    if (tid < 8) s_wb[wend + tid] = 0;                               // what a dword compare reads behind the last byte
    for (int i = tid; i < (1 << DF_HBITS); i += DF_T) s_hash[i] = 0;
    for (int i = tid; i < 288; i += DF_T) s_llf[i] = i == 256 ? 1u : 0u;   // one end-of-block
    if (tid < 32) s_df[tid] = 0;
    if (tid < 20) s_clf[tid] = 0;
    if (tid < 2) s_adler[tid] = 0;
    __syncthreads();

    // ---- the chains: every window position's link, segment by segment.  A position first links to what the table holds -- the
    // largest position of the EARLIER segments with its hash; after the segment's atomicMax every position but the largest of
    // its hash looks upwards for the next one of its hash in the segment and makes that one link to itself instead.
    for (int seg = w0; seg < wend; seg += DF_T) {
        const int wp = seg + tid;
        const bool hashed = wp + 2 < wend;
        const uint32_t key = static_cast<uint32_t>(wp) + 1u;
        uint32_t h = 0xffffu;                                        // no position's hash
        if (wp < wend) {
            uint32_t link = 0;
            if (hashed) {
                const uint32_t v = s_wb[wp] | (static_cast<uint32_t>(s_wb[wp + 1]) << 8) | (static_cast<uint32_t>(s_wb[wp + 2]) << 16);
                h = (v * 0x9e3779b1u) >> (32 - DF_HBITS);
                const uint32_t seen = s_hash[h];
                link = seen ? key - seen : 0u;
                if (link > 32768u) link = 0;
            }
            if (wp < DF_C) plink[wp] = static_cast<uint16_t>(link);
            else s_link[wp - DF_C] = static_cast<uint16_t>(link);
        }
        __syncthreads();                                             // every lane has looked up (and is past the search below)
        s_segh[tid] = static_cast<uint16_t>(h);
        if (hashed) atomicMax(&s_hash[h], key);
        __syncthreads();
        if (hashed && s_hash[h] != key) {                            // not the largest: one of the lanes above has the hash
            int up = 1;
            while (tid + up < DF_T - 1 && s_segh[tid + up] != h) up++;   // (it is there: the bound only keeps the search inside the segment)
            if (wp + up < DF_C) plink[wp + up] = static_cast<uint16_t>(up);
            else s_link[wp + up - DF_C] = static_cast<uint16_t>(up);
        }
    }
    __syncthreads();

    // ---- (L, D) of this lane's positions
    const int s0 = tid * DF_S, e0 = min(s0 + DF_S, len);
    for (int p = s0; p < e0; p++) {
        const int wp = DF_C + p;
        const int maxl = min(258, len - p);                          // clipped to the CHUNK's end, not the sub-chunk's
        int best = 0, bestd = 0;
        if (maxl >= 3) {
            const int maxd = has_prev ? 32768 : p;                   // min(the position in the stream, 32768)
            auto consider = [&](int d) {
                if (d <= 0 || d > maxd) return;
                if (best == maxl && d >= bestd) return;              // as long as can be, and nearer
                // to win it needs `best` bytes at a smaller distance, best + 1 at a larger: look at the last of them first
                const int need = max(d < bestd ? best : best + 1, 3);
                if (need > maxl || s_wb[wp + need - 1] != s_wb[wp - d + need - 1]) return;
                const int l = df_match_len(s_win, wp, wp - d, maxl);
                if (l < 3 || (l == 3 && d > 4096)) return;
                if (l > best || (l == best && d < bestd)) { best = l; bestd = d; }
            };
            consider(1); consider(2); consider(3); consider(4); consider(6); consider(8); consider(a.row);
            int wq = wp;
            for (int k = 0; k < FNX_DEFLATE_DENSE_DEPTH; k++) {
                const int link = wq >= DF_C ? s_link[wq - DF_C] : plink[wq];
                if (!link) break;
                wq -= link;
                if (wp - wq > maxd) break;                           // nearest first: the rest is further still
                consider(wp - wq);
            }
        }
        tab[p] = best >= 3 ? (static_cast<uint32_t>(best) << 16) | static_cast<uint32_t>(bestd - 1) : 0u;
    }
    __syncthreads();                                                 // the table is whole; the heads are dead

    // ---- the lazy walk's part of this lane
    auto step = [&](int p) -> int {                                  // the position behind the token that starts at p
        const int l = static_cast<int>(tab[p] >> 16);
        if (l < 3) return p + 1;
        return p + 1 < len && static_cast<int>(tab[p + 1] >> 16) > l ? p + 1 : p + l;
    };
    auto walk = [&](int from) -> int {                               // from >= s0; -> the first position at or behind e0
        mark[0] = mark[1] = mark[2] = mark[3] = 0;
        int p = from;
        while (p < e0) {
            mark[(p - s0) >> 5] |= 1u << ((p - s0) & 31);
            p = step(p);
        }
        return p;
    };
    int entry = s0, exitp = walk(s0);
    for (;;) {
        s_scan[tid] = static_cast<uint32_t>(exitp);
        if (tid == 0) s_moved = 0;
        __syncthreads();
        const int want = tid ? static_cast<int>(s_scan[tid - 1]) : 0;
        if (want != entry) {
            entry = want;
            // a marked entry lies on the path walked last, which ends in exitp whatever it started from
            const bool on_path = want < e0 && ((mark[(want - s0) >> 5] >> ((want - s0) & 31)) & 1u) != 0;
            if (!on_path) {
                const int x = walk(want);
                if (x != exitp) { exitp = x; atomicOr(&s_moved, 1u); }
            }
        }
        __syncthreads();
        const bool again = s_moved != 0;
        __syncthreads();                                             // read before lane 0 clears it
        if (!again) break;
    }

    // ---- the tokens of [entry, exit), the histograms, Adler-32
    int ntok = 0;
    {
        for (int p = entry; p < e0;) {
            const uint32_t t = tab[p];
            const int l = static_cast<int>(t >> 16);
            if (l >= 3 && !(p + 1 < len && static_cast<int>(tab[p + 1] >> 16) > l)) {
                const int d = static_cast<int>(t & 0xffffu) + 1;
                int sym, eb, ev;
                df_len_sym(l, sym, eb, ev);
                atomicAdd(&s_llf[sym], 1u);
                df_dist_sym(d, sym, eb, ev);
                atomicAdd(&s_df[sym], 1u);
                tok[s0 + ntok++] = df_match_tok(l, d);
                p += l;
            } else {
                const uint32_t b = s_b[p];
                atomicAdd(&s_llf[b], 1u);
                tok[s0 + ntok++] = b;
                p++;
            }
        }
        // Adler-32's sums of the sub-chunk, b against the CHUNK's end: at most 128 * 255 * 32768 < 2^32
        uint32_t asum = 0, bsum = 0;
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
