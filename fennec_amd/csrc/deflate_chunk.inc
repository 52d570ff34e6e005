// The body of deflate.hip's two chunk kernels, included into each: chunk DF_CHUNK_INDEX of the stream `a` (a DeflateArgs)
// describes, every lane of its workgroup -- the parse into the chunk's token words, the block into its slot, its four meta
// words.  It is a file and not a __device__ function because a function, simplified on its own before it is inlined, gives
// deflate_chunk_kernel other registers than the body written into it, and that kernel's figures are pinned (DESIGN.md 5.7).
    __shared__ uint32_t s_w[(DF_C + 64) / 4];                        // the chunk's bytes, later its output bits
    __shared__ uint32_t s_hash[1 << DF_HBITS];                       // position + 1; later three HuffWork
    __shared__ uint32_t s_llf[288], s_df[32], s_clf[20];
    __shared__ uint8_t s_lll[288], s_dl[32], s_cll[20];
    __shared__ uint16_t s_llc[288], s_dc[32], s_clc[20];
    __shared__ uint16_t s_cltok[320];                                // symbol | extra value << 8
    __shared__ uint32_t s_scan[DF_T];
    __shared__ uint32_t s_adler[2];
    __shared__ uint32_t s_form, s_hlit, s_hdist, s_hclen, s_ncl, s_hdr_bits, s_nbytes;
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

    // ---- the codes
    df_rank(s_llf, 286, hw[0].order, tid);
    df_rank(s_df, 30, hw[1].order, tid);
    __syncthreads();
    if (tid == 0) df_build_lengths(s_llf, 286, 15, s_lll, hw[0]);
    if (tid == 64) {
        df_build_lengths(s_df, 30, 15, s_dl, hw[1]);
        bool any = false;
        for (int j = 0; j < 30; j++) any = any || s_dl[j] != 0;
        if (!any) s_dl[0] = 1;                                       // no match in the block: one distance code all the same
    }
    __syncthreads();
    if (tid == 0) {
        int hlit = 286, hdist = 30;
        while (hlit > 257 && s_lll[hlit - 1] == 0) hlit--;
        while (hdist > 1 && s_dl[hdist - 1] == 0) hdist--;
        // the HLIT + HDIST lengths as one sequence in the code-length code
        int ncl = 0;
        const int nseq = hlit + hdist;
        for (int i = 0; i < nseq;) {
            const int v = i < hlit ? s_lll[i] : s_dl[i - hlit];
            int r = 1;
            while (i + r < nseq && (i + r < hlit ? s_lll[i + r] : s_dl[i + r - hlit]) == v) r++;
            i += r;
            if (v == 0) {
                while (r >= 11) { const int t = min(r, 138); s_cltok[ncl++] = static_cast<uint16_t>(18 | ((t - 11) << 8)); s_clf[18]++; r -= t; }
                if (r >= 3) { s_cltok[ncl++] = static_cast<uint16_t>(17 | ((r - 3) << 8)); s_clf[17]++; r = 0; }
            } else {
                s_cltok[ncl++] = static_cast<uint16_t>(v); s_clf[v]++; r--;
                while (r >= 3) { const int t = min(r, 6); s_cltok[ncl++] = static_cast<uint16_t>(16 | ((t - 3) << 8)); s_clf[16]++; r -= t; }
            }
            for (; r > 0; r--) { s_cltok[ncl++] = static_cast<uint16_t>(v); s_clf[v]++; }
        }
        int m = 0;
        for (int s = 0; s < 19; s++) {
            const uint32_t f = s_clf[s];
            if (!f) continue;
            int r = 0;
            for (int j = 0; j < 19; j++) {
                const uint32_t g = s_clf[j];
                r += (g != 0 && (g < f || (g == f && j < s))) ? 1 : 0;
            }
            hw[2].order[r] = static_cast<uint16_t>(s);
            m++;
        }
        df_build_lengths(s_clf, 19, 7, s_cll, hw[2]);
        if (m == 1) s_cll[hw[2].order[0] == 0 ? 1 : 0] = 1;         // inflate refuses an incomplete code-length code
        int hclen = 19;
        while (hclen > 4 && s_cll[DF_CLORD[hclen - 1]] == 0) hclen--;
        uint32_t hdr = 3 + 5 + 5 + 4 + 3 * static_cast<uint32_t>(hclen);
        for (int i = 0; i < ncl; i++) {
            const int s = s_cltok[i] & 0xff;
            hdr += s_cll[s] + (s == 16 ? 2 : (s == 17 ? 3 : (s == 18 ? 7 : 0)));
        }
        uint32_t dyn = hdr, fix = 3;
        for (int s = 0; s < 286; s++) {
            const uint32_t f = s_llf[s];
            dyn += f * (s_lll[s] + df_len_ebits(s));
            fix += f * (df_fixed_len(s) + df_len_ebits(s));
        }
        for (int s = 0; s < 30; s++) {
            const uint32_t f = s_df[s];
            dyn += f * (s_dl[s] + df_dist_ebits(s));
            fix += f * (5 + df_dist_ebits(s));
        }
        int form = DF_DYNAMIC;
        uint32_t bits = dyn;
        if (fix < bits) { form = DF_FIXED; bits = fix; }
        if (8u * (5u + static_cast<uint32_t>(len)) <= bits) form = DF_STORED;
        s_form = form; s_hlit = hlit; s_hdist = hdist; s_hclen = hclen; s_ncl = ncl;
        s_hdr_bits = form == DF_DYNAMIC ? hdr : 3;
    }
    __syncthreads();
    const int form = static_cast<int>(s_form);
    uint32_t *slot = reinterpret_cast<uint32_t *>(a.slots + static_cast<size_t>(c) * DF_SLOT);

    if (form == DF_STORED) {
        // header, LEN, ~LEN, the bytes, and behind every chunk but the last the empty stored block (whose header byte is zero too)
        const int nb = 5 + len + (last ? 0 : 5);
        for (int j = tid; 4 * j < nb; j += DF_T) {
            uint32_t v = 0;
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int k = 4 * j + e;
                uint32_t b = 0;
                if (k == 0) b = last ? 1u : 0u;
                else if (k < 3) b = (static_cast<uint32_t>(len) >> (8 * (k - 1))) & 0xffu;
                else if (k < 5) b = (~static_cast<uint32_t>(len) >> (8 * (k - 3))) & 0xffu;
                else if (k < 5 + len) b = s_b[k - 5];
                else if (k < nb) b = k >= 5 + len + 3 ? 0xffu : 0u;
                v |= b << (8 * e);
            }
            *(g_u32w *)(slot + j) = v;
        }
        if (tid == 0) s_nbytes = nb;
    } else {
        if (form == DF_DYNAMIC) {
            df_assign_codes(s_lll, 286, s_llc, tid);
            df_assign_codes(s_dl, 30, s_dc, tid);
            df_assign_codes(s_cll, 19, s_clc, tid);
        } else {
            for (int s = tid; s < 288; s += DF_T) {
                const int L = df_fixed_len(s);
                const uint32_t code = s < 144 ? 0x30u + s : (s < 256 ? 0x190u + (s - 144) : (s < 280 ? s - 256u : 0xc0u + (s - 280)));
                s_lll[s] = static_cast<uint8_t>(L);
                s_llc[s] = static_cast<uint16_t>(__brev(code) >> (32 - L));
            }
            if (tid < 32) {
                s_dl[tid] = 5;
                s_dc[tid] = static_cast<uint16_t>(__brev(static_cast<uint32_t>(tid)) >> 27);
            }
        }
        for (int i = tid; i < (DF_C + 64) / 4; i += DF_T) s_w[i] = 0;    // the chunk's bytes are not read again
        __syncthreads();
        uint32_t mybits = 0;
        for (int k = 0; k < ntok; k++) {
            const uint32_t t = tok[s0 + k];
            if (t & 0x80000000u) {
                int sym, eb, ev;
                df_len_sym(static_cast<int>((t >> 16) & 0xffu) + 3, sym, eb, ev);
                mybits += s_lll[sym] + eb;
                df_dist_sym(static_cast<int>(t & 0xffffu) + 1, sym, eb, ev);
                mybits += s_dl[sym] + eb;
            } else {
                mybits += s_lll[t];
            }
        }
        s_scan[tid] = mybits;
        __syncthreads();
        uint32_t off = s_hdr_bits;
        for (int j = 0; j < tid; j++) off += s_scan[j];
        if (tid == 0) {
            DfBits hb(s_w, 0);
            hb.put(last ? 1u : 0u, 1);
            hb.put(static_cast<uint32_t>(form), 2);
            if (form == DF_DYNAMIC) {
                hb.put(s_hlit - 257, 5);
                hb.put(s_hdist - 1, 5);
                hb.put(s_hclen - 4, 4);
                for (uint32_t i = 0; i < s_hclen; i++) hb.put(s_cll[DF_CLORD[i]], 3);
                for (uint32_t i = 0; i < s_ncl; i++) {
                    const int s = s_cltok[i] & 0xff;
                    hb.put(s_clc[s], s_cll[s]);
                    if (s >= 16) hb.put(s_cltok[i] >> 8, s == 16 ? 2 : (s == 17 ? 3 : 7));
                }
            }
            hb.flush();
        }
        DfBits bw(s_w, off);
        for (int k = 0; k < ntok; k++) {
            const uint32_t t = tok[s0 + k];
            if (t & 0x80000000u) {
                int sym, eb, ev;
                df_len_sym(static_cast<int>((t >> 16) & 0xffu) + 3, sym, eb, ev);
                bw.put(s_llc[sym], s_lll[sym]);
                if (eb) bw.put(static_cast<uint32_t>(ev), eb);
                df_dist_sym(static_cast<int>(t & 0xffffu) + 1, sym, eb, ev);
                bw.put(s_dc[sym], s_dl[sym]);
                if (eb) bw.put(static_cast<uint32_t>(ev), eb);
            } else {
                bw.put(s_llc[t], s_lll[t]);
            }
        }
        if (tid == DF_T - 1) {                                       // behind the last lane's tokens: the block's end
            bw.put(s_llc[256], s_lll[256]);
            if (!last) {
                bw.put(0u, 3);
                bw.align8();
                bw.put(0u, 16);
                bw.put(0xffffu, 16);
            } else {
                bw.align8();
            }
            s_nbytes = bw.pos() >> 3;
        }
        bw.flush();
        __syncthreads();
        const int nb = static_cast<int>(s_nbytes);
        for (int j = tid; 4 * j < nb; j += DF_T) *(g_u32w *)(slot + j) = s_w[j];
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t *m = a.meta + 4 * static_cast<size_t>(c);
        m[0] = s_nbytes;
        m[1] = s_adler[0] % DF_ADLER;
        m[2] = s_adler[1] % DF_ADLER;
        m[3] = static_cast<uint32_t>(len);
    }
