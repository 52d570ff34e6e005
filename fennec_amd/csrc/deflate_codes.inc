// The second half of a chunk kernel's body (deflate_chunk.inc, deflate_dense_chunk.inc), behind the parse: the codes from the two
// histograms, the choice of form, the block into the chunk's slot, its four meta words.  It reads what the including body has
// set up under these names: tid, a, c, len, last, s0, ntok, tok (lane t's ntok tokens from tok[s0] on), s_b / s_w (the chunk's
// bytes; (DF_C + 64) / 4 words that become the output bits), hw (three HuffWork) and the s_ arrays of deflate_chunk.inc.
// DF_SIZE_ONLY (0 or 1, set by the including kernel): 1 stops where the block's form and bit count are known -- no codes, no
// emit, no slot, no Adler-32 words; meta[0] alone gets the byte count the emitting form writes there for the same chunk.
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
#if DF_SIZE_ONLY
        // what the emit below arrives at: stored is header, LEN, ~LEN, the bytes; a coded block (`bits` counts its header and its
        // end-of-block) is padded to a byte; behind every chunk but the last the empty stored block: 3 bits, padding, 00 00 ff ff
        uint32_t nb = form == DF_STORED ? 5u + static_cast<uint32_t>(len) + (last ? 0u : 5u) : (last ? (bits + 7u) >> 3 : ((bits + 3u + 7u) >> 3) + 4u);
        a.meta[4 * static_cast<size_t>(c)] = nb;
    }
#else
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
#endif
