// The body of png_filter.hip's two pack kernels, included into each (see png_filter_rows.inc): rows PF_FIRST_ROW, + PF_ROW_STEP,
// ... below a.h of the index plane `a` (a PngPackArgs) describes; DEPTH is the kernels' template argument.
    constexpr int K = DEPTH == 8 ? 4 : 1, PPB = 8 / DEPTH;           // raw dwords per unit, pixels per raw byte
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t n = static_cast<uint32_t>(a.n);
    const uint32_t units = (n + 4 * K - 1) / (4 * K);
    for (int y = PF_FIRST_ROW; y < a.h; y += PF_ROW_STEP) {
        const uint8_t *row = a.src + static_cast<size_t>(y) * a.sstride;
        uint8_t *orow = a.out + static_cast<size_t>(y) * (static_cast<size_t>(n) + 1);
        if (tid == 0) orow[0] = 0;                                   // paletted rows are never filtered
        for (uint32_t base = wave * 64; base < units; base += PF_T) {
            const uint32_t u = base + lane;
            const bool active = u < units;
            uint32_t D[K];
            int nvalid = 0;
            if (DEPTH == 8) {
                uint32_t R[5] = {0, 0, 0, 0, 0};
                if (active) nvalid = pf_load<PNG_ROW_GRAY>(row, u, a.w, a.al4 != 0, R);
#pragma unroll
                for (int j = 0; j < K; j++) D[j] = R[1 + j];
            } else {
                D[0] = 0;
                if (active) {
                    nvalid = min(4, static_cast<int>(n - 4u * u));
                    const int x0 = 4 * PPB * static_cast<int>(u);    // 4 raw bytes of PPB pixels each
                    if (a.al4 && x0 + 4 * PPB <= a.w) {
#pragma unroll
                        for (int q = 0; q < PPB; q++) {              // source dword q: pixels 4q .. 4q + 3, raw byte 4q / PPB
                            const uint32_t v = *(g_u32 *)(row + x0 + 4 * q);
#pragma unroll
                            for (int e = 0; e < 4; e++) {
                                const int px = 4 * q + e, k = px / PPB, slot = PPB - 1 - px % PPB;
                                D[0] |= (((v >> (8 * e)) & 0xffu) << (DEPTH * slot) & 0xffu) << (8 * k);
                            }
                        }
                    } else {
#pragma unroll
                        for (int px = 0; px < 4 * PPB; px++) {
                            const int k = px / PPB, slot = PPB - 1 - px % PPB;
                            const uint32_t v = x0 + px < a.w ? row[x0 + px] : 0u;
                            D[0] |= ((v << (DEPTH * slot)) & 0xffu) << (8 * k);
                        }
                    }
                }
            }
            const uint32_t i0 = 4u * K * u;
            pf_store<K>(orow + 1, i0, D, nvalid, active, i0 + 8u * K <= n, lane);
        }
    }
