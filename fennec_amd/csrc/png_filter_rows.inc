// The body of png_filter.hip's two filter kernels, included into each: rows PF_FIRST_ROW, + PF_ROW_STEP, ... below a.h of the
// image `a` (a PngFilterArgs) describes, every lane of the workgroup; MODE is the kernels' template argument.  A file and not a
// __device__ function: a function, simplified on its own before it is inlined, gives the single kernels other registers than
// the body written into them, and their figures are pinned (the head comment of png_filter.hip).
    constexpr int K = pf_k(MODE), BPP = pf_bpp(MODE);
    __shared__ uint32_t s_sum[2][PF_T / 64][5];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t n = static_cast<uint32_t>(a.n);
    const uint32_t units = (n + 4 * K - 1) / (4 * K);
    const bool al4 = a.al4 != 0;
    int parity = 0;
    for (int y = PF_FIRST_ROW; y < a.h; y += PF_ROW_STEP, parity ^= 1) {
        const uint8_t *cur = a.src + static_cast<size_t>(y) * a.sstride;
        const uint8_t *prev = cur - a.sstride;                       // read for y > 0 only
        // ---- pass 1: the five sums, in the order of the type numbers: None, Sub, Up, Average, Paeth
        uint32_t sum[5] = {0, 0, 0, 0, 0};
        for (uint32_t u = tid; u < units; u += PF_T) {
            uint32_t C[5], P[5] = {0, 0, 0, 0, 0};
            const int nvalid = pf_load<MODE>(cur, u, a.w, al4, C);
            if (y > 0) pf_load<MODE>(prev, u, a.w, al4, P);
#pragma unroll
            for (int j = 0; j < K; j++) {
                // a residual behind the row's end is not part of the sum (Sub, Average and Paeth see a left neighbour there)
                const int v = nvalid - 4 * j;
                const uint32_t m = v >= 4 ? 0xffffffffu : (v <= 0 ? 0u : (1u << (8 * v)) - 1u);
                const uint32_t c = C[1 + j], up = P[1 + j];
                const uint32_t l = left_of<BPP>(C[j], c), ul = left_of<BPP>(P[j], up);
                sum[0] = cost8(c, sum[0]);
                sum[1] = cost8(sub8(c, l) & m, sum[1]);
                sum[2] = cost8(sub8(c, up), sum[2]);
                sum[3] = cost8(sub8(c, avg8(l, up)) & m, sum[3]);
                sum[4] = cost8(sub8(c, paeth8(l, up, ul)) & m, sum[4]);
            }
        }
#pragma unroll
        for (int f = 0; f < 5; f++) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum[f] += __shfl_xor(sum[f], off, 64);
        }
        // two sets of words, by the parity of the workgroup's row count: a wave can be at most one barrier ahead of another
        if (lane == 0) {
#pragma unroll
            for (int f = 0; f < 5; f++) s_sum[parity][wave][f] = sum[f];
        }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < 5; f++) sum[f] = s_sum[parity][0][f] + s_sum[parity][1][f] + s_sum[parity][2][f] + s_sum[parity][3][f];
        // tried in the order Up, Paeth, None, Sub, Average; a later one wins only when strictly smaller
        int ft = 2;
        uint32_t best = sum[2];
        if (sum[4] < best) { best = sum[4]; ft = 4; }
        if (sum[0] < best) { best = sum[0]; ft = 0; }
        if (sum[1] < best) { best = sum[1]; ft = 1; }
        if (sum[3] < best) { best = sum[3]; ft = 3; }

        // ---- pass 2: the chosen filter, stored
        uint8_t *orow = a.out + static_cast<size_t>(y) * (static_cast<size_t>(n) + 1);
        if (tid == 0) orow[0] = static_cast<uint8_t>(ft);
        const bool need_prev = ft >= 2 && y > 0;
        for (uint32_t base = wave * 64; base < units; base += PF_T) {
            const uint32_t u = base + lane;
            const bool active = u < units;
            uint32_t C[5] = {0, 0, 0, 0, 0}, P[5] = {0, 0, 0, 0, 0}, D[K];
            int nvalid = 0;
            if (active) {
                nvalid = pf_load<MODE>(cur, u, a.w, al4, C);
                if (need_prev) pf_load<MODE>(prev, u, a.w, al4, P);
            }
#pragma unroll
            for (int j = 0; j < K; j++) {
                const uint32_t c = C[1 + j], up = P[1 + j];
                const uint32_t l = left_of<BPP>(C[j], c), ul = left_of<BPP>(P[j], up);
                uint32_t d = c;
                if (ft == 1) d = sub8(c, l);
                else if (ft == 2) d = sub8(c, up);
                else if (ft == 3) d = sub8(c, avg8(l, up));
                else if (ft == 4) d = sub8(c, paeth8(l, up, ul));
                D[j] = d;
            }
            const uint32_t i0 = 4u * K * u;
            pf_store<K>(orow + 1, i0, D, nvalid, active, i0 + 8u * K <= n, lane);
        }
    }
