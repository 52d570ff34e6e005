// medianCut (targetsize.go:422-486) as ONE workgroup's run: the text median_cut.hip's kernel and tools/median_cut_hostsim both
// include.  Plain C++; whoever includes it defines
//   MC_FN                 the qualifier of a function (__device__ __forceinline__ / static inline)
//   MC_PHASE(call)        a phase: `call` for every lane of the workgroup (the names `tid` and `ln` are the lane's number and
//                         its McLane), then a workgroup barrier.  Device: { call; } __syncthreads();  host: a loop over the lanes
//   MC_ATOMIC_ADD(p, v)   an LDS atomic add (uint32_t), MC_ATOMIC_MAX64(p, v) an LDS atomic maximum (unsigned long long)
//   MC_LOAD4(p)           the McVec4 at the 16-byte aligned sample pointer p
//   MC_UNIFORM(x)         the uint32_t x, which every lane holds alike (device: read from the first lane, so that it and what
//                         follows from it live in scalar registers; host: x)
//   MC_RUN_PARAMS         mc_run's parameters behind (const McArgs &a, McShared &s ...): the lane (device) or the lanes (host)
// Everything between two phases is uniform: every lane of the device computes it from shared memory that no lane writes before
// the next barrier.  A shared word that steers the run (v, eq_left, kpart, part, a box record) is written in ONE phase, read behind that
// phase's barrier, and the phase that follows the read does not write it.
//
// The rule (include/fennec_hip.h has it in full): boxes are contiguous runs of the sample array, each in ascending sample
// number j.  A split takes the FIRST box of the largest 64-bit score among those with two samples or more, the axis R / G / B
// by the reference's >= chain, and orders the box by (axis value, j): with v the axis value of the sorted box's element
// mid - 1 (mid = count / 2), the samples below v and the first eq_left = mid - #{< v} samples equal to v, in their order, are
// the left half, the rest in their order the right half -- one stable partition, no sort.  Both halves are written to the
// OTHER sample buffer at the box's own offsets (the box records say which buffer holds a box).

constexpr int MC_LANES = 512;                      // eight waves: two a SIMD, 256 VGPRs each -- the phases keep whole rows of LDS reads in flight
constexpr int MC_RUN = 16;                         // samples a lane takes of a tile: four aligned 16-byte loads
constexpr int MC_TILE = MC_LANES * MC_RUN;         // samples a partition step stages in LDS
constexpr int MC_MAX_SAMPLES = 199999;             // n / (n / 100000) < 200000
constexpr int MC_STAT = 5;                         // a half's statistics: packed minima, packed maxima, three sums

struct McBox {
    uint32_t start, count;
    uint32_t mn, mx;                               // r | g << 8 | b << 16 of the per-channel minima / maxima
    uint32_t sum[3];
    uint32_t buf;                                  // which sample buffer holds it
};

struct McStat {
    uint32_t mn, mx, sum[3];
};

struct McLane {                                    // what a lane carries from one phase of a split to the next
    McStat half[2];
    uint32_t x[MC_RUN], in;                        // its samples of the tile, and which of them lie in the box (mc_lane_samples)
};

struct McArgs {
    uint32_t *buf[2];                              // samples r | g << 8 | b << 16; each (n + 3 & ~3) + 4 words, 16-byte aligned
    uint32_t n;                                    // 1 .. MC_MAX_SAMPLES, in buf[0]
    uint32_t level_mask[8];                        // bit c - 1: a palette is wanted when the list first has c boxes
    uint32_t nlevels;
    uint32_t *out;                                 // [nlevels][256] entries r | g << 8 | b << 16 | 255 << 24, then ncolors[nlevels]
};

struct McShared {
    McBox box[256];
    unsigned long long kpart[16];                  // the argmax's partial results: score << 8 | 255 - index; 0: no box with two samples
    alignas(16) uint32_t hist[256];
    uint32_t hpart[16];
    alignas(16) uint32_t cnt[MC_LANES];                        // a tile's per-lane counts: #{< v} | #{== v} << 16
    alignas(16) uint32_t part[MC_LANES / 16];
    alignas(16) uint32_t stage[MC_TILE];        // a tile's samples in their new order (MC_TILE words); the lanes' statistics
    uint32_t v, eq_left;
};

struct McVec4 { uint32_t x, y, z, w; };

static_assert(MC_TILE >= 2 * MC_STAT * MC_LANES && MC_TILE < 65536 && MC_RUN % 4 == 0 && MC_RUN <= 32 && MC_LANES % 32 == 0 && MC_LANES >= 258 && 3 * (MC_LANES / 32) <= 64,
              "stage holds the lanes' statistics; a tile's counts fit 16 bits; whole 16-byte groups; the phases' lane counts");

MC_FN uint32_t mc_min3(uint32_t a, uint32_t b)     // per byte
{
    const uint32_t r0 = a & 0xffu, r1 = b & 0xffu, g0 = a & 0xff00u, g1 = b & 0xff00u, b0 = a & 0xff0000u, b1 = b & 0xff0000u;
    return (r0 < r1 ? r0 : r1) | (g0 < g1 ? g0 : g1) | (b0 < b1 ? b0 : b1);
}

MC_FN uint32_t mc_max3(uint32_t a, uint32_t b)
{
    const uint32_t r0 = a & 0xffu, r1 = b & 0xffu, g0 = a & 0xff00u, g1 = b & 0xff00u, b0 = a & 0xff0000u, b1 = b & 0xff0000u;
    return (r0 > r1 ? r0 : r1) | (g0 > g1 ? g0 : g1) | (b0 > b1 ? b0 : b1);
}

MC_FN void mc_stat_clear(McStat &t)
{
    t.mn = 0x00ffffffu; t.mx = 0u; t.sum[0] = t.sum[1] = t.sum[2] = 0u;
}

MC_FN void mc_stat_add(McStat &t, uint32_t x)
{
    t.mn = mc_min3(t.mn, x); t.mx = mc_max3(t.mx, x);
    t.sum[0] += x & 255u; t.sum[1] += (x >> 8) & 255u; t.sum[2] += (x >> 16) & 255u;
}

// the reference's score (targetsize.go:447-459) and its place in the argmax: larger score first, then the lower index
MC_FN unsigned long long mc_key(const McBox &b, uint32_t index)
{
    if (b.count < 2u) return 0ull;
    unsigned long long vol = 1ull;
    for (int k = 0; k < 24; k += 8) vol *= static_cast<unsigned long long>(((b.mx >> k) & 255u) - ((b.mn >> k) & 255u) + 1u);
    return ((vol * b.count) << 8) | (255u - index);
}

// R when rRange >= gRange and rRange >= bRange, else G when gRange >= bRange, else B -> the shift of the axis byte
MC_FN uint32_t mc_axis_shift(const McBox &b)
{
    const uint32_t rr = (b.mx & 255u) - (b.mn & 255u), gr = ((b.mx >> 8) & 255u) - ((b.mn >> 8) & 255u),
                   br = ((b.mx >> 16) & 255u) - ((b.mn >> 16) & 255u);
    return rr >= gr && rr >= br ? 0u : (gr >= br ? 8u : 16u);
}

// ---- phases ------------------------------------------------------------------------------------------------------------
MC_FN void mc_ph_clear(McShared &s, McLane &ln, int tid)
{
    mc_stat_clear(ln.half[0]);
    mc_stat_clear(ln.half[1]);
    if (tid < 256) { s.box[tid].count = 0u; s.hist[tid] = 0u; }      // a box past the list's end never wins the argmax
    if (tid < 16) s.kpart[tid] = 0ull;
}

// the first box's statistics: every sample once, lane by lane
MC_FN void mc_ph_first(const McArgs &a, McLane &ln, int tid)
{
    for (uint32_t i = static_cast<uint32_t>(tid); i < a.n; i += MC_LANES) mc_stat_add(ln.half[0], a.buf[0][i]);
}

// the lanes' statistics -> s.stage[word][lane]; then MC_LANES / 32 lanes a word fold 32 lanes' values each; then mc_ph_boxes folds the rest
MC_FN void mc_ph_stats_out(McShared &s, const McLane &ln, int tid)
{
    for (int h = 0; h < 2; h++) {
        uint32_t *w = s.stage + h * MC_STAT * MC_LANES + tid;
        w[0] = ln.half[h].mn; w[MC_LANES] = ln.half[h].mx;
        for (int k = 0; k < 3; k++) w[(2 + k) * MC_LANES] = ln.half[h].sum[k];
    }
}

template <int N>
MC_FN uint32_t mc_fold(const uint32_t *p, int stride, int kind)   // kind 0: minima, 1: maxima, else sums
{
    uint32_t x[N];
    for (int i = 0; i < N; i++) x[i] = p[i * stride];             // the reads go out together
    uint32_t r = x[0];
    if (kind == 0) { for (int i = 1; i < N; i++) r = mc_min3(r, x[i]); }
    else if (kind == 1) { for (int i = 1; i < N; i++) r = mc_max3(r, x[i]); }
    else { for (int i = 1; i < N; i++) r += x[i]; }
    return r;
}

// which lanes fold what: a statistic's kind is the same for a whole wave (lanes 0-63 minima, 64-127 maxima, 128-191 the sums of
// half 0, 192-255 the sums of half 1), so no wave runs more than one of mc_fold's loops.  -> the word (half * MC_STAT + statistic)
// of s.stage the lane's group g belongs to, or -1
MC_FN int mc_fold_word(int tid, int groups, int *g)
{
    const int blk = tid >> 6, j = (tid & 63) / groups;
    *g = (tid & 63) % groups;
    if (blk < 2) return j < 2 ? j * MC_STAT + blk : -1;
    if (blk < 4) return j < 3 ? (blk - 2) * MC_STAT + 2 + j : -1;
    return -1;
}

MC_FN void mc_ph_stats_fold(McShared &s, int tid)
{
    int g;
    const int word = mc_fold_word(tid, MC_LANES / 32, &g);
    if (word < 0) return;
    uint32_t *p = s.stage + word * MC_LANES + g * 32;
    p[0] = mc_fold<32>(p, 1, word % MC_STAT < 2 ? word % MC_STAT : 2);
}

// the records of the split's two boxes: one lane per (half, statistic) -- the first lane of its group in mc_fold_word's layout --
// folds the MC_LANES / 32 partial values left and writes its field of box at0 (half 0) or at1 (half 1); lanes 256 and 257
// write where the boxes lie.  at1 < 0: one half only (the first box).
MC_FN void mc_ph_boxes(McShared &s, int tid, int at0, int at1, uint32_t st0, uint32_t st1, uint32_t cnt0, uint32_t cnt1, uint32_t buf)
{
    if (tid == 256 || tid == 257) {
        const int half = tid - 256, at = half == 0 ? at0 : at1;
        if (at < 0) return;
        s.box[at].start = half == 0 ? st0 : st1;
        s.box[at].count = half == 0 ? cnt0 : cnt1;
        s.box[at].buf = buf;
        return;
    }
    int g;
    const int word = mc_fold_word(tid, 1, &g);            // (groups of one lane: the (half, statistic) pairs at the head of each wave)
    if (word < 0) return;
    const int at = word < MC_STAT ? at0 : at1, k = word % MC_STAT;
    if (at < 0) return;
    const uint32_t x = mc_fold<MC_LANES / 32>(s.stage + word * MC_LANES, 32, k < 2 ? k : 2);
    if (k == 0) s.box[at].mn = x;
    else if (k == 1) s.box[at].mx = x;
    else s.box[at].sum[k - 2] = x;
}

// a level's palette: per box in list order (rSum / count, gSum / count, bSum / count, 255), truncating (targetsize.go:399-411)
MC_FN void mc_ph_palette(const McArgs &a, const McShared &s, int tid, uint32_t level, uint32_t nb)
{
    if (static_cast<uint32_t>(tid) < nb) {
        const McBox &b = s.box[tid];
        a.out[level * 256u + tid] = (b.sum[0] / b.count) | ((b.sum[1] / b.count) << 8) | ((b.sum[2] / b.count) << 16) | 0xff000000u;
    }
    if (tid == 0) a.out[a.nlevels * 256u + level] = nb;
}

// the argmax's first half: every box's key into the maximum of its 16 (kpart is zero: mc_ph_clear, mc_ph_median); the histogram
// is cleared for the split on the way
MC_FN void mc_ph_pick(McShared &s, int tid)
{
    if (tid >= 256) return;
    s.hist[tid] = 0u;
    const unsigned long long k = mc_key(s.box[tid], static_cast<uint32_t>(tid));
    if (k) MC_ATOMIC_MAX64(&s.kpart[tid >> 4], k);
}

// the box's histogram on the axis; a lane adds a run of equal values at once (a flat box is one add per lane, not one per sample)
MC_FN void mc_ph_hist(const McArgs &a, McShared &s, int tid, const McBox &b, uint32_t shift)
{
    const uint32_t *src = a.buf[b.buf] + b.start;
    uint32_t cur = 0u, run = 0u;
    for (uint32_t i = static_cast<uint32_t>(tid); i < b.count; i += MC_LANES) {
        const uint32_t c = (src[i] >> shift) & 255u;
        if (run && c != cur) { MC_ATOMIC_ADD(&s.hist[cur], run); run = 0u; }
        cur = c;
        run++;
    }
    if (run) MC_ATOMIC_ADD(&s.hist[cur], run);
}

MC_FN void mc_ph_median_parts(McShared &s, int tid)
{
    if (tid >= 16) return;
    uint32_t t = 0u;
    for (int i = 0; i < 16; i++) t += s.hist[tid * 16 + i];
    s.hpart[tid] = t;
}

// bin v holds the sorted box's element mid - 1: #{< v} < mid <= #{<= v}; eq_left = mid - #{< v} of the samples equal to v go left
MC_FN void mc_ph_median(McShared &s, McLane &ln, int tid, uint32_t mid)
{
    mc_stat_clear(ln.half[0]);
    mc_stat_clear(ln.half[1]);
    if (tid < 16) s.kpart[tid] = 0ull;                // read behind mc_ph_pick's barrier, two phases ago
    if (tid >= 256) return;
    uint32_t below = 0u;                              // (fixed trip counts: the reads go out together)
    for (int i = 0; i < 16; i++) below += i < (tid >> 4) ? s.hpart[i] : 0u;
    for (int i = 0; i < 16; i++) below += i < (tid & 15) ? s.hist[(tid & ~15) + i] : 0u;
    if (below < mid && mid <= below + s.hist[tid]) { s.v = static_cast<uint32_t>(tid); s.eq_left = mid - below; }
}

// what one partition step works on: the tile's first sample tile0 (a multiple of 4), the box's [lo, hi), all as indices of
// the sample buffer
struct McTile {
    const uint32_t *src;
    uint32_t tile0, lo, hi;
    uint32_t shift, v;
};

// the lane's MC_RUN samples of the tile -> x[]; bit k of the result: sample k lies in the box
MC_FN uint32_t mc_lane_samples(const McTile &t, int tid, uint32_t x[MC_RUN])
{
    const uint32_t e0 = t.tile0 + static_cast<uint32_t>(tid) * MC_RUN;
    uint32_t in = 0u;
    for (int q = 0; q < MC_RUN; q += 4) {
        const uint32_t g = e0 + q;
        McVec4 w = {0u, 0u, 0u, 0u};
        if (g < t.hi && g + 4u > t.lo) w = MC_LOAD4(t.src + g);       // a 16-byte group with a sample of the box in it
        x[q] = w.x; x[q + 1] = w.y; x[q + 2] = w.z; x[q + 3] = w.w;
        for (uint32_t k = 0; k < 4u; k++)
            if (g + k >= t.lo && g + k < t.hi) in |= 1u << (q + k);
    }
    return in;
}

// a box that lies in one tile: the lane's samples are loaded here, once for the split, and the histogram is made from them
MC_FN void mc_ph_hist_tile(McShared &s, McLane &ln, int tid, const McTile &t)
{
    ln.in = mc_lane_samples(t, tid, ln.x);
    uint32_t cur = 0u, run = 0u;
    for (int k = 0; k < MC_RUN; k++) {
        if (!((ln.in >> k) & 1u)) continue;
        const uint32_t c = (ln.x[k] >> t.shift) & 255u;
        if (run && c != cur) { MC_ATOMIC_ADD(&s.hist[cur], run); run = 0u; }
        cur = c;
        run++;
    }
    if (run) MC_ATOMIC_ADD(&s.hist[cur], run);
}

// loaded: the lane holds the tile's samples already (mc_ph_hist_tile)
MC_FN void mc_ph_count(McShared &s, McLane &ln, int tid, const McTile &t, bool loaded)
{
    if (!loaded) ln.in = mc_lane_samples(t, tid, ln.x);
    const uint32_t *x = ln.x;
    const uint32_t in = ln.in;
    uint32_t c = 0u;
    for (int k = 0; k < MC_RUN; k++) {
        if (!((in >> k) & 1u)) continue;
        const uint32_t ch = (x[k] >> t.shift) & 255u;
        c += ch < t.v ? 1u : (ch == t.v ? 0x10000u : 0u);
    }
    s.cnt[tid] = c;
}

MC_FN void mc_ph_count_parts(McShared &s, int tid)
{
    if (tid >= MC_LANES / 16) return;
    uint32_t t = 0u;
    for (int i = 0; i < 16; i++) t += s.cnt[tid * 16 + i];
    s.part[tid] = t;
}

// how many of the first `eq` samples equal to v (counted from the box's start) go left
MC_FN uint32_t mc_eq_left_of(uint32_t eq, uint32_t eq_left) { return eq < eq_left ? eq : eq_left; }

// the lane's samples into the tile's new order in LDS: the left-going ones from stage[0], the right-going ones behind them;
// eq_done: samples equal to v in the tiles before.  *tile_left: how many of the tile go left (the same for every lane)
MC_FN void mc_ph_place(McShared &s, const McLane &ln, int tid, const McTile &t, uint32_t eq_done, uint32_t eq_left, uint32_t *tile_left)
{
    const int g = tid >> 4;
    uint32_t total = 0u, pre = 0u;
    for (int i = 0; i < MC_LANES / 16; i++) { const uint32_t p = s.part[i]; total += p; pre += i < g ? p : 0u; }
    for (int i = 0; i < 16; i++) pre += (g * 16 + i) < tid ? s.cnt[g * 16 + i] : 0u;
    const uint32_t lt_pre = pre & 0xffffu, eq_pre = pre >> 16;
    const uint32_t left_of_tile = (total & 0xffffu) + mc_eq_left_of(eq_done + (total >> 16), eq_left) - mc_eq_left_of(eq_done, eq_left);
    *tile_left = left_of_tile;
    const uint32_t *x = ln.x;                                             // (mc_ph_count's)
    const uint32_t in = ln.in;
    const uint32_t e0 = t.tile0 + static_cast<uint32_t>(tid) * MC_RUN;
    const uint32_t first = t.tile0 > t.lo ? t.tile0 : t.lo;               // the tile's first sample of the box
    const uint32_t before = (e0 < t.hi ? e0 : t.hi) > first ? (e0 < t.hi ? e0 : t.hi) - first : 0u;
    uint32_t l = lt_pre + mc_eq_left_of(eq_done + eq_pre, eq_left) - mc_eq_left_of(eq_done, eq_left);
    uint32_t r = left_of_tile + (before - l);
    uint32_t eq = eq_done + eq_pre;
    for (int k = 0; k < MC_RUN; k++) {
        if (!((in >> k) & 1u)) continue;
        const uint32_t ch = (x[k] >> t.shift) & 255u;
        bool left = ch < t.v;
        if (ch == t.v) { left = eq < eq_left; eq++; }
        if (left) s.stage[l++] = x[k];
        else s.stage[r++] = x[k];
    }
}

// the tile's new order from LDS to the other buffer: tile_left samples to dl[0 ..], the other tile_n - tile_left to dr[0 ..].
// Both halves' statistics are gathered here, where a small box is spread over as many lanes as it has samples.
MC_FN void mc_ph_store(const McShared &s, McLane &ln, int tid, uint32_t *dl, uint32_t *dr, uint32_t tile_left, uint32_t tile_n)
{
    for (uint32_t i = static_cast<uint32_t>(tid); i < tile_n; i += MC_LANES) {
        const uint32_t x = s.stage[i];
        if (i < tile_left) { dl[i] = x; mc_stat_add(ln.half[0], x); }
        else { dr[i - tile_left] = x; mc_stat_add(ln.half[1], x); }
    }
}

// ---- the run --------------------------------------------------------------------------------------------------------
MC_FN bool mc_level_at(const McArgs &a, uint32_t nb) { return nb >= 1u && nb <= 256u && ((a.level_mask[(nb - 1u) >> 5] >> ((nb - 1u) & 31u)) & 1u); }

MC_FN void mc_run(const McArgs &a, McShared &s MC_RUN_PARAMS)
{
    uint32_t top = 0u;                              // the largest level
    for (uint32_t c = 1u; c <= 256u; c++) top = mc_level_at(a, c) ? c : top;

    MC_PHASE(mc_ph_clear(s, ln, tid));
    MC_PHASE(mc_ph_first(a, ln, tid));
    MC_PHASE(mc_ph_stats_out(s, ln, tid));
    MC_PHASE(mc_ph_stats_fold(s, tid));
    MC_PHASE(mc_ph_boxes(s, tid, 0, -1, 0u, 0u, a.n, 0u, 0u));

    uint32_t nb = 1u, level = 0u;
    for (;;) {
        if (mc_level_at(a, nb)) {
            MC_PHASE(mc_ph_palette(a, s, tid, level, nb));
            level++;
        }
        if (nb >= top) break;
        MC_PHASE(mc_ph_pick(s, tid));
        unsigned long long best = 0ull;
        for (int i = 0; i < 16; i++) best = s.kpart[i] > best ? s.kpart[i] : best;
        if (MC_UNIFORM(static_cast<uint32_t>(best >> 8) | static_cast<uint32_t>(best >> 40)) == 0u) break;   // no box has two samples: the reference's loop ends (targetsize.go:461-463)
        const uint32_t bi = 255u - MC_UNIFORM(static_cast<uint32_t>(best & 255ull));
        McBox b;
        b.start = MC_UNIFORM(s.box[bi].start); b.count = MC_UNIFORM(s.box[bi].count); b.buf = MC_UNIFORM(s.box[bi].buf);
        b.mn = MC_UNIFORM(s.box[bi].mn); b.mx = MC_UNIFORM(s.box[bi].mx);
        b.sum[0] = b.sum[1] = b.sum[2] = 0u;        // (not needed here)
        const uint32_t shift = mc_axis_shift(b), mid = b.count / 2u;
        McTile t;
        t.src = a.buf[b.buf];
        t.lo = b.start; t.hi = b.start + b.count;
        t.shift = shift; t.v = 0u;
        t.tile0 = b.start & ~3u;
        const bool one = t.hi - t.tile0 <= static_cast<uint32_t>(MC_TILE);     // the box lies in one tile: its samples are loaded once
        if (one) {
            MC_PHASE(mc_ph_hist_tile(s, ln, tid, t));
        } else {
            MC_PHASE(mc_ph_hist(a, s, tid, b, shift));
        }
        MC_PHASE(mc_ph_median_parts(s, tid));
        MC_PHASE(mc_ph_median(s, ln, tid, mid));
        const uint32_t v = MC_UNIFORM(s.v), eq_left = MC_UNIFORM(s.eq_left);
        t.v = v;
        uint32_t *dl = a.buf[b.buf ^ 1u] + b.start, *dr = dl + mid;
        uint32_t eq_done = 0u;
        for (t.tile0 = b.start & ~3u; t.tile0 < t.hi; t.tile0 += MC_TILE) {
            const uint32_t first = t.tile0 > t.lo ? t.tile0 : t.lo, last = t.tile0 + MC_TILE < t.hi ? t.tile0 + MC_TILE : t.hi;
            uint32_t tile_left = 0u;
            MC_PHASE(mc_ph_count(s, ln, tid, t, one));
            MC_PHASE(mc_ph_count_parts(s, tid));
            MC_PHASE(mc_ph_place(s, ln, tid, t, eq_done, eq_left, &tile_left));
            MC_PHASE(mc_ph_store(s, ln, tid, dl, dr, tile_left, last - first));
            uint32_t total = 0u;
            for (int i = 0; i < MC_LANES / 16; i++) total += s.part[i];
            total = MC_UNIFORM(total);
            tile_left = MC_UNIFORM(tile_left);
            eq_done += total >> 16;
            dl += tile_left;
            dr += (last - first) - tile_left;
        }
        MC_PHASE(mc_ph_stats_out(s, ln, tid));
        MC_PHASE(mc_ph_stats_fold(s, tid));
        MC_PHASE(mc_ph_boxes(s, tid, static_cast<int>(bi), static_cast<int>(nb), b.start, b.start + mid, mid, b.count - mid, b.buf ^ 1u));
        nb++;
    }
    // the loop stopped before these levels were reached: each is the final list (what medianCut(img, max_colors[l]) returns)
    for (; level < a.nlevels; level++) {
        MC_PHASE(mc_ph_palette(a, s, tid, level, nb));
    }
}
