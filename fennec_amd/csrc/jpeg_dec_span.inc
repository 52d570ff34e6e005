// jpeg_dec.hip's lane body and what it stands on: the spans' geometry, the arguments, the state word, the span decoder of the sync
// and write passes, and the host's sync-table builder.  jpeg_dec.hip includes this text inside namespace fnx; so does
// tools/jpeg_dec_hostsim, which runs it lane after lane on the CPU (there __device__, __forceinline__ and __constant__ are the
// HIP headers' host definitions).  Needs common.hpp (DecTables, DecSyncTables, DEC_FAST_BITS) and <cstring>.
constexpr int DEC_WPT = 32;                          // words of the bit string per lane
constexpr int DEC_WARM = 16;                         // first pass: spans a workgroup decodes ahead of the ones it owns, so that its
constexpr int DEC_OWN = 256 - DEC_WARM;              // first own span almost always starts from a synchronised state
constexpr int DEC_SPAN = 32 * DEC_WPT;               // ... in bits
constexpr int DEC_WG_WORDS = 256 * DEC_WPT;
constexpr int DEC_SEGW = 256 * (DEC_WPT + 1) + 4;    // a workgroup's words in LDS: one pad word per span (a span's words sit in
                                                     // different banks than its neighbours'), 3 words of look-ahead

struct DecArgs {
    const uint32_t *ecs;                             // the scan without stuffing, bytes as in the file, zero-padded
    const DecTables *tab;                            // write pass: fast[] = length << 8 | symbol
    const DecSyncTables *tab_sync;                   // sync passes: what one symbol -- or two -- does to the state
    unsigned long long *s_in, *s_out;                // per lane: the state it starts in / ends in
    uint32_t *cnt;                                   // per lane: blocks finished inside its span
    uint32_t *flag;                                  // <true>: set by a workgroup that decoded again
    const unsigned long long *first_blk;             // write: exclusive prefix sum of cnt
    int16_t *coef;                                   // write: [nblk][64], natural order, zeroed
    uint32_t *err;                                   // write: != 0: a code outside its table or a run past the block
    uint32_t *dbg;                                   // sync: [0] max passes of a workgroup, [1] sum of passes, [2] lane-decodes (FNX_JPEG_TRACE)
    long long nwords;                                // words of ecs that may be read
    unsigned long long nbits;                        // length of the string
    int nlanes;                                      // spans in the string
    int nblk, nslots;
    uint64_t dcpack, acpack;                         // table of slot s: (pack >> 4 s) & 15
    const uint32_t *rst;                             // byte offsets at which restart intervals 1, 2, ... start (ascending)
    int nrst;
    int ri_blocks;                                   // blocks per restart interval
    // per boundary k: (the lane that stood on it) << 32 | the blocks that lane had counted before it -- written by the sync
    // passes, read by the write pass (see jpeg_dwrite_kernel: block numbers are counted from the interval's start)
    unsigned long long *rst_rec;
};

// Restart intervals (DRI): interval k starts on a byte boundary, in the state (block start, slot 0), with every DC
// prediction at 0; what is left of the byte before it is padding (1 bits, never a complete code: T.81 forbids the
// all-ones code).  For a decoder that means: standing on a boundary, start over; a symbol that would reach across
// the next boundary is not one -- go to the boundary.  A decoder in a WRONG state obeys the same two rules, so every
// boundary puts it right: with restart intervals no desynchronised run is longer than an interval.
__device__ __forceinline__ uint32_t rst_rel(const DecArgs &a, int k, long long wg_bit)
{
    if (k >= a.nrst) return 0xffffffffu;
    const long long b = 8ll * a.rst[k] - wg_bit;
    return b > 0xfffffff0ll ? 0xffffffffu : (b < 0 ? 0u : static_cast<uint32_t>(b));
}

// state: bit position | position in the block (0..63) << 40 | slot in the MCU << 48
__device__ __forceinline__ unsigned long long dec_state(unsigned long long p, int z, int slot)
{
    return p | (static_cast<unsigned long long>(z) << 40) | (static_cast<unsigned long long>(slot) << 48);
}

__device__ __constant__ uint8_t c_unzig[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct DecShared {
    uint32_t seg[DEC_SEGW];
    unsigned long long out[256];
    // the first sync kernel's later passes: the few lanes that decode again, packed into the workgroup's first wave
    unsigned long long tin[64], rout[64];
    uint32_t rcnt[64];
    uint16_t todo[64];
    uint32_t wcnt[4];
    union {
        DecTables tab;                               // write pass
        DecSyncTables stab;                          // sync passes
    };
    uint8_t unzig[64];
};

__device__ __forceinline__ uint32_t dec_word(const uint32_t *seg, uint32_t wi)
{
    return seg[wi + wi / DEC_WPT];
}

// Decodes from (rel, z, slot) to the first symbol that starts at or after `end`.  WRITE: with the values.
// The loop is one dependent chain per symbol -- window, table look-up, new position -- and a wave has at most one other
// wave on its SIMD to hide it behind, so the chain is kept short: three words of the string live in registers (the
// third is fetched a symbol ahead), the symbol's effect on (position, z) is two selects instead of branches, and a code
// longer than the fast table's 11 bits finds its length by counting, not by a loop.
template <bool WRITE, bool RST>
__device__ __forceinline__ void dec_span(const DecShared &sh, const DecArgs &a, uint32_t &rel, int &z, int &slot, uint32_t end, uint32_t &cnt,
                                         long long blk, uint32_t &bad, long long wg_bit, uint32_t lim = 0xffffffffu)
{
    uint32_t wi = rel >> 5;
    uint32_t hi = dec_word(sh.seg, wi), lo = dec_word(sh.seg, wi + 1), nxt = dec_word(sh.seg, wi + 2);
    int rk = 0;
    uint32_t bnext = 0xffffffffu;
    if (RST) {                                                     // the first boundary at or after this lane's start
        const unsigned long long at = static_cast<unsigned long long>(wg_bit + rel);
        int lo_k = 0, hi_k = a.nrst;
        while (lo_k < hi_k) {
            const int mid = (lo_k + hi_k) >> 1;
            if (8ull * a.rst[mid] < at) lo_k = mid + 1; else hi_k = mid;
        }
        rk = lo_k;
        bnext = rst_rel(a, rk, wg_bit);
    }
    while (rel < end) {
        if (WRITE && blk + cnt >= a.nblk) break;                   // what follows the last block is padding
        if (WRITE && rel >= lim) {                                 // a block the image needs starts past the end of the string
            bad |= 8u;
            break;
        }
        // write pass: every block of the intervals before the next boundary is complete -- what is left before it is not data.
        // (In a sound file that is the padding, which the symbol rule below skips as well; in a DAMAGED interval whose blocks
        // end early the leftover bits can read as the start of one more block: a decoder that counts MCUs never looks at
        // them, and written here they would stay in the coefficients of the next interval's first block -- the fuzzer's
        // find, seed 41: tests/golden/damaged_interval_ends_early.jpg.)
        if (WRITE && RST && rel < bnext && rk < a.nrst && blk + cnt >= static_cast<long long>(rk + 1) * a.ri_blocks) {
            rel = bnext;
            if (rel >= end) break;                                 // the boundary lies in a later span: that lane starts over there
            // the jump can be any length (a damaged interval that ends bytes early): the three words follow it here, the
            // steps below move them one word per symbol (tests/jpeg_craft_cases.py: g_ends_16_early)
            wi = rel >> 5;
            hi = dec_word(sh.seg, wi); lo = dec_word(sh.seg, wi + 1); nxt = dec_word(sh.seg, wi + 2);
        }
        if (RST && rel >= bnext) {                                 // on a boundary: the interval's first block, first slot
            // (write pass: exactly the intervals before it must be complete -- a damaged interval that yields a block too
            // many or too few would shift every block behind it)
            if (WRITE && blk + cnt != static_cast<long long>(rk + 1) * a.ri_blocks) bad |= 16u;
            if (!WRITE && blk >= 0) a.rst_rec[rk] = (static_cast<unsigned long long>(blk) << 32) | cnt;   // (sync passes: blk = the lane, or -1)
            z = 0; slot = 0;
            bnext = rst_rel(a, ++rk, wg_bit);
        }
        uint32_t off = rel - 32u * wi;                             // < 64: a symbol is at most 16 + 15 bits
        const bool adv = off >= 32u;
        hi = adv ? lo : hi;
        lo = adv ? nxt : lo;
        wi += adv ? 1u : 0u;
        off -= adv ? 32u : 0u;
        nxt = dec_word(sh.seg, wi + 2);
        const unsigned long long pair = (static_cast<unsigned long long>(hi) << 32) | lo;
        const uint32_t c16 = static_cast<uint32_t>((pair << off) >> 48);
        const int t = static_cast<int>(((z == 0 ? a.dcpack : a.acpack) >> (4 * slot)) & 15ull);
        uint32_t e;
        if constexpr (!WRITE) {
            // the sync passes' tables hold what a symbol does to the state, ready made -- and, for the AC tables, what the
            // next one does as well when its code lies inside the same 11 bits (about every second look-up on a photograph)
            const uint32_t px = c16 >> (16 - DEC_FAST_BITS);
            e = sh.stab.st[t][px];
            const uint32_t a1 = e & 0xffu, s1 = (e >> 8) & 0xffu, a2 = (e >> 16) & 0xffu, s2 = e >> 24;
            // both symbols only if the second one belongs to this span and to this block (and, with restart intervals,
            // never: the boundary tests are per symbol); DC entries hold one symbol (a2 == 0)
            const bool two = !RST && a2 != 0 && rel + a1 < end && z + static_cast<int>(s1) < 64;
            const uint32_t adv = two ? a2 : a1, step = two ? s2 : s1;
            if (e) {
                if (RST && rel + adv > bnext) {                    // padding before a boundary
                    rel = bnext;
                    continue;
                }
                rel += adv;
                z += static_cast<int>(step);
                const bool fin = z >= 64;
                z = fin ? 0 : z;
                cnt += fin ? 1u : 0u;
                const int s1n = slot + 1 == a.nslots ? 0 : slot + 1;
                slot = fin ? s1n : slot;
                continue;
            }
        } else {
            e = sh.tab.fast[t][c16 >> (16 - DEC_FAST_BITS)];
        }
        int len = static_cast<int>(e >> 8), sym = static_cast<int>(e & 0xffu);
        bool nocode = false;
        if (e == 0) {
            // limit[] rises with the length: the code's length is the first L with c16 < limit[L]
            int L = DEC_FAST_BITS + 1;
            const uint32_t (*limit)[18] = WRITE ? sh.tab.limit : sh.stab.limit;
            const int32_t (*delta)[18] = WRITE ? sh.tab.delta : sh.stab.delta;
            const uint8_t (*value)[256] = WRITE ? sh.tab.value : sh.stab.value;
#pragma unroll
            for (int k = DEC_FAST_BITS + 1; k < 16; k++) L += c16 >= limit[t][k] ? 1 : 0;
            const bool hit = c16 < limit[t][16];
            len = L;
            sym = hit ? value[t][(static_cast<int>(c16 >> (16 - L)) + delta[t][L]) & 255] : 0;
            nocode = !hit;
        }
        const int s = sym & 15, r = sym >> 4;
        const bool dc = z == 0;
        if (RST && rel + static_cast<uint32_t>(len + s) > bnext) {  // padding before a boundary (the boundary resets the state)
            rel = bnext;
            continue;
        }
        if (WRITE && nocode) bad |= 1u;                            // (after the boundary test: padding is not a code either)
        if (WRITE && rel + static_cast<uint32_t>(len + s) > lim) { // a code or a value that straddles the string's end would be completed
            bad |= 8u;                                             // from the zero padding behind it: Go reports unexpected EOF here
            break;
        }
        if (WRITE) {
            int32_t v = 0;
            if (s) {                                               // receive + extend (T.81 F.2.2.1)
                const uint32_t o2 = off + static_cast<uint32_t>(len);
                const unsigned long long w2 = o2 < 32u ? pair << o2 : ((static_cast<unsigned long long>(lo) << 32) | nxt) << (o2 - 32u);
                const uint32_t raw = static_cast<uint32_t>(w2 >> (64 - s));
                v = raw < (1u << (s - 1)) ? static_cast<int32_t>(raw) - (1 << s) + 1 : static_cast<int32_t>(raw);
            }
            if (dc) {
                if (sym > 11) bad |= 2u;
                a.coef[(blk + cnt) * 64] = static_cast<int16_t>(v);
            } else if (s) {
                if (z + r > 63) bad |= 4u;
                else a.coef[(blk + cnt) * 64 + sh.unzig[z + r]] = static_cast<int16_t>(v);
            }
        }
        rel += static_cast<uint32_t>(len + s);
        // DC: on to the first AC.  AC: a value after r zeros, or sixteen zeros (r = 15, s = 0), both z + r + 1; any other
        // s = 0 ends the block
        z = dc ? 1 : ((s == 0 && r != 15) ? 64 : z + r + 1);
        if (z >= 64) {
            z = 0;
            slot = slot + 1 == a.nslots ? 0 : slot + 1;
            cnt++;
        }
    }
}

// the sync passes' form of a file's tables (common.hpp: DecSyncTables)
static void dec_sync_tables(const DecTables &tab, DecSyncTables *ts)
{
    std::memcpy(ts->limit, tab.limit, sizeof(ts->limit));
    std::memcpy(ts->delta, tab.delta, sizeof(ts->delta));
    std::memcpy(ts->value, tab.value, sizeof(ts->value));
    auto effect = [](uint32_t e, bool ac, uint32_t *bits, uint32_t *step) {        // one symbol of the write pass's table
        const uint32_t len = e >> 8, sym = e & 0xffu, sz = sym & 15u, r = sym >> 4;
        *bits = len + sz;
        *step = !ac ? 1u : ((sz == 0 && r != 15) ? 64u : r + 1u);
    };
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < (1 << DEC_FAST_BITS); i++) {
            const uint32_t e = tab.fast[t][i];
            uint32_t b1 = 0, s1 = 0;
            if (e) effect(e, false, &b1, &s1);
            ts->st[t][i] = e ? (b1 | (s1 << 8)) : 0u;
        }
    for (int t = 0; t < 2; t++)
        for (int i = 0; i < (1 << DEC_FAST_BITS); i++) {
            const uint32_t e = tab.fast[2 + t][i];
            uint32_t v = 0;
            if (e) {
                uint32_t b1, s1;
                effect(e, true, &b1, &s1);
                v = b1 | (s1 << 8);
                // a second symbol: the block goes on, and the code after symbol 1's bits lies inside the prefix
                if (s1 < 64 && b1 < static_cast<uint32_t>(DEC_FAST_BITS)) {
                    const uint32_t rest = (static_cast<uint32_t>(i) << b1) & ((1u << DEC_FAST_BITS) - 1u);   // what is known of the bits behind it
                    const uint32_t e2 = tab.fast[2 + t][rest];
                    if (e2 && (e2 >> 8) <= static_cast<uint32_t>(DEC_FAST_BITS) - b1) {      // every prefix with these known bits holds this code
                        uint32_t b2, s2;
                        effect(e2, true, &b2, &s2);
                        v |= ((b1 + b2) << 16) | ((s1 + s2) << 24);
                    }
                }
            }
            ts->st[2 + t][i] = v;
        }
}
