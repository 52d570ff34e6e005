// One optimised Huffman table (ITU T.81 Annex K.2, figures K.1 to K.4, in libjpeg's tie order) as ONE wave's run: the text
// jpeg.hip's jpeg_hufftab_kernel and tools/jpeg_hufftab_hostsim both include.  Plain C++; whoever includes it defines
//   HT_FN                 the qualifier of a function (__device__ __forceinline__ / static inline)
//   HT_UNROLL             in front of a loop over a lane's slots (device: unrolled, so that the slots stay in registers)
//   HT_PHASE(call)        a phase: `call` for every lane of the wave (the names `lane` and `ln` are the lane's number and its
//                         HtLane), then a barrier.  Device: { call; } __syncthreads();  host: a loop over the lanes
//   HT_MIN2               the wave's two smallest keys: every lane's (ln.k1, ln.k2) -- its own two smallest, k1 <= k2 -- become
//                         the two smallest of all lanes' (device: a butterfly of lane exchanges; host: a loop)
//   HT_LANE0(field)       ln.field where every lane holds it alike (device: ln.field; host: lanes[0].field)
//   HT_ATOMIC_ADD(p, v)   a shared-memory atomic add (uint32_t), HT_ATOMIC_OR(p, v) an atomic or
//   HT_RUN_PARAMS         ht_run's parameters behind the shared state: the lane (device) or the lanes (host)
//
// The rule (include/fennec_hip.h has it in full).  Slots 0..255 are the symbols with their counts, slot 256 the reserved
// symbol of frequency 1.  A merge takes the slot V1 of least non-zero frequency and then the slot V2 of least non-zero
// frequency among the others, among equal frequencies the LARGEST slot index both times; V2's frequency is added to V1's slot
// and V2's becomes zero; every leaf of either tree is one bit longer.  K.2's others[] chains are a serial walk over exactly
// those leaves: here every leaf carries its tree's slot (root) and its code size in a register, and a merge is one parallel
// update -- root in {V1, V2}: size + 1, root = V1.  The two minima are ONE reduction over 64-bit keys frequency << 16 |
// 0xffff - slot (frequencies stay below 2^40: 256 counts of 32 bits and the 1), carried as a (smallest, second) pair.
// Then figure K.3 from length 32 down to 17, the reserved symbol taken from the longest length in use, HUFFVAL ordered by
// (unlimited code size, symbol), canonical codes (Annex C).  A code size above 32 takes the class's standard table.

constexpr int HT_LANES = 64;
constexpr int HT_PER = 5;                          // slots a lane: slot = k * 64 + lane, 320 >= 257
constexpr int HT_MAX_CLEN = 32;                    // K.3's bits[] holds lengths 1..32
constexpr int HT_REC_WORDS = 70;                   // a table's record: nvals, "standard table taken", 16 counts (4 words), 256 values (64 words)
constexpr uint32_t HT_NONE = 0xffffffffu;
constexpr unsigned long long HT_NOKEY = ~0ull;

struct HtLane {
    unsigned long long freq[HT_PER];               // the tree's frequency in its slot; 0: no tree here
    uint32_t root[HT_PER], size[HT_PER];           // the slot's leaf: its tree's slot (HT_NONE: no leaf), its code size
    unsigned long long k1, k2;
};

struct HtShared {
    uint32_t bits[HT_MAX_CLEN + 2];                // [L]: codes of length L
    uint32_t nsize[HT_MAX_CLEN + 2];               // [L]: symbols 0..255 of unlimited size L; ht_ph_limit: the first HUFFVAL index of that size
    uint32_t first[18], cum[18];                   // [L]: the first code of final length L, the HUFFVAL index it belongs to; cum[17]: values in all
    uint32_t size4[65];                            // the unlimited size of symbol t in byte t & 3 of word t >> 2 (0: no code)
    uint32_t vals4[64];                            // HUFFVAL, four values a word
    uint32_t over;                                 // a code size above 32 (or a length count that cannot be): the standard table
};

HT_FN void ht_ph_init(const uint32_t *hist, HtShared &s, HtLane &ln, int lane)
{
    HT_UNROLL
    for (int k = 0; k < HT_PER; k++) {
        const int slot = k * HT_LANES + lane;
        const uint32_t f = slot < 256 ? hist[slot] : (slot == 256 ? 1u : 0u);
        ln.freq[k] = f;
        ln.root[k] = f ? static_cast<uint32_t>(slot) : HT_NONE;
        ln.size[k] = 0;
    }
    if (lane < HT_MAX_CLEN + 2) s.bits[lane] = s.nsize[lane] = 0;
    if (lane < 18) s.first[lane] = s.cum[lane] = 0;
    s.size4[lane] = 0;
    s.vals4[lane] = 0;
    if (lane == 0) {
        s.size4[64] = 0;
        s.over = 0;
    }
}

// the lane's own two smallest keys
HT_FN void ht_ph_keys(HtLane &ln, int lane)
{
    unsigned long long k1 = HT_NOKEY, k2 = HT_NOKEY;
    HT_UNROLL
    for (int k = 0; k < HT_PER; k++) {
        if (ln.freq[k] == 0) continue;
        const unsigned long long key = (ln.freq[k] << 16) | static_cast<unsigned long long>(0xffff - (k * HT_LANES + lane));
        if (key < k1) { k2 = k1; k1 = key; }
        else if (key < k2) k2 = key;
    }
    ln.k1 = k1; ln.k2 = k2;
}

HT_FN void ht_ph_merge(HtLane &ln, int lane, uint32_t c1, uint32_t c2, unsigned long long fsum)
{
    HT_UNROLL
    for (int k = 0; k < HT_PER; k++) {
        const uint32_t slot = static_cast<uint32_t>(k * HT_LANES + lane);
        if (slot == c1) ln.freq[k] = fsum;
        if (slot == c2) ln.freq[k] = 0;
        if (ln.root[k] == c1 || ln.root[k] == c2) {        // HT_NONE is neither
            ln.size[k]++;
            ln.root[k] = c1;
        }
    }
}

// figure K.3's input: the count of every code size, the reserved symbol's among them; the symbols' sizes for the ordering
HT_FN void ht_ph_sizes(HtShared &s, const HtLane &ln, int lane)
{
    HT_UNROLL
    for (int k = 0; k < HT_PER; k++) {
        const int slot = k * HT_LANES + lane;
        const uint32_t sz = ln.size[k];
        if (ln.root[k] == HT_NONE || sz == 0) continue;
        if (sz > static_cast<uint32_t>(HT_MAX_CLEN)) {
            HT_ATOMIC_OR(&s.over, 1u);
            continue;
        }
        HT_ATOMIC_ADD(&s.bits[sz], 1u);
        if (slot < 256) {
            HT_ATOMIC_ADD(&s.nsize[sz], 1u);
            HT_ATOMIC_OR(&s.size4[slot >> 2], sz << (8 * (slot & 3)));
        }
    }
}

// one lane: figure K.3 from 32 down to 17, the reserved symbol out of the longest length in use, then per final length its
// first code and first HUFFVAL index, and per unlimited size its first HUFFVAL index
HT_FN void ht_ph_limit(HtShared &s, int lane)
{
    if (lane != 0 || s.over) return;
    for (int i = HT_MAX_CLEN; i > 16; i--) {
        while (s.bits[i] > 0) {
            int j = i - 2;
            while (j > 0 && s.bits[j] == 0) j--;
            if (j == 0 || s.bits[i] < 2) {                 // not the counts of a prefix code: cannot be
                s.over = 1;
                return;
            }
            s.bits[i] -= 2;
            s.bits[i - 1]++;
            s.bits[j + 1] += 2;
            s.bits[j]--;
        }
    }
    int i = 16;
    while (i > 0 && s.bits[i] == 0) i--;
    if (i == 0) {
        s.over = 1;
        return;
    }
    s.bits[i]--;
    uint32_t code = 0, at = 0;
    for (int len = 1; len <= 16; len++) {
        s.first[len] = code;
        s.cum[len] = at;
        code = (code + s.bits[len]) << 1;
        at += s.bits[len];
    }
    s.cum[17] = at;
    uint32_t o = 0;
    for (int len = 1; len <= HT_MAX_CLEN; len++) {
        const uint32_t t = s.nsize[len];
        s.nsize[len] = o;
        o += t;
    }
}

// a symbol's place in HUFFVAL: behind every symbol of a smaller unlimited size and every smaller symbol of its own; the
// final length of that place and its canonical code
HT_FN void ht_ph_place(HtShared &s, const HtLane &ln, int lane, uint32_t *lut)
{
    if (s.over) return;
    uint32_t rank[4] = {0, 0, 0, 0};
    for (int w = 0; w < 64; w++) {
        const uint32_t four = s.size4[w];
        for (int b = 0; b < 4; b++) {
            const uint32_t szt = (four >> (8 * b)) & 0xffu;
            const int t = 4 * w + b;
            HT_UNROLL
            for (int k = 0; k < 4; k++) rank[k] += (szt == ln.size[k] && t < k * HT_LANES + lane) ? 1u : 0u;
        }
    }
    HT_UNROLL
    for (int k = 0; k < 4; k++) {
        const int sym = k * HT_LANES + lane;
        uint32_t word = 0;
        if (ln.root[k] != HT_NONE && ln.size[k] != 0) {
            const uint32_t p = s.nsize[ln.size[k]] + rank[k];
            for (uint32_t len = 1; len <= 16; len++) {
                if (p >= s.cum[len] && p - s.cum[len] < s.bits[len]) word = (len << 24) | (s.first[len] + p - s.cum[len]);
            }
            HT_ATOMIC_OR(&s.vals4[(p >> 2) & 63u], static_cast<uint32_t>(sym) << (8 * (p & 3u)));
        }
        lut[sym] = word;
    }
}

HT_FN void ht_ph_out(const HtShared &s, int lane, uint32_t *lut, uint32_t *rec, const uint32_t *std_lut, const uint32_t *std_rec)
{
    if (s.over) {
        for (int i = lane; i < 256; i += HT_LANES) lut[i] = std_lut[i];
        for (int i = lane; i < HT_REC_WORDS; i += HT_LANES) rec[i] = i == 1 ? 1u : std_rec[i];
        return;
    }
    for (int i = lane; i < HT_REC_WORDS; i += HT_LANES) {
        uint32_t v;
        if (i == 0) v = s.cum[17];
        else if (i == 1) v = 0;
        else if (i < 6) {
            const int l0 = 4 * (i - 2) + 1;                // counts of lengths l0 .. l0 + 3, a byte each in memory order
            v = s.bits[l0] | (s.bits[l0 + 1] << 8) | (s.bits[l0 + 2] << 16) | (s.bits[l0 + 3] << 24);
        } else {
            v = s.vals4[i - 6];
        }
        rec[i] = v;
    }
}

// hist: the table's [256] counts (not all zero).  lut: its [256] code look-up words (length << 24 | code, 0: no code); rec: its
// record (HT_REC_WORDS).  std_lut / std_rec: the same two of the class's standard table
HT_FN void ht_run(const uint32_t *hist, uint32_t *lut, uint32_t *rec, const uint32_t *std_lut, const uint32_t *std_rec, HtShared &s HT_RUN_PARAMS)
{
    HT_PHASE(ht_ph_init(hist, s, ln, lane));
    for (;;) {
        HT_PHASE(ht_ph_keys(ln, lane));
        HT_MIN2;
        const unsigned long long k1 = HT_LANE0(k1), k2 = HT_LANE0(k2);
        if (k2 == HT_NOKEY) break;
        const uint32_t c1 = 0xffffu - static_cast<uint32_t>(k1 & 0xffffu), c2 = 0xffffu - static_cast<uint32_t>(k2 & 0xffffu);
        const unsigned long long fsum = (k1 >> 16) + (k2 >> 16);
        HT_PHASE(ht_ph_merge(ln, lane, c1, c2, fsum));
    }
    HT_PHASE(ht_ph_sizes(s, ln, lane));
    HT_PHASE(ht_ph_limit(s, lane));
    HT_PHASE(ht_ph_place(s, ln, lane, lut));
    HT_PHASE(ht_ph_out(s, lane, lut, rec, std_lut, std_rec));
}
