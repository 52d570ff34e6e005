// CRC-32 (png_frame.cpp's: reflected polynomial 0xedb88320, register from all ones, inverted at the end) of a run of bytes as
// workgroups' runs: the text crc32.hip's kernels and tools/crc32_hostsim both include.  Plain C++; whoever includes it defines
//   CRC_FN                the qualifier of a function (__device__ __forceinline__ / static inline)
//   CRC_CONST             the qualifier of a constant table (__device__ const / static const)
//   CRC_UNROLL            in front of a loop of fixed length
//   CRC_LD32(p)           the aligned dword at p (device: a global load; host: memcpy)
//   CRC_PHASE(call)       a phase: `call` for every lane of the workgroup (the names `lane` and `ln` are the lane's number and
//                         its CrcLane), then a barrier.  Device: { call; } __syncthreads();  host: a loop over the lanes
//   CRC_RUN_PARAMS        crc_piece's / crc_stream's parameters behind the shared state: the lane (device) or the lanes (host)
//
// The arithmetic.  A register value v stands for the polynomial whose coefficient of x^i is bit 31 - i of v (the reflected
// representation: one is 0x80000000, a step to the next power a shift to the RIGHT).  R(M) is the register after the bytes M
// when started from 0, with no inversion; R is linear over GF(2) and R(0...0 M) = R(M): zero bytes leave a zero register zero.
// shift(v, n) = v x^(8 n) mod P is the register v after n zero bytes.  Everything rests on
//   R(A B) = shift(R(A), |B|) xor R(B)          the register after M from a start s = shift(s, |M|) xor R(M)
//
// crc_piece: 256 lanes, FNX_CRC_PIECE = 256 FNX_CRC_RUN bytes.  A piece of fewer bytes stands at the END of its 256 runs, as if
// zero bytes led it -- they change nothing (above) and are never read, and every run that holds bytes but the first is then a
// whole one: the true lengths enter by which lane a byte falls to, and each of the eight fold steps is one multiplication by a
// constant.  A lane computes R(its run) by slice-by-4 from four tables of 256 words in shared memory (single bytes up to the
// first aligned dword and behind the last one); step k of the fold turns the 256 >> k remainders of 2^k runs each into half
// as many: left x^(8 RUN 2^k) xor right.
// crc_stream: the pieces' words of one stream -> its CRC.  Piece j of an n-byte stream has n - min(n, (j + 1) PIECE) bytes
// behind it; a lane shifts its pieces' words by that many, by square-and-multiply over CRC_POW (x^(8 2^k), k = 0..31; x has the
// order 2^32 - 1, P being primitive, so the byte count is taken mod 2^32 - 1 first); the seed -- the register the stream starts
// from -- is one more term, shifted by n; the workgroup xors the terms, and the answer is inverted.

constexpr int CRC_LANES = 256;
constexpr int CRC_RUN = FNX_CRC_RUN;
constexpr int CRC_PIECE = FNX_CRC_PIECE;
constexpr int CRC_RUN_LOG = 6;                     // RUN = 2^6: the fold's constants are CRC_POW's entries 6..13
constexpr uint32_t CRC_POLY = 0xedb88320u;
static_assert(CRC_PIECE == CRC_LANES * CRC_RUN && CRC_RUN == (1 << CRC_RUN_LOG), "a piece is 256 runs of 2^6 bytes");

struct CrcLane {
    uint32_t v;
};

struct CrcShared {
    uint32_t tab[4][256];                          // tab[s][b]: the register after byte b and s zero bytes, from 0
    uint32_t red[CRC_LANES];
};

// a b mod P: 32 steps of one conditional xor and one step of b to the next power (constexpr: the tables below are the
// compiler's work; the kernels and the host program call it as it stands)
constexpr uint32_t crc_mulmod(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= b & (0u - (a >> 31));
        a <<= 1;
        b = (b >> 1) ^ (CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}

struct CrcPow {
    uint32_t v[32];                                // x^(8 2^k)
};
constexpr CrcPow crc_pow_make()
{
    CrcPow t{};
    uint32_t p = 0x00800000u;                      // x^8
    for (int k = 0; k < 32; k++) {
        t.v[k] = p;
        p = crc_mulmod(p, p);
    }
    return t;
}
CRC_CONST CrcPow CRC_POW = crc_pow_make();

// v after nbytes zero bytes
CRC_FN uint32_t crc_shift(uint32_t v, unsigned long long nbytes)
{
    unsigned long long t = (nbytes & 0xffffffffull) + (nbytes >> 32);      // 2^32 = 1 mod 2^32 - 1
    t = (t & 0xffffffffull) + (t >> 32);
    uint32_t e = static_cast<uint32_t>(t);                                  // (2^32 - 1 itself may stay: x^(8 (2^32 - 1)) = 1)
    for (int k = 0; e; k++, e >>= 1) {
        if (e & 1u) v = crc_mulmod(v, CRC_POW.v[k]);
    }
    return v;
}

CRC_FN void crc_ph_tab0(CrcShared &s, int lane)
{
    uint32_t c = static_cast<uint32_t>(lane);
    CRC_UNROLL
    for (int k = 0; k < 8; k++) c = (c >> 1) ^ (CRC_POLY & (0u - (c & 1u)));
    s.tab[0][lane] = c;
}

CRC_FN void crc_ph_tab123(CrcShared &s, int lane)
{
    uint32_t c = s.tab[0][lane];
    CRC_UNROLL
    for (int t = 1; t < 4; t++) {
        c = s.tab[0][c & 0xffu] ^ (c >> 8);
        s.tab[t][lane] = c;
    }
}

// R(the len bytes at p): nothing outside [p, p + len) is read
CRC_FN uint32_t crc_run(const uint8_t *p, uint32_t len, const CrcShared &s)
{
    uint32_t c = 0;
    uint32_t head = static_cast<uint32_t>((4u - (reinterpret_cast<uintptr_t>(p) & 3u)) & 3u);
    if (head > len) head = len;
    for (uint32_t i = 0; i < head; i++) c = s.tab[0][(c ^ p[i]) & 0xffu] ^ (c >> 8);
    p += head;
    len -= head;
    const uint32_t nd = len >> 2;
    for (uint32_t i = 0; i < nd; i++) {
        c ^= CRC_LD32(p + 4 * static_cast<size_t>(i));
        c = s.tab[3][c & 0xffu] ^ s.tab[2][(c >> 8) & 0xffu] ^ s.tab[1][(c >> 16) & 0xffu] ^ s.tab[0][c >> 24];
    }
    for (uint32_t i = 4 * nd; i < len; i++) c = s.tab[0][(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return c;
}

// R(lane's run) of a piece of plen <= PIECE bytes that ends where run 255 ends
CRC_FN uint32_t crc_lane_run(const uint8_t *piece, uint32_t plen, const CrcShared &s, int lane)
{
    const uint32_t pad = static_cast<uint32_t>(CRC_PIECE) - plen;
    const uint32_t end = static_cast<uint32_t>(lane + 1) * CRC_RUN;
    if (end <= pad) return 0;
    const uint32_t begin = end - CRC_RUN > pad ? end - CRC_RUN : pad;
    return crc_run(piece + (begin - pad), end - begin, s);
}

// R(piece), in every lane; 1 <= plen <= PIECE
CRC_FN uint32_t crc_piece(const uint8_t *piece, uint32_t plen, CrcShared &s CRC_RUN_PARAMS)
{
    CRC_PHASE(crc_ph_tab0(s, lane))
    CRC_PHASE(crc_ph_tab123(s, lane))
    CRC_PHASE(s.red[lane] = crc_lane_run(piece, plen, s, lane))
    for (int k = 0; k < 8; k++) {
        CRC_PHASE(if (lane < (CRC_LANES >> (k + 1))) ln.v = crc_mulmod(s.red[2 * lane], CRC_POW.v[CRC_RUN_LOG + k]) ^ s.red[2 * lane + 1])
        CRC_PHASE(if (lane < (CRC_LANES >> (k + 1))) s.red[lane] = ln.v)
    }
    return s.red[0];
}

// the pieces behind a stream of n bytes
CRC_FN unsigned long long crc_pieces_of(unsigned long long n) { return (n + CRC_PIECE - 1) / CRC_PIECE; }

// lane's terms: the words of pieces lane, lane + 256, ... of an n-byte stream, and the seed's as piece number crc_pieces_of(n)
CRC_FN uint32_t crc_lane_terms(const uint32_t *words, unsigned long long n, uint32_t seed, int lane)
{
    const unsigned long long np = crc_pieces_of(n);
    uint32_t acc = 0;
    for (unsigned long long j = static_cast<unsigned long long>(lane); j <= np; j += CRC_LANES) {
        if (j == np) {
            acc ^= crc_shift(seed, n);
        } else {
            const unsigned long long end = (j + 1) * CRC_PIECE < n ? (j + 1) * CRC_PIECE : n;
            acc ^= crc_shift(words[j], n - end);
        }
    }
    return acc;
}

// the CRC of an n-byte stream from its pieces' words and the register it starts from, in every lane
CRC_FN uint32_t crc_stream(const uint32_t *words, unsigned long long n, uint32_t seed, CrcShared &s CRC_RUN_PARAMS)
{
    CRC_PHASE(s.red[lane] = crc_lane_terms(words, n, seed, lane))
    for (int off = CRC_LANES / 2; off > 0; off >>= 1) {
        CRC_PHASE(if (lane < off) s.red[lane] ^= s.red[lane + off])
    }
    return ~s.red[0];
}
