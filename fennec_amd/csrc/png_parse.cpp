// The host side of fnx_png_decode: everything that reads a PNG file's untrusted bytes.  Plain C++, no HIP calls -- the file
// is also built alone, under sanitizers, by tools/fuzz_png_host.sh.
//   png_parse        the chunk walk (signature, CRCs, IHDR / PLTE / tRNS / IDAT / IEND and their order)
//   png_inflate      RFC 1950 / 1951 inflate (the library links no zlib)
//   png_row_plan     the h filter-type bytes of the inflated stream -> the work units of png_unfilter_kernel
//   png_adam7_geometry  the seven passes of an Adam7 file (accepted where the ctx says so: fnx_ctx_set_png_adam7) as images of
//                    their own; png_probe fills PngFile's pass table from it, png_stream_size and png_row_plan go pass by pass
//   png_palette_table  a colour-type-3 file's 256 pixel values, toNRGBA already applied
//   png_prepare_many those four for a list of files on several threads (fnx_png_decode_batch; tools/png_batch_host.cpp runs it
//                    under the address and the thread sanitizer)
//   png_expand_of, png_adam7_passes  the file as the kernels' descriptors: what fnx_png_decode and the decode batch upload
#include "common.hpp"

#include <atomic>
#include <system_error>
#include <thread>

namespace fnx {

namespace {
thread_local const char *t_what = nullptr;   // the text of this thread's last refusal: png_prepare_many carries it in the item
}

int png_corrupt(const char *what)
{
    t_what = what;
    set_error("invalid PNG: %s", what);
    return FNX_ERR_INVALID;
}

int png_unsupported(const char *what)
{
    t_what = what;
    set_error("unsupported PNG (decode it on the host): %s", what);
    return FNX_ERR_UNSUPPORTED;
}

namespace {

uint32_t be32(const uint8_t *p) { return (uint32_t(p[0]) << 24) | (uint32_t(p[1]) << 16) | (uint32_t(p[2]) << 8) | p[3]; }

// CRC-32 of a chunk's tag and body (ISO 3309), four bytes a step
struct Crc {
    uint32_t t[4][256];
    Crc()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++)
            for (int s = 1; s < 4; s++) t[s][i] = t[0][t[s - 1][i] & 0xffu] ^ (t[s - 1][i] >> 8);
    }
};

uint32_t crc32(const uint8_t *p, size_t n)
{
    static const Crc tab;
    uint32_t c = 0xffffffffu;
    for (; n >= 4; n -= 4, p += 4) {
        c ^= uint32_t(p[0]) | (uint32_t(p[1]) << 8) | (uint32_t(p[2]) << 16) | (uint32_t(p[3]) << 24);
        c = tab.t[3][c & 0xffu] ^ tab.t[2][(c >> 8) & 0xffu] ^ tab.t[1][(c >> 16) & 0xffu] ^ tab.t[0][c >> 24];
    }
    for (; n; n--) c = tab.t[0][(c ^ *p++) & 0xffu] ^ (c >> 8);
    return ~c;
}

bool tag_is(const uint8_t *p, const char *t) { return std::memcmp(p, t, 4) == 0; }

// the chunk at data[pos ..): its body's offset and length once length, bounds and CRC hold
int next_chunk(const uint8_t *data, size_t n, size_t pos, size_t *body, uint32_t *len)
{
    if (n - pos < 12) return png_corrupt("the file ends inside a chunk");
    *len = be32(data + pos);
    if (*len > 0x7fffffffu || n - pos - 12 < *len) return png_corrupt("a chunk longer than the file");
    *body = pos + 8;
    if (crc32(data + pos + 4, 4 + size_t(*len)) != be32(data + pos + 8 + *len)) return png_corrupt("a chunk's CRC-32 does not match");
    return FNX_OK;
}

int read_ihdr(const uint8_t *data, size_t n, PngFile *f)
{
    if (!png_signature(data, n)) return png_corrupt("no PNG signature");
    size_t body = 0;
    uint32_t len = 0;
    FNX_TRY(next_chunk(data, n, 8, &body, &len));
    if (!tag_is(data + 12, "IHDR") || len != 13) return png_corrupt("the first chunk is not a 13-byte IHDR");
    const uint8_t *p = data + body;
    const uint32_t w = be32(p), h = be32(p + 4);
    if (w == 0 || h == 0 || w > 0x7fffffffu || h > 0x7fffffffu) return png_corrupt("IHDR: a dimension of 0 or above 2^31 - 1");
    f->color_type = p[9];
    f->depth = p[8];
    f->interlace = p[12];
    const int ct = f->color_type, d = f->depth;
    const bool pair = (ct == 0 && (d == 1 || d == 2 || d == 4 || d == 8 || d == 16)) || (ct == 3 && (d == 1 || d == 2 || d == 4 || d == 8)) ||
                      ((ct == 2 || ct == 4 || ct == 6) && (d == 8 || d == 16));
    if (!pair) return png_corrupt("IHDR: not one of the 15 colour type / bit depth pairs");
    if (p[10] != 0) return png_corrupt("IHDR: compression method is not 0");
    if (p[11] != 0) return png_corrupt("IHDR: filter method is not 0");
    if (f->interlace > 1) return png_corrupt("IHDR: interlace method is not 0 or 1");
    f->w = static_cast<int>(w);
    f->h = static_cast<int>(h);
    f->channels = ct == 0 || ct == 3 ? 1 : ct == 4 ? 2 : ct == 2 ? 3 : 4;
    const int bits = f->channels * d;
    f->bpp = bits >= 8 ? bits / 8 : 1;
    f->rowbytes = (static_cast<size_t>(w) * bits + 7) / 8;
    return FNX_OK;
}

}  // namespace

size_t png_adam7_geometry(int w, int h, int bits, int pw[7], int ph[7], size_t rowbytes[7])
{
    size_t total = 0;
    for (int p = 0; p < 7; p++) {
        const int cw = w > ADAM7_X0[p] ? (w - ADAM7_X0[p] + ADAM7_DX[p] - 1) / ADAM7_DX[p] : 0;
        const int ch = h > ADAM7_Y0[p] ? (h - ADAM7_Y0[p] + ADAM7_DY[p] - 1) / ADAM7_DY[p] : 0;
        const bool present = cw > 0 && ch > 0;
        pw[p] = present ? cw : 0;
        ph[p] = present ? ch : 0;
        rowbytes[p] = present ? (static_cast<size_t>(cw) * bits + 7) / 8 : 0;
        total += static_cast<size_t>(ph[p]) * (1 + rowbytes[p]);
    }
    return total;
}

int png_probe(const uint8_t *data, size_t n, PngFile *f, bool adam7)
{
    FNX_TRY(read_ihdr(data, n, f));
    if (f->interlace == 1 && !adam7) return png_unsupported("Adam7 interlace");
    if (f->w > 65535 || f->h > 65535) return png_unsupported("a dimension above 65535");
    if (f->interlace == 1) {
        f->pstream = png_adam7_geometry(f->w, f->h, f->channels * f->depth, f->pw, f->ph, f->prow);
        size_t off = 0;
        for (int p = 0; p < 7; p++) {
            f->poff[p] = off;
            off += static_cast<size_t>(f->ph[p]) * (1 + f->prow[p]);
        }
    }
    return FNX_OK;
}

int png_parse(const uint8_t *data, size_t n, PngFile *f, bool adam7)
{
    FNX_TRY(png_probe(data, n, f, adam7));
    f->npal = f->ntrns = 0;
    f->has_trns = false;
    f->idat.clear();
    enum { HDR, PLTE, TRNS, IDAT, AFTER_IDAT } stage = HDR;
    size_t pos = 8 + 12 + 13;
    for (;;) {
        size_t body = 0;
        uint32_t len = 0;
        FNX_TRY(next_chunk(data, n, pos, &body, &len));
        const uint8_t *tag = data + pos + 4, *p = data + body;
        pos = body + len + 4;
        if (tag_is(tag, "IHDR")) return png_corrupt("a second IHDR");
        if (tag_is(tag, "PLTE")) {
            if (stage != HDR) return png_corrupt("PLTE out of order (it comes once, before tRNS and IDAT)");
            if (f->color_type == 0 || f->color_type == 4) return png_corrupt("PLTE in a greyscale file");
            if (len == 0 || len % 3 != 0 || len > 768) return png_corrupt("PLTE: 1..256 entries of 3 bytes");
            if (f->color_type == 3 && len / 3 > (1u << f->depth)) return png_corrupt("PLTE: more entries than the bit depth can index");
            f->npal = static_cast<int>(len / 3);
            std::memcpy(f->plte, p, len);
            stage = PLTE;
        } else if (tag_is(tag, "tRNS")) {
            if (stage == TRNS) return png_corrupt("a second tRNS");
            if (stage > TRNS) return png_corrupt("tRNS after IDAT");
            if (f->color_type == 4 || f->color_type == 6) return png_corrupt("tRNS in a file with an alpha channel");
            if (f->color_type == 3) {
                if (stage != PLTE) return png_corrupt("tRNS before PLTE");
                if (len > 256) return png_corrupt("tRNS: more than 256 alphas");
                f->ntrns = static_cast<int>(len);
                std::memcpy(f->trns, p, len);
            } else {
                const uint32_t want = f->color_type == 0 ? 2 : 6;
                if (len != want) return png_corrupt("tRNS: one 16-bit sample for greyscale, three for truecolour");
                for (uint32_t i = 0; i < want / 2; i++) f->trns16[i] = static_cast<uint16_t>((p[2 * i] << 8) | p[2 * i + 1]);
            }
            f->has_trns = true;
            stage = TRNS;
        } else if (tag_is(tag, "IDAT")) {
            if (stage == AFTER_IDAT) return png_corrupt("IDAT chunks that are not consecutive");
            if (f->color_type == 3 && f->npal == 0) return png_corrupt("a paletted file without PLTE");
            f->idat.insert(f->idat.end(), p, p + len);
            stage = IDAT;
        } else if (tag_is(tag, "IEND")) {
            if (len != 0) return png_corrupt("IEND with a body");
            if (stage < IDAT) return png_corrupt("IEND before any IDAT");
            return FNX_OK;
        } else {
            // every other chunk is skipped, its CRC checked (image/png does the same with critical chunks it does not know)
            if (stage == IDAT) stage = AFTER_IDAT;
        }
    }
}

// ---- inflate (RFC 1950 / 1951) --------------------------------------------------------------------------------------------
namespace {

constexpr int FAST_BITS = 10;

// a canonical Huffman code: by the next FAST_BITS bits of the stream (symbol << 4 | length; 0: a longer code or none), and
// -- for the longer ones -- the per-length counts and the symbols in code order (RFC 1951, 3.2.2)
struct Huff {
    uint16_t fast[1 << FAST_BITS];
    uint16_t count[16];
    uint16_t symbol[288];
};

// -> 0: complete; > 0: incomplete (codes left over); < 0: over-subscribed
int huff_build(Huff *h, const uint8_t *lens, int n)
{
    std::memset(h->count, 0, sizeof h->count);
    for (int i = 0; i < n; i++) h->count[lens[i]]++;
    h->count[0] = 0;
    int left = 1;
    for (int l = 1; l < 16; l++) {
        left = 2 * left - h->count[l];
        if (left < 0) return left;
    }
    uint16_t offs[17], code[16];
    offs[1] = 0;
    uint32_t c = 0;
    code[0] = 0;
    for (int l = 1; l < 16; l++) {
        offs[l + 1] = static_cast<uint16_t>(offs[l] + h->count[l]);
        c = (c + h->count[l - 1]) << 1;
        code[l] = static_cast<uint16_t>(c);
    }
    std::memset(h->fast, 0, sizeof h->fast);
    for (int s = 0; s < n; s++) {
        const int l = lens[s];
        if (!l) continue;
        h->symbol[offs[l]++] = static_cast<uint16_t>(s);
        const uint32_t cw = code[l]++;
        if (l > FAST_BITS) continue;
        uint32_t rev = 0;                                  // the stream carries a code's most significant bit first
        for (int b = 0; b < l; b++) rev |= ((cw >> b) & 1u) << (l - 1 - b);
        for (uint32_t k = rev; k < (1u << FAST_BITS); k += 1u << l) h->fast[k] = static_cast<uint16_t>((s << 4) | l);
    }
    return left;
}

struct Bits {
    const uint8_t *p, *end;
    uint64_t buf = 0;
    int cnt = 0;             // valid bits in buf
    void fill()
    {
        while (cnt <= 56 && p < end) {
            buf |= static_cast<uint64_t>(*p++) << cnt;
            cnt += 8;
        }
    }
    // n <= 16 bits, least significant first; false: the stream ends first
    bool get(int n, uint32_t *v)
    {
        if (cnt < n) {
            fill();
            if (cnt < n) return false;
        }
        *v = static_cast<uint32_t>(buf) & ((1u << n) - 1u);
        buf >>= n;
        cnt -= n;
        return true;
    }
};

// the next symbol of code h; -1: the stream ends inside it, -2: a bit pattern that is no code
int huff_read(const Huff &h, Bits &br)
{
    if (br.cnt < 15) br.fill();
    const uint32_t peek = static_cast<uint32_t>(br.buf);           // bits past cnt are zero
    const uint16_t e = h.fast[peek & ((1u << FAST_BITS) - 1u)];
    if (e) {
        const int l = e & 15;
        if (l > br.cnt) return -1;
        br.buf >>= l;
        br.cnt -= l;
        return e >> 4;
    }
    int code = 0, first = 0, index = 0;
    for (int l = 1; l < 16; l++) {
        code |= static_cast<int>((peek >> (l - 1)) & 1u);
        const int c = h.count[l];
        if (code - c < first) {
            if (l > br.cnt) return -1;
            br.buf >>= l;
            br.cnt -= l;
            return h.symbol[index + (code - first)];
        }
        index += c;
        first = (first + c) << 1;
        code <<= 1;
    }
    return br.cnt < 15 ? -1 : -2;
}

const uint16_t LEN_BASE[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
const uint8_t LEN_EXTRA[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
const uint16_t DIST_BASE[30] = {1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145,
                                8193, 12289, 16385, 24577};
const uint8_t DIST_EXTRA[30] = {0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13};

struct FixedCodes {
    Huff ll, d;
    FixedCodes()
    {
        uint8_t l[288];
        for (int i = 0; i < 288; i++) l[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : 8;
        huff_build(&ll, l, 288);
        for (int i = 0; i < 30; i++) l[i] = 5;
        huff_build(&d, l, 30);                             // 30 of the 32 five-bit codes: 30 and 31 never decode
    }
};

// an incomplete literal/length or distance code passes only in the forms zlib's inflate_table and Go's compress/flate pass:
// no code at all (meeting it in the data is the error) or a single code of one bit
bool incomplete_ok(const Huff &h)
{
    int used = 0;
    for (int l = 1; l < 16; l++) used += h.count[l];
    return used == 0 || (used == 1 && h.count[1] == 1);
}

int read_dynamic(Bits &br, Huff *ll, Huff *d)
{
    static const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
    uint32_t hlit, hdist, hclen, v;
    if (!br.get(5, &hlit) || !br.get(5, &hdist) || !br.get(4, &hclen)) return png_corrupt("deflate: the stream ends inside a block header");
    hlit += 257; hdist += 1; hclen += 4;
    if (hlit > 286 || hdist > 30) return png_corrupt("deflate: too many literal/length or distance codes");
    uint8_t lens[320];
    std::memset(lens, 0, 19);
    for (uint32_t i = 0; i < hclen; i++) {
        if (!br.get(3, &v)) return png_corrupt("deflate: the stream ends inside a block header");
        lens[order[i]] = static_cast<uint8_t>(v);
    }
    Huff cl;
    if (huff_build(&cl, lens, 19) != 0) return png_corrupt("deflate: the code-length code is over-subscribed or incomplete");
    const uint32_t total = hlit + hdist;
    uint32_t i = 0;
    while (i < total) {
        const int s = huff_read(cl, br);
        if (s < 0) return png_corrupt(s == -1 ? "deflate: the stream ends inside a block header" : "deflate: a bit pattern that is no code-length code");
        if (s < 16) {
            lens[i++] = static_cast<uint8_t>(s);
            continue;
        }
        uint32_t run = 0;
        uint8_t val = 0;
        if (s == 16) {
            if (i == 0) return png_corrupt("deflate: a repeat with no length before it");
            val = lens[i - 1];
            if (!br.get(2, &run)) return png_corrupt("deflate: the stream ends inside a block header");
            run += 3;
        } else if (s == 17) {
            if (!br.get(3, &run)) return png_corrupt("deflate: the stream ends inside a block header");
            run += 3;
        } else {
            if (!br.get(7, &run)) return png_corrupt("deflate: the stream ends inside a block header");
            run += 11;
        }
        if (i + run > total) return png_corrupt("deflate: a run of code lengths past HLIT + HDIST");
        std::memset(lens + i, val, run);
        i += run;
    }
    if (lens[256] == 0) return png_corrupt("deflate: no end-of-block code");
    int left = huff_build(ll, lens, static_cast<int>(hlit));
    if (left < 0) return png_corrupt("deflate: over-subscribed literal/length code");
    if (left > 0 && !incomplete_ok(*ll)) return png_corrupt("deflate: incomplete literal/length code");
    left = huff_build(d, lens + hlit, static_cast<int>(hdist));
    if (left < 0) return png_corrupt("deflate: over-subscribed distance code");
    if (left > 0 && !incomplete_ok(*d)) return png_corrupt("deflate: incomplete distance code");
    return FNX_OK;
}

uint32_t adler32(const uint8_t *p, size_t n)
{
    uint32_t a = 1, b = 0;
    while (n) {
        const size_t k = n < 5552 ? n : 5552;               // the largest run whose sums fit 32 bits
        for (size_t i = 0; i < k; i++) {
            a += p[i];
            b += a;
        }
        a %= 65521u;
        b %= 65521u;
        p += k;
        n -= k;
    }
    return (b << 16) | a;
}

}  // namespace

int png_inflate(const uint8_t *src, size_t n, uint8_t *out, size_t cap, size_t *nbytes)
{
    *nbytes = 0;
    if (n < 2) return png_corrupt("zlib: no header");
    const uint32_t cmf = src[0], flg = src[1];
    if ((cmf & 15u) != 8 || (cmf >> 4) > 7) return png_corrupt("zlib: not deflate with a window of at most 32 KiB");
    if (((cmf << 8) | flg) % 31u) return png_corrupt("zlib: the header check fails");
    if (flg & 0x20u) return png_corrupt("zlib: a preset dictionary");
    static const FixedCodes fixed;
    Bits br{src + 2, src + n};
    Huff dyn_ll, dyn_d;
    size_t at = 0;
    for (;;) {
        uint32_t bfinal, btype;
        if (!br.get(1, &bfinal) || !br.get(2, &btype)) return png_corrupt("deflate: the stream ends before its last block");
        if (btype == 3) return png_corrupt("deflate: reserved block type 3");
        if (btype == 0) {
            uint32_t v, len, nlen;
            br.get(br.cnt & 7, &v);                         // to the byte boundary (the buffer holds whole bytes behind it)
            if (!br.get(16, &len) || !br.get(16, &nlen)) return png_corrupt("deflate: the stream ends inside a stored block");
            if (len != (nlen ^ 0xffffu)) return png_corrupt("deflate: LEN is not the complement of NLEN");
            if (len > cap - at) {
                *nbytes = cap + 1;          // "cap is too small", told apart from damage
                return png_corrupt("the stream holds more bytes than the output takes");
            }
            uint32_t k = 0;
            for (; k < len && br.cnt >= 8; k++) {           // the bytes already in the bit buffer, then the rest in one copy
                out[at + k] = static_cast<uint8_t>(br.buf);
                br.buf >>= 8;
                br.cnt -= 8;
            }
            if (static_cast<size_t>(br.end - br.p) < len - k) return png_corrupt("deflate: the stream ends inside a stored block");
            if (len - k) std::memcpy(out + at + k, br.p, len - k);
            br.p += len - k;
            at += len;
        } else {
            const Huff *ll = &fixed.ll, *d = &fixed.d;
            if (btype == 2) {
                FNX_TRY(read_dynamic(br, &dyn_ll, &dyn_d));
                ll = &dyn_ll;
                d = &dyn_d;
            }
            for (;;) {
                const int s = huff_read(*ll, br);
                if (s < 0) return png_corrupt(s == -1 ? "deflate: the stream ends inside a block" : "deflate: a bit pattern that is no literal/length code");
                if (s < 256) {
                    if (at >= cap) {
                        *nbytes = cap + 1;          // "cap is too small", told apart from damage
                        return png_corrupt("the stream holds more bytes than the output takes");
                    }
                    out[at++] = static_cast<uint8_t>(s);
                    continue;
                }
                if (s == 256) break;
                if (s > 285) return png_corrupt("deflate: literal/length symbol 286 or 287");
                uint32_t e = 0;
                if (!br.get(LEN_EXTRA[s - 257], &e)) return png_corrupt("deflate: the stream ends inside a block");
                const size_t len = LEN_BASE[s - 257] + e;
                const int ds = huff_read(*d, br);
                if (ds < 0) return png_corrupt(ds == -1 ? "deflate: the stream ends inside a block" : "deflate: a bit pattern that is no distance code");
                if (ds > 29) return png_corrupt("deflate: distance symbol 30 or 31");
                if (!br.get(DIST_EXTRA[ds], &e)) return png_corrupt("deflate: the stream ends inside a block");
                const size_t dist = DIST_BASE[ds] + e;
                if (dist > at) return png_corrupt("deflate: a distance that reaches before the start of the output");
                if (len > cap - at) {
                    *nbytes = cap + 1;          // "cap is too small", told apart from damage
                    return png_corrupt("the stream holds more bytes than the output takes");
                }
                if (dist >= len) {
                    std::memcpy(out + at, out + at - dist, len);
                } else {
                    for (size_t i = 0; i < len; i++) out[at + i] = out[at - dist + i];
                }
                at += len;
            }
        }
        if (bfinal) break;
    }
    *nbytes = at;
    uint32_t v, check = 0;
    br.get(br.cnt & 7, &v);
    for (int i = 0; i < 4; i++) {
        if (!br.get(8, &v)) return png_corrupt("zlib: the stream ends before its Adler-32 does");
        check = (check << 8) | v;
    }
    if (check != adler32(out, at)) return png_corrupt("zlib: the Adler-32 does not match the output");
    return FNX_OK;
}

size_t png_stream_bytes(const PngFile &f) { return f.interlace == 1 ? f.pstream : static_cast<size_t>(f.h) * (1 + f.rowbytes); }

size_t png_planes_bytes(const PngFile &f)
{
    if (f.interlace != 1) return ((f.rowbytes + 15) & ~size_t(15)) * f.h;
    size_t total = 0;
    for (int p = 0; p < 7; p++) total += ((f.prow[p] + 15) & ~size_t(15)) * f.ph[p];
    return total;
}

PngExpand png_expand_of(const PngFile &f)
{
    return PngExpand{f.w, f.h, f.color_type, f.depth, f.has_trns ? 1 : 0, {f.trns16[0], f.trns16[1], f.trns16[2]}};
}

int png_adam7_passes(const PngFile &f, const uint8_t *stream, uint8_t *rows, uint32_t first, PngBatchFile passes[7], PngAdam7File *a, uint32_t slot[7])
{
    int n = 0;
    for (int p = 0; p < 7; p++) {
        slot[p] = 0;
        if (f.ph[p] == 0) continue;
        PngBatchFile &dp = passes[n];                 // the unfilter kernel's view of the pass: an image of its own
        std::memset(&dp, 0, sizeof dp);
        dp.stream = stream + f.poff[p];
        dp.spitch = 1 + f.prow[p];
        dp.rows = rows;
        dp.ppitch = align16(f.prow[p]);
        dp.rowbytes = static_cast<int>(f.prow[p]);
        dp.npix = static_cast<int>(f.prow[p] / f.bpp);
        a->plane[p] = rows;
        a->ppitch[p] = static_cast<uint32_t>(dp.ppitch);
        rows += dp.ppitch * f.ph[p];
        slot[p] = first + n++;
    }
    return n;
}

int png_stream_size(const PngFile &f, size_t *want)
{
    *want = png_stream_bytes(f);
    // a deflate stream grows at most 1032-fold (258 bytes from a one-bit length code and a one-bit distance code): a header
    // that promises more than its IDAT bytes can hold is refused before a byte of memory is sized by it
    if (*want / 1032 > f.idat.size()) return png_corrupt("not enough pixel data");
    return FNX_OK;
}

namespace {

// the units of one image of h rows, `pitch` bytes apart, appended
int plan_rows(const uint8_t *stream, size_t pitch, int h, std::vector<uint32_t> *units)
{
    uint32_t start = 0;
    for (int y = 0; y < h; y++) {
        const uint8_t t = stream[static_cast<size_t>(y) * pitch];
        if (t > 4) return png_corrupt("a filter type above 4");
        // a None or Sub row does not read the row above: a chain segment starts here, and with it -- once the unit in hand
        // holds PNG_UNIT_MIN_ROWS rows -- a new unit
        if (t <= 1 && static_cast<uint32_t>(y) - start >= static_cast<uint32_t>(PNG_UNIT_MIN_ROWS)) {
            units->push_back(start);
            units->push_back(static_cast<uint32_t>(y));
            start = static_cast<uint32_t>(y);
        }
    }
    units->push_back(start);
    units->push_back(static_cast<uint32_t>(h));
    return FNX_OK;
}

}  // namespace

int png_row_plan(const uint8_t *stream, const PngFile &f, std::vector<uint32_t> *units, std::vector<uint8_t> *passes)
{
    units->clear();
    if (passes) passes->clear();
    if (f.interlace != 1) return plan_rows(stream, 1 + f.rowbytes, f.h, units);
    for (int p = 0; p < 7; p++) {
        if (f.ph[p] == 0) continue;
        FNX_TRY(plan_rows(stream + f.poff[p], 1 + f.prow[p], f.ph[p], units));
        if (passes) passes->resize(units->size() / 2, static_cast<uint8_t>(p));
    }
    return FNX_OK;
}

void png_palette_table(const PngFile &f, uint32_t table[256])
{
    for (int i = 0; i < 256; i++) {
        // an entry behind the palette's end reads as opaque black; tRNS gives entry i its alpha
        const uint32_t r = i < f.npal ? f.plte[3 * i] : 0, g = i < f.npal ? f.plte[3 * i + 1] : 0, b = i < f.npal ? f.plte[3 * i + 2] : 0;
        const uint32_t t = i < f.ntrns ? f.trns[i] : 255;
        uint32_t o[3] = {r, g, b};
        if (t == 0) {
            o[0] = o[1] = o[2] = 0;
        } else if (t != 255) {
            const uint32_t a16 = t * 0x101u;
            for (int k = 0; k < 3; k++) {
                const uint32_t pre = (o[k] * 0x101u) * t / 0xffu;       // color.NRGBA.RGBA()
                o[k] = (pre * 0xffffu / a16) >> 8;                      // convertToNRGBA (convert.go:34-64)
            }
        }
        table[i] = o[0] | (o[1] << 8) | (o[2] << 16) | (t << 24);
    }
}

// ---- a list of files on several threads (fnx_png_decode_batch) ------------------------------------------------------------
namespace {

int prepare_one(const uint8_t *data, size_t n, PngPrepared *it, bool adam7)
{
    FNX_TRY(png_parse(data, n, &it->f, adam7));
    FNX_TRY(png_stream_size(it->f, &it->want));
    if (it->stream == nullptr || it->want > it->cap) return png_corrupt("internal: no staging for a file's stream");
    size_t got = 0;
    FNX_TRY(png_inflate(it->f.idat.data(), it->f.idat.size(), it->stream, it->want, &got));
    if (got != it->want) return png_corrupt("not enough pixel data");
    FNX_TRY(png_row_plan(it->stream, it->f, &it->units, &it->unit_pass));
    if (it->f.color_type == 3) png_palette_table(it->f, it->table);
    return FNX_OK;
}

}  // namespace

int png_workers(int workers, int m)
{
    if (workers == 0) workers = 8;
    return workers < m ? workers : m;
}

void png_prepare_many(const uint8_t *const *files, const size_t *sizes, int m, int workers, PngPrepared *items, bool adam7)
{
    std::atomic<int> next(0);
    auto run = [&]() {
        for (int i = next.fetch_add(1); i < m; i = next.fetch_add(1)) {
            PngPrepared &it = items[i];
            std::memset(it.table, 0, sizeof it.table);
            it.what = nullptr;
            it.status = prepare_one(files[i], sizes[i], &it, adam7);
            if (it.status != FNX_OK) it.what = t_what;
            it.f.idat = std::vector<uint8_t>();          // the compressed bytes are not needed again
        }
    };
    const int nthreads = png_workers(workers, m);
    std::vector<std::thread> pool;
    try {
        for (int t = 1; t < nthreads; t++) pool.emplace_back(run);
    } catch (const std::system_error &) {
        // no (further) thread to be had: the ones that started and this one share the files
    }
    run();
    for (std::thread &t : pool) t.join();
}

int png_reissue(const PngPrepared &it)
{
    if (it.status == FNX_OK) return FNX_OK;
    return it.status == FNX_ERR_UNSUPPORTED ? png_unsupported(it.what ? it.what : "") : png_corrupt(it.what ? it.what : "");
}

}  // namespace fnx

extern "C" {

int fnx_inflate(const uint8_t *src, size_t n, uint8_t *out, size_t cap, size_t *nbytes)
{
    if (!src || !nbytes || (!out && cap)) {
        fnx::set_error("invalid argument: fnx_inflate: src, nbytes, or out with cap > 0, is null");
        return FNX_ERR_INVALID;
    }
    uint8_t none = 0;
    return fnx::png_inflate(src, n, out ? out : &none, cap, nbytes);
}

int fnx_png_info(const uint8_t *data, size_t n, int *w, int *h, int *color_type, int *bit_depth, int *interlace)
{
    if (!data || !w || !h || !color_type || !bit_depth || !interlace) {
        fnx::set_error("invalid argument: fnx_png_info: a null pointer");
        return FNX_ERR_INVALID;
    }
    fnx::PngFile f;
    FNX_TRY(fnx::read_ihdr(data, n, &f));
    *w = f.w; *h = f.h; *color_type = f.color_type; *bit_depth = f.depth; *interlace = f.interlace;
    return FNX_OK;
}

int fnx_png_adam7_passes(int w, int h, int color_type, int depth, int pw[7], int ph[7], size_t rowbytes[7], size_t *stream_bytes)
{
    if (!pw || !ph || !rowbytes || !stream_bytes) {
        fnx::set_error("invalid argument: fnx_png_adam7_passes: a null pointer");
        return FNX_ERR_INVALID;
    }
    const int ct = color_type, d = depth;
    const bool pair = (ct == 0 && (d == 1 || d == 2 || d == 4 || d == 8 || d == 16)) || (ct == 3 && (d == 1 || d == 2 || d == 4 || d == 8)) ||
                      ((ct == 2 || ct == 4 || ct == 6) && (d == 8 || d == 16));
    if (!pair || w < 1 || h < 1 || w > 65535 || h > 65535) {
        fnx::set_error("invalid argument: fnx_png_adam7_passes: one of the 15 colour type / bit depth pairs, dimensions 1..65535");
        return FNX_ERR_INVALID;
    }
    const int channels = ct == 0 || ct == 3 ? 1 : ct == 4 ? 2 : ct == 2 ? 3 : 4;
    *stream_bytes = fnx::png_adam7_geometry(w, h, channels * d, pw, ph, rowbytes);
    return FNX_OK;
}

}  // extern "C"
