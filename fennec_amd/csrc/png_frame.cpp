// The file around a zlib stream: signature, IHDR, PLTE + tRNS for colour type 3, one IDAT, IEND, and the chunks' CRCs -- what
// fnx_png_encode and the compress batch write on the host (on a ctx at FNX_PNG_CRC_DEVICE the IDAT chunk's CRC is handed in:
// crc32.hip).  Plain C++: no HIP call, no ctx (tools/png_frame_host.cpp and tools/png_frame_crc_host.cpp run it under the
// sanitizers).
#include "common.hpp"

namespace fnx {

namespace {

// CRC-32 of PNG's chunks (ISO 3309, polynomial 0xedb88320 reflected), eight bytes a step
struct CrcTables {
    uint32_t t[8][256];
    CrcTables()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++) {
            for (int s = 1; s < 8; s++) t[s][i] = t[0][t[s - 1][i] & 0xffu] ^ (t[s - 1][i] >> 8);
        }
    }
};

uint32_t crc32_update(uint32_t crc, const uint8_t *p, size_t n)     // crc: the running register (start 0xffffffff, invert at the end)
{
    static const CrcTables tab;
    while (n >= 8) {
        uint32_t a, b;
        std::memcpy(&a, p, 4);
        std::memcpy(&b, p + 4, 4);
        a ^= crc;
        crc = tab.t[7][a & 0xffu] ^ tab.t[6][(a >> 8) & 0xffu] ^ tab.t[5][(a >> 16) & 0xffu] ^ tab.t[4][a >> 24] ^
              tab.t[3][b & 0xffu] ^ tab.t[2][(b >> 8) & 0xffu] ^ tab.t[1][(b >> 16) & 0xffu] ^ tab.t[0][b >> 24];
        p += 8;
        n -= 8;
    }
    for (; n; n--) crc = tab.t[0][(crc ^ *p++) & 0xffu] ^ (crc >> 8);
    return crc;
}

void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = static_cast<uint8_t>(v >> 24); p[1] = static_cast<uint8_t>(v >> 16); p[2] = static_cast<uint8_t>(v >> 8); p[3] = static_cast<uint8_t>(v);
}

// a chunk whose `len` body bytes already sit at at + 8 and whose CRC is given: length and tag in front, CRC behind (the body
// is not read); returns the chunk's end
uint8_t *close_chunk(uint8_t *at, const char *tag, size_t len, uint32_t crc)
{
    put_be32(at, static_cast<uint32_t>(len));
    std::memcpy(at + 4, tag, 4);
    put_be32(at + 8 + len, crc);
    return at + 12 + len;
}

// the same with the CRC computed here, over the tag and the body
uint8_t *close_chunk(uint8_t *at, const char *tag, size_t len)
{
    std::memcpy(at + 4, tag, 4);
    return close_chunk(at, tag, len, ~crc32_update(0xffffffffu, at + 4, 4 + len));
}

}  // namespace

uint8_t *png_frame_head(const PngFrame &f, uint8_t *out)
{
    std::memcpy(out, PNG_SIG, 8);
    uint8_t *at = out + 8;
    put_be32(at + 8, static_cast<uint32_t>(f.w));
    put_be32(at + 12, static_cast<uint32_t>(f.h));
    at[16] = static_cast<uint8_t>(f.bit_depth); at[17] = static_cast<uint8_t>(f.color_type); at[18] = 0; at[19] = 0; at[20] = 0;
    at = close_chunk(at, "IHDR", 13);
    if (f.color_type == 3) {
        const int ntrns = f.ntrns();
        for (int i = 0; i < f.ncolors; i++) std::memcpy(at + 8 + 3 * i, f.palette + 4 * i, 3);
        at = close_chunk(at, "PLTE", 3 * static_cast<size_t>(f.ncolors));
        if (ntrns) {
            for (int i = 0; i < ntrns; i++) at[8 + i] = f.palette[4 * i + 3];
            at = close_chunk(at, "tRNS", static_cast<size_t>(ntrns));
        }
    }
    return at;
}

void png_frame_tail(uint8_t *idat, size_t zsize)
{
    close_chunk(close_chunk(idat, "IDAT", zsize), "IEND", 0);
}

void png_frame_tail(uint8_t *idat, size_t zsize, uint32_t idat_crc)
{
    close_chunk(close_chunk(idat, "IDAT", zsize, idat_crc), "IEND", 0);
}

uint32_t png_idat_seed()
{
    return crc32_update(0xffffffffu, reinterpret_cast<const uint8_t *>("IDAT"), 4);
}

}  // namespace fnx
