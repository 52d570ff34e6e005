// crc32_piece.inc on the CPU: the text crc32.hip's kernels include, with a workgroup's 256 lanes as a loop -- a launch of
// crc32_pieces_kernel as a loop over the pieces, then crc32_fold_kernel's workgroup.
//   crc32_hostsim <file of cases>
// reads one case per line -- <name> <offset 0..15> <length> <crc, hexadecimal> <file of bytes> -- takes the file's first
// <length> bytes, puts them <offset> bytes behind an aligned address (in a buffer that ends with them, unrelated bytes in front)
// and prints per case
//   <name> <CRC, 8 hexadecimal digits>
// the value zlib.crc32(bytes, crc) has: crc is the finished CRC of what came before, 0 for none.  Exit status 1 on a line it
// cannot read, a file shorter than the case's length, or a failed self-check of the constants.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "fennec_hip.h"

namespace {

#define CRC_FN static inline
#define CRC_CONST static const
#define CRC_UNROLL
#define CRC_LD32(p) crc_ld32(p)
#define CRC_PHASE(call)                                 \
    for (int lane = 0; lane < CRC_LANES; lane++) {      \
        CrcLane &ln = lanes[lane];                      \
        (void)ln;                                       \
        call;                                           \
    }
#define CRC_RUN_PARAMS , CrcLane *lanes

inline uint32_t crc_ld32(const uint8_t *p)
{
    if (reinterpret_cast<uintptr_t>(p) & 3u) {
        std::fprintf(stderr, "a dword load from an address that is not a multiple of 4\n");
        std::exit(1);
    }
    uint32_t v;
    std::memcpy(&v, p, 4);
    return v;
}

#include "crc32_piece.inc"

bool read_file(const std::string &path, std::vector<uint8_t> *g)
{
    std::ifstream in(path, std::ios::binary);
    if (!in) return false;
    g->assign(std::istreambuf_iterator<char>(in), std::istreambuf_iterator<char>());
    return true;
}

// what the two launches compute for the n bytes at p
uint32_t crc_of(const uint8_t *p, size_t n, uint32_t crc)
{
    std::vector<uint32_t> words(crc_pieces_of(n), 0xa5a5a5a5u);   // (exactly the pieces: a word past them is a report)
    std::vector<CrcLane> lanes(CRC_LANES);
    CrcShared s;
    for (size_t j = 0; j < words.size(); j++) {
        std::memset(&s, 0xa5, sizeof s);                           // nothing may be read before a phase wrote it
        std::memset(static_cast<void *>(lanes.data()), 0xa5, sizeof(CrcLane) * lanes.size());
        const size_t off = j * CRC_PIECE;
        words[j] = crc_piece(p + off, static_cast<uint32_t>(n - off < CRC_PIECE ? n - off : CRC_PIECE), s, lanes.data());
    }
    std::memset(&s, 0xa5, sizeof s);
    return crc_stream(words.data(), n, ~crc, s, lanes.data());
}

bool self_check()
{
    // x^(8 2^k) by single steps for the first entries, the squaring rule for the rest, and the order of x
    uint32_t p = 0x80000000u;
    for (int i = 0; i < 8; i++) p = (p >> 1) ^ (CRC_POLY & (0u - (p & 1u)));
    if (p != CRC_POW.v[0]) return false;
    for (int k = 0; k + 1 < 32; k++) {
        if (crc_mulmod(CRC_POW.v[k], CRC_POW.v[k]) != CRC_POW.v[k + 1]) return false;
    }
    for (uint32_t v : {0x80000000u, 0x12345678u, 0xffffffffu}) {
        if (crc_shift(v, 0) != v || crc_shift(v, 0xffffffffull) != v || crc_shift(v, (1ull << 32) + 5) != crc_shift(v, 6)) return false;
    }
    return true;
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: crc32_hostsim <file of cases>\n");
        return 1;
    }
    if (!self_check()) {
        std::fprintf(stderr, "the constants of crc32_piece.inc fail their self-check\n");
        return 1;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    std::map<std::string, std::vector<uint8_t>> files;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string name, path;
        unsigned long long offset = 0, length = 0;
        uint32_t crc = 0;
        ls >> name >> offset >> length >> std::hex >> crc >> path;
        if (!ls || offset > 15) {
            std::fprintf(stderr, "bad line: %.80s\n", line.c_str());
            return 1;
        }
        if (!files.count(path) && !read_file(path, &files[path])) {
            std::fprintf(stderr, "cannot read %s\n", path.c_str());
            return 1;
        }
        const std::vector<uint8_t> &bytes = files[path];
        if (bytes.size() < length) {
            std::fprintf(stderr, "%s: %s holds %zu bytes, not %llu\n", name.c_str(), path.c_str(), bytes.size(), length);
            return 1;
        }
        // operator new's memory is 16-byte aligned; the case's bytes end the buffer, so a read behind them is a report
        std::vector<uint8_t> buf(offset + length, 0x5a);
        if (length) std::memcpy(buf.data() + offset, bytes.data(), length);
        std::printf("%s %08x\n", name.c_str(), crc_of(buf.data() + offset, length, crc));
    }
    return 0;
}
