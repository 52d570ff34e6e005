// png_frame.cpp's tail with the IDAT chunk's CRC handed in (the form the device-CRC routes use: fnx_ctx_set_png_crc) without a
// GPU and without the rest of the library, under the address and undefined-behaviour sanitizers.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -Ifennec_amd/csrc tools/png_frame_crc_host.cpp fennec_amd/csrc/png_frame.cpp fennec_amd/csrc/png_parse.cpp \
//       fennec_amd/csrc/png_compress_plan.cpp -o /tmp/png_frame_crc_host
//   /tmp/png_frame_crc_host cases out     cases: records of seven little-endian uint32 (w, h, colour type, bit depth, ncolors,
//                                         zsize, the IDAT chunk's CRC), ncolors x 4 palette bytes r g b a, zsize stream bytes.
//                                         Each record's file is built in a buffer of exactly file_bytes(zsize) bytes with canary
//                                         bytes behind it, once by each form of png_frame_tail; out: per record a uint32
//                                         length and the file of the given-CRC form, then the same of the computing form
// The first line of stdout is png_idat_seed() in hexadecimal.  tests/test_png_crc_abi.py writes the inputs and checks the outputs.
//   /tmp/png_frame_crc_host time bodies reps   bodies: records of a little-endian uint32 zsize and zsize bytes.  Times the
//                                         computing form of png_frame_tail -- crc32_update over "IDAT" and the body -- over all
//                                         records, reps times, and prints the median in ms per pass (tools/time_png_crc.py
//                                         builds it with -O3 and no sanitizer for that)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "common.hpp"

namespace fnx {
void set_error(const char *, ...) {}
}  // namespace fnx

static bool read_file(const char *path, std::vector<uint8_t> *g)
{
    FILE *fp = std::fopen(path, "rb");
    if (!fp) { std::perror(path); return false; }
    uint8_t buf[65536];
    size_t k;
    while ((k = std::fread(buf, 1, sizeof buf, fp)) > 0) g->insert(g->end(), buf, buf + k);
    std::fclose(fp);
    return true;
}

static int time_tail(const char *path, int reps)
{
    std::vector<uint8_t> in;
    if (!read_file(path, &in) || reps < 1) return 2;
    std::vector<std::vector<uint8_t>> chunks;                        // 8 bytes of length and tag, the body, 12 + 12 bytes behind
    for (size_t at = 0; at < in.size();) {
        uint32_t zsize;
        if (in.size() - at < sizeof zsize) return 2;
        std::memcpy(&zsize, in.data() + at, sizeof zsize);
        at += sizeof zsize;
        if (in.size() - at < zsize) return 2;
        chunks.emplace_back(8 + static_cast<size_t>(zsize) + 24);
        std::memcpy(chunks.back().data() + 8, in.data() + at, zsize);
        at += zsize;
    }
    std::vector<double> ms;
    for (int r = 0; r < reps; r++) {
        const auto t0 = std::chrono::steady_clock::now();
        for (auto &c : chunks) fnx::png_frame_tail(c.data(), c.size() - 32);
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("%.6f ms per pass over %zu chunks (median of %d)\n", ms[ms.size() / 2], chunks.size(), reps);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && std::strcmp(argv[1], "time") == 0) return time_tail(argv[2], std::atoi(argv[3]));
    if (argc != 3) {
        std::fprintf(stderr, "usage: %s cases out | time bodies reps\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> in;
    if (!read_file(argv[1], &in)) return 2;
    FILE *fp = std::fopen(argv[2], "wb");
    if (!fp) { std::perror(argv[2]); return 2; }
    std::printf("%08x\n", fnx::png_idat_seed());
    constexpr size_t CANARY = 32;
    int count = 0;
    for (size_t at = 0; at < in.size(); count++) {
        uint32_t v[7];
        if (in.size() - at < sizeof v) { std::fprintf(stderr, "case %d: a short record\n", count); return 2; }
        std::memcpy(v, in.data() + at, sizeof v);
        at += sizeof v;
        const size_t pal = 4 * static_cast<size_t>(v[4]), zsize = v[5];
        if (in.size() - at < pal + zsize) { std::fprintf(stderr, "case %d: a short record\n", count); return 2; }
        const std::vector<uint8_t> palette(in.begin() + at, in.begin() + at + pal);
        const uint8_t *z = in.data() + at + pal;
        at += pal + zsize;
        const fnx::PngFrame frame{static_cast<int>(v[0]), static_cast<int>(v[1]), static_cast<int>(v[2]), static_cast<int>(v[3]), static_cast<int>(v[4]),
                                  palette.data()};
        const size_t n = frame.file_bytes(zsize);
        for (int form = 0; form < 2; form++) {
            std::vector<uint8_t> file(n + CANARY, 0xa5);
            uint8_t *idat = fnx::png_frame_head(frame, file.data());
            std::memcpy(idat + 8, z, zsize);
            if (form == 0) fnx::png_frame_tail(idat, zsize, v[6]);
            else fnx::png_frame_tail(idat, zsize);
            for (size_t k = 0; k < CANARY; k++) {
                if (file[n + k] != 0xa5) { std::fprintf(stderr, "case %d: byte %zu behind the file was written\n", count, k); return 1; }
            }
            const uint32_t len = static_cast<uint32_t>(n);
            std::fwrite(&len, sizeof len, 1, fp);
            std::fwrite(file.data(), 1, n, fp);
        }
    }
    std::fclose(fp);
    std::printf("png_frame_crc_host: %d frames; no sanitizer report\n", count);
    return 0;
}
