// The PNG host code that writes a file's frame (png_frame.cpp) and that describes an Adam7 file's passes to the device
// (png_parse.cpp: png_adam7_passes) without a GPU and without the rest of the library, under the address and
// undefined-behaviour sanitizers.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -Ifennec_amd/csrc tools/png_frame_host.cpp fennec_amd/csrc/png_frame.cpp fennec_amd/csrc/png_parse.cpp \
//       fennec_amd/csrc/png_compress_plan.cpp -o /tmp/png_frame_host
//   /tmp/png_frame_host frame cases out     cases: records of six little-endian uint32 (w, h, colour type, bit depth, ncolors,
//                                           zsize), ncolors x 4 palette bytes r g b a, zsize stream bytes.  Each record's file
//                                           is built in a buffer of exactly file_bytes(zsize) bytes with canary bytes behind
//                                           it; out: per record a uint32 length and the file
//   /tmp/png_frame_host adam7 file.png      an Adam7 file's pass descriptors with first index 0 and 5, as text
// tests/test_png_frame_host.py writes the inputs and checks the outputs.
#include <cstdio>
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

static int frames(const char *cases, const char *out)
{
    std::vector<uint8_t> in;
    if (!read_file(cases, &in)) return 2;
    FILE *fp = std::fopen(out, "wb");
    if (!fp) { std::perror(out); return 2; }
    constexpr size_t CANARY = 32;
    int count = 0;
    for (size_t at = 0; at < in.size(); count++) {
        uint32_t v[6];
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
        std::vector<uint8_t> file(n + CANARY, 0xa5);
        uint8_t *idat = fnx::png_frame_head(frame, file.data());
        if (static_cast<size_t>(idat - file.data()) + 12 + zsize + 12 != n) {
            std::fprintf(stderr, "case %d: the head ends %zu bytes in, file_bytes is %zu\n", count, static_cast<size_t>(idat - file.data()), n);
            return 1;
        }
        std::memcpy(idat + 8, z, zsize);
        fnx::png_frame_tail(idat, zsize);
        for (size_t k = 0; k < CANARY; k++) {
            if (file[n + k] != 0xa5) { std::fprintf(stderr, "case %d: byte %zu behind the file was written\n", count, k); return 1; }
        }
        if (!fnx::png_signature(file.data(), n) || fnx::png_signature(file.data(), 7) || fnx::png_signature(file.data() + 1, n - 1)) {
            std::fprintf(stderr, "case %d: png_signature\n", count);
            return 1;
        }
        const uint32_t len = static_cast<uint32_t>(n);
        std::fwrite(&len, sizeof len, 1, fp);
        std::fwrite(file.data(), 1, n, fp);
    }
    std::fclose(fp);
    std::printf("png_frame_host: %d frames; no sanitizer report\n", count);
    return 0;
}

struct Passes {
    fnx::PngBatchFile d[7];
    fnx::PngAdam7File a;
    uint32_t slot[7];
    int n;
};

static int adam7(const char *path)
{
    std::vector<uint8_t> g;
    if (!read_file(path, &g)) return 2;
    fnx::PngFile f;
    if (fnx::png_probe(g.data(), g.size(), &f, true) != FNX_OK || f.interlace != 1) { std::fprintf(stderr, "%s: no Adam7 file\n", path); return 2; }
    // stand-ins for the device's stream and planes: the descriptors only point into them
    std::vector<uint8_t> stream(fnx::png_stream_bytes(f) + 64), planes(fnx::png_planes_bytes(f) + 16);
    Passes r[2];
    const uint32_t firsts[2] = {0, 5};
    for (int k = 0; k < 2; k++) {
        std::memset(&r[k], 0, sizeof r[k]);
        r[k].n = fnx::png_adam7_passes(f, stream.data(), planes.data(), firsts[k], r[k].d, &r[k].a, r[k].slot);
    }
    bool same = r[0].n == r[1].n && std::memcmp(r[0].d, r[1].d, sizeof r[0].d) == 0 && std::memcmp(&r[0].a, &r[1].a, sizeof r[0].a) == 0;
    for (int p = 0; p < 7; p++) same = same && (f.ph[p] ? r[1].slot[p] == r[0].slot[p] + 5 : r[0].slot[p] == 0 && r[1].slot[p] == 0);
    if (!same) { std::fprintf(stderr, "first index 0 and 5 differ by more than the offset\n"); return 1; }
    std::printf("count %d planes_bytes %zu stream_bytes %zu\n", r[0].n, fnx::png_planes_bytes(f), fnx::png_stream_bytes(f));
    for (int p = 0, k = 0; p < 7; p++) {
        if (f.ph[p] == 0) {
            if (r[0].a.plane[p] != nullptr || r[0].a.ppitch[p] != 0) { std::fprintf(stderr, "an absent pass has a plane\n"); return 1; }
            continue;
        }
        const fnx::PngBatchFile &d = r[0].d[k++];
        if (d.rows != r[0].a.plane[p] || d.ppitch != r[0].a.ppitch[p]) { std::fprintf(stderr, "pass %d: descriptor and plane table disagree\n", p); return 1; }
        std::printf("pass %d slot %u slot5 %u off %zu spitch %zu rows %zu ppitch %zu rowbytes %d npix %d ph %d\n", p, r[0].slot[p], r[1].slot[p],
                    static_cast<size_t>(d.stream - stream.data()), d.spitch, static_cast<size_t>(d.rows - planes.data()), d.ppitch, d.rowbytes, d.npix,
                    f.ph[p]);
    }
    std::printf("png_frame_host: no sanitizer report\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && std::strcmp(argv[1], "frame") == 0) return frames(argv[2], argv[3]);
    if (argc == 3 && std::strcmp(argv[1], "adam7") == 0) return adam7(argv[2]);
    std::fprintf(stderr, "usage: %s frame cases out | adam7 file.png\n", argv[0]);
    return 2;
}
