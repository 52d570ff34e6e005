// fnx_png_decode_batch's host side (png_parse.cpp: png_prepare_many -- chunk walk, inflate, row plan, palette table of a list of
// files on several threads) without a GPU and without the rest of the library, to be built twice: under the address and
// undefined-behaviour sanitizers, and under the thread sanitizer.
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -Ifennec_amd/csrc tools/png_batch_host.cpp fennec_amd/csrc/png_parse.cpp -o /tmp/png_batch_host
//   (and the same with -fsanitize=thread)
//   /tmp/png_batch_host file1 file2 ...        any files: PNG, damaged, interlaced, empty, something else
// Every file gets room for exactly the bytes its header promises (so a byte too many is a report), the list is prepared
// with workers = 1, 3 and 8 (and 0), and each item's status, refusal text, stream bytes, unit table and palette table must
// equal the workers = 1 result.  tests/test_png_batch_host.py writes the files and runs both builds.
#include <cstdio>
#include <cstring>
#include <vector>
#include "common.hpp"

namespace fnx {
void set_error(const char *, ...) {}
}  // namespace fnx

struct Run {
    std::vector<fnx::PngPrepared> items;
    std::vector<std::vector<uint8_t>> streams;
};

static void prepare(const std::vector<std::vector<uint8_t>> &files, int workers, Run *r)
{
    const int m = static_cast<int>(files.size());
    std::vector<const uint8_t *> ptrs(m);
    std::vector<size_t> sizes(m);
    r->items.assign(m, fnx::PngPrepared());
    r->streams.assign(m, std::vector<uint8_t>());
    static const uint8_t none = 0;
    for (int i = 0; i < m; i++) {
        ptrs[i] = files[i].empty() ? &none : files[i].data();
        sizes[i] = files[i].size();
        // as fnx_png_decode_batch sizes the staging area: from the IHDR alone, nothing for a file that cannot hold its rows
        fnx::PngFile head;
        if (fnx::png_probe(ptrs[i], sizes[i], &head) != FNX_OK) continue;
        const size_t want = static_cast<size_t>(head.h) * (1 + head.rowbytes);
        if (want / 1032 > sizes[i]) continue;
        r->streams[i].assign(want, 0xee);
        r->items[i].stream = r->streams[i].data();
        r->items[i].cap = want;
    }
    fnx::png_prepare_many(ptrs.data(), sizes.data(), m, workers, r->items.data());
}

int main(int argc, char **argv)
{
    if (argc < 2) { std::fprintf(stderr, "usage: %s file...\n", argv[0]); return 2; }
    std::vector<std::vector<uint8_t>> files;
    for (int a = 1; a < argc; a++) {
        FILE *fp = std::fopen(argv[a], "rb");
        if (!fp) { std::perror(argv[a]); return 2; }
        std::vector<uint8_t> g;
        uint8_t buf[65536];
        size_t k;
        while ((k = std::fread(buf, 1, sizeof buf, fp)) > 0) g.insert(g.end(), buf, buf + k);
        std::fclose(fp);
        files.push_back(g);
    }
    const int m = static_cast<int>(files.size());
    if (fnx::png_workers(0, 40) != 8 || fnx::png_workers(0, 3) != 3 || fnx::png_workers(16, 5) != 5 || fnx::png_workers(1, 9) != 1) {
        std::fprintf(stderr, "png_workers: 0 is min(8, files), and never more threads than files\n");
        return 1;
    }
    Run base;
    prepare(files, 1, &base);
    int ok = 0, unsupported = 0, invalid = 0;
    for (const fnx::PngPrepared &it : base.items) {
        if (it.status == FNX_OK) ok++;
        else if (it.status == FNX_ERR_UNSUPPORTED) unsupported++;
        else invalid++;
        if ((it.status == FNX_OK) != (it.what == nullptr)) { std::fprintf(stderr, "a refusal carries its text, a pass none\n"); return 1; }
    }
    const int counts[] = {3, 8, 0, 3, 8};
    for (int workers : counts) {
        Run r;
        prepare(files, workers, &r);
        for (int i = 0; i < m; i++) {
            const fnx::PngPrepared &a = base.items[i], &b = r.items[i];
            bool same = a.status == b.status && a.want == b.want && a.units == b.units && std::memcmp(a.table, b.table, sizeof a.table) == 0;
            same = same && ((a.what == nullptr) == (b.what == nullptr)) && (a.what == nullptr || std::strcmp(a.what, b.what) == 0);
            if (same && a.status == FNX_OK)
                same = a.f.w == b.f.w && a.f.h == b.f.h && a.f.bpp == b.f.bpp && base.streams[i] == r.streams[i];
            if (!same) {
                std::fprintf(stderr, "%s: workers = %d differs from workers = 1 (status %d / %d)\n", argv[1 + i], workers, b.status, a.status);
                return 1;
            }
        }
    }
    std::printf("png_batch_host: %d files: %d prepared, %d unsupported, %d invalid; workers 1, 3, 8 and 0 agree; no sanitizer report\n", m, ok,
                unsupported, invalid);
    return 0;
}
