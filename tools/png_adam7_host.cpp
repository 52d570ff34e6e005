// The host side of an Adam7 decode (png_parse.cpp: parse with the accept flag, png_stream_size, png_inflate, the per-pass row
// plan) without a GPU and without the rest of the library, to be built under the address and undefined-behaviour sanitizers:
//   g++ -O1 -g -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -Ifennec_amd/csrc tools/png_adam7_host.cpp fennec_amd/csrc/png_parse.cpp -o /tmp/png_adam7_host
//   /tmp/png_adam7_host file... [--off file...]      the files behind --off are parsed with the accept flag off
// Every stream gets exactly the bytes its header promises (so a byte too many is a report).  Per file one line:
//   <status> <stream bytes> <units of pass 1> ... <units of pass 7>        (zeros behind a status other than 0)
// and the same files once more through png_prepare_many on three threads, which must agree.  A unit must lie inside its pass
// and the units of a pass must tile its rows.  tests/test_png_adam7_host.py writes the files and checks the lines.
#include <cstdio>
#include <cstring>
#include <vector>
#include "common.hpp"

namespace fnx {
void set_error(const char *, ...) {}
}  // namespace fnx

struct Answer {
    int status = 0;
    size_t want = 0;
    int units[7] = {0, 0, 0, 0, 0, 0, 0};
    bool operator==(const Answer &o) const { return status == o.status && want == o.want && std::memcmp(units, o.units, sizeof units) == 0; }
};

// the units of a planned file per pass; false where they do not tile the passes' rows
static bool count_units(const fnx::PngFile &f, const std::vector<uint32_t> &units, const std::vector<uint8_t> &passes, Answer *a)
{
    if (passes.size() * 2 != units.size()) return false;
    uint32_t next[7] = {0, 0, 0, 0, 0, 0, 0};
    for (size_t u = 0; u < passes.size(); u++) {
        const int p = passes[u];
        if (p > 6 || (u && passes[u - 1] > p)) return false;
        if (units[2 * u] != next[p] || units[2 * u + 1] <= units[2 * u] || units[2 * u + 1] > static_cast<uint32_t>(f.ph[p])) return false;
        next[p] = units[2 * u + 1];
        a->units[p]++;
    }
    for (int p = 0; p < 7; p++) {
        if (next[p] != static_cast<uint32_t>(f.ph[p])) return false;
    }
    return true;
}

static int one_file(const std::vector<uint8_t> &g, bool accept, Answer *a)
{
    static const uint8_t none = 0;
    const uint8_t *data = g.empty() ? &none : g.data();
    fnx::PngFile f;
    int rc = fnx::png_parse(data, g.size(), &f, accept);
    if (rc == FNX_OK) rc = fnx::png_stream_size(f, &a->want);
    if (rc == FNX_OK) {
        std::vector<uint8_t> stream(a->want);
        size_t got = 0;
        rc = fnx::png_inflate(f.idat.data(), f.idat.size(), stream.data(), a->want, &got);
        if (rc == FNX_OK && got != a->want) rc = FNX_ERR_INVALID;
        if (rc == FNX_OK) {
            std::vector<uint32_t> units;
            std::vector<uint8_t> passes;
            rc = fnx::png_row_plan(stream.data(), f, &units, &passes);
            if (rc == FNX_OK && f.interlace == 1 && !count_units(f, units, passes, a)) return -100;
        }
    }
    a->status = rc;
    if (rc != FNX_OK) {
        a->want = 0;
        std::memset(a->units, 0, sizeof a->units);
    }
    return 0;
}

int main(int argc, char **argv)
{
    std::vector<std::vector<uint8_t>> files;
    std::vector<char> accept;
    std::vector<const char *> names;
    bool on = true;
    for (int k = 1; k < argc; k++) {
        if (std::strcmp(argv[k], "--off") == 0) { on = false; continue; }
        FILE *fp = std::fopen(argv[k], "rb");
        if (!fp) { std::perror(argv[k]); return 2; }
        std::vector<uint8_t> g;
        uint8_t buf[65536];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, fp)) > 0) g.insert(g.end(), buf, buf + n);
        std::fclose(fp);
        files.push_back(g);
        accept.push_back(on);
        names.push_back(argv[k]);
    }
    if (files.empty()) { std::fprintf(stderr, "usage: %s file... [--off file...]\n", argv[0]); return 2; }
    const int m = static_cast<int>(files.size());
    std::vector<Answer> answers(m);
    for (int i = 0; i < m; i++) {
        if (one_file(files[i], accept[i] != 0, &answers[i]) != 0) {
            std::fprintf(stderr, "%s: the units do not tile the passes\n", names[i]);
            return 1;
        }
    }
    // the batch's workers: the accepted files on three threads
    std::vector<const uint8_t *> ptrs;
    std::vector<size_t> sizes;
    std::vector<int> which;
    static const uint8_t none = 0;
    for (int i = 0; i < m; i++) {
        if (!accept[i]) continue;
        ptrs.push_back(files[i].empty() ? &none : files[i].data());
        sizes.push_back(files[i].size());
        which.push_back(i);
    }
    const int k = static_cast<int>(ptrs.size());
    std::vector<fnx::PngPrepared> items(k);
    std::vector<std::vector<uint8_t>> streams(k);
    for (int j = 0; j < k; j++) {
        fnx::PngFile head;
        if (fnx::png_probe(ptrs[j], sizes[j], &head, true) != FNX_OK) continue;
        const size_t want = fnx::png_stream_bytes(head);
        if (want / 1032 > sizes[j]) continue;
        streams[j].assign(want, 0xee);
        items[j].stream = streams[j].data();
        items[j].cap = want;
    }
    if (k) fnx::png_prepare_many(ptrs.data(), sizes.data(), k, 3, items.data(), true);
    for (int j = 0; j < k; j++) {
        Answer b;
        b.status = items[j].status;
        if (b.status == FNX_OK) {
            b.want = items[j].want;
            if (items[j].f.interlace == 1 && !count_units(items[j].f, items[j].units, items[j].unit_pass, &b)) b.status = -100;
        }
        if (!(b == answers[which[j]])) {
            std::fprintf(stderr, "%s: png_prepare_many differs from the single path (status %d / %d)\n", names[which[j]], b.status,
                         answers[which[j]].status);
            return 1;
        }
    }
    for (int i = 0; i < m; i++) {
        const Answer &a = answers[i];
        std::printf("%d %zu %d %d %d %d %d %d %d\n", a.status, a.want, a.units[0], a.units[1], a.units[2], a.units[3], a.units[4], a.units[5],
                    a.units[6]);
    }
    std::printf("png_adam7_host: %d files; no sanitizer report\n", m);
    return 0;
}
