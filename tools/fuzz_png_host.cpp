// ASan + UBSan over the file of the PNG decoder that reads untrusted bytes on the host (png_parse.cpp: chunk walk, inflate,
// filter bytes, palette table), without a GPU and without the rest of the library: every file given on the command line goes
// through what fnx_png_decode does before its first launch -- as it is, in every truncation, and under `iters` mutations each.
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include \
//       -Ifennec_amd/csrc tools/fuzz_png_host.cpp fennec_amd/csrc/png_parse.cpp -o /tmp/fuzz_png_host
//   /tmp/fuzz_png_host 20000 file1.png file2.png ...        (tools/fuzz_png_host.sh writes the files and runs it)
// A third of the mutations are plain byte damage (they die at the first CRC: the chunk walk's bounds); a third repair the
// CRCs afterwards, so that the damage reaches the header rules, the inflater and the filter bytes; a third replace the IDAT
// stream by stored blocks around a mutated copy of the inflated rows, so that any filter byte and any size gets through.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>
#include "common.hpp"

namespace fnx {
void set_error(const char *, ...) {}
}  // namespace fnx

static long n_ok = 0, n_unsupported = 0, n_invalid = 0, n_skipped = 0;

static void one(const std::vector<uint8_t> &d)
{
    // the pure entry points on the raw bytes first: any input, any capacity
    {
        uint8_t small[97];
        size_t nb = 0;
        fnx_inflate(d.data(), d.size(), small, sizeof small, &nb);
        if (nb > sizeof small + 1) std::abort();                          // cap + 1 says "cap is too small"
        int w, h, ct, bd, il;
        fnx_png_info(d.data(), d.size(), &w, &h, &ct, &bd, &il);
    }
    fnx::PngFile f;
    int rc = fnx::png_parse(d.data(), d.size(), &f);
    if (rc == 0) {
        size_t want = 0, got = 0;
        rc = fnx::png_stream_size(f, &want);                               // bounds the memory by the file's own size, as in the library
        if (rc == 0 && want > (size_t(1) << 26)) { n_skipped++; return; }
        std::vector<uint8_t> stream(rc == 0 && want ? want : 1);
        if (rc == 0) rc = fnx::png_inflate(f.idat.data(), f.idat.size(), stream.data(), want, &got);
        if (got > want + 1) std::abort();
        if (rc == 0 && got != want) rc = FNX_ERR_INVALID;
        if (rc == 0) {
            std::vector<uint32_t> units;
            rc = fnx::png_row_plan(stream.data(), f, &units);
            if (rc == 0) {
                // the plan covers the rows once, in order, and cuts only where a row does not read the one above
                uint32_t at = 0;
                for (size_t u = 0; u + 1 < units.size(); u += 2) {
                    if (units[u] != at || units[u + 1] <= units[u]) std::abort();
                    if (u && stream[static_cast<size_t>(units[u]) * (1 + f.rowbytes)] > 1) std::abort();
                    at = units[u + 1];
                }
                if (at != static_cast<uint32_t>(f.h)) std::abort();
                uint32_t table[256];
                if (f.color_type == 3) fnx::png_palette_table(f, table);
            }
        }
    }
    if (rc == 0) n_ok++; else if (rc == FNX_ERR_UNSUPPORTED) n_unsupported++; else n_invalid++;
}

static uint32_t crc_of(const uint8_t *p, size_t n)
{
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; i++) {
        c ^= p[i];
        for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
    }
    return ~c;
}

static void put32(uint8_t *p, uint32_t v) { p[0] = v >> 24; p[1] = v >> 16; p[2] = v >> 8; p[3] = v; }

// every chunk whose length field still fits the file gets the CRC of its present bytes
static void repair_crcs(std::vector<uint8_t> &c)
{
    size_t pos = 8;
    while (pos + 12 <= c.size()) {
        const uint32_t len = (uint32_t(c[pos]) << 24) | (uint32_t(c[pos + 1]) << 16) | (uint32_t(c[pos + 2]) << 8) | c[pos + 3];
        if (len > c.size() - pos - 12) break;
        put32(&c[pos + 8 + len], crc_of(&c[pos + 4], 4 + size_t(len)));
        pos += 12 + size_t(len);
    }
}

static void append_chunk(std::vector<uint8_t> &c, const char *tag, const std::vector<uint8_t> &body)
{
    const size_t at = c.size();
    c.resize(at + 12 + body.size());
    put32(&c[at], static_cast<uint32_t>(body.size()));
    std::memcpy(&c[at + 4], tag, 4);
    if (!body.empty()) std::memcpy(&c[at + 8], body.data(), body.size());
    put32(&c[at + 8 + body.size()], crc_of(&c[at + 4], 4 + body.size()));
}

// the file's head (everything in front of its first IDAT) + one IDAT of stored blocks around `raw` + IEND
static std::vector<uint8_t> with_stream(const std::vector<uint8_t> &g, const std::vector<uint8_t> &raw)
{
    size_t pos = 8;
    while (pos + 12 <= g.size() && std::memcmp(&g[pos + 4], "IDAT", 4) != 0) {
        const uint32_t len = (uint32_t(g[pos]) << 24) | (uint32_t(g[pos + 1]) << 16) | (uint32_t(g[pos + 2]) << 8) | g[pos + 3];
        if (len > g.size() - pos - 12) break;
        pos += 12 + size_t(len);
    }
    std::vector<uint8_t> c(g.begin(), g.begin() + pos), z = {0x78, 0x01};
    size_t at = 0;
    do {
        const size_t k = raw.size() - at < 65535 ? raw.size() - at : 65535;
        const uint8_t hdr[5] = {static_cast<uint8_t>(at + k == raw.size()), static_cast<uint8_t>(k), static_cast<uint8_t>(k >> 8),
                                static_cast<uint8_t>(~k), static_cast<uint8_t>(~k >> 8)};
        z.insert(z.end(), hdr, hdr + 5);
        z.insert(z.end(), raw.begin() + at, raw.begin() + at + k);
        at += k;
    } while (at < raw.size());
    uint32_t a = 1, b = 0;
    for (uint8_t v : raw) { a = (a + v) % 65521u; b = (b + a) % 65521u; }
    const uint8_t ad[4] = {static_cast<uint8_t>(b >> 8), static_cast<uint8_t>(b), static_cast<uint8_t>(a >> 8), static_cast<uint8_t>(a)};
    z.insert(z.end(), ad, ad + 4);
    append_chunk(c, "IDAT", z);
    append_chunk(c, "IEND", {});
    return c;
}

int main(int argc, char **argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s iters file...\n", argv[0]); return 2; }
    const long iters = std::atol(argv[1]);
    std::mt19937_64 rng(12345);
    for (int a = 2; a < argc; a++) {
        FILE *fp = std::fopen(argv[a], "rb");
        if (!fp) { std::perror(argv[a]); return 2; }
        std::vector<uint8_t> g;
        uint8_t buf[65536];
        size_t k;
        while ((k = std::fread(buf, 1, sizeof buf, fp)) > 0) g.insert(g.end(), buf, buf + k);
        std::fclose(fp);
        if (g.size() < 60) { std::fprintf(stderr, "%s: too short to be a seed\n", argv[a]); return 2; }
        const long ok_before = n_ok;
        one(g);
        if (n_ok != ok_before + 1) { std::fprintf(stderr, "%s: the seed itself is refused\n", argv[a]); return 3; }
        // the seed's inflated rows, for the mutations that rewrite the stream
        fnx::PngFile f;
        fnx::png_parse(g.data(), g.size(), &f);
        std::vector<uint8_t> rows(static_cast<size_t>(f.h) * (1 + f.rowbytes));
        size_t got = 0;
        fnx::png_inflate(f.idat.data(), f.idat.size(), rows.data(), rows.size(), &got);
        for (size_t cut = 0; cut < g.size(); cut += (cut < 700 ? 1 : 13)) one(std::vector<uint8_t>(g.begin(), g.begin() + cut));
        for (long it = 0; it < iters; it++) {
            std::vector<uint8_t> c;
            if (it % 3 == 2) {
                std::vector<uint8_t> r = rows;
                const int nm = static_cast<int>(rng() % 4);
                for (int m = 0; m < nm; m++) {
                    const size_t at = rng() % r.size();
                    r[at] = (rng() & 1) ? static_cast<uint8_t>(rng() % 7) : static_cast<uint8_t>(rng());
                }
                if (rng() % 6 == 0) r.resize(rng() % (r.size() + 40));          // not enough / too much pixel data
                c = with_stream(g, r);
            } else {
                c = g;
            }
            const int nm = it % 3 == 2 ? static_cast<int>(rng() % 2) : 1 + static_cast<int>(rng() % 4);
            for (int m = 0; m < nm; m++) {
                const size_t at = 8 + rng() % (c.size() - 8);
                switch (rng() % 4) {
                case 0: c[at] = static_cast<uint8_t>(rng()); break;
                case 1: c[at] = 0xff; break;
                case 2: c[at] ^= static_cast<uint8_t>(1u << (rng() % 8)); break;
                default: c[at] = 0; break;
                }
            }
            if (it % 3 >= 1) repair_crcs(c);
            one(c);
        }
    }
    std::printf("fuzz_png_host: %ld decoded, %ld unsupported, %ld invalid, %ld skipped for their size; no sanitizer report\n", n_ok, n_unsupported,
                n_invalid, n_skipped);
    return 0;
}
