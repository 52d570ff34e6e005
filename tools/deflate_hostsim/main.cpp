// deflate.hip's two kernels on the CPU, lanes as threads: deflate_hostsim IN OUT [row [src_offset [dst_offset [TOKENS]]]] reads
// the file IN, runs launch_deflate over its bytes and writes the zlib stream to OUT; TOKENS takes the parse as the kernel left
// it in its scratch, per chunk a count and that many token words (a chunk that took the stored form has its parse there too).
// The source and the destination are placed src_offset / dst_offset bytes behind a 16-byte boundary (the kernels take other
// branches when they are not dword aligned); the destination is exactly as long as the stream's bound and is fenced by 64
// sentinel bytes either side.
// deflate_hostsim --batch ROW OUT IN1 IN2 ...: the batched kernels (launch_deflate_batch) over several inputs at once -- input
// i is laid i % 4 bytes behind a 16-byte boundary of one source area, its units and stream record are made as the PNG compress
// batch's planner makes them -- and stream i written to OUT.i.  The program checks that the streams lie back to back at their
// true sizes and that nothing behind the last one was written.
// Switches, anywhere on the line, that leave the other arguments' meaning as it is: --dense runs the dense level's kernels
// (FNX_DEFLATE_LEVEL_DENSE; TOKENS then holds the lazy walk's tokens); --table FILE (with --dense, single stream) writes the
// dense parse's per-position table beside them, per chunk its length and that many words L << 16 | D - 1 (0: no match).
// --size-only (single stream, with or without --dense): IN [row [src_offset]] alone; runs launch_deflate_size -- the chunk kernels'
// size-only forms and deflate_size_kernel -- and prints a line "chunk C BYTES" per chunk and "total BYTES"; the program checks that
// neither the slot area nor the output slot was asked for.
// Built by the Makefile beside it from a COPY of fennec_amd/csrc/deflate.hip against the stand-in common.hpp / devutil.hpp of
// this directory; meant for sanitizer builds (-fsanitize=address,undefined) and for reading a stream without a GPU.
#include "deflate_hip.inc"

#include <cstdio>
#include <cstring>
#include <string>

static int fail(const char *what)
{
    fprintf(stderr, "deflate_hostsim: %s\n", what);
    return 1;
}

static bool read_file(const char *name, std::vector<uint8_t> *out)
{
    FILE *f = fopen(name, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) out->insert(out->end(), buf, buf + k);
    fclose(f);
    return true;
}

static int g_level = FNX_DEFLATE_LEVEL_FAST;
static const char *g_table = nullptr;

static int size_only(int argc, char **argv)
{
    if (argc < 2) return fail("usage: deflate_hostsim --size-only IN [row [src_offset]]");
    const int row = argc > 2 ? atoi(argv[2]) : 0;
    const size_t soff = argc > 3 ? static_cast<size_t>(atoi(argv[3])) : 0;
    if (soff > 15) return fail("offsets are 0 .. 15");
    std::vector<uint8_t> in;
    if (!read_file(argv[1], &in) || in.empty()) return fail("cannot read IN, or it is empty");
    const size_t n = in.size();
    uint8_t *src = static_cast<uint8_t *>(aligned_alloc(16, (soff + n + 15) & ~size_t(15)));
    if (!src) return fail("out of memory");
    memcpy(src + soff, in.data(), n);
    fnx_ctx ctx{};
    ctx.deflate_level = g_level;
    const unsigned long long *size = nullptr;
    if (fnx::launch_deflate_size(&ctx, src + soff, n, row, &size) != FNX_OK) return fail("launch_deflate_size failed");
    if (ctx.slot[fnx::SLOT_DEFLATE_SLOTS] || ctx.slot[fnx::SLOT_DEFLATE_OUT]) return fail("the size-only form asked for the slot area or the output");
    const uint32_t *meta = reinterpret_cast<const uint32_t *>(static_cast<const uint8_t *>(ctx.slot[fnx::SLOT_DEFLATE_SIZE]) + 16);
    for (size_t c = 0; c < fnx::deflate_chunks(n); c++) printf("chunk %zu %u\n", c, meta[4 * c]);
    printf("total %llu\n", *size);
    for (void *p : ctx.slot) free(p);
    free(src);
    return 0;
}

static int batch(int argc, char **argv)
{
    if (argc < 5) return fail("usage: deflate_hostsim --batch ROW OUT IN1 [IN2 ...]");
    const int row = atoi(argv[2]);
    const int m = argc - 4;
    std::vector<std::vector<uint8_t>> in(m);
    std::vector<size_t> at(m);
    size_t area = 0, bounds = 0;
    for (int i = 0; i < m; i++) {
        if (!read_file(argv[4 + i], &in[i]) || in[i].empty()) return fail("cannot read an input, or it is empty");
        at[i] = ((area + 15) & ~size_t(15)) + static_cast<size_t>(i % 4);
        area = at[i] + in[i].size();
        bounds += fnx::deflate_bound(in[i].size());
    }
    uint8_t *src = static_cast<uint8_t *>(aligned_alloc(16, (area + 15) & ~size_t(15)));
    if (!src) return fail("out of memory");
    std::vector<fnx::DeflateBatchUnit> units;
    std::vector<fnx::DeflateBatchImage> images(m);
    for (int i = 0; i < m; i++) {
        memcpy(src + at[i], in[i].data(), in[i].size());
        const size_t n = in[i].size(), k = fnx::deflate_chunks(n);
        images[i] = fnx::DeflateBatchImage{n, static_cast<uint32_t>(units.size()), static_cast<uint32_t>(k)};
        for (size_t c = 0; c < k; c++) {
            const size_t off = c * fnx::DF_C;
            units.push_back(fnx::DeflateBatchUnit{src + at[i] + off, static_cast<uint32_t>(std::min<size_t>(fnx::DF_C, n - off)), fnx::deflate_row_hint(row),
                                                  c + 1 == k ? 1u : 0u, static_cast<uint32_t>(i)});
        }
    }
    fnx_ctx ctx{};
    ctx.deflate_level = g_level;
    const uint8_t *out = nullptr;
    const unsigned long long *sizes = nullptr;
    if (fnx::launch_deflate_batch(&ctx, units.data(), images.data(), static_cast<uint32_t>(units.size()), static_cast<uint32_t>(m), bounds, &out, &sizes) != FNX_OK)
        return fail("launch_deflate_batch failed");
    size_t off = 0;
    for (int i = 0; i < m; i++) {
        const size_t nb = static_cast<size_t>(sizes[i]);
        if (nb > fnx::deflate_bound(in[i].size()) || off + nb > bounds) return fail("a stream is longer than its bound");
        const std::string name = std::string(argv[3]) + "." + std::to_string(i);
        FILE *f = fopen(name.c_str(), "wb");
        if (!f || fwrite(out + off, 1, nb, f) != nb || fclose(f) != 0) return fail("cannot write a stream");
        off += nb;
    }
    for (void *p : ctx.slot) free(p);
    free(src);
    return 0;
}

int main(int argc, char **argv)
{
    int kept = 1;
    bool sizes = false;
    for (int i = 1; i < argc; i++) {
        if (strcmp(argv[i], "--dense") == 0) g_level = FNX_DEFLATE_LEVEL_DENSE;
        else if (strcmp(argv[i], "--size-only") == 0) sizes = true;
        else if (strcmp(argv[i], "--table") == 0 && i + 1 < argc) g_table = argv[++i];
        else argv[kept++] = argv[i];
    }
    argc = kept;
    const bool dense = g_level == FNX_DEFLATE_LEVEL_DENSE;
    if (g_table && !dense) return fail("--table goes with --dense");
    if (sizes && (g_table || (argc > 1 && strcmp(argv[1], "--batch") == 0))) return fail("--size-only goes with a single stream and no --table");
    if (sizes) return size_only(argc, argv);
    if (argc > 1 && strcmp(argv[1], "--batch") == 0) return batch(argc, argv);
    if (argc < 3) return fail("usage: deflate_hostsim IN OUT [row [src_offset [dst_offset [TOKENS]]]]");
    const int row = argc > 3 ? atoi(argv[3]) : 0;
    const size_t soff = argc > 4 ? static_cast<size_t>(atoi(argv[4])) : 0, doff = argc > 5 ? static_cast<size_t>(atoi(argv[5])) : 0;
    if (soff > 15 || doff > 15) return fail("offsets are 0 .. 15");
    FILE *f = fopen(argv[1], "rb");
    if (!f) return fail("cannot read IN");
    std::vector<uint8_t> in;
    uint8_t buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + k);
    fclose(f);
    const size_t n = in.size();
    if (!n) return fail("IN is empty");

    constexpr size_t FENCE = 64;
    const size_t cap = fnx::deflate_bound(n);
    uint8_t *src = static_cast<uint8_t *>(aligned_alloc(16, (soff + n + 15) & ~size_t(15)));
    uint8_t *dst = static_cast<uint8_t *>(aligned_alloc(16, (FENCE + doff + cap + FENCE + 15) & ~size_t(15)));
    if (!src || !dst) return fail("out of memory");
    memcpy(src + soff, in.data(), n);
    memset(dst, 0xA5, FENCE + doff + cap + FENCE);
    uint8_t *out = dst + FENCE + doff;

    fnx_ctx ctx{};
    ctx.deflate_level = g_level;
    const unsigned long long *size = nullptr;
    if (fnx::launch_deflate(&ctx, src + soff, n, row, out, cap, &size) != FNX_OK) return fail("launch_deflate failed");
    const size_t nb = static_cast<size_t>(*size);
    if (nb > cap) return fail("the stream is longer than deflate_bound");
    for (size_t i = 0; i < FENCE + doff; i++) if (dst[i] != 0xA5) return fail("bytes in front of the stream were written");
    for (size_t i = 0; i < FENCE; i++) if (out[nb + i] != 0xA5) return fail("bytes behind the stream were written");
    f = fopen(argv[2], "wb");
    if (!f || fwrite(out, 1, nb, f) != nb || fclose(f) != 0) return fail("cannot write OUT");
    if (argc > 6) {
        const uint32_t *tok = static_cast<const uint32_t *>(ctx.slot[fnx::SLOT_DEFLATE_TOK]);
        std::vector<uint32_t> words;
        for (size_t c = 0; c * fnx::DF_C < n; c++) {
            const size_t len = std::min<size_t>(fnx::DF_C, n - c * fnx::DF_C), first = words.size();
            words.push_back(0);
            if (dense) {                                              // a token belongs to the lane in whose sub-chunk it starts
                const uint32_t *ct = tok + c * fnx::DF_DENSE_WORDS;
                size_t lane = ~size_t(0), k = 0;
                for (size_t p = 0; p < len;) {
                    if (p / fnx::DF_S != lane) { lane = p / fnx::DF_S; k = 0; }
                    const uint32_t t = ct[lane * fnx::DF_S + k++];
                    words.push_back(t);
                    p += (t >> 31) ? ((t >> 16) & 0xffu) + 3 : 1;
                }
            } else
            for (size_t s0 = 0; s0 < len; s0 += fnx::DF_S) {          // a lane's tokens lie from its sub-chunk's first word on
                const uint32_t *t = tok + c * fnx::DF_C + s0;
                for (size_t p = s0, e = std::min<size_t>(s0 + fnx::DF_S, len); p < e; t++) {
                    words.push_back(*t);
                    p += (*t >> 31) ? ((*t >> 16) & 0xffu) + 3 : 1;
                }
            }
            words[first] = static_cast<uint32_t>(words.size() - first - 1);
        }
        f = fopen(argv[6], "wb");
        if (!f || fwrite(words.data(), 4, words.size(), f) != words.size() || fclose(f) != 0) return fail("cannot write TOKENS");
    }
    if (g_table) {
        const uint32_t *tok = static_cast<const uint32_t *>(ctx.slot[fnx::SLOT_DEFLATE_TOK]);
        std::vector<uint32_t> words;
        for (size_t c = 0; c * fnx::DF_C < n; c++) {
            const size_t len = std::min<size_t>(fnx::DF_C, n - c * fnx::DF_C);
            const uint32_t *tab = tok + c * fnx::DF_DENSE_WORDS + fnx::DF_C;
            words.push_back(static_cast<uint32_t>(len));
            words.insert(words.end(), tab, tab + len);
        }
        f = fopen(g_table, "wb");
        if (!f || fwrite(words.data(), 4, words.size(), f) != words.size() || fclose(f) != 0) return fail("cannot write the table");
    }
    for (void *p : ctx.slot) free(p);
    free(src);
    free(dst);
    return 0;
}
