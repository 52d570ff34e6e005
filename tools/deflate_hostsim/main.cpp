// deflate.hip's two kernels on the CPU, lanes as threads: deflate_hostsim IN OUT [row [src_offset [dst_offset [TOKENS]]]] reads
// the file IN, runs launch_deflate over its bytes and writes the zlib stream to OUT; TOKENS takes the parse as the kernel left
// it in its scratch, per chunk a count and that many token words (a chunk that took the stored form has its parse there too).
// The source and the destination are placed src_offset / dst_offset bytes behind a 16-byte boundary (the kernels take other
// branches when they are not dword aligned); the destination is exactly as long as the stream's bound and is fenced by 64
// sentinel bytes either side.
// Built by the Makefile beside it from a COPY of fennec_amd/csrc/deflate.hip against the stand-in common.hpp / devutil.hpp of
// this directory; meant for sanitizer builds (-fsanitize=address,undefined) and for reading a stream without a GPU.
#include "deflate_hip.inc"

#include <cstdio>
#include <cstring>

static int fail(const char *what)
{
    fprintf(stderr, "deflate_hostsim: %s\n", what);
    return 1;
}

int main(int argc, char **argv)
{
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
    for (void *p : ctx.slot) free(p);
    free(src);
    free(dst);
    return 0;
}
