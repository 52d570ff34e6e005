// median_cut_split.inc on the CPU: median_cut_hostsim W H LEVEL [LEVEL ...] < rgba-bytes reads the 4 W H bytes of a tight NRGBA
// image from standard input, takes fnx_median_cut's samples of it (targetsize.go:352-373: every step-th flat 4-byte group),
// runs the kernel's workgroup as a loop over its 1024 lanes, phase by phase, and prints per level one line
//   <level> <ncolors> <ncolors entries of 8 hex digits r g b a>
// The sample buffers are exactly as long as the library allocates them, so that a sanitizer build sees every access the
// kernel would make past them.  Exit status 2 for bad arguments or a short input.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#define MC_FN static inline
#define MC_PHASE(call)                                  \
    for (int tid = 0; tid < MC_LANES; tid++) {          \
        McLane &ln = lanes[tid];                        \
        (void)ln;                                       \
        call;                                           \
    }
#define MC_ATOMIC_ADD(p, v) (*(p) += (v))
#define MC_ATOMIC_MAX64(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define MC_LOAD4(p) mc_load4(p)
#define MC_UNIFORM(x) (x)
#define MC_RUN_PARAMS , McLane *lanes

struct McVec4;
static inline McVec4 mc_load4(const uint32_t *p);
#include "median_cut_split.inc"

static inline McVec4 mc_load4(const uint32_t *p)
{
    if (reinterpret_cast<uintptr_t>(p) & 15u) { std::fprintf(stderr, "median_cut_hostsim: a 16-byte load at %p\n", static_cast<const void *>(p)); std::abort(); }
    McVec4 v;
    std::memcpy(&v, p, sizeof v);
    return v;
}

int main(int argc, char **argv)
{
    if (argc < 4) { std::fprintf(stderr, "usage: median_cut_hostsim W H LEVEL [LEVEL ...] < rgba-bytes\n"); return 2; }
    const long long w = std::atoll(argv[1]), h = std::atoll(argv[2]);
    if (w < 1 || h < 1 || w > 65535 || h > 65535) { std::fprintf(stderr, "median_cut_hostsim: W and H are 1 .. 65535\n"); return 2; }
    McArgs a{};
    std::vector<int> levels;
    for (int i = 3; i < argc; i++) {
        const int c = std::atoi(argv[i]);
        if (c < 1 || c > 256 || (!levels.empty() && c <= levels.back())) { std::fprintf(stderr, "median_cut_hostsim: levels ascend within 1 .. 256\n"); return 2; }
        levels.push_back(c);
        a.level_mask[(c - 1) >> 5] |= 1u << ((c - 1) & 31);
    }
    a.nlevels = static_cast<uint32_t>(levels.size());
    const long long n = w * h;
    std::vector<uint8_t> pix(static_cast<size_t>(4 * n));
    if (std::fread(pix.data(), 1, pix.size(), stdin) != pix.size()) { std::fprintf(stderr, "median_cut_hostsim: standard input is shorter than 4 W H bytes\n"); return 2; }

    const long long step = n > 100000 ? n / 100000 : 1;
    const long long ns = (n + step - 1) / step;
    if (ns > MC_MAX_SAMPLES) { std::fprintf(stderr, "median_cut_hostsim: %lld samples\n", ns); return 2; }
    const size_t cap = ((static_cast<size_t>(ns) + 3) & ~size_t(3)) + 4;
    for (int k = 0; k < 2; k++) {
        a.buf[k] = static_cast<uint32_t *>(std::aligned_alloc(16, cap * sizeof(uint32_t)));
        if (!a.buf[k]) return 2;
        std::memset(a.buf[k], 0xA5, cap * sizeof(uint32_t));
    }
    for (long long j = 0; j < ns; j++) {
        const uint8_t *p = pix.data() + 4 * j * step;
        a.buf[0][j] = p[0] | (p[1] << 8) | (static_cast<uint32_t>(p[2]) << 16);
    }
    a.n = static_cast<uint32_t>(ns);
    std::vector<uint32_t> out(static_cast<size_t>(a.nlevels) * 257, 0u);
    a.out = out.data();

    McShared *s = new McShared;
    std::memset(s, 0xA5, sizeof *s);
    std::vector<McLane> lanes(MC_LANES);
    mc_run(a, *s, lanes.data());

    for (uint32_t l = 0; l < a.nlevels; l++) {
        const uint32_t nc = out[a.nlevels * 256u + l];
        std::printf("%d %u", levels[l], nc);
        for (uint32_t i = 0; i < nc; i++) {
            const uint32_t e = out[l * 256u + i];
            std::printf(" %02x%02x%02x%02x", e & 255u, (e >> 8) & 255u, (e >> 16) & 255u, e >> 24);
        }
        std::printf("\n");
    }
    delete s;
    std::free(a.buf[0]);
    std::free(a.buf[1]);
    return 0;
}
