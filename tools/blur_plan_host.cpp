// GaussianBlur's host plan (fennec_amd/csrc/blur_plan.cpp) as a stand-alone program: which kernel a call gets, and whether it
// has a one-pass blur + SSIMFast form.  Built from this file and blur_plan.cpp alone (tests/test_blur_plan.py: g++ with
// AddressSanitizer and UndefinedBehaviorSanitizer); no HIP, no GPU.
// stdin, one case per line:  num_cus n w h exact dstW dstH radius  and the 2 radius + 1 weights (hex floats are read exactly)
// stdout, one line per case:
//   plain FAMILY nkh=. R=. tall=. guard=. wdp=. seg=. gq=. route=NAME | scored matrix|direct seg=. nbx=. nby=. tall=. route=NAME | tab=CRC geom=CRC
// with "none" for the second field where the call has no one-pass form (matrix / direct: whose tile the geometry is); tab: the matrix kernels' device table, geom: the one-pass
// form's table blob (0: there is none).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "blur_plan.hpp"

using namespace fnx;

static uint32_t crc32(const void *data, size_t bytes)
{
    static uint32_t table[256];
    if (!table[1])
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c >> 1) ^ (0xedb88320u & (0u - (c & 1u)));
            table[i] = c;
        }
    uint32_t c = 0xffffffffu;
    const unsigned char *p = static_cast<const unsigned char *>(data);
    for (size_t i = 0; i < bytes; i++) c = table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return ~c;
}

static const char *const FAMILY[] = {"mfma", "mfma_wide", "direct", "exact", "generic_f32", "generic_f64"};

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty() || line[0] == '#') continue;
        std::istringstream in(line);
        int num_cus, n, w, h, exact, dstW, dstH, radius;
        if (!(in >> num_cus >> n >> w >> h >> exact >> dstW >> dstH >> radius) || radius < 0 || radius > 4096) {
            std::fprintf(stderr, "bad case: %s\n", line.c_str());
            return 2;
        }
        std::vector<double> kernel(2 * radius + 1);
        for (double &v : kernel) {
            std::string tok;
            if (!(in >> tok)) { std::fprintf(stderr, "too few weights: %s\n", line.c_str()); return 2; }
            v = std::strtod(tok.c_str(), nullptr);
        }
        const BlurPlan p = plan_blur(num_cus, n, w, h, kernel.data(), radius, exact != 0);
        const bool matrix = p.family == BLUR_MFMA || p.family == BLUR_MFMA_WIDE;
        std::printf("plain %s nkh=%d R=%d tall=%d guard=%d wdp=%d seg=%d gq=%lld route=%s | ", FAMILY[p.family], p.nkh, radius,
                    p.family == BLUR_DIRECT && p.tall, (matrix || p.family == BLUR_DIRECT) && p.exact, p.wdp, matrix ? p.seg : 0,
                    matrix ? p.gq : 0LL, blur_route(p, false));
        uint32_t tab_crc = 0, geom_crc = 0;
        if (matrix) {
            const std::vector<uint32_t> tab = mfma_table(p, kernel.data());
            tab_crc = crc32(tab.data(), sizeof(uint32_t) * tab.size());
        }
        ScoreGeom g;               // a fresh cache per case: nothing carries over from the case before
        if (plan_blur_scored(p, dstW, dstH, g)) {
            std::printf("scored %s seg=%d nbx=%d nby=%d tall=%d route=%s | ", g.mfma ? "matrix" : "direct", g.th, g.nbx, g.nby, !g.mfma && g.tall,
                        blur_route(p, true));
            geom_crc = crc32(g.map.data(), sizeof(int32_t) * g.map.size());
        } else {
            std::printf("none | ");
        }
        std::printf("tab=%08x geom=%08x\n", tab_crc, geom_crc);
    }
    return 0;
}
