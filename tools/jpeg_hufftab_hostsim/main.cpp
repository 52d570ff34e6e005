// jpeg_hufftab.inc on the CPU: the text jpeg.hip's jpeg_hufftab_kernel includes, with the wave's 64 lanes as a loop.
//   jpeg_hufftab_hostsim <file>
// reads one histogram per line -- <name> <class 0..3> <256 counts> (class: 0 luminance DC, 1 luminance AC, 2 chrominance DC,
// 3 chrominance AC; it only chooses the standard table a code size above 32 falls back to) -- and prints per histogram
//   <name> standard=<0|1> nvals=<n>
//   bits <16 counts>
//   vals <n values>
//   lut <256 words, hexadecimal>
// Exit status 1 on a line it cannot read or a histogram that is all zero.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

namespace {

#include "jpeg_huffman_std.inc"

#define HT_FN static inline
#define HT_UNROLL
#define HT_PHASE(call)                                  \
    for (int lane = 0; lane < HT_LANES; lane++) {       \
        HtLane &ln = lanes[lane];                       \
        (void)ln;                                       \
        call;                                           \
    }
#define HT_MIN2 ht_all_min2(lanes)
#define HT_LANE0(field) lanes[0].field
#define HT_ATOMIC_ADD(p, v) (*(p) += (v))
#define HT_ATOMIC_OR(p, v) (*(p) |= (v))
#define HT_RUN_PARAMS , HtLane *lanes

struct HtLane;
void ht_all_min2(HtLane *lanes);

#include "jpeg_hufftab.inc"

// every lane's (k1, k2) become the two smallest keys of all lanes' (a lane's own two are distinct or "none")
void ht_all_min2(HtLane *lanes)
{
    unsigned long long k1 = HT_NOKEY, k2 = HT_NOKEY;
    for (int l = 0; l < HT_LANES; l++)
        for (unsigned long long key : {lanes[l].k1, lanes[l].k2}) {
            if (key < k1) { k2 = k1; k1 = key; }
            else if (key < k2) k2 = key;
        }
    for (int l = 0; l < HT_LANES; l++) { lanes[l].k1 = k1; lanes[l].k2 = k2; }
}

// the standard table of a class as the kernel's host side prepares it: look-up words and record
void standard(int t, uint32_t *lut, uint32_t *rec)
{
    std::memset(lut, 0, sizeof(uint32_t) * 256);
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int j = 0; j < HCOUNT[t][len - 1]; j++) lut[HVAL[t][k++]] = (static_cast<uint32_t>(len) << 24) | code++;
        code <<= 1;
    }
    std::memset(rec, 0, sizeof(uint32_t) * HT_REC_WORDS);
    rec[0] = static_cast<uint32_t>(HNVAL[t]);
    uint8_t *body = reinterpret_cast<uint8_t *>(rec + 2);
    std::memcpy(body, HCOUNT[t], 16);
    std::memcpy(body + 16, HVAL[t], static_cast<size_t>(HNVAL[t]));
}

}  // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        std::fprintf(stderr, "usage: jpeg_hufftab_hostsim <file of histograms>\n");
        return 1;
    }
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 1;
    }
    std::string line;
    std::vector<HtLane> lanes(HT_LANES);
    while (std::getline(in, line)) {
        if (line.empty()) continue;
        std::istringstream ls(line);
        std::string name;
        int cls = -1;
        std::vector<uint32_t> hist(256);
        ls >> name >> cls;
        bool any = false;
        for (auto &c : hist) {
            unsigned long long v = 0;
            ls >> v;
            c = static_cast<uint32_t>(v);
            any = any || c != 0;
        }
        if (!ls || cls < 0 || cls > 3 || !any) {
            std::fprintf(stderr, "bad line: %.60s\n", line.c_str());
            return 1;
        }
        std::vector<uint32_t> lut(256, 0xffffffffu), rec(HT_REC_WORDS, 0xffffffffu), std_lut(256), std_rec(HT_REC_WORDS);
        standard(cls, std_lut.data(), std_rec.data());
        HtShared s;
        std::memset(&s, 0xa5, sizeof(s));                  // nothing may be read before a phase wrote it
        std::memset(static_cast<void *>(lanes.data()), 0xa5, sizeof(HtLane) * lanes.size());
        ht_run(hist.data(), lut.data(), rec.data(), std_lut.data(), std_rec.data(), s, lanes.data());
        const uint8_t *body = reinterpret_cast<const uint8_t *>(rec.data() + 2);
        if (rec[0] < 1 || rec[0] > 256 || rec[1] > 1) {
            std::fprintf(stderr, "%s: no table (nvals %u, flag %u)\n", name.c_str(), rec[0], rec[1]);
            return 1;
        }
        std::printf("%s standard=%u nvals=%u\nbits", name.c_str(), rec[1], rec[0]);
        for (int i = 0; i < 16; i++) std::printf(" %u", body[i]);
        std::printf("\nvals");
        for (uint32_t i = 0; i < rec[0]; i++) std::printf(" %u", body[16 + i]);
        std::printf("\nlut");
        for (int i = 0; i < 256; i++) std::printf(" %x", lut[i]);
        std::printf("\n");
    }
    return 0;
}
