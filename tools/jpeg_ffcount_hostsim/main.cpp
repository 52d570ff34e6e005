// jpeg_ffcount_strips.inc on the CPU: random block sequences as the strips, bit counts and positions jpeg_code_kernel and
// the scan would leave, the lane body run for every block, the sum against a plain pack-then-count written here on its own.
// One line per case on stdout:  <name> nblk=<n> bits=<b> ff=<lanes' sum> want=<packed count> last_ff=<0|1>
// Exit status 1 when a case disagrees.  No arguments.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

namespace {

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd()
{
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return static_cast<uint32_t>(g_rng >> 32);
}

using Block = std::vector<uint8_t>;      // one bit per element, in string order

Block block(int len, int ones_per_1024)
{
    Block b(static_cast<size_t>(len));
    for (auto &x : b) x = static_cast<int>(rnd() & 1023u) < ones_per_1024 ? 1 : 0;
    return b;
}

// the lanes' side: the arrays as the device holds them, unused strip words and the bits behind a block's end set to ones
// (a lane that reads them counts too many)
uint64_t by_lanes(const std::vector<Block> &blocks)
{
    const int nblk = static_cast<int>(blocks.size());
    size_t maxw = 1;
    for (const Block &b : blocks) maxw = std::max(maxw, (b.size() + 31) / 32);
    std::vector<uint32_t> strip_v(maxw * static_cast<size_t>(nblk), 0xffffffffu), nbits_v(static_cast<size_t>(nblk));
    std::vector<unsigned long long> pos_v(static_cast<size_t>(nblk));
    unsigned long long at = 0;
    for (int i = 0; i < nblk; i++) {
        const Block &b = blocks[static_cast<size_t>(i)];
        for (size_t k = 0; k < b.size(); k++)
            if (!b[k]) strip_v[(k / 32) * static_cast<size_t>(nblk) + static_cast<size_t>(i)] &= ~(0x80000000u >> (k % 32));
        nbits_v[static_cast<size_t>(i)] = static_cast<uint32_t>(b.size());
        pos_v[static_cast<size_t>(i)] = at;
        at += b.size();
    }
    const uint32_t *strip = strip_v.data(), *nbits = nbits_v.data();
    const unsigned long long *pos = pos_v.data();
    uint64_t total = 0;
    for (int blk = 0; blk < nblk; blk++) {
        uint32_t count = 0;
#include "jpeg_ffcount_strips.inc"
        total += count;
    }
    return total;
}

// the plain side: the string packed into bytes, the last one padded with ones, the 0xff bytes counted
uint64_t by_packing(const std::vector<Block> &blocks, uint64_t *bits, int *last_ff)
{
    std::vector<uint8_t> bytes;
    uint64_t n = 0;
    for (const Block &b : blocks)
        for (uint8_t x : b) {
            if (n % 8 == 0) bytes.push_back(0);
            if (x) bytes.back() = static_cast<uint8_t>(bytes.back() | (0x80u >> (n % 8)));
            n++;
        }
    if (n % 8) bytes.back() = static_cast<uint8_t>(bytes.back() | (0xffu >> (n % 8)));
    uint64_t ff = 0;
    for (uint8_t v : bytes) ff += v == 0xff;
    *bits = n;
    *last_ff = !bytes.empty() && bytes.back() == 0xff;
    return ff;
}

int g_bad = 0;

void run(const std::string &name, const std::vector<Block> &blocks)
{
    uint64_t bits = 0;
    int last_ff = 0;
    const uint64_t want = by_packing(blocks, &bits, &last_ff), got = by_lanes(blocks);
    std::printf("%s nblk=%zu bits=%llu ff=%llu want=%llu last_ff=%d\n", name.c_str(), blocks.size(), static_cast<unsigned long long>(bits),
                static_cast<unsigned long long>(got), static_cast<unsigned long long>(want), last_ff);
    if (got != want) g_bad++;
}

int length(int lo, int hi) { return lo + static_cast<int>(rnd() % static_cast<uint32_t>(hi - lo + 1)); }

// the last block grows or shrinks (within 4 .. 1600) until the string's length has the remainder `rem` modulo 8
void settle(std::vector<Block> &blocks, int rem, int ones)
{
    uint64_t n = 0;
    for (const Block &b : blocks) n += b.size();
    Block &l = blocks.back();
    while (static_cast<int>(n % 8) != rem) {
        if (l.size() < 1600) { l.push_back(static_cast<uint8_t>(static_cast<int>(rnd() & 1023u) < ones)); n++; }
        else { l.pop_back(); n--; rem = static_cast<int>(n % 8); }
    }
}

}  // namespace

int main()
{
    for (int seed = 0; seed < 6; seed++) {
        // lengths over the whole range, three densities of ones: fair bits, mostly ones (many 0xff, many straddling bytes), all ones
        const int ones = seed % 3 == 0 ? 512 : (seed % 3 == 1 ? 960 : 1024);
        std::vector<Block> v;
        const int nblk = 300 + 257 * seed;
        for (int i = 0; i < nblk; i++) v.push_back(block(i % 7 == 0 ? length(4, 1600) : length(4, 90), ones));
        run("random_" + std::to_string(seed), v);
    }
    for (int ones : {512, 1000, 1024}) {
        std::vector<Block> v;
        for (int i = 0; i < 777; i++) v.push_back(block(4, ones));
        run("run_of_4_bit_blocks_" + std::to_string(ones), v);
        v.clear();
        for (int i = 0; i < 600; i++) v.push_back(block(i % 3 == 0 ? 4 : length(4, 6), ones));   // bytes over three blocks and more
        run("short_blocks_" + std::to_string(ones), v);
    }
    for (int len : {4, 7, 8, 9, 31, 32, 33, 64, 1599, 1600})
        for (int ones : {512, 1024}) run("single_block_" + std::to_string(len) + "_" + std::to_string(ones), {block(len, ones)});
    for (int rem = 0; rem < 8; rem++) {
        // all-one value bits: every whole byte is 0xff; rem != 0: so is the padded last byte; rem == 0: no padding at all
        std::vector<Block> v;
        for (int i = 0; i < 64 + rem; i++) v.push_back(block(length(4, 200), 1024));
        settle(v, rem, 1024);
        run("all_ones_rem_" + std::to_string(rem), v);
        // fair bits in front, the string's end all ones
        v.clear();
        for (int i = 0; i < 50; i++) v.push_back(block(length(4, 300), 512));
        v.push_back(block(4, 1024));
        v.push_back(block(4, 1024));
        v.push_back(block(5, 1024));
        settle(v, rem, 1024);
        run("ones_at_the_end_rem_" + std::to_string(rem), v);
        // and the opposite: the string's last bit is a zero, so its last byte is not 0xff, padded or not
        v.back().back() = 0;
        run("zero_in_the_last_byte_rem_" + std::to_string(rem), v);
    }
    if (g_bad) std::fprintf(stderr, "%d case(s) disagree\n", g_bad);
    return g_bad ? 1 : 0;
}
