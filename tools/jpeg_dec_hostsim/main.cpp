// jpeg_dec.hip's span decoder (fennec_amd/csrc/jpeg_dec_span.inc, the text the kernels include) on the CPU, behind the real
// jpeg_parse and jpeg_unstuff of jpeg_parse.cpp: a stand-alone program for AddressSanitizer + UndefinedBehaviorSanitizer.
//   jpeg_dec_hostsim FILE [replay]
// 1. the file's segments and tables (jpeg_parse), the scan without its stuffing (jpeg_unstuff), both table forms
// 2. chain: dec_span<false, RST> lane after lane from the string's first bit, every lane starting where the one before it
//    ended -- the fixed point jpeg_dec.hip's header promises, reached the slow way; 256 spans staged at a time as dec_stage does
// 3. dec_span<true, RST> per lane from those states (dec_write_body's block numbering restated), into the coefficient array
// 4. `replay`: the device's pass structure run sequentially instead -- per group of 16 + 240 spans every lane starts from its
//    guess and corrections repeat until nothing changes, then rounds across groups (every group reads its predecessor's state
//    as the round found it) until a round changes nothing; its states must equal the chained ones (exit status 3 if not)
// stdout: one text line
//   route=device err=E blocks=B nblk=N nlanes=L nbits=T rst=R passes=P rounds=Q replay_ok=0|1
// then L x uint64 (every lane's start state, dec_state's packing) and N x 64 x int16 (natural order, DC as the difference),
// little endian.  A file the parser sends to the host's scans prints route=host and nothing else; one it refuses, route=refused rc=.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "common.hpp"

namespace fnx {
void set_error(const char *, ...) {}

#include "jpeg_dec_span.inc"

// dec_stage's loop for every lane of a workgroup: the 256 spans from span0 on + 3 words of look-ahead
static void stage(DecShared &sh, const DecArgs &a, long long span0, const void *tab, size_t tab_bytes)
{
    const long long base = span0 * DEC_WPT;
    for (int i = 0; i < DEC_WG_WORDS + 3; i++) {
        const long long w = base + i;
        sh.seg[i + i / DEC_WPT] = (w >= 0 && w < a.nwords) ? __builtin_bswap32(a.ecs[w]) : 0u;
    }
    std::memcpy(&sh.tab, tab, tab_bytes);
    std::memcpy(sh.unzig, c_unzig, 64);
}

template <bool RST>
static void sync_lane(const DecShared &sh, const DecArgs &a, unsigned long long in, long long wg_bit, int t, long long blk,
                      unsigned long long *out, uint32_t *cnt)
{
    uint32_t rel = static_cast<uint32_t>(static_cast<long long>(in & 0xffffffffffull) - wg_bit);
    int z = static_cast<int>((in >> 40) & 0xffu), slot = static_cast<int>(in >> 48);
    uint32_t bad = 0;
    *cnt = 0;
    dec_span<false, RST>(sh, a, rel, z, slot, static_cast<uint32_t>(t + 1) * DEC_SPAN, *cnt, blk, bad, wg_bit);
    *out = dec_state(static_cast<unsigned long long>(wg_bit + rel), z, slot);
}

// dec_write_body (jpeg_dec.hip) for lane gt of a single file
template <bool RST>
static void write_lane(const DecShared &sh, const DecArgs &a, int g, int t, uint32_t *err)
{
    const int gt = g * 256 + t;
    if (gt >= a.nlanes) return;
    const unsigned long long st = a.s_in[gt];
    long long blk = static_cast<long long>(a.first_blk[gt]);
    if (RST && a.nrst > 0) {
        const unsigned long long at = st & 0xffffffffffull;
        int lo_k = 0, hi_k = a.nrst;
        while (lo_k < hi_k) {
            const int mid = (lo_k + hi_k) >> 1;
            if (8ull * a.rst[mid] <= at) lo_k = mid + 1; else hi_k = mid;
        }
        const int j = lo_k - 1;
        if (j >= 0) {
            const unsigned long long rec = a.rst_rec[j];
            const long long before = static_cast<long long>(a.first_blk[rec >> 32]) + static_cast<long long>(rec & 0xffffffffull);
            blk = static_cast<long long>(j + 1) * a.ri_blocks + (blk - before);
        }
    }
    if (blk >= a.nblk) return;
    const unsigned long long wg_bit = static_cast<unsigned long long>(g) * 256u * DEC_SPAN;
    uint32_t rel = static_cast<uint32_t>((st & 0xffffffffffull) - wg_bit);
    int z = static_cast<int>((st >> 40) & 0xffu), slot = static_cast<int>(st >> 48);
    uint32_t cnt = 0, bad = 0;
    const unsigned long long left = a.nbits - wg_bit;
    dec_span<true, RST>(sh, a, rel, z, slot, static_cast<uint32_t>(t + 1) * DEC_SPAN, cnt, blk, bad, static_cast<long long>(wg_bit),
                        left > 0xfffffff0ull ? 0xfffffff0u : static_cast<uint32_t>(left));
    *err |= bad;
}

struct Run {
    DecArgs a;
    DecShared *sh;
    DecTables tab;
    DecSyncTables stab;
    std::vector<unsigned long long> s_in, s_out, first, rec;
    std::vector<uint32_t> cnt;
};

template <bool RST>
static void chain(Run &r)
{
    const DecArgs &a = r.a;
    unsigned long long prev = dec_state(0, 0, 0);
    for (int gs = 0; gs < a.nlanes; gs++) {
        const int g = gs / 256, t = gs % 256;
        if (t == 0) stage(*r.sh, a, static_cast<long long>(g) * 256, &r.stab, sizeof(DecSyncTables));
        r.s_in[gs] = prev;
        sync_lane<RST>(*r.sh, a, prev, static_cast<long long>(g) * 256 * DEC_SPAN, t, gs, &r.s_out[gs], &r.cnt[gs]);
        prev = r.s_out[gs];
    }
}

// dec_sync_body's passes for one group, lanes in turn: FIX = false from the guesses (span0 = g OWN - WARM, the warm-up lanes'
// results dropped), FIX = true from the stored states with lane 0 corrected to `prev`.  Returns the passes it took.
template <bool FIX, bool RST>
static uint32_t group(Run &r, int g, unsigned long long prev)
{
    const DecArgs &a = r.a;
    const long long span0 = static_cast<long long>(g) * DEC_OWN - (FIX ? 0 : DEC_WARM);
    const long long wg_bit = span0 * DEC_SPAN;
    unsigned long long my_in[256], my_out[256], out[256];
    uint32_t my_cnt[256];
    bool need[256], live[256];
    for (int t = 0; t < 256; t++) {
        const long long gs = span0 + t;
        live[t] = gs >= 0 && gs < a.nlanes && (!FIX || t < DEC_OWN);
        if (!FIX) {
            my_in[t] = dec_state(static_cast<unsigned long long>(live[t] ? gs : 0) * DEC_SPAN, 0, 0);
            my_out[t] = my_in[t];
            my_cnt[t] = 0;
            need[t] = live[t];
        } else {
            my_in[t] = live[t] ? r.s_in[gs] : 0;
            my_out[t] = live[t] ? r.s_out[gs] : 0;
            my_cnt[t] = live[t] ? r.cnt[gs] : 0;
            need[t] = t == 0;
            if (t == 0) my_in[t] = prev;
        }
        out[t] = my_out[t];
    }
    stage(*r.sh, a, span0, &r.stab, sizeof(DecSyncTables));
    uint32_t passes = 0;
    for (;;) {
        passes++;
        for (int t = 0; t < 256; t++)
            if (need[t]) {
                sync_lane<RST>(*r.sh, a, my_in[t], wg_bit, t, (FIX || t >= DEC_WARM) ? span0 + t : -1ll, &my_out[t], &my_cnt[t]);
            }
        for (int t = 0; t < 256; t++) out[t] = my_out[t];
        bool any = false;
        for (int t = 0; t < 256; t++) {
            need[t] = false;
            if (t > 0 && live[t] && span0 + t > 0 && out[t - 1] != my_in[t]) {
                my_in[t] = out[t - 1];
                need[t] = true;
                any = true;
            }
        }
        if (!any) break;
    }
    for (int t = 0; t < 256; t++)
        if (live[t] && (FIX || t >= DEC_WARM)) {
            r.s_in[span0 + t] = my_in[t];
            r.s_out[span0 + t] = my_out[t];
            r.cnt[span0 + t] = my_cnt[t];
        }
    return passes;
}

template <bool RST>
static void replay(Run &r, uint32_t *passes, int *rounds)
{
    const int nwg = (r.a.nlanes + DEC_OWN - 1) / DEC_OWN;
    *passes = 0;
    *rounds = 0;
    for (int g = 0; g < nwg; g++) {
        const uint32_t p = group<false, RST>(r, g, 0);
        if (p > *passes) *passes = p;
    }
    for (;;) {
        // a round's workgroups run side by side: each reads its predecessor's last state as the round before left it
        std::vector<unsigned long long> prev(static_cast<size_t>(nwg), 0);
        for (int g = 1; g < nwg; g++) prev[g] = r.s_out[static_cast<size_t>(g) * DEC_OWN - 1];
        bool changed = false;
        for (int g = 1; g < nwg; g++) {
            if (prev[g] == r.s_in[static_cast<size_t>(g) * DEC_OWN]) continue;
            const uint32_t p = group<true, RST>(r, g, prev[g]);
            if (p > *passes) *passes = p;
            changed = true;
        }
        ++*rounds;                                             // (the quiet round is launched too, as on the device)
        if (!changed) break;
    }
}

}  // namespace fnx

int main(int argc, char **argv)
{
    using namespace fnx;
    if (argc < 2) {
        std::fprintf(stderr, "usage: jpeg_dec_hostsim FILE [replay]\n");
        return 2;
    }
    const bool do_replay = argc > 2 && std::strcmp(argv[2], "replay") == 0;
    std::vector<uint8_t> data;
    {
        FILE *fp = std::fopen(argv[1], "rb");
        if (!fp) { std::perror(argv[1]); return 2; }
        uint8_t buf[65536];
        size_t k;
        while ((k = std::fread(buf, 1, sizeof(buf), fp)) > 0) data.insert(data.end(), buf, buf + k);
        std::fclose(fp);
    }
    static JpegFile f;
    int rc = jpeg_parse(data.data(), data.size(), &f);
    if (rc != 0) { std::printf("route=refused rc=%d\n", rc); return 0; }
    if (f.progressive) { std::printf("route=host\n"); return 0; }
    const size_t cap = (data.size() - f.scan + 64 + 63) & ~size_t(63);
    std::vector<uint8_t> ecs(cap + 64, 0);
    std::vector<uint32_t> rst;
    size_t nb = 0;
    rc = jpeg_unstuff(data.data(), data.size(), f, ecs.data(), &nb, &rst);
    if (rc != 0) { std::printf("route=refused rc=%d\n", rc); return 0; }
    const size_t nwords = (nb + 3) / 4 + 4;
    std::memset(ecs.data() + nb, 0, nwords * 4 - nb);
    const unsigned long long nbits = 8ull * nb;
    const long long nlanes_ll = static_cast<long long>((nbits + DEC_SPAN - 1) / DEC_SPAN);
    const long long nblk_ll = static_cast<long long>(f.mx) * f.my * f.nslots;
    if (nlanes_ll == 0 || nlanes_ll >= (1ll << 30) || nblk_ll >= (1ll << 30) || nbits < 2ull * static_cast<unsigned long long>(nblk_ll)) {
        std::printf("route=refused rc=%d\n", FNX_ERR_INVALID);                 // jpeg_decode_planes' refusals before anything is sized
        return 0;
    }
    const int nlanes = static_cast<int>(nlanes_ll), nblk = static_cast<int>(nblk_ll);
    std::vector<uint32_t> words(nwords);
    std::memcpy(words.data(), ecs.data(), nwords * 4);

    static Run r;
    static DecShared sh;
    r.sh = &sh;
    r.tab = f.tab;
    dec_sync_tables(f.tab, &r.stab);
    const size_t lanes_pad = (static_cast<size_t>(nlanes) + 2 * 256) & ~size_t(255);
    r.s_in.assign(lanes_pad, 0); r.s_out.assign(lanes_pad, 0); r.first.assign(lanes_pad + 1, 0); r.cnt.assign(lanes_pad, 0);
    r.rec.assign(rst.size() + 1, 0);
    std::vector<int16_t> coef(static_cast<size_t>(nblk) * 64, 0);
    uint32_t err = 0;
    DecArgs &a = r.a;
    a = DecArgs{};
    a.ecs = words.data(); a.tab = &r.tab; a.tab_sync = &r.stab; a.s_in = r.s_in.data(); a.s_out = r.s_out.data(); a.cnt = r.cnt.data();
    a.flag = nullptr; a.first_blk = r.first.data(); a.coef = coef.data(); a.err = &err; a.dbg = nullptr;
    a.nwords = static_cast<long long>(nwords); a.nbits = nbits; a.nlanes = nlanes; a.nblk = nblk; a.nslots = f.nslots;
    a.dcpack = f.dcpack; a.acpack = f.acpack;
    a.rst = rst.data(); a.nrst = static_cast<int>(rst.size()); a.ri_blocks = f.ri * f.nslots; a.rst_rec = r.rec.data();
    const bool has_rst = !rst.empty();

    if (has_rst) chain<true>(r); else chain<false>(r);
    const std::vector<unsigned long long> chained_in(r.s_in.begin(), r.s_in.begin() + nlanes), chained_out(r.s_out.begin(), r.s_out.begin() + nlanes);
    const std::vector<uint32_t> chained_cnt(r.cnt.begin(), r.cnt.begin() + nlanes);
    const std::vector<unsigned long long> chained_rec = r.rec;

    uint32_t passes = 0;
    int rounds = 0, replay_ok = 1;
    if (do_replay) {
        std::fill(r.s_in.begin(), r.s_in.end(), 0ull); std::fill(r.s_out.begin(), r.s_out.end(), 0ull);
        std::fill(r.cnt.begin(), r.cnt.end(), 0u); std::fill(r.rec.begin(), r.rec.end(), 0ull);
        if (has_rst) replay<true>(r, &passes, &rounds); else replay<false>(r, &passes, &rounds);
        for (int i = 0; i < nlanes; i++)
            if (r.s_in[i] != chained_in[i] || r.s_out[i] != chained_out[i] || r.cnt[i] != chained_cnt[i]) {
                if (replay_ok) std::fprintf(stderr, "replay: lane %d differs from the chain (in %llx / %llx, out %llx / %llx, cnt %u / %u)\n", i,
                                            r.s_in[i], chained_in[i], r.s_out[i], chained_out[i], r.cnt[i], chained_cnt[i]);
                replay_ok = 0;
            }
        for (size_t k = 0; k < rst.size(); k++)
            if (r.rec[k] != chained_rec[k]) {
                if (replay_ok) std::fprintf(stderr, "replay: boundary record %zu differs from the chain\n", k);
                replay_ok = 0;
            }
    }

    // the block every lane starts in, then the write pass
    unsigned long long sum = 0;
    for (int i = 0; i < nlanes; i++) { r.first[i] = sum; sum += r.cnt[i]; }
    r.first[nlanes] = sum;
    const int nwg_write = (nlanes + 255) / 256;
    for (int g = 0; g < nwg_write; g++) {
        stage(sh, a, static_cast<long long>(g) * 256, &r.tab, sizeof(DecTables));
        for (int t = 0; t < 256; t++) {
            if (has_rst) write_lane<true>(sh, a, g, t, &err); else write_lane<false>(sh, a, g, t, &err);
        }
    }
    std::printf("route=device err=%u blocks=%llu nblk=%d nlanes=%d nbits=%llu rst=%zu passes=%u rounds=%d replay_ok=%d\n", err, sum, nblk, nlanes,
                nbits, rst.size(), passes, rounds, replay_ok);
    std::fwrite(r.s_in.data(), 8, static_cast<size_t>(nlanes), stdout);
    std::fwrite(coef.data(), 2, coef.size(), stdout);
    std::fflush(stdout);
    return replay_ok ? 0 : 3;
}
