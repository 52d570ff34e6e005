// The deflate entry points: fnx_deflate_bound, fnx_deflate (deflate.hip's two kernels behind the argument checks and the
// staging of the three spaces) and fnx_png_encode (png_filter.hip's row stage, then the deflate, on the device; the file's
// chunks and their CRCs on the host); and fnx_png_decode, the other direction: png_parse.cpp's host side (chunk walk, inflate,
// the filter bytes), then png_decode.hip's two kernels (an Adam7 file on a ctx that accepts it: a descriptor per pass, the batched
// unfilter kernel once, png_expand_adam7_kernel); and fnx_png_decode_batch, which does the host side of a chunk of files
// on several threads and sends the chunk through one set of launches; and fnx_png_compress_batch / fnx_png_recompress_batch,
// compressPNG for a list of resident images (or of files) with one set of launches and three host waits per chunk.
#include "common.hpp"

#include <algorithm>

using namespace fnx;

namespace {

// CRC-32 of PNG's chunks (ISO 3309, polynomial 0xedb88320 reflected), eight bytes a step
struct CrcTables {
    uint32_t t[8][256];
    CrcTables()
    {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++) c = (c & 1u) ? 0xedb88320u ^ (c >> 1) : c >> 1;
            t[0][i] = c;
        }
        for (uint32_t i = 0; i < 256; i++) {
            for (int s = 1; s < 8; s++) t[s][i] = t[0][t[s - 1][i] & 0xffu] ^ (t[s - 1][i] >> 8);
        }
    }
};

uint32_t crc32_update(uint32_t crc, const uint8_t *p, size_t n)     // crc: the running register (start 0xffffffff, invert at the end)
{
    static const CrcTables tab;
    while (n >= 8) {
        uint32_t a, b;
        std::memcpy(&a, p, 4);
        std::memcpy(&b, p + 4, 4);
        a ^= crc;
        crc = tab.t[7][a & 0xffu] ^ tab.t[6][(a >> 8) & 0xffu] ^ tab.t[5][(a >> 16) & 0xffu] ^ tab.t[4][a >> 24] ^
              tab.t[3][b & 0xffu] ^ tab.t[2][(b >> 8) & 0xffu] ^ tab.t[1][(b >> 16) & 0xffu] ^ tab.t[0][b >> 24];
        p += 8;
        n -= 8;
    }
    for (; n; n--) crc = tab.t[0][(crc ^ *p++) & 0xffu] ^ (crc >> 8);
    return crc;
}

void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = static_cast<uint8_t>(v >> 24); p[1] = static_cast<uint8_t>(v >> 16); p[2] = static_cast<uint8_t>(v >> 8); p[3] = static_cast<uint8_t>(v);
}

// a chunk whose `len` body bytes already sit at at + 8: length and tag in front, CRC behind; returns the chunk's end
uint8_t *close_chunk(uint8_t *at, const char *tag, size_t len)
{
    put_be32(at, static_cast<uint32_t>(len));
    std::memcpy(at + 4, tag, 4);
    put_be32(at + 8 + len, ~crc32_update(0xffffffffu, at + 4, 4 + len));
    return at + 12 + len;
}

// ---- the file around a zlib stream: signature, IHDR, PLTE + tRNS for colour type 3, one IDAT, IEND ---------------------------
struct PngFrame {
    int w, h, color_type, bit_depth;
    int ncolors;                         // colour type 3: the palette's entries
    const uint8_t *palette;              // HOST, ncolors x 4 bytes r, g, b, a
    int ntrns() const                    // the alphas tRNS holds: up to and including the last one that is not 255
    {
        int n = 0;
        if (color_type == 3) {
            for (int i = 0; i < ncolors; i++) {
                if (palette[4 * i + 3] != 255) n = i + 1;
            }
        }
        return n;
    }
    size_t file_bytes(size_t zsize) const { return 8 + 25 + (color_type == 3 ? png_palette_chunks(ncolors, ntrns()) : 0) + 12 + zsize + 12; }
};

// everything in front of the stream; returns where the IDAT chunk starts (its body, the stream, goes to that + 8)
uint8_t *png_frame_head(const PngFrame &f, uint8_t *out)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::memcpy(out, sig, 8);
    uint8_t *at = out + 8;
    put_be32(at + 8, static_cast<uint32_t>(f.w));
    put_be32(at + 12, static_cast<uint32_t>(f.h));
    at[16] = static_cast<uint8_t>(f.bit_depth); at[17] = static_cast<uint8_t>(f.color_type); at[18] = 0; at[19] = 0; at[20] = 0;
    at = close_chunk(at, "IHDR", 13);
    if (f.color_type == 3) {
        const int ntrns = f.ntrns();
        for (int i = 0; i < f.ncolors; i++) std::memcpy(at + 8 + 3 * i, f.palette + 4 * i, 3);
        at = close_chunk(at, "PLTE", 3 * static_cast<size_t>(f.ncolors));
        if (ntrns) {
            for (int i = 0; i < ntrns; i++) at[8 + i] = f.palette[4 * i + 3];
            at = close_chunk(at, "tRNS", static_cast<size_t>(ntrns));
        }
    }
    return at;
}

// the IDAT chunk whose zsize body bytes are in place, and IEND
void png_frame_tail(uint8_t *idat, size_t zsize)
{
    close_chunk(close_chunk(idat, "IDAT", zsize), "IEND", 0);
}

// ---- fnx_png_decode_batch ---------------------------------------------------------------------------------------------------
// the device scratch (inflated streams + reconstructed planes) a chunk may ask for; a file that alone needs more is a chunk of one
constexpr size_t PNG_BATCH_SCRATCH = FNX_PNG_DECODE_CHUNK_BYTES;

size_t align16(size_t v) { return (v + 15) & ~size_t(15); }

struct BatchEntry {              // a file of the chunk in hand
    int index = 0;               // in the caller's arrays
    size_t stream_off = 0;       // in the staging area and in SLOT_PNG_DEC_STREAM alike: 16-byte aligned, want + 64 bytes
    size_t rows_off = 0;         // in SLOT_PNG_DEC_ROWS
};

// the batch's answer for its error text: the message of the lowest-indexed refused item
struct FirstRefusal {
    int index = -1;
    char text[512] = "";
    void note(int i)             // item i was refused just now: its message is this thread's last error
    {
        if (index >= 0 && index < i) return;
        index = i;
        std::snprintf(text, sizeof text, "%s", fnx_last_error());
    }
};

// the chunk's pinned staging area, free to be written: the uploads of the chunk before it have completed
int png_stage(fnx_ctx *ctx, size_t bytes, uint8_t **out)
{
    if (!ctx->png_stage_ev) FNX_HIP(hipEventCreateWithFlags(&ctx->png_stage_ev, hipEventDisableTiming));
    if (ctx->png_stage_busy) {
        FNX_HIP(hipEventSynchronize(ctx->png_stage_ev));
        ctx->png_stage_busy = false;
    }
    if (bytes > ctx->png_stage_cap) {
        if (ctx->png_stage) FNX_HIP(hipHostFree(ctx->png_stage));
        ctx->png_stage = nullptr;
        ctx->png_stage_cap = 0;
        const size_t cap = (bytes + bytes / 4 + 4095) & ~size_t(4095);
        FNX_HIP(hipHostMalloc(reinterpret_cast<void **>(&ctx->png_stage), cap, hipHostMallocDefault));
        ctx->png_stage_cap = cap;
    }
    *out = ctx->png_stage;
    return FNX_OK;
}

// One chunk: the host side of its files on `workers` threads, then -- on this thread, which owns the stream -- the uploads of
// the files that passed, the tables, and one set of launches.  Below 0 only where the chunk could not run at all.
int png_decode_chunk(fnx_ctx *ctx, const std::vector<BatchEntry> &chunk, const std::vector<PngFile> &heads, size_t stage_bytes, size_t rows_bytes,
                     const uint8_t *const *files, const size_t *sizes, uint8_t *const *dsts, const int *dstrides, int workers, int *status,
                     FirstRefusal *first)
{
    const int m = static_cast<int>(chunk.size());
    uint8_t *stage = nullptr;
    FNX_TRY(png_stage(ctx, stage_bytes ? stage_bytes : 16, &stage));
    std::vector<PngPrepared> items(m);
    std::vector<const uint8_t *> cf(m);
    std::vector<size_t> cs(m);
    for (int j = 0; j < m; j++) {
        const size_t want = png_stream_bytes(heads[j]);
        cf[j] = files[chunk[j].index];
        cs[j] = sizes[chunk[j].index];
        if (want / 1032 <= cs[j]) {                      // else png_stream_size refuses the file: it gets no room
            items[j].stream = stage + chunk[j].stream_off;
            items[j].cap = want;
        }
    }
    png_prepare_many(cf.data(), cs.data(), m, workers, items.data(), ctx->png_adam7 != 0);

    // verdicts in index order; the files that passed get a descriptor each -- an Adam7 file one per present pass, behind the
    // non-interlaced files' (png_expand_batch_kernel searches descriptors [0, nplain) alone) --, and the units are sorted by bpp
    std::vector<PngBatchFile> desc;
    std::vector<PngAdam7File> adesc;
    std::vector<int> ok;
    std::vector<PngBatchUnit> units[6];
    size_t npal = 0;
    uint32_t nplain = 0, npass = 0, plain_seen = 0;
    for (int j = 0; j < m; j++) {
        if (items[j].status == FNX_OK && items[j].f.interlace != 1) nplain++;
    }
    for (int j = 0; j < m; j++) {
        const int i = chunk[j].index;
        status[i] = items[j].status;
        if (items[j].status != FNX_OK) {
            png_reissue(items[j]);
            first->note(i);
            continue;
        }
        int k = 0;
        while (k < 5 && PNG_BPPS[k] != items[j].f.bpp) k++;
        if (items[j].f.interlace == 1) {
            // the passes' descriptors follow in pass order (below): slot[p] is pass p's
            uint32_t slot[7];
            for (int p = 0; p < 7; p++) slot[p] = items[j].f.ph[p] ? nplain + npass++ : 0;
            for (size_t u = 0; u + 1 < items[j].units.size(); u += 2)
                units[k].push_back(PngBatchUnit{slot[items[j].unit_pass[u / 2]], items[j].units[u], items[j].units[u + 1]});
        } else {
            for (size_t u = 0; u + 1 < items[j].units.size(); u += 2)
                units[k].push_back(PngBatchUnit{plain_seen, items[j].units[u], items[j].units[u + 1]});
            plain_seen++;
        }
        if (items[j].f.color_type == 3) npal++;
        ok.push_back(j);
    }
    if (ok.empty()) return FNX_OK;
    void *ds = nullptr, *dr = nullptr;
    FNX_TRY(scratch(ctx, SLOT_PNG_DEC_STREAM, stage_bytes + 16, &ds));
    FNX_TRY(scratch(ctx, SLOT_PNG_DEC_ROWS, rows_bytes + 16, &dr));
    for (int j : ok)
        FNX_HIP(hipMemcpyAsync(static_cast<uint8_t *>(ds) + chunk[j].stream_off, items[j].stream, items[j].want, hipMemcpyHostToDevice, ctx->stream));
    FNX_HIP(hipEventRecord(ctx->png_stage_ev, ctx->stream));
    ctx->png_stage_busy = true;

    // the tables: the sorted units, the descriptors, a palette's 256 pixel values per paletted file.  The descriptors hold
    // pointers into the table slot itself, so its address is asked for first (same size: the same buffer)
    std::vector<PngBatchUnit> sorted;
    int nunits[6];
    for (int k = 0; k < 6; k++) {
        nunits[k] = static_cast<int>(units[k].size());
        sorted.insert(sorted.end(), units[k].begin(), units[k].end());
    }
    std::vector<uint32_t> pals(256 * (npal ? npal : 1), 0);
    const size_t na = ok.size() - nplain;
    const size_t tsizes[4] = {sizeof(PngBatchUnit) * sorted.size(), sizeof(PngBatchFile) * (nplain + npass), sizeof(uint32_t) * pals.size(),
                              sizeof(PngAdam7File) * na};
    void *tab = nullptr;
    FNX_TRY(scratch(ctx, SLOT_PNG_DEC_TAB, align16(tsizes[0]) + align16(tsizes[1]) + align16(tsizes[2]) + align16(tsizes[3]), &tab));
    const uint32_t *d_pals = reinterpret_cast<const uint32_t *>(static_cast<uint8_t *>(tab) + align16(tsizes[0]) + align16(tsizes[1]));
    unsigned long long tiles = 0, atiles = 0;
    size_t pal = 0;
    desc.assign(nplain + npass, PngBatchFile());
    size_t plain_at = 0, pass_at = nplain;
    for (int j : ok) {
        const PngFile &f = items[j].f;
        const int i = chunk[j].index;
        PngBatchFile d;
        std::memset(&d, 0, sizeof d);
        d.e.w = f.w; d.e.h = f.h; d.e.color_type = f.color_type; d.e.depth = f.depth;
        d.e.has_trns = f.has_trns ? 1 : 0;
        for (int k = 0; k < 3; k++) d.e.key[k] = f.trns16[k];
        d.table = d_pals;
        if (f.color_type == 3) {
            std::memcpy(pals.data() + 256 * pal, items[j].table, sizeof items[j].table);
            d.table = d_pals + 256 * pal++;
        }
        d.dst = dsts[i];
        d.dstride = dstrides[i];
        const uint8_t *stream = static_cast<const uint8_t *>(ds) + chunk[j].stream_off;
        uint8_t *rows = static_cast<uint8_t *>(dr) + chunk[j].rows_off;
        if (f.interlace == 1) {
            PngAdam7File a;
            std::memset(&a, 0, sizeof a);
            a.e = d.e; a.table = d.table; a.dst = d.dst; a.dstride = d.dstride;
            a.tile0 = static_cast<uint32_t>(atiles);
            atiles += static_cast<unsigned long long>((f.w + 255) / 256) * f.h;
            for (int p = 0; p < 7; p++) {
                if (f.ph[p] == 0) continue;
                PngBatchFile dp = d;                      // the unfilter kernel's view of the pass: an image of its own
                dp.stream = stream + f.poff[p];
                dp.spitch = 1 + f.prow[p];
                dp.rows = rows;
                dp.ppitch = align16(f.prow[p]);
                dp.rowbytes = static_cast<int>(f.prow[p]);
                dp.npix = static_cast<int>(f.prow[p] / f.bpp);
                dp.e.w = f.pw[p]; dp.e.h = f.ph[p];
                dp.dst = nullptr;
                desc[pass_at++] = dp;
                a.plane[p] = rows;
                a.ppitch[p] = static_cast<uint32_t>(dp.ppitch);
                rows += dp.ppitch * f.ph[p];
            }
            adesc.push_back(a);
            continue;
        }
        d.stream = stream;
        d.spitch = 1 + f.rowbytes;
        d.rows = rows;
        d.ppitch = png_plane_pitch(f);
        d.rowbytes = static_cast<int>(f.rowbytes);
        d.npix = static_cast<int>(f.rowbytes / f.bpp);
        d.tile0 = static_cast<uint32_t>(tiles);
        tiles += static_cast<unsigned long long>((f.w + 255) / 256) * f.h;
        desc[plain_at++] = d;
    }
    if (tiles > 0x7fffffffull || atiles > 0x7fffffffull) {
        set_error("internal: a chunk of %llu workgroups of png_expand_batch_kernel", tiles > atiles ? tiles : atiles);
        return FNX_ERR_INVALID;
    }
    if (plain_at != nplain || pass_at != nplain + npass || adesc.size() != na) {
        set_error("internal: the chunk's descriptors do not add up");
        return FNX_ERR_INVALID;
    }
    const void *hosts[4] = {sorted.data(), desc.data(), pals.data(), adesc.data()};
    void *dp[4];
    FNX_TRY(upload_tables(ctx, SLOT_PNG_DEC_TAB, hosts, tsizes, na ? 4 : 3, dp));
    if (dp[2] != static_cast<const void *>(d_pals)) {
        set_error("internal: the table slot moved between two requests of one size");
        return FNX_ERR_INVALID;
    }
    return launch_png_decode_chunk(ctx, static_cast<const PngBatchUnit *>(dp[0]), nunits, static_cast<const PngBatchFile *>(dp[1]),
                                   static_cast<int>(nplain), static_cast<uint32_t>(tiles), na ? static_cast<const PngAdam7File *>(dp[3]) : nullptr,
                                   static_cast<int>(na), static_cast<uint32_t>(atiles));
}

int png_decode_batch_device(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes, uint8_t *const *dsts, const int *dstrides,
                            int workers, int *ws, int *hs, int *status, FirstRefusal *firstp);

}  // namespace

namespace fnx {

int deflate_device(fnx_ctx *ctx, const uint8_t *d_src, size_t n, int row, bool out_on_device, uint8_t *out, size_t cap, size_t *nbytes)
{
    uint8_t *d_out = out;
    size_t d_cap = cap;
    if (!out_on_device) {                                            // the stream is gathered on the device and copied once its size is known
        void *t = nullptr;
        d_cap = deflate_bound(n);
        FNX_TRY(scratch(ctx, SLOT_DEFLATE_OUT, d_cap + 16, &t));
        d_out = static_cast<uint8_t *>(t);
    }
    const unsigned long long *d_size = nullptr;
    FNX_TRY(launch_deflate(ctx, d_src, n, row, d_out, d_cap, &d_size));
    unsigned long long size = 0;
    FNX_TRY(fetch_bytes(ctx, d_size, &size, sizeof(size)));
    *nbytes = static_cast<size_t>(size);
    if (cap < *nbytes || !out) {
        set_error("invalid argument: the zlib stream needs %zu bytes of output, cap is %zu", *nbytes, cap);
        return FNX_ERR_INVALID;
    }
    if (!out_on_device) {
        FNX_HIP(hipMemcpyAsync(out, d_out, *nbytes, hipMemcpyDeviceToHost, ctx->stream));
        FNX_HIP(hipStreamSynchronize(ctx->stream));
    }
    return FNX_OK;
}

int png_encode_device(fnx_ctx *ctx, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque, const uint8_t *palette,
                      uint8_t *out, size_t cap, size_t *nbytes)
{
    // the row stage into device scratch: room for RGBA rows when the call itself finds the opacity
    const size_t row_max = kind == FNX_PNG_NRGBA ? static_cast<size_t>(w) * (opaque == 1 ? 3 : 4) : static_cast<size_t>(w);
    const size_t stream_cap = static_cast<size_t>(h) * (row_max + 1);
    void *dstream = nullptr;
    FNX_TRY(scratch(ctx, SLOT_PNG_STREAM, stream_cap + 16, &dstream));
    size_t stream_bytes = 0;
    int color_type = 0, bit_depth = 0;
    FNX_TRY(png_filter_device(ctx, kind, src, sstride, w, h, ncolors, opaque, true, static_cast<uint8_t *>(dstream), stream_cap, &stream_bytes,
                              &color_type, &bit_depth));
    // the deflate, gathered on the device
    const size_t zcap = deflate_bound(stream_bytes);
    void *dz = nullptr;
    FNX_TRY(scratch(ctx, SLOT_DEFLATE_OUT, zcap + 16, &dz));
    const unsigned long long *d_size = nullptr;
    FNX_TRY(launch_deflate(ctx, static_cast<const uint8_t *>(dstream), stream_bytes, static_cast<int>(stream_bytes / h), static_cast<uint8_t *>(dz),
                           zcap, &d_size));
    unsigned long long zsize = 0;
    FNX_TRY(fetch_bytes(ctx, d_size, &zsize, sizeof(zsize)));

    const PngFrame frame{w, h, color_type, bit_depth, ncolors, palette};
    *nbytes = frame.file_bytes(static_cast<size_t>(zsize));
    if (cap < *nbytes || !out) {
        set_error("invalid argument: the PNG file needs %zu bytes of output, cap is %zu", *nbytes, cap);
        return FNX_ERR_INVALID;
    }
    if (zsize > 0x7fffffffull) {
        set_error("invalid argument: a PNG chunk holds at most 2^31 - 1 bytes");
        return FNX_ERR_INVALID;
    }
    uint8_t *at = png_frame_head(frame, out);
    FNX_HIP(hipMemcpyAsync(at + 8, dz, static_cast<size_t>(zsize), hipMemcpyDeviceToHost, ctx->stream));
    FNX_HIP(hipStreamSynchronize(ctx->stream));
    png_frame_tail(at, static_cast<size_t>(zsize));
    return FNX_OK;
}

}  // namespace fnx

extern "C" {

size_t fnx_deflate_bound(size_t n) { return deflate_bound(n); }

int fnx_deflate(fnx_ctx *ctx, int space, const uint8_t *src, size_t n, int row, uint8_t *out, size_t cap, size_t *nbytes)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_REQUIRE(src != nullptr && nbytes != nullptr, "src and nbytes");
    FNX_REQUIRE(n >= 1, "n: at least one byte");
    FNX_REQUIRE(out != nullptr || cap == 0, "out is null");
    FNX_REQUIRE(row >= 0, "row: a length, or 0 for none");
    const uint8_t *dsrc = src;
    if (space == FNX_HOST) {
        void *d = nullptr;
        FNX_TRY(scratch(ctx, SLOT_IN_A, n + 16, &d));
        FNX_HIP(hipMemcpyAsync(d, src, n, hipMemcpyHostToDevice, ctx->stream));
        dsrc = static_cast<const uint8_t *>(d);
    }
    return deflate_device(ctx, dsrc, n, row, space == FNX_DEVICE, out, cap, nbytes);
}

int fnx_png_encode(fnx_ctx *ctx, int space, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque,
                   const uint8_t *palette, uint8_t *out, size_t cap, size_t *nbytes)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_REQUIRE(kind == FNX_PNG_PALETTED || kind == FNX_PNG_GRAY || kind == FNX_PNG_NRGBA, "kind: 1 (paletted), 2 (gray) or 3 (NRGBA)");
    FNX_REQUIRE(src != nullptr && nbytes != nullptr, "src and nbytes");
    FNX_REQUIRE(out != nullptr || cap == 0, "out is null");
    FNX_REQUIRE(w >= 1 && h >= 1 && w <= 65535 && h <= 65535, "dims: 1..65535");
    FNX_REQUIRE(kind != FNX_PNG_PALETTED || (ncolors >= 1 && ncolors <= 256), "ncolors: 1..256 (image.Paletted indices are uint8)");
    FNX_REQUIRE(kind != FNX_PNG_PALETTED || palette != nullptr, "a paletted image needs its palette");
    FNX_REQUIRE(opaque >= -1 && opaque <= 1, "opaque: 1, 0, or -1 to decide as Opaque() does");
    const bool nrgba = kind == FNX_PNG_NRGBA;
    if (nrgba) {
        FNX_TRY(check_img(src, sstride, w, h, "src"));
        FNX_REQUIRE(space == FNX_HOST || (reinterpret_cast<uintptr_t>(src) & 3u) == 0, "a device image is 4-byte aligned");
    } else {
        FNX_REQUIRE(sstride >= w, "plane stride");
    }
    const uint8_t *dsrc = src;
    if (space == FNX_HOST) {
        const size_t len = static_cast<size_t>(h - 1) * sstride + static_cast<size_t>(w) * (nrgba ? 4 : 1);
        void *d = nullptr;
        FNX_TRY(scratch(ctx, SLOT_IN_A, len + 16, &d));
        FNX_HIP(hipMemcpyAsync(d, src, len, hipMemcpyHostToDevice, ctx->stream));
        dsrc = static_cast<const uint8_t *>(d);
    }
    return png_encode_device(ctx, kind, dsrc, sstride, w, h, ncolors, opaque, palette, out, cap, nbytes);
}

int fnx_png_decode(fnx_ctx *ctx, const uint8_t *data, size_t n, int space, uint8_t *dst, int dstride, int *w, int *h)
{
    FNX_REQUIRE(data != nullptr && w != nullptr && h != nullptr, "decode arguments");
    FNX_REQUIRE(space == FNX_HOST || space == FNX_DEVICE, "space: FNX_HOST or FNX_DEVICE (also where only the dimensions are asked for)");
    PngFile f;
    if (dst == nullptr) {                        // png.DecodeConfig: the dimensions only (and whether the device takes the file);
        FNX_TRY(png_parse(data, n, &f, ctx && ctx->png_adam7));   // host work, no ctx needed (with one: its fnx_ctx_set_png_adam7)
        *w = f.w; *h = f.h;
        return FNX_OK;
    }
    FNX_ENTER(ctx);
    FNX_TRY(png_parse(data, n, &f, ctx->png_adam7 != 0));
    *w = f.w; *h = f.h;
    FNX_TRY(check_img(dst, dstride, f.w, f.h, "dst"));
    FNX_REQUIRE(space != FNX_DEVICE || (reinterpret_cast<uintptr_t>(dst) & 3u) == 0, "a device image is 4-byte aligned");
    // the stream's size is known beforehand; fewer or more bytes are image/png's "not enough" / "too much pixel data"
    size_t want = 0;
    FNX_TRY(png_stream_size(f, &want));
    void *pin = nullptr;
    FNX_TRY(pinned_alloc(ctx, want + 64, &pin));
    uint8_t *stream = static_cast<uint8_t *>(pin);
    size_t got = 0;
    FNX_TRY(png_inflate(f.idat.data(), f.idat.size(), stream, want, &got));
    if (got != want) return png_corrupt("not enough pixel data");
    std::vector<uint32_t> units;
    std::vector<uint8_t> unit_pass;
    FNX_TRY(png_row_plan(stream, f, &units, &unit_pass));    // a filter type above 4 is refused here: nothing has been launched
    DevOut d;
    FNX_TRY(stage_out(ctx, space, dst, dstride, f.w, f.h, SLOT_OUT, &d));
    void *ds = nullptr, *dr = nullptr;
    FNX_TRY(scratch(ctx, SLOT_PNG_DEC_STREAM, want + 64, &ds));            // the kernel's 16-byte loads reach up to 15 bytes past a row
    FNX_TRY(scratch(ctx, SLOT_PNG_DEC_ROWS, png_planes_bytes(f) + 16, &dr));
    FNX_HIP(hipMemcpyAsync(ds, stream, want, hipMemcpyHostToDevice, ctx->stream));
    uint32_t table[256];
    std::memset(table, 0, sizeof table);
    if (f.color_type == 3) png_palette_table(f, table);
    if (f.interlace == 1) {
        // the passes as a list of images of one bpp: a descriptor per present pass, every pass's units in one launch.  A pass's
        // 16-byte loads past a row's end read the next pass's bytes; the slot's 64 spare bytes stand behind the last one
        PngBatchFile passes[7];
        PngAdam7File a;
        std::memset(passes, 0, sizeof passes);
        std::memset(&a, 0, sizeof a);
        a.e.w = f.w; a.e.h = f.h; a.e.color_type = f.color_type; a.e.depth = f.depth;
        a.e.has_trns = f.has_trns ? 1 : 0;
        for (int k = 0; k < 3; k++) a.e.key[k] = f.trns16[k];
        a.dst = d.p;
        a.dstride = d.stride;
        uint32_t slot[7] = {0, 0, 0, 0, 0, 0, 0}, npass = 0;
        uint8_t *rows = static_cast<uint8_t *>(dr);
        for (int p = 0; p < 7; p++) {
            if (f.ph[p] == 0) continue;
            PngBatchFile &dp = passes[npass];
            dp.stream = static_cast<const uint8_t *>(ds) + f.poff[p];
            dp.spitch = 1 + f.prow[p];
            dp.rows = rows;
            dp.ppitch = align16(f.prow[p]);
            dp.rowbytes = static_cast<int>(f.prow[p]);
            dp.npix = static_cast<int>(f.prow[p] / f.bpp);
            a.plane[p] = rows;
            a.ppitch[p] = static_cast<uint32_t>(dp.ppitch);
            rows += dp.ppitch * f.ph[p];
            slot[p] = npass++;
        }
        std::vector<PngBatchUnit> bu;
        for (size_t u = 0; u + 1 < units.size(); u += 2) bu.push_back(PngBatchUnit{slot[unit_pass[u / 2]], units[u], units[u + 1]});
        const void *hosts[3] = {bu.data(), passes, table};
        const size_t sizes[3] = {sizeof(PngBatchUnit) * bu.size(), sizeof(PngBatchFile) * npass, sizeof table};
        void *dp[3];
        FNX_TRY(upload_tables(ctx, SLOT_PNG_DEC_TAB, hosts, sizes, 3, dp));
        a.table = static_cast<const uint32_t *>(dp[2]);
        FNX_TRY(launch_png_adam7(ctx, f.bpp, static_cast<const PngBatchUnit *>(dp[0]), static_cast<int>(bu.size()),
                                 static_cast<const PngBatchFile *>(dp[1]), a));
        return finish(ctx, space, &d);
    }
    const void *hosts[2] = {units.data(), table};
    const size_t sizes[2] = {sizeof(uint32_t) * units.size(), sizeof table};
    void *dp[2];
    FNX_TRY(upload_tables(ctx, SLOT_PNG_DEC_TAB, hosts, sizes, 2, dp));
    FNX_TRY(launch_png_unfilter(ctx, static_cast<const uint8_t *>(ds), f, static_cast<const uint32_t *>(dp[0]), static_cast<int>(units.size() / 2),
                                static_cast<uint8_t *>(dr)));
    FNX_TRY(launch_png_expand(ctx, static_cast<const uint8_t *>(dr), f, static_cast<const uint32_t *>(dp[1]), d.p, d.stride));
    return finish(ctx, space, &d);
}

int fnx_png_decode_batch(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes, uint8_t *const *dsts, const int *dstrides,
                         int workers, int *ws, int *hs, int *status)
{
    FNX_ENTER(ctx);
    FNX_REQUIRE(n >= 1 && n <= FNX_BATCH_MAX, "decode batch: n must be 1..FNX_BATCH_MAX (65535)");
    FNX_REQUIRE(files && sizes && dsts && dstrides && ws && hs && status, "decode batch: NULL array");
    FNX_REQUIRE(workers >= 0 && workers <= 64, "decode batch: workers must be 0..64 (0: min(8, files in the chunk))");
    FirstRefusal first;
    FNX_TRY(png_decode_batch_device(ctx, n, files, sizes, dsts, dstrides, workers, ws, hs, status, &first));
    if (first.index >= 0) set_error("%s", first.text);
    return FNX_OK;
}

}  // extern "C"

namespace {

// fnx_png_decode_batch behind its argument checks; first: the lowest-indexed refused item's message so far
int png_decode_batch_device(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes, uint8_t *const *dsts, const int *dstrides,
                            int workers, int *ws, int *hs, int *status, FirstRefusal *firstp)
{
    FirstRefusal &first = *firstp;
    std::vector<BatchEntry> chunk;
    std::vector<PngFile> heads;
    size_t stage_bytes = 0, rows_bytes = 0;
    auto flush = [&]() -> int {
        if (chunk.empty()) return FNX_OK;
        const int rc = png_decode_chunk(ctx, chunk, heads, stage_bytes, rows_bytes, files, sizes, dsts, dstrides, workers, status, &first);
        chunk.clear();
        heads.clear();
        stage_bytes = rows_bytes = 0;
        return rc;
    };
    for (int i = 0; i < n; i++) {
        ws[i] = hs[i] = 0;
        status[i] = FNX_ERR_INVALID;
        if (!files[i]) {
            set_error("invalid argument: decode batch: files[%d] is NULL", i);
            first.note(i);
            continue;
        }
        // the signature and IHDR on this thread: the dimensions, what the device does not take, and the item's own arguments --
        // the order of fnx_png_decode's refusals.  The rest of the file is the workers' business
        PngFile head;
        const int rc = png_probe(files[i], sizes[i], &head, ctx->png_adam7 != 0);
        if (rc == FNX_OK || rc == FNX_ERR_UNSUPPORTED) { ws[i] = head.w; hs[i] = head.h; }
        if (rc < 0) {
            status[i] = rc;
            first.note(i);
            continue;
        }
        if (!dsts[i]) {
            set_error("invalid argument: decode batch: dsts[%d] is NULL", i);
            first.note(i);
            continue;
        }
        if (check_img(dsts[i], dstrides[i], head.w, head.h, "dst") < 0) {
            first.note(i);
            continue;
        }
        if (reinterpret_cast<uintptr_t>(dsts[i]) & 3u) {
            set_error("invalid argument: a device image is 4-byte aligned");
            first.note(i);
            continue;
        }
        const size_t want = png_stream_bytes(head);
        const bool room = want / 1032 <= sizes[i];       // else the file cannot hold its rows: refused before its inflate, no room needed
        const size_t sbytes = room ? align16(want + 64) : 0, rbytes = room ? align16(png_planes_bytes(head) + 16) : 0;
        if (!chunk.empty() && (static_cast<int>(chunk.size()) >= FNX_PNG_DECODE_CHUNK || stage_bytes + rows_bytes + sbytes + rbytes > PNG_BATCH_SCRATCH)) {
            const int frc = flush();
            if (frc < 0) return frc;
        }
        BatchEntry e;
        e.index = i;
        e.stream_off = stage_bytes;
        e.rows_off = rows_bytes;
        stage_bytes += sbytes;
        rows_bytes += rbytes;
        chunk.push_back(e);
        heads.push_back(head);
    }
    return flush();
}

// ---- fnx_png_compress_batch ---------------------------------------------------------------------------------------------------
constexpr const char *PNG_CB_ROUTE =
    "png_colors_batch_kernel, png_finish_batch_kernel, png_flags_batch_kernel, png_plane_batch_kernel, png_filter_batch_kernel, "
    "png_pack_batch_kernel, deflate_chunk_batch_kernel, deflate_gather_batch_kernel";
constexpr const char *PNG_CB_ROUTE_DENSE =                            // on a ctx at FNX_DEFLATE_LEVEL_DENSE
    "png_colors_batch_kernel, png_finish_batch_kernel, png_flags_batch_kernel, png_plane_batch_kernel, png_filter_batch_kernel, "
    "png_pack_batch_kernel, deflate_dense_chunk_batch_kernel, deflate_gather_batch_kernel";

// `bytes` device bytes into pinned host memory, waited for: one of a chunk's three host waits
int png_cb_fetch(fnx_ctx *ctx, const void *d, size_t bytes, const uint8_t **host)
{
    void *pin = nullptr;
    FNX_TRY(pinned_alloc(ctx, bytes ? bytes : 16, &pin));
    if (bytes) FNX_HIP(hipMemcpyAsync(pin, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
    FNX_HIP(hipStreamSynchronize(ctx->stream));
    *host = static_cast<const uint8_t *>(pin);
    return FNX_OK;
}

// One chunk: m images that passed their argument checks (at[j]: image j's place in the caller's arrays) through one set of
// launches and three host waits -- the classification words, the streams' sizes, the streams' bytes.  (The three fetches and
// the table uploads take their pinned bytes from the ctx's ring: where the ring grows or wraps, pinned_alloc waits for the
// stream once more -- by then the stream is idle or nearly so, but it is a wait.)
int png_compress_chunk(fnx_ctx *ctx, int m, const PngCbSrc *imgs, const int *at, int base, uint8_t *const *outs, const size_t *caps, size_t *nbytes,
                       int *kinds, int *status, FirstRefusal *first)
{
    note_route(ctx, FNX_PROF_MAIN, ctx->deflate_level == FNX_DEFLATE_LEVEL_DENSE ? PNG_CB_ROUTE_DENSE : PNG_CB_ROUTE);
    const void *d_results = nullptr;
    FNX_TRY(launch_png_classify_batch(ctx, m, imgs, &d_results));
    const size_t rb = png_result_bytes();
    const uint8_t *pin = nullptr;
    FNX_TRY(png_cb_fetch(ctx, d_results, rb * m, &pin));                       // wait 1
    std::vector<uint8_t> results(pin, pin + rb * m);                         // (the pinned ring is used again below)

    // compress.go:92-107 per image: tryPalettize, else isGrayscale + toGray, else the image as it is (RGB rows when Opaque())
    std::vector<PngCbClass> cls(m);
    std::vector<int> ws(m), hs(m), which(m);
    for (int j = 0; j < m; j++) {
        uint32_t r[4];
        std::memcpy(r, results.data() + rb * j, sizeof r);
        ws[j] = imgs[j].w; hs[j] = imgs[j].h;
        if (!r[0]) cls[j] = PngCbClass{FNX_PNG_PALETTED, static_cast<int>(r[2]), 0};
        else if (!(r[3] & 2u)) cls[j] = PngCbClass{FNX_PNG_GRAY, 0, 0};
        else cls[j] = PngCbClass{FNX_PNG_NRGBA, 0, (r[3] & 1u) ? 0 : 1};
        which[j] = cls[j].kind == FNX_PNG_PALETTED ? 1 : (cls[j].kind == FNX_PNG_GRAY ? 2 : 0);
    }
    PngCbPlan plan;
    png_cb_plan(ws.data(), hs.data(), cls.data(), m, &plan);

    void *dpl = nullptr, *dst = nullptr;
    FNX_TRY(scratch(ctx, SLOT_PNG_CB_PLANES, plan.plane_bytes + 16, &dpl));
    FNX_TRY(scratch(ctx, SLOT_PNG_CB_STREAMS, plan.stream_bytes + 16, &dst));
    uint8_t *planes = static_cast<uint8_t *>(dpl), *streams = static_cast<uint8_t *>(dst);
    std::vector<uint8_t *> pp(m);
    std::vector<int> ps(m);
    for (int j = 0; j < m; j++) {
        pp[j] = which[j] ? planes + plan.images[j].plane_off : nullptr;
        ps[j] = static_cast<int>(plan.images[j].plane_pitch);
    }
    FNX_TRY(launch_png_planes_batch(ctx, m, imgs, which.data(), pp.data(), ps.data()));

    // the row stage: a record per image, the units of the forms back to back
    std::vector<PngCbRows> rows(m);
    std::vector<PngCbUnit> units;
    int nunits[PNG_CB_FORMS];
    for (int j = 0; j < m; j++) {
        PngCbRows &r = rows[j];
        r.src = which[j] ? pp[j] : imgs[j].src;
        r.sstride = which[j] ? ps[j] : imgs[j].sstride;
        r.w = imgs[j].w; r.h = imgs[j].h;
        r.n = static_cast<int>(plan.images[j].rowbytes);
        r.al4 = png_cb_al4(r.src, r.sstride);
        r.out = streams + plan.images[j].stream_off;
    }
    for (int k = 0; k < PNG_CB_FORMS; k++) {
        nunits[k] = static_cast<int>(plan.rows[k].size());
        units.insert(units.end(), plan.rows[k].begin(), plan.rows[k].end());
    }
    {
        const void *hosts[2] = {rows.data(), units.data()};
        const size_t sizes[2] = {sizeof(PngCbRows) * rows.size(), sizeof(PngCbUnit) * units.size()};
        void *dp[2];
        FNX_TRY(upload_tables(ctx, SLOT_PNG_CB_TAB2, hosts, sizes, 2, dp));
        FNX_TRY(launch_png_rows_batch(ctx, static_cast<const PngCbUnit *>(dp[1]), nunits, static_cast<const PngCbRows *>(dp[0])));
    }

    // the deflate: a workgroup per 32 KiB of any stream
    std::vector<DeflateBatchUnit> du(plan.deflate.size());
    std::vector<DeflateBatchImage> di(m);
    for (size_t k = 0; k < du.size(); k++) {
        const PngCbDeflateUnit &u = plan.deflate[k];
        du[k] = DeflateBatchUnit{streams + u.src_off, u.len, u.row, u.last, u.image};
    }
    for (int j = 0; j < m; j++) di[j] = DeflateBatchImage{plan.images[j].stream_bytes, plan.images[j].chunk0, plan.images[j].nchunks};
    const uint8_t *d_out = nullptr;
    const unsigned long long *d_sizes = nullptr;
    {
        const void *hosts[2] = {du.data(), di.data()};
        const size_t sizes[2] = {sizeof(DeflateBatchUnit) * du.size(), sizeof(DeflateBatchImage) * di.size()};
        void *dp[2];
        FNX_TRY(upload_tables(ctx, SLOT_PNG_CB_TAB3, hosts, sizes, 2, dp));
        FNX_TRY(launch_deflate_batch(ctx, static_cast<const DeflateBatchUnit *>(dp[0]), static_cast<const DeflateBatchImage *>(dp[1]),
                                     static_cast<uint32_t>(du.size()), static_cast<uint32_t>(m), plan.out_bytes, &d_out, &d_sizes));
    }
    FNX_TRY(png_cb_fetch(ctx, d_sizes, sizeof(unsigned long long) * m, &pin));  // wait 2
    std::vector<unsigned long long> zsizes(m);
    std::memcpy(zsizes.data(), pin, sizeof(unsigned long long) * m);
    size_t total = 0;
    for (int j = 0; j < m; j++) {
        if (zsizes[j] > deflate_bound(plan.images[j].stream_bytes)) {
            set_error("internal: a stream of the compress batch is longer than its bound");
            return FNX_ERR_INVALID;
        }
        total += static_cast<size_t>(zsizes[j]);
    }
    FNX_TRY(png_cb_fetch(ctx, d_out, total, &pin));                           // wait 3: the streams' own bytes, back to back

    // the files: the chunks around each stream and their CRCs, on this thread
    size_t off = 0;
    for (int j = 0; j < m; j++) {
        const int i = at[j];
        const PngCbImage &im = plan.images[j];
        const size_t zsize = static_cast<size_t>(zsizes[j]);
        const PngFrame frame{im.w, im.h, im.color_type, im.depth, cls[j].ncolors, results.data() + rb * j + 16};
        nbytes[i] = frame.file_bytes(zsize);
        kinds[i] = im.kind;
        if (caps[i] < nbytes[i] || !outs[i]) {
            set_error("invalid argument: compress batch: the PNG file of image %d needs %zu bytes of output, cap is %zu", base + i, nbytes[i], caps[i]);
            status[i] = FNX_ERR_INVALID;
            first->note(base + i);
        } else if (zsize > 0x7fffffffull) {
            set_error("invalid argument: a PNG chunk holds at most 2^31 - 1 bytes");
            status[i] = FNX_ERR_INVALID;
            first->note(base + i);
        } else {
            uint8_t *idat = png_frame_head(frame, outs[i]);
            std::memcpy(idat + 8, pin + off, zsize);
            png_frame_tail(idat, zsize);
            status[i] = FNX_OK;
        }
        off += zsize;
    }
    return FNX_OK;
}

// The batch behind its argument checks: every item's own checks, then the items that passed, chunk by chunk.  skip[i] != 0
// (may be NULL): item i is not this call's business (fnx_png_recompress_batch: its file was refused), nothing of it is touched.
// base: item 0's index in the caller's batch, for the messages.
int png_compress_items(fnx_ctx *ctx, int base, int n, const uint8_t *const *srcs, const int *sstrides, const int *ws, const int *hs, uint8_t *const *outs,
                       const size_t *caps, size_t *nbytes, int *kinds, int *status, const char *skip, FirstRefusal *first)
{
    std::vector<PngCbSrc> imgs;
    std::vector<int> at, vw, vh;
    for (int i = 0; i < n; i++) {
        if (skip && skip[i]) continue;
        nbytes[i] = 0;
        kinds[i] = 0;
        status[i] = FNX_ERR_INVALID;
        const char *why = nullptr;
        if (!srcs[i]) why = "srcs[%d] is NULL";
        else if (!outs[i] && caps[i] != 0) why = "outs[%d] is NULL and its cap is not 0";
        else if (ws[i] < 1 || hs[i] < 1 || ws[i] > 65535 || hs[i] > 65535) why = "image %d: dims are 1..65535";
        else if (sstrides[i] < 4 * ws[i] || (sstrides[i] & 3)) why = "image %d: the stride is at least 4w and a multiple of 4";
        else if (reinterpret_cast<uintptr_t>(srcs[i]) & 3u) why = "image %d: a device image is 4-byte aligned";
        if (why) {
            char fmt[160];
            std::snprintf(fmt, sizeof fmt, "invalid argument: compress batch: %s", why);
            set_error(fmt, base + i);
            first->note(base + i);
            continue;
        }
        imgs.push_back(PngCbSrc{srcs[i], sstrides[i], ws[i], hs[i]});
        at.push_back(i);
        vw.push_back(ws[i]);
        vh.push_back(hs[i]);
    }
    if (imgs.empty()) return FNX_OK;
    std::vector<int> firsts;
    png_cb_split(vw.data(), vh.data(), static_cast<int>(imgs.size()), &firsts);
    for (size_t c = 0; c + 1 < firsts.size(); c++) {
        const int j0 = firsts[c], m = firsts[c + 1] - j0;
        FNX_TRY(png_compress_chunk(ctx, m, imgs.data() + j0, at.data() + j0, base, outs, caps, nbytes, kinds, status, first));
    }
    return FNX_OK;
}

bool is_png_file(const uint8_t *data, size_t n)
{
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    return n >= 8 && std::memcmp(data, sig, 8) == 0;
}

}  // namespace

extern "C" {

int fnx_png_compress_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, const int *sstrides, const int *ws, const int *hs, uint8_t *const *outs,
                           const size_t *caps, size_t *nbytes, int *kinds, int *status)
{
    FNX_REQUIRE(n >= 1 && n <= FNX_BATCH_MAX, "compress batch: n must be 1..FNX_BATCH_MAX (65535)");
    FNX_REQUIRE(srcs && sstrides && ws && hs && outs && caps && nbytes && kinds && status, "compress batch: NULL array");
    FNX_ENTER(ctx);
    FNX_REQUIRE(ctx->res_count == 0, "enqueued batches are waiting for fnx_results_fetch: fetch them before a blocking batch call");
    FirstRefusal first;
    FNX_TRY(png_compress_items(ctx, 0, n, srcs, sstrides, ws, hs, outs, caps, nbytes, kinds, status, nullptr, &first));
    if (first.index >= 0) set_error("%s", first.text);
    return FNX_OK;
}

// CompressBatch's item body for n files that end as PNG: the files of a span -- as many as decode into
// FNX_PNG_COMPRESS_CHUNK_BYTES of tight images in SLOT_PNG_CB_IMG, at least one -- go through fnx_png_decode_batch's chunk path
// (the PNG ones) and fnx_jpeg_decode_batch's (the others), then the images that decoded through the compress batch.
int fnx_png_recompress_batch(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes, int workers, uint8_t *const *outs,
                             const size_t *caps, size_t *nbytes, int *kinds, int *ws, int *hs, int *status)
{
    FNX_REQUIRE(n >= 1 && n <= FNX_BATCH_MAX, "recompress batch: n must be 1..FNX_BATCH_MAX (65535)");
    FNX_REQUIRE(files && sizes && outs && caps && nbytes && kinds && ws && hs && status, "recompress batch: NULL array");
    FNX_REQUIRE(workers >= 0 && workers <= 64, "recompress batch: workers must be 0..64 (0: min(8, files in the chunk))");
    FNX_ENTER(ctx);
    FNX_REQUIRE(ctx->res_count == 0, "enqueued batches are waiting for fnx_results_fetch: fetch them before a blocking batch call");
    FirstRefusal first;
    std::vector<size_t> off;
    std::vector<char> png;
    for (int s0 = 0; s0 < n;) {
        // the span: the dimensions from the headers alone (a file whose header does not parse gets no room; its decoder answers)
        int s1 = s0;
        size_t total = 0;
        off.clear();
        png.clear();
        for (; s1 < n; s1++) {
            int w = 0, h = 0;
            const bool isp = files[s1] && is_png_file(files[s1], sizes[s1]);
            if (isp) {
                PngFile head;
                if (png_probe(files[s1], sizes[s1], &head, ctx->png_adam7 != 0) == FNX_OK) { w = head.w; h = head.h; }
            } else if (files[s1]) {
                JpegFile f;
                if (jpeg_parse(files[s1], sizes[s1], &f) >= 0) { w = f.w; h = f.h; }
            }
            const size_t b = (static_cast<size_t>(w) * h * 4 + 16 + 255) & ~size_t(255);
            if (s1 > s0 && total + b > FNX_PNG_COMPRESS_CHUNK_BYTES) break;
            off.push_back(total);
            png.push_back(isp ? 1 : 0);
            total += b;
            ws[s1] = w; hs[s1] = h;
        }
        const int m = s1 - s0;
        void *t = nullptr;
        const int src = scratch(ctx, SLOT_PNG_CB_IMG, total, &t);
        if (src == FNX_ERR_OOM && m == 1) {
            // one file whose header asks for more than the device has (the span's first file is exempt from the byte cap): that
            // item's refusal, not the call's -- the other spans go on
            status[s0] = FNX_ERR_OOM;
            nbytes[s0] = 0;
            kinds[s0] = 0;
            first.note(s0);
            s0 = s1;
            continue;
        }
        FNX_TRY(src);
        // the two decoders, each over its own files of the span in the span's order
        std::vector<uint8_t *> dst(m, nullptr);
        std::vector<int> dstride(m, 0);
        for (int j = 0; j < m; j++) {
            nbytes[s0 + j] = 0;
            kinds[s0 + j] = 0;
            if (ws[s0 + j] <= 0) continue;
            dst[j] = static_cast<uint8_t *>(t) + off[j];
            dstride[j] = ws[s0 + j] * 4;
        }
        for (int pass = 0; pass < 2; pass++) {
            std::vector<int> idx;
            for (int j = 0; j < m; j++) {
                if ((png[j] != 0) == (pass == 0)) idx.push_back(j);
            }
            if (idx.empty()) continue;
            const int k = static_cast<int>(idx.size());
            std::vector<const uint8_t *> f(k);
            std::vector<size_t> fs(k);
            std::vector<uint8_t *> d(k);
            std::vector<int> dstr(k), w(k), h(k), st(k);
            for (int q = 0; q < k; q++) { f[q] = files[s0 + idx[q]]; fs[q] = sizes[s0 + idx[q]]; d[q] = dst[idx[q]]; dstr[q] = dstride[idx[q]]; }
            if (pass == 0) {
                FirstRefusal sub;
                FNX_TRY(png_decode_batch_device(ctx, k, f.data(), fs.data(), d.data(), dstr.data(), workers, w.data(), h.data(), st.data(), &sub));
                if (sub.index >= 0 && (first.index < 0 || s0 + idx[sub.index] < first.index)) {
                    first.index = s0 + idx[sub.index];
                    std::snprintf(first.text, sizeof first.text, "%s", sub.text);
                }
            } else {
                FNX_TRY(jpeg_decode_batch_device(ctx, k, f.data(), fs.data(), d.data(), dstr.data(), w.data(), h.data(), st.data()));
            }
            for (int q = 0; q < k; q++) { ws[s0 + idx[q]] = w[q]; hs[s0 + idx[q]] = h[q]; status[s0 + idx[q]] = st[q]; }
        }
        std::vector<char> skip(m);
        std::vector<const uint8_t *> srcs(m);
        for (int j = 0; j < m; j++) {
            skip[j] = status[s0 + j] != FNX_OK;
            srcs[j] = dst[j];
        }
        FNX_TRY(png_compress_items(ctx, s0, m, srcs.data(), dstride.data(), ws + s0, hs + s0, outs + s0, caps + s0, nbytes + s0, kinds + s0, status + s0,
                                   skip.data(), &first));
        s0 = s1;
    }
    if (first.index >= 0) set_error("%s", first.text);
    return FNX_OK;
}

}  // extern "C"
