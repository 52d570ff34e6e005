// The PNG entry points.  Towards a file: fnx_png_reduce (png_reduce.hip: compressPNG's pixel stages), fnx_png_filter
// (png_filter.hip's row stage), fnx_deflate_bound and fnx_deflate (deflate.hip's two kernels behind the argument checks and the
// staging of the three spaces), fnx_png_encode (the row stage, then the deflate, on the device; the file's chunks and their
// CRCs on the host: png_frame.cpp -- the IDAT chunk's from crc32.hip's kernels on a ctx at FNX_PNG_CRC_DEVICE), fnx_crc32
// (those kernels on any bytes).  From a file: fnx_png_decode -- png_parse.cpp's host side (chunk walk, inflate, the filter
// bytes), then png_decode.hip's two kernels (an Adam7 file on a ctx that accepts it: a descriptor per pass, the batched
// unfilter kernel once, png_expand_adam7_kernel) -- and fnx_png_decode_batch, which does the host side of a chunk of files
// on several threads and sends the chunk through one set of launches.  Both ways: fnx_png_compress_batch /
// fnx_png_recompress_batch, compressPNG for a list of resident images (or of files) with one set of launches and three host
// waits per chunk.
#include "common.hpp"

#include <algorithm>

using namespace fnx;

namespace {

// ---- fnx_png_decode_batch ---------------------------------------------------------------------------------------------------
// the device scratch (inflated streams + reconstructed planes) a chunk may ask for; a file that alone needs more is a chunk of one
constexpr size_t PNG_BATCH_SCRATCH = FNX_PNG_DECODE_CHUNK_BYTES;

struct BatchEntry {              // a file of the chunk in hand
    int index = 0;               // in the caller's arrays
    size_t stream_off = 0;       // in the staging area and in SLOT_PNG_DEC_STREAM alike: 16-byte aligned, want + 64 bytes
    size_t rows_off = 0;         // in SLOT_PNG_DEC_ROWS
};

// the batch's answer for its error text: the message of the lowest-indexed refused item
struct FirstRefusal {
    int index = -1;
    char text[512] = "";
    void take(int i, const char *msg)
    {
        if (index >= 0 && index < i) return;
        index = i;
        std::snprintf(text, sizeof text, "%s", msg);
    }
    void note(int i) { take(i, fnx_last_error()); }     // item i was refused just now: its message is this thread's last error
    // a sub-batch's first refusal, where the sub-batch's item k is this batch's item base + at[k]
    void merge(const FirstRefusal &sub, int base, const int *at)
    {
        if (sub.index >= 0) take(base + at[sub.index], sub.text);
    }
    int publish() const          // the batch call's last word: the first refusal's text is its error text
    {
        if (index >= 0) set_error("%s", text);
        return FNX_OK;
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
    // non-interlaced files' (png_expand_batch_kernel searches descriptors [0, nplain) alone)
    std::vector<int> ok;
    size_t npal = 0, nunit = 0;
    uint32_t nplain = 0, npass = 0;
    for (int j = 0; j < m; j++) {
        const int i = chunk[j].index;
        status[i] = items[j].status;
        if (items[j].status != FNX_OK) {
            png_reissue(items[j]);
            first->note(i);
            continue;
        }
        const PngFile &f = items[j].f;
        if (f.interlace != 1) nplain++;
        else for (int p = 0; p < 7; p++) npass += f.ph[p] != 0;
        nunit += items[j].units.size() / 2;
        if (f.color_type == 3) npal++;
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

    // the tables: the units sorted by bpp, the descriptors, a palette's 256 pixel values per paletted file.  The descriptors
    // hold pointers into the table slot itself, so its address is asked for first (same size: the same buffer)
    std::vector<uint32_t> pals(256 * (npal ? npal : 1), 0);
    const size_t na = ok.size() - nplain;
    const size_t tsizes[4] = {sizeof(PngBatchUnit) * nunit, sizeof(PngBatchFile) * (nplain + npass), sizeof(uint32_t) * pals.size(),
                              sizeof(PngAdam7File) * na};
    void *tab = nullptr;
    FNX_TRY(scratch(ctx, SLOT_PNG_DEC_TAB, align16(tsizes[0]) + align16(tsizes[1]) + align16(tsizes[2]) + align16(tsizes[3]), &tab));
    const uint32_t *d_pals = reinterpret_cast<const uint32_t *>(static_cast<uint8_t *>(tab) + align16(tsizes[0]) + align16(tsizes[1]));
    unsigned long long tiles = 0, atiles = 0;
    size_t pal = 0;
    std::vector<PngBatchFile> desc(nplain + npass);
    std::vector<PngAdam7File> adesc;
    std::vector<PngBatchUnit> units[6];
    size_t plain_at = 0, pass_at = nplain;
    for (int j : ok) {
        const PngFile &f = items[j].f;
        const int i = chunk[j].index;
        int k = 0;
        while (k < 5 && PNG_BPPS[k] != f.bpp) k++;
        const uint32_t *table = d_pals;
        if (f.color_type == 3) {
            std::memcpy(pals.data() + 256 * pal, items[j].table, sizeof items[j].table);
            table = d_pals + 256 * pal++;
        }
        const uint8_t *stream = static_cast<const uint8_t *>(ds) + chunk[j].stream_off;
        uint8_t *rows = static_cast<uint8_t *>(dr) + chunk[j].rows_off;
        const unsigned long long ftiles = static_cast<unsigned long long>((f.w + 255) / 256) * f.h;
        if (f.interlace == 1) {
            PngAdam7File a;
            std::memset(&a, 0, sizeof a);
            a.e = png_expand_of(f); a.table = table; a.dst = dsts[i]; a.dstride = dstrides[i];
            a.tile0 = static_cast<uint32_t>(atiles);
            atiles += ftiles;
            uint32_t slot[7];
            pass_at += png_adam7_passes(f, stream, rows, static_cast<uint32_t>(pass_at), desc.data() + pass_at, &a, slot);
            for (size_t u = 0; u + 1 < items[j].units.size(); u += 2)
                units[k].push_back(PngBatchUnit{slot[items[j].unit_pass[u / 2]], items[j].units[u], items[j].units[u + 1]});
            adesc.push_back(a);
            continue;
        }
        for (size_t u = 0; u + 1 < items[j].units.size(); u += 2)
            units[k].push_back(PngBatchUnit{static_cast<uint32_t>(plain_at), items[j].units[u], items[j].units[u + 1]});
        PngBatchFile d;
        std::memset(&d, 0, sizeof d);
        d.e = png_expand_of(f); d.table = table; d.dst = dsts[i]; d.dstride = dstrides[i];
        d.stream = stream;
        d.spitch = 1 + f.rowbytes;
        d.rows = rows;
        d.ppitch = png_plane_pitch(f);
        d.rowbytes = static_cast<int>(f.rowbytes);
        d.npix = static_cast<int>(f.rowbytes / f.bpp);
        d.tile0 = static_cast<uint32_t>(tiles);
        tiles += ftiles;
        desc[plain_at++] = d;
    }
    std::vector<PngBatchUnit> sorted;
    int nunits[6];
    for (int k = 0; k < 6; k++) {
        nunits[k] = static_cast<int>(units[k].size());
        sorted.insert(sorted.end(), units[k].begin(), units[k].end());
    }
    if (tiles > 0x7fffffffull || atiles > 0x7fffffffull) {
        set_error("internal: a chunk of %llu workgroups of png_expand_batch_kernel", tiles > atiles ? tiles : atiles);
        return FNX_ERR_INVALID;
    }
    if (plain_at != nplain || pass_at != nplain + npass || adesc.size() != na || sorted.size() != nunit) {
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

// ---- compressPNG's pixel stages: tryPalettize, isGrayscale + toGray (compress.go:90-153, convert.go:76-100) ----------
int png_reduce_device(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, int max_colors, uint8_t *d_plane, int pstride,
                      int *kind, uint8_t *palette, int *ncolors)
{
    const void *dres = nullptr;
    FNX_TRY(launch_png_palettize(ctx, src, sstride, w, h, max_colors, d_plane, pstride, &dres));
    std::vector<uint32_t> res(png_result_bytes() / sizeof(uint32_t));
    FNX_TRY(fetch_bytes(ctx, dres, res.data(), png_result_bytes()));
    *ncolors = 0;
    if (!res[0]) {                                                   // compress.go:92-96
        *kind = FNX_PNG_PALETTED;
        *ncolors = static_cast<int>(res[2]);
        std::memcpy(palette, &res[4], sizeof(uint32_t) * res[2]);    // r, g, b, a: the words' bytes in memory order
        if (d_plane) note_route(ctx, FNX_PROF_MAIN, "png_plane_kernel");
        return FNX_OK;
    }
    // compress.go:98: isGrayscale walks the flat Pix, row padding included.  A non-grey VISIBLE pixel met by the colours
    // pass already answers it (every photograph); otherwise the flat scan decides.
    bool gray = false;
    if (!res[1]) {
        void *df = nullptr;
        FNX_TRY(scratch(ctx, SLOT_RESULT, 16, &df));
        FNX_TRY(launch_scan_flags(ctx, src, static_cast<size_t>(h - 1) * sstride + static_cast<size_t>(w) * 4, static_cast<uint32_t *>(df)));
        uint32_t flags = 0;
        FNX_TRY(fetch_bytes(ctx, df, &flags, sizeof(flags)));
        gray = !(flags & 2u);
    }
    *kind = gray ? FNX_PNG_GRAY : FNX_PNG_NRGBA;
    if (gray && d_plane) {                                           // compress.go:99-103: toGray
        FNX_TRY(launch_png_plane(ctx, src, sstride, w, h, true, d_plane, pstride));
        note_route(ctx, FNX_PROF_MAIN, "png_plane_kernel");
    }
    return FNX_OK;
}

// ---- the PNG encoder's row stage: pack, five filters, smallest sum (compress.go:94-107, targetsize.go:189, 342) -------
int png_filter_device(fnx_ctx *ctx, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque, bool out_on_device,
                      uint8_t *out, size_t cap, size_t *nbytes, int *color_type, int *bit_depth)
{
    int form = PNG_ROW_GRAY, depth = 8;
    if (kind == FNX_PNG_PALETTED) {
        form = PNG_ROW_PALETTED;
        depth = png_palette_depth(ncolors);
        *color_type = 3;
    } else if (kind == FNX_PNG_GRAY) {
        *color_type = 0;
    } else {
        if (opaque < 0) {                                            // image.NRGBA.Opaque(): visible pixels only
            void *df = nullptr;
            FNX_TRY(scratch(ctx, SLOT_RESULT, 16, &df));
            FNX_TRY(launch_png_alpha(ctx, src, sstride, w, h, static_cast<uint32_t *>(df)));
            uint32_t translucent = 0;
            FNX_TRY(fetch_bytes(ctx, df, &translucent, sizeof(translucent)));
            opaque = translucent ? 0 : 1;
        }
        form = opaque ? PNG_ROW_RGB : PNG_ROW_RGBA;
        *color_type = opaque ? 2 : 6;
    }
    *bit_depth = depth;
    *nbytes = static_cast<size_t>(h) * (static_cast<size_t>(png_row_bytes(form, w, depth)) + 1);
    if (cap < *nbytes || !out) {
        set_error("invalid argument: the PNG stream needs %zu bytes of output, cap is %zu", *nbytes, cap);
        return FNX_ERR_INVALID;
    }
    uint8_t *d_out = out;
    if (!out_on_device) {
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_PNG_STREAM, *nbytes + 16, &t));
        d_out = static_cast<uint8_t *>(t);
    }
    FNX_TRY(launch_png_filter(ctx, form, src, sstride, w, h, depth, d_out));
    if (!out_on_device) {
        FNX_HIP(hipMemcpyAsync(out, d_out, *nbytes, hipMemcpyDeviceToHost, ctx->stream));
        FNX_HIP(hipStreamSynchronize(ctx->stream));
    }
    return FNX_OK;
}

// ---- the deflate, and the file around it ---------------------------------------------------------------------------
// the zlib stream of n device bytes into d_out (device, cap bytes), its size waited for.  idat_crc (a PNG route on a ctx at
// FNX_PNG_CRC_DEVICE; else nullptr): the CRC-32 of "IDAT" and the stream, from the CRC kernels behind the gather -- their grid
// covers cap bytes, the length is the gather's size word, and the CRC word lies behind that word and comes down with it
static int deflate_into(fnx_ctx *ctx, const uint8_t *d_src, size_t n, int row, uint8_t *d_out, size_t cap, size_t *size, uint32_t *idat_crc = nullptr)
{
    const unsigned long long *d_size = nullptr;
    FNX_TRY(launch_deflate(ctx, d_src, n, row, d_out, cap, &d_size));
    if (idat_crc) {
        uint32_t *d_crc = reinterpret_cast<uint32_t *>(const_cast<unsigned long long *>(d_size) + 1);
        FNX_TRY(launch_crc32(ctx, d_out, cap, d_size, png_idat_seed(), d_crc));
        note_route(ctx, FNX_PROF_MAIN, ctx->deflate_level == FNX_DEFLATE_LEVEL_DENSE ? "deflate_dense_chunk_kernel, crc32_pieces_kernel"
                                                                                     : "deflate_chunk_kernel, crc32_pieces_kernel");
    }
    unsigned long long got[2] = {0, 0};
    FNX_TRY(fetch_bytes(ctx, d_size, got, idat_crc ? sizeof got : sizeof got[0]));
    *size = static_cast<size_t>(got[0]);
    if (idat_crc) *idat_crc = static_cast<uint32_t>(got[1]);
    return FNX_OK;
}

// the same, gathered on the device in SLOT_DEFLATE_OUT (*d_out), from where it is copied once its size is known
static int deflate_gathered(fnx_ctx *ctx, const uint8_t *d_src, size_t n, int row, uint8_t **d_out, size_t *size, uint32_t *idat_crc = nullptr)
{
    void *t = nullptr;
    const size_t cap = deflate_bound(n);
    FNX_TRY(scratch(ctx, SLOT_DEFLATE_OUT, cap + 16, &t));
    *d_out = static_cast<uint8_t *>(t);
    return deflate_into(ctx, d_src, n, row, *d_out, cap, size, idat_crc);
}

int deflate_device(fnx_ctx *ctx, const uint8_t *d_src, size_t n, int row, bool out_on_device, uint8_t *out, size_t cap, size_t *nbytes)
{
    uint8_t *d_out = out;
    if (out_on_device) FNX_TRY(deflate_into(ctx, d_src, n, row, out, cap, nbytes));
    else FNX_TRY(deflate_gathered(ctx, d_src, n, row, &d_out, nbytes));
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

// a file's row stage into SLOT_PNG_STREAM (*d_stream, *stream_bytes): room for RGBA rows when the call itself finds the opacity
static int png_rows_to_stream(fnx_ctx *ctx, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque,
                              const uint8_t **d_stream, size_t *stream_bytes, int *color_type, int *bit_depth)
{
    const size_t row_max = kind == FNX_PNG_NRGBA ? static_cast<size_t>(w) * (opaque == 1 ? 3 : 4) : static_cast<size_t>(w);
    const size_t stream_cap = static_cast<size_t>(h) * (row_max + 1);
    void *dstream = nullptr;
    FNX_TRY(scratch(ctx, SLOT_PNG_STREAM, stream_cap + 16, &dstream));
    *d_stream = static_cast<const uint8_t *>(dstream);
    return png_filter_device(ctx, kind, src, sstride, w, h, ncolors, opaque, true, static_cast<uint8_t *>(dstream), stream_cap, stream_bytes,
                             color_type, bit_depth);
}

int png_size_device(fnx_ctx *ctx, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque, const uint8_t *palette,
                    size_t *nbytes)
{
    const uint8_t *dstream = nullptr;
    size_t stream_bytes = 0;
    int color_type = 0, bit_depth = 0;
    FNX_TRY(png_rows_to_stream(ctx, kind, src, sstride, w, h, ncolors, opaque, &dstream, &stream_bytes, &color_type, &bit_depth));
    const unsigned long long *d_size = nullptr;
    FNX_TRY(launch_deflate_size(ctx, dstream, stream_bytes, static_cast<int>(stream_bytes / h), &d_size));
    unsigned long long zsize = 0;
    FNX_TRY(fetch_bytes(ctx, d_size, &zsize, sizeof(zsize)));
    const PngFrame frame{w, h, color_type, bit_depth, ncolors, palette};
    *nbytes = frame.file_bytes(static_cast<size_t>(zsize));
    return FNX_OK;
}

int png_encode_device(fnx_ctx *ctx, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque, const uint8_t *palette,
                      uint8_t *out, size_t cap, size_t *nbytes)
{
    const uint8_t *dstream = nullptr;
    size_t stream_bytes = 0, zsize = 0;
    int color_type = 0, bit_depth = 0;
    FNX_TRY(png_rows_to_stream(ctx, kind, src, sstride, w, h, ncolors, opaque, &dstream, &stream_bytes, &color_type, &bit_depth));
    uint8_t *dz = nullptr;
    const bool device_crc = ctx->png_crc == FNX_PNG_CRC_DEVICE;
    uint32_t idat_crc = 0;
    FNX_TRY(deflate_gathered(ctx, dstream, stream_bytes, static_cast<int>(stream_bytes / h), &dz, &zsize, device_crc ? &idat_crc : nullptr));

    const PngFrame frame{w, h, color_type, bit_depth, ncolors, palette};
    *nbytes = frame.file_bytes(zsize);
    if (cap < *nbytes || !out) {
        set_error("invalid argument: the PNG file needs %zu bytes of output, cap is %zu", *nbytes, cap);
        return FNX_ERR_INVALID;
    }
    if (zsize > 0x7fffffffull) {
        set_error("invalid argument: a PNG chunk holds at most 2^31 - 1 bytes");
        return FNX_ERR_INVALID;
    }
    uint8_t *at = png_frame_head(frame, out);
    FNX_HIP(hipMemcpyAsync(at + 8, dz, zsize, hipMemcpyDeviceToHost, ctx->stream));
    FNX_HIP(hipStreamSynchronize(ctx->stream));
    if (device_crc) png_frame_tail(at, zsize, idat_crc);
    else png_frame_tail(at, zsize);
    return FNX_OK;
}

}  // namespace fnx

namespace {

// the checks fnx_png_filter and fnx_png_encode make of their source and output arguments, in their order; ptrs / ptrs_text:
// the entry's own non-NULL test and what it is called; palette_ok: false where the entry needs a paletted image's palette
int check_rows_source(int space, int kind, bool ptrs, const char *ptrs_text, const uint8_t *src, int sstride, int w, int h, int ncolors,
                      bool palette_ok, int opaque, const uint8_t *out, size_t cap)
{
    FNX_TRY(check_space_io(space));
    FNX_REQUIRE(kind == FNX_PNG_PALETTED || kind == FNX_PNG_GRAY || kind == FNX_PNG_NRGBA, "kind: 1 (paletted), 2 (gray) or 3 (NRGBA)");
    FNX_REQUIRE(ptrs, ptrs_text);
    FNX_REQUIRE(out != nullptr || cap == 0, "out is null");
    FNX_REQUIRE(w >= 1 && h >= 1 && w <= 65535 && h <= 65535, "dims: 1..65535");
    FNX_REQUIRE(kind != FNX_PNG_PALETTED || (ncolors >= 1 && ncolors <= 256), "ncolors: 1..256 (image.Paletted indices are uint8)");
    FNX_REQUIRE(kind != FNX_PNG_PALETTED || palette_ok, "a paletted image needs its palette");
    FNX_REQUIRE(opaque >= -1 && opaque <= 1, "opaque: 1, 0, or -1 to decide as Opaque() does");
    if (kind == FNX_PNG_NRGBA) {
        FNX_TRY(check_img(src, sstride, w, h, "src"));
        FNX_REQUIRE(space == FNX_HOST || (reinterpret_cast<uintptr_t>(src) & 3u) == 0, "a device image is 4-byte aligned");
    } else {
        FNX_REQUIRE(sstride >= w, "plane stride");
    }
    return FNX_OK;
}

// the row stage's source on the device: a host image or plane goes into SLOT_IN_A as it lies, the caller's stride kept
// (stage_in_flat for a pixel of 1 or 4 bytes, and with FNX_DEVICE_SRC's source in place)
int stage_rows_source(fnx_ctx *ctx, int space, int kind, const uint8_t *src, int sstride, int w, int h, const uint8_t **dsrc)
{
    *dsrc = src;
    if (space != FNX_HOST) return FNX_OK;
    const size_t len = static_cast<size_t>(h - 1) * sstride + static_cast<size_t>(w) * (kind == FNX_PNG_NRGBA ? 4 : 1);
    void *d = nullptr;
    FNX_TRY(scratch(ctx, SLOT_IN_A, len + 16, &d));
    FNX_HIP(hipMemcpyAsync(d, src, len, hipMemcpyHostToDevice, ctx->stream));
    *dsrc = static_cast<const uint8_t *>(d);
    return FNX_OK;
}

}  // namespace

extern "C" {

int fnx_png_reduce(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int max_colors, int *kind, uint8_t *palette,
                   int *ncolors, uint8_t *plane, int pstride)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_REQUIRE(max_colors >= 1 && max_colors <= 256, "max_colors: 1..256 (image.Paletted indices are uint8)");
    FNX_REQUIRE(kind != nullptr && palette != nullptr && ncolors != nullptr, "kind, palette and ncolors are outputs");
    FNX_REQUIRE(w <= 65535 && h <= 65535, "dims: at most 65535 (first-occurrence indices are 32-bit)");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    if (plane) FNX_REQUIRE(pstride >= w, "plane stride");
    if (w <= 0 || h <= 0) {                                           // an empty colorMap: a palette of no colours (compress.go:116-141)
        *kind = FNX_PNG_PALETTED;
        *ncolors = 0;
        return FNX_OK;
    }
    DevImg s;
    FNX_TRY(stage_in_flat(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    uint8_t *dplane = plane;
    int dpitch = pstride;
    if (plane && space != FNX_DEVICE) {
        dpitch = (w + 3) & ~3;
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_OUT, static_cast<size_t>(dpitch) * h + 16, &t));
        dplane = static_cast<uint8_t *>(t);
    }
    FNX_TRY(png_reduce_device(ctx, s.p, s.stride, w, h, max_colors, dplane, dpitch, kind, palette, ncolors));
    if (*kind == FNX_PNG_NRGBA) return FNX_OK;                        // the plane stays as it was
    if (plane && space != FNX_DEVICE) {
        FNX_HIP(hipMemcpy2DAsync(plane, pstride, dplane, dpitch, w, h, hipMemcpyDeviceToHost, ctx->stream));
        FNX_HIP(hipStreamSynchronize(ctx->stream));
    } else if (plane && *kind == FNX_PNG_GRAY) {
        FNX_HIP(hipStreamSynchronize(ctx->stream));                   // (the gray plane was launched after the last wait)
    }
    return FNX_OK;
}

int fnx_png_filter(fnx_ctx *ctx, int space, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque, uint8_t *out,
                   size_t cap, size_t *nbytes, int *color_type, int *bit_depth)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_rows_source(space, kind, src != nullptr && nbytes != nullptr && color_type != nullptr && bit_depth != nullptr,
                              "src, nbytes, color_type and bit_depth", src, sstride, w, h, ncolors, true, opaque, out, cap));
    const uint8_t *dsrc = nullptr;
    FNX_TRY(stage_rows_source(ctx, space, kind, src, sstride, w, h, &dsrc));
    return png_filter_device(ctx, kind, dsrc, sstride, w, h, ncolors, opaque, space == FNX_DEVICE, out, cap, nbytes, color_type, bit_depth);
}

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

int fnx_crc32(fnx_ctx *ctx, int space, const uint8_t *src, size_t n, uint32_t crc, uint32_t *out)
{
    FNX_REQUIRE(ctx != nullptr, "ctx is null");
    FNX_REQUIRE(space == FNX_HOST || space == FNX_DEVICE, "space: FNX_HOST or FNX_DEVICE");
    FNX_REQUIRE(out != nullptr, "out is null");
    FNX_REQUIRE(src != nullptr || n == 0, "src is null");
    if (n == 0) {
        *out = crc;
        return FNX_OK;
    }
    FNX_ENTER(ctx);
    const uint8_t *dsrc = src;
    if (space == FNX_HOST) {
        void *d = nullptr;
        FNX_TRY(scratch(ctx, SLOT_IN_A, n + 16, &d));
        FNX_HIP(hipMemcpyAsync(d, src, n, hipMemcpyHostToDevice, ctx->stream));
        dsrc = static_cast<const uint8_t *>(d);
    }
    void *dres = nullptr;
    FNX_TRY(scratch(ctx, SLOT_RESULT, 16, &dres));
    note_route(ctx, FNX_PROF_MAIN, "crc32_pieces_kernel");
    FNX_TRY(launch_crc32(ctx, dsrc, n, nullptr, ~crc, static_cast<uint32_t *>(dres)));
    return fetch_bytes(ctx, dres, out, sizeof *out);
}

int fnx_png_encode(fnx_ctx *ctx, int space, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque,
                   const uint8_t *palette, uint8_t *out, size_t cap, size_t *nbytes)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_rows_source(space, kind, src != nullptr && nbytes != nullptr, "src and nbytes", src, sstride, w, h, ncolors, palette != nullptr,
                              opaque, out, cap));
    const uint8_t *dsrc = nullptr;
    FNX_TRY(stage_rows_source(ctx, space, kind, src, sstride, w, h, &dsrc));
    return png_encode_device(ctx, kind, dsrc, sstride, w, h, ncolors, opaque, palette, out, cap, nbytes);
}

int fnx_png_encoded_size(fnx_ctx *ctx, int space, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque,
                         const uint8_t *palette, size_t *nbytes)
{
    FNX_TRY(check_rows_source(space, kind, src != nullptr && nbytes != nullptr, "src and nbytes", src, sstride, w, h, ncolors, palette != nullptr,
                              opaque, nullptr, 0));
    FNX_ENTER(ctx);
    const uint8_t *dsrc = nullptr;
    FNX_TRY(stage_rows_source(ctx, space, kind, src, sstride, w, h, &dsrc));
    return png_size_device(ctx, kind, dsrc, sstride, w, h, ncolors, opaque, palette, nbytes);
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
        std::memset(&a, 0, sizeof a);
        a.e = png_expand_of(f);
        a.dst = d.p;
        a.dstride = d.stride;
        uint32_t slot[7];
        const int npass = png_adam7_passes(f, static_cast<const uint8_t *>(ds), static_cast<uint8_t *>(dr), 0, passes, &a, slot);
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
    return first.publish();
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
constexpr const char *PNG_CB_ROUTE_CRC =                              // on a ctx at FNX_PNG_CRC_DEVICE
    "png_colors_batch_kernel, png_finish_batch_kernel, png_flags_batch_kernel, png_plane_batch_kernel, png_filter_batch_kernel, "
    "png_pack_batch_kernel, deflate_chunk_batch_kernel, deflate_gather_batch_kernel, crc32_pieces_batch_kernel, crc32_fold_batch_kernel";
constexpr const char *PNG_CB_ROUTE_DENSE_CRC =                        // at both
    "png_colors_batch_kernel, png_finish_batch_kernel, png_flags_batch_kernel, png_plane_batch_kernel, png_filter_batch_kernel, "
    "png_pack_batch_kernel, deflate_dense_chunk_batch_kernel, deflate_gather_batch_kernel, crc32_pieces_batch_kernel, crc32_fold_batch_kernel";

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
// launches and three host waits -- the classification words, the streams' sizes (on a ctx at FNX_PNG_CRC_DEVICE: and their IDAT
// CRCs, from the CRC kernels behind the gather), the streams' bytes.  (The three fetches and
// the table uploads take their pinned bytes from the ctx's ring: where the ring grows or wraps, pinned_alloc waits for the
// stream once more -- by then the stream is idle or nearly so, but it is a wait.)
int png_compress_chunk(fnx_ctx *ctx, int m, const PngCbSrc *imgs, const int *at, int base, uint8_t *const *outs, const size_t *caps, size_t *nbytes,
                       int *kinds, int *status, FirstRefusal *first)
{
    const bool dense = ctx->deflate_level == FNX_DEFLATE_LEVEL_DENSE, device_crc = ctx->png_crc == FNX_PNG_CRC_DEVICE;
    note_route(ctx, FNX_PROF_MAIN, device_crc ? (dense ? PNG_CB_ROUTE_DENSE_CRC : PNG_CB_ROUTE_CRC) : (dense ? PNG_CB_ROUTE_DENSE : PNG_CB_ROUTE));
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
    if (device_crc) {                                                        // the CRC words lie behind the sizes
        std::vector<size_t> bounds(m);
        for (int j = 0; j < m; j++) bounds[j] = deflate_bound(plan.images[j].stream_bytes);
        FNX_TRY(launch_crc32_batch(ctx, d_out, d_sizes, bounds.data(), static_cast<uint32_t>(m), png_idat_seed(),
                                   reinterpret_cast<uint32_t *>(const_cast<unsigned long long *>(d_sizes) + m)));
    }
    FNX_TRY(png_cb_fetch(ctx, d_sizes, (sizeof(unsigned long long) + (device_crc ? sizeof(uint32_t) : 0)) * m, &pin));  // wait 2
    std::vector<unsigned long long> zsizes(m);
    std::memcpy(zsizes.data(), pin, sizeof(unsigned long long) * m);
    std::vector<uint32_t> idat_crcs(device_crc ? m : 0);
    if (device_crc) std::memcpy(idat_crcs.data(), pin + sizeof(unsigned long long) * m, sizeof(uint32_t) * m);
    size_t total = 0;
    for (int j = 0; j < m; j++) {
        if (zsizes[j] > deflate_bound(plan.images[j].stream_bytes)) {
            set_error("internal: a stream of the compress batch is longer than its bound");
            return FNX_ERR_INVALID;
        }
        total += static_cast<size_t>(zsizes[j]);
    }
    FNX_TRY(png_cb_fetch(ctx, d_out, total, &pin));                           // wait 3: the streams' own bytes, back to back

    // the files: the chunks around each stream and their CRCs (the IDAT chunk's as fnx_ctx_set_png_crc says), on this thread
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
            if (device_crc) png_frame_tail(idat, zsize, idat_crcs[j]);
            else png_frame_tail(idat, zsize);
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
    return first.publish();
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
            const bool isp = files[s1] && png_signature(files[s1], sizes[s1]);
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
                first.merge(sub, s0, idx.data());
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
    return first.publish();
}

}  // extern "C"
