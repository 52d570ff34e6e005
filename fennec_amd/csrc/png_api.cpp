// The deflate entry points: fnx_deflate_bound, fnx_deflate (deflate.hip's two kernels behind the argument checks and the
// staging of the three spaces) and fnx_png_encode (png_filter.hip's row stage, then the deflate, on the device; the file's
// chunks and their CRCs on the host); and fnx_png_decode, the other direction: png_parse.cpp's host side (chunk walk, inflate,
// the filter bytes), then png_decode.hip's two kernels.
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

    // the file: signature, IHDR, PLTE + tRNS for colour type 3, one IDAT, IEND
    int ntrns = 0;
    if (color_type == 3) {
        for (int i = 0; i < ncolors; i++) {
            if (palette[4 * i + 3] != 255) ntrns = i + 1;
        }
    }
    const size_t plte = color_type == 3 ? 12 + 3 * static_cast<size_t>(ncolors) + (ntrns ? 12 + static_cast<size_t>(ntrns) : 0) : 0;
    *nbytes = 8 + 25 + plte + 12 + static_cast<size_t>(zsize) + 12;
    if (cap < *nbytes || !out) {
        set_error("invalid argument: the PNG file needs %zu bytes of output, cap is %zu", *nbytes, cap);
        return FNX_ERR_INVALID;
    }
    if (zsize > 0x7fffffffull) {
        set_error("invalid argument: a PNG chunk holds at most 2^31 - 1 bytes");
        return FNX_ERR_INVALID;
    }
    static const uint8_t sig[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
    std::memcpy(out, sig, 8);
    uint8_t *at = out + 8;
    put_be32(at + 8, static_cast<uint32_t>(w));
    put_be32(at + 12, static_cast<uint32_t>(h));
    at[16] = static_cast<uint8_t>(bit_depth); at[17] = static_cast<uint8_t>(color_type); at[18] = 0; at[19] = 0; at[20] = 0;
    at = close_chunk(at, "IHDR", 13);
    if (color_type == 3) {
        for (int i = 0; i < ncolors; i++) std::memcpy(at + 8 + 3 * i, palette + 4 * i, 3);
        at = close_chunk(at, "PLTE", 3 * static_cast<size_t>(ncolors));
        if (ntrns) {
            for (int i = 0; i < ntrns; i++) at[8 + i] = palette[4 * i + 3];
            at = close_chunk(at, "tRNS", static_cast<size_t>(ntrns));
        }
    }
    FNX_HIP(hipMemcpyAsync(at + 8, dz, static_cast<size_t>(zsize), hipMemcpyDeviceToHost, ctx->stream));
    FNX_HIP(hipStreamSynchronize(ctx->stream));
    at = close_chunk(at, "IDAT", static_cast<size_t>(zsize));
    close_chunk(at, "IEND", 0);
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
        FNX_TRY(png_parse(data, n, &f));         // host work, no ctx needed
        *w = f.w; *h = f.h;
        return FNX_OK;
    }
    FNX_ENTER(ctx);
    FNX_TRY(png_parse(data, n, &f));
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
    FNX_TRY(png_row_plan(stream, f, &units));    // a filter type above 4 is refused here: nothing has been launched
    DevOut d;
    FNX_TRY(stage_out(ctx, space, dst, dstride, f.w, f.h, SLOT_OUT, &d));
    void *ds = nullptr, *dr = nullptr;
    FNX_TRY(scratch(ctx, SLOT_PNG_DEC_STREAM, want + 64, &ds));            // the kernel's 16-byte loads reach up to 15 bytes past a row
    FNX_TRY(scratch(ctx, SLOT_PNG_DEC_ROWS, png_plane_pitch(f) * f.h + 16, &dr));
    FNX_HIP(hipMemcpyAsync(ds, stream, want, hipMemcpyHostToDevice, ctx->stream));
    uint32_t table[256];
    std::memset(table, 0, sizeof table);
    if (f.color_type == 3) png_palette_table(f, table);
    const void *hosts[2] = {units.data(), table};
    const size_t sizes[2] = {sizeof(uint32_t) * units.size(), sizeof table};
    void *dp[2];
    FNX_TRY(upload_tables(ctx, SLOT_PNG_DEC_TAB, hosts, sizes, 2, dp));
    FNX_TRY(launch_png_unfilter(ctx, static_cast<const uint8_t *>(ds), f, static_cast<const uint32_t *>(dp[0]), static_cast<int>(units.size() / 2),
                                static_cast<uint8_t *>(dr)));
    FNX_TRY(launch_png_expand(ctx, static_cast<const uint8_t *>(dr), f, static_cast<const uint32_t *>(dp[1]), d.p, d.stride));
    return finish(ctx, space, &d);
}

}  // extern "C"
