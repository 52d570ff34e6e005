// fnx_png_compress_batch's host plan (see png_compress_plan.hpp) and fnx_png_file_bound.  Plain C++: no HIP call, no ctx.
#include "png_compress_plan.hpp"

#include <algorithm>

namespace fnx {

namespace {

// the arrays of an image whose rows have n raw bytes (pitch: its plane's, 0 for none), the work area aside
struct Cost {
    size_t stream, plane, tok, slot, out;
};

Cost cost(int h, size_t n, size_t pitch)
{
    Cost c;
    const size_t bytes = static_cast<size_t>(h) * (n + 1), chunks = deflate_chunks(bytes);
    c.stream = align16(bytes);
    c.plane = align16(pitch * static_cast<size_t>(h));
    c.tok = chunks * FNX_DEFLATE_CHUNK * sizeof(uint32_t);
    c.slot = chunks * (DEFLATE_SLOT_BYTES + 16) + 8;                  // the slot, the four meta words; the stream's size word
    c.out = deflate_bound(bytes);
    return c;
}

size_t plane_pitch(int w) { return (static_cast<size_t>(w) + 3) & ~size_t(3); }

}  // namespace

int png_cb_grid(int w, int h, bool tight)
{
    const long long units = tight ? (static_cast<long long>(w) * h + 3) / 4 : h;
    const long long want = tight ? (units + 255) / 256 : units;
    return static_cast<int>(std::max<long long>(1, std::min<long long>(want, PNG_CB_GRID)));
}

int png_cb_unit_rows(size_t rowbytes) { return static_cast<int>(std::max<size_t>(1, std::min<size_t>(16, 1024 / (rowbytes + 1)))); }

size_t png_cb_worst_bytes(int w, int h)
{
    const Cost c = cost(h, 4 * static_cast<size_t>(w), plane_pitch(w));
    return c.stream + c.plane + c.tok + c.slot + c.out + PNG_CB_WORK_BYTES;
}

void png_cb_split(const int *ws, const int *hs, int n, std::vector<int> *first)
{
    first->clear();
    first->push_back(0);
    size_t bytes = 0;
    int count = 0;
    for (int i = 0; i < n; i++) {
        const size_t b = png_cb_worst_bytes(ws[i], hs[i]);
        if (count > 0 && (count >= FNX_PNG_COMPRESS_CHUNK || bytes + b > FNX_PNG_COMPRESS_CHUNK_BYTES)) {
            first->push_back(i);
            bytes = 0;
            count = 0;
        }
        bytes += b;
        count++;
    }
    first->push_back(n);
}

int png_palette_depth(int ncolors) { return ncolors <= 2 ? 1 : (ncolors <= 4 ? 2 : (ncolors <= 16 ? 4 : 8)); }

size_t png_palette_chunks(int ncolors, int ntrns) { return 12 + 3 * static_cast<size_t>(ncolors) + (ntrns ? 12 + static_cast<size_t>(ntrns) : 0); }

void png_cb_plan(const int *ws, const int *hs, const PngCbClass *cls, int m, PngCbPlan *plan)
{
    *plan = PngCbPlan();
    plan->images.resize(m);
    for (int i = 0; i < m; i++) {
        PngCbImage &im = plan->images[i];
        const int w = ws[i], h = hs[i];
        im.w = w; im.h = h; im.kind = cls[i].kind;
        im.depth = 8;
        im.plane_pitch = 0;
        if (im.kind == FNX_PNG_PALETTED) {
            im.depth = png_palette_depth(cls[i].ncolors);
            im.form = im.depth == 8 ? PNG_CB_PACK8 : (im.depth == 4 ? PNG_CB_PACK4 : (im.depth == 2 ? PNG_CB_PACK2 : PNG_CB_PACK1));
            im.color_type = 3;
            im.rowbytes = static_cast<uint32_t>((static_cast<long long>(w) * im.depth + 7) / 8);
            im.plane_pitch = static_cast<uint32_t>(plane_pitch(w));
        } else if (im.kind == FNX_PNG_GRAY) {
            im.form = PNG_CB_GRAY;
            im.color_type = 0;
            im.rowbytes = static_cast<uint32_t>(w);
            im.plane_pitch = static_cast<uint32_t>(plane_pitch(w));
        } else {
            im.form = cls[i].opaque ? PNG_CB_RGB : PNG_CB_RGBA;
            im.color_type = cls[i].opaque ? 2 : 6;
            im.rowbytes = static_cast<uint32_t>(w) * (cls[i].opaque ? 3u : 4u);
        }
        const Cost c = cost(h, im.rowbytes, im.plane_pitch);
        im.stream_bytes = static_cast<size_t>(h) * (static_cast<size_t>(im.rowbytes) + 1);
        im.stream_off = plan->stream_bytes;
        im.plane_off = plan->plane_bytes;
        plan->stream_bytes += c.stream;
        plan->plane_bytes += c.plane;
        plan->tok_bytes += c.tok;
        plan->slot_bytes += c.slot;
        plan->out_bytes += c.out;

        const int per = png_cb_unit_rows(im.rowbytes);
        for (int y = 0; y < h; y += per)
            plan->rows[im.form].push_back(PngCbUnit{static_cast<uint32_t>(i), static_cast<uint32_t>(y), static_cast<uint32_t>(std::min(h, y + per))});

        im.chunk0 = static_cast<uint32_t>(plan->deflate.size());
        im.nchunks = static_cast<uint32_t>(deflate_chunks(im.stream_bytes));
        const int row = deflate_row_hint(static_cast<long long>(im.rowbytes) + 1);
        for (uint32_t k = 0; k < im.nchunks; k++) {
            PngCbDeflateUnit u;
            const size_t at = static_cast<size_t>(k) * FNX_DEFLATE_CHUNK;
            u.src_off = im.stream_off + at;
            u.len = static_cast<uint32_t>(std::min<size_t>(FNX_DEFLATE_CHUNK, im.stream_bytes - at));
            u.row = row;
            u.last = k + 1 == im.nchunks ? 1u : 0u;
            u.image = static_cast<uint32_t>(i);
            plan->deflate.push_back(u);
        }
    }
}

}  // namespace fnx

extern "C" size_t fnx_png_file_bound(int w, int h)
{
    if (w < 1 || h < 1 || w > 65535 || h > 65535) return 0;
    const size_t frame = 8 + 25 + 12 + 12;                           // signature, IHDR, IDAT's and IEND's twelve bytes
    const size_t rgba = fnx::deflate_bound(static_cast<size_t>(h) * (4 * static_cast<size_t>(w) + 1));
    const size_t paletted = fnx::png_palette_chunks(256, 256) + fnx::deflate_bound(static_cast<size_t>(h) * (static_cast<size_t>(w) + 1));
    return frame + std::max(rgba, paletted);
}
