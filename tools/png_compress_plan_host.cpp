// fnx_png_compress_batch's host plan (fennec_amd/csrc/png_compress_plan.cpp) as a stand-alone program: it builds descriptor
// sets -- lists of (w, h, what classification said) --, runs the split and the planner over them and checks what the launches
// rely on: the units tile every image exactly once and in order, no two regions of an area overlap, the split into chunks is a
// function of the dimensions alone, and a chunk of more than one image stays under the byte cap whatever its images hold.
// Built from this file and png_compress_plan.cpp alone (tests/test_png_compress_plan_host.py: g++ with AddressSanitizer and
// UndefinedBehaviorSanitizer); no HIP, no GPU.  Prints one line per set and "N sets: ok", or the first failure and exits 1.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "png_compress_plan.hpp"

using namespace fnx;

namespace {

struct Item {
    int w, h;
    PngCbClass c;
};
struct Set {
    std::string name;
    std::vector<Item> items;
};

int g_failures = 0;
const char *g_set = "";

#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("FAILED %s: %s -- ", g_set, #cond);           \
            std::printf(__VA_ARGS__);                                 \
            std::printf("\n");                                        \
            g_failures++;                                             \
            return;                                                   \
        }                                                             \
    } while (0)

PngCbClass paletted(int n) { return PngCbClass{FNX_PNG_PALETTED, n, 0}; }
PngCbClass gray() { return PngCbClass{FNX_PNG_GRAY, 0, 0}; }
PngCbClass rgb() { return PngCbClass{FNX_PNG_NRGBA, 0, 1}; }
PngCbClass rgba() { return PngCbClass{FNX_PNG_NRGBA, 0, 0}; }

// the row's raw bytes, restated from include/fennec_hip.h's table above fnx_png_filter
size_t want_rowbytes(const Item &it, int *depth, int *color_type, int *form)
{
    const size_t w = static_cast<size_t>(it.w);
    *depth = 8;
    if (it.c.kind == FNX_PNG_PALETTED) {
        *depth = it.c.ncolors > 16 ? 8 : (it.c.ncolors > 4 ? 4 : (it.c.ncolors > 2 ? 2 : 1));
        *color_type = 3;
        *form = *depth == 8 ? PNG_CB_PACK8 : (*depth == 4 ? PNG_CB_PACK4 : (*depth == 2 ? PNG_CB_PACK2 : PNG_CB_PACK1));
        return (w * *depth + 7) / 8;
    }
    if (it.c.kind == FNX_PNG_GRAY) { *color_type = 0; *form = PNG_CB_GRAY; return w; }
    *color_type = it.c.opaque ? 2 : 6;
    *form = it.c.opaque ? PNG_CB_RGB : PNG_CB_RGBA;
    return w * (it.c.opaque ? 3 : 4);
}

// one chunk's plan against its images
void check_plan(const std::vector<Item> &items, size_t *total)
{
    const int m = static_cast<int>(items.size());
    std::vector<int> ws(m), hs(m);
    std::vector<PngCbClass> cls(m);
    for (int i = 0; i < m; i++) { ws[i] = items[i].w; hs[i] = items[i].h; cls[i] = items[i].c; }
    PngCbPlan plan;
    png_cb_plan(ws.data(), hs.data(), cls.data(), m, &plan);
    CHECK(static_cast<int>(plan.images.size()) == m, "%zu images", plan.images.size());

    size_t stream_end = 0, plane_end = 0, worst = 0, out = 0;
    std::vector<size_t> next_unit(PNG_CB_FORMS, 0);
    uint32_t next_chunk = 0;
    for (int i = 0; i < m; i++) {
        const PngCbImage &im = plan.images[i];
        int depth, ct, form;
        const size_t n = want_rowbytes(items[i], &depth, &ct, &form);
        CHECK(im.w == items[i].w && im.h == items[i].h && im.kind == items[i].c.kind, "image %d", i);
        CHECK(im.depth == depth && im.color_type == ct && im.form == form && im.rowbytes == n, "image %d: depth %d type %d form %d n %u", i,
              im.depth, im.color_type, im.form, im.rowbytes);
        CHECK(im.stream_bytes == static_cast<size_t>(im.h) * (n + 1), "image %d: %zu stream bytes", i, im.stream_bytes);
        // the areas: in index order, no overlap, inside the area
        CHECK(im.stream_off >= stream_end && im.stream_off % 16 == 0, "image %d: stream at %zu behind %zu", i, im.stream_off, stream_end);
        stream_end = im.stream_off + im.stream_bytes;
        CHECK(stream_end <= plan.stream_bytes, "image %d: stream ends at %zu of %zu", i, stream_end, plan.stream_bytes);
        const bool has_plane = im.kind != FNX_PNG_NRGBA;
        CHECK((im.plane_pitch != 0) == has_plane, "image %d: pitch %u", i, im.plane_pitch);
        if (has_plane) {
            CHECK(im.plane_pitch >= static_cast<uint32_t>(im.w) && im.plane_pitch % 4 == 0, "image %d: pitch %u", i, im.plane_pitch);
            CHECK(im.plane_off >= plane_end && im.plane_off % 16 == 0, "image %d: plane at %zu behind %zu", i, im.plane_off, plane_end);
            plane_end = im.plane_off + static_cast<size_t>(im.plane_pitch) * im.h;
            CHECK(plane_end <= plan.plane_bytes, "image %d: plane ends at %zu of %zu", i, plane_end, plan.plane_bytes);
        }
        // the row units of its form: its rows exactly once, in order, behind the units of the images in front
        const std::vector<PngCbUnit> &units = plan.rows[form];
        uint32_t y = 0;
        size_t &k = next_unit[form];
        while (y < static_cast<uint32_t>(im.h)) {
            CHECK(k < units.size(), "image %d: rows from %u on have no unit", i, y);
            const PngCbUnit &u = units[k];
            CHECK(u.image == static_cast<uint32_t>(i) && u.first == y && u.end > u.first && u.end <= static_cast<uint32_t>(im.h),
                  "image %d: unit %zu is {%u, %u, %u} at row %u", i, k, u.image, u.first, u.end, y);
            CHECK(static_cast<int>(u.end - u.first) <= png_cb_unit_rows(n), "image %d: a unit of %u rows", i, u.end - u.first);
            y = u.end;
            k++;
        }
        // its deflate units: its stream exactly once, in order
        CHECK(im.chunk0 == next_chunk && im.nchunks == deflate_chunks(im.stream_bytes), "image %d: chunks %u + %u", i, im.chunk0, im.nchunks);
        size_t at = 0;
        for (uint32_t c = 0; c < im.nchunks; c++) {
            CHECK(im.chunk0 + c < plan.deflate.size(), "image %d: chunk %u is missing", i, c);
            const PngCbDeflateUnit &u = plan.deflate[im.chunk0 + c];
            CHECK(u.image == static_cast<uint32_t>(i) && u.src_off == im.stream_off + at && u.len >= 1 && u.len <= FNX_DEFLATE_CHUNK,
                  "image %d: chunk %u at %zu + %u", i, c, u.src_off, u.len);
            CHECK(u.last == (c + 1 == im.nchunks ? 1u : 0u), "image %d: chunk %u last %u", i, c, u.last);
            CHECK(c + 1 == im.nchunks || u.len == FNX_DEFLATE_CHUNK, "image %d: chunk %u is short", i, c);
            CHECK(u.row == (n + 1 < FNX_DEFLATE_CHUNK ? static_cast<int>(n + 1) : 0), "image %d: row hint %d", i, u.row);
            at += u.len;
        }
        CHECK(at == im.stream_bytes, "image %d: the chunks hold %zu of %zu bytes", i, at, im.stream_bytes);
        next_chunk += im.nchunks;
        out += deflate_bound(im.stream_bytes);
        worst += png_cb_worst_bytes(im.w, im.h);
    }
    for (int f = 0; f < PNG_CB_FORMS; f++) CHECK(next_unit[f] == plan.rows[f].size(), "form %d: %zu units left over", f, plan.rows[f].size() - next_unit[f]);
    CHECK(next_chunk == plan.deflate.size(), "%zu chunks left over", plan.deflate.size() - next_chunk);
    CHECK(plan.out_bytes == out, "out %zu, the bounds add up to %zu", plan.out_bytes, out);
    CHECK(plan.tok_bytes == plan.deflate.size() * FNX_DEFLATE_CHUNK * 4, "token words: %zu bytes", plan.tok_bytes);
    CHECK(plan.slot_bytes >= plan.deflate.size() * (FNX_DEFLATE_CHUNK + 32 + 16), "slots: %zu bytes", plan.slot_bytes);
    // whatever the images hold, the plan (and the colours pass's work area) stays under what the split counted
    CHECK(plan.total() + static_cast<size_t>(m) * PNG_CB_WORK_BYTES <= worst, "the plan takes %zu bytes, the split counted %zu", plan.total(), worst);
    *total = plan.total() + static_cast<size_t>(m) * PNG_CB_WORK_BYTES;
}

void check_set(const Set &set)
{
    g_set = set.name.c_str();
    const int n = static_cast<int>(set.items.size());
    std::vector<int> ws(n), hs(n);
    for (int i = 0; i < n; i++) { ws[i] = set.items[i].w; hs[i] = set.items[i].h; }
    std::vector<int> first;
    png_cb_split(ws.data(), hs.data(), n, &first);
    CHECK(first.size() >= 2 && first.front() == 0 && first.back() == n, "split ends");
    size_t largest = 0;
    for (size_t c = 0; c + 1 < first.size(); c++) {
        const int j0 = first[c], m = first[c + 1] - j0;
        CHECK(m >= 1 && m <= FNX_PNG_COMPRESS_CHUNK, "chunk %zu holds %d images", c, m);
        size_t worst = 0;
        for (int j = j0; j < j0 + m; j++) worst += png_cb_worst_bytes(ws[j], hs[j]);
        CHECK(m == 1 || worst <= FNX_PNG_COMPRESS_CHUNK_BYTES, "chunk %zu of %d images counts %zu bytes", c, m, worst);
        // no room was left unused: the next image did not fit (or the chunk is full)
        if (c + 2 < first.size())
            CHECK(m == FNX_PNG_COMPRESS_CHUNK || worst + png_cb_worst_bytes(ws[j0 + m], hs[j0 + m]) > FNX_PNG_COMPRESS_CHUNK_BYTES, "chunk %zu ends early", c);
        // the same chunk under every classification: the set's own, all RGBA, all 1-bit paletted, all gray
        for (int variant = 0; variant < 4; variant++) {
            std::vector<Item> items(set.items.begin() + j0, set.items.begin() + j0 + m);
            for (Item &it : items) {
                if (variant == 1) it.c = rgba();
                if (variant == 2) it.c = paletted(2);
                if (variant == 3) it.c = gray();
            }
            size_t total = 0;
            const int before = g_failures;
            check_plan(items, &total);
            if (g_failures != before) return;
            CHECK(m == 1 || total <= FNX_PNG_COMPRESS_CHUNK_BYTES, "chunk %zu, variant %d: %zu bytes", c, variant, total);
            largest = total > largest ? total : largest;
        }
    }
    std::printf("%-28s %3d images, %2zu chunks, largest %zu bytes\n", set.name.c_str(), n, first.size() - 1, largest);
}

std::vector<Set> sets()
{
    std::vector<Set> s;
    // every kind and depth, alone and at the edges of the geometry
    const PngCbClass kinds[] = {rgb(), rgba(), gray(), paletted(1), paletted(2), paletted(3), paletted(4), paletted(5), paletted(16), paletted(17), paletted(200), paletted(256)};
    const char *names[] = {"rgb", "rgba", "gray", "pal1", "pal2", "pal3", "pal4", "pal5", "pal16", "pal17", "pal200", "pal256"};
    for (int k = 0; k < 12; k++) {
        Set one{std::string("kind ") + names[k], {}};
        const int dims[][2] = {{1, 1}, {1, 77}, {77, 1}, {5, 3}, {67, 7}, {260, 130}, {1031, 37}, {8, 8}, {9, 9}, {65535, 1}, {1, 65535}};
        for (const auto &d : dims) one.items.push_back(Item{d[0], d[1], kinds[k]});
        s.push_back(one);
    }
    // streams of exactly one chunk and of one chunk and a byte; of one chunk less a byte
    s.push_back(Set{"stream 32768", {Item{127, 256, gray()}}});
    s.push_back(Set{"stream 32769", {Item{32768, 1, gray()}}});
    s.push_back(Set{"stream 32767", {Item{32766, 1, gray()}}});
    s.push_back(Set{"stream 32768 + 128", {Item{127, 257, gray()}}});
    s.push_back(Set{"chunk edges among others", {Item{5, 3, rgb()}, Item{127, 256, gray()}, Item{9, 5, paletted(4)}, Item{127, 257, gray()}, Item{1031, 37, rgb()},
                                                 Item{1, 1, rgba()}}});
    // a row longer than a chunk: no row hint
    s.push_back(Set{"rows above a chunk", {Item{40000, 3, gray()}, Item{9000, 2, rgba()}, Item{65535, 2, paletted(2)}}});
    // every kind side by side
    Set mixed{"mixed", {}};
    for (int k = 0; k < 12; k++) mixed.items.push_back(Item{3 + 17 * k, 1 + 5 * k, kinds[k]});
    s.push_back(mixed);
    // widths around the packed bytes' edges, per bit depth
    for (int nc : {2, 4, 16}) {
        Set pack{"packing of " + std::to_string(nc) + " colours", {}};
        for (int w = 1; w <= 18; w++) pack.items.push_back(Item{w, 1 + w % 4, paletted(nc)});
        s.push_back(pack);
    }
    // heights and row lengths around the rows a unit takes (16 short rows, one row from 512 bytes on)
    Set unit_rows{"rows per unit", {}};
    for (int w : {1, 15, 62, 63, 64, 127, 340, 341, 511, 512, 1023, 1024})
        for (int h : {15, 16, 17, 33}) unit_rows.items.push_back(Item{w, h, (w + h) % 2 ? gray() : rgb()});
    s.push_back(unit_rows);
    s.push_back(Set{"tall and narrow", {Item{1, 40000, rgba()}, Item{2, 65535, paletted(3)}, Item{3, 33000, gray()}, Item{1, 32768, gray()}, Item{1, 16384, gray()}}});
    s.push_back(Set{"wide and short", {Item{65535, 1, rgba()}, Item{65535, 2, rgb()}, Item{40000, 1, paletted(2)}, Item{32767, 1, gray()}}});
    // chunks of the stream that end with a row, in the middle of one, one byte into one
    s.push_back(Set{"rows against chunk ends", {Item{255, 128, gray()}, Item{255, 129, gray()}, Item{85, 128, rgb()}, Item{63, 257, rgba()}, Item{8191, 4, rgba()},
                                                Item{8191, 5, rgba()}, Item{2047, 16, paletted(200)}, Item{2047, 17, paletted(200)}}});
    // 32 images of which the last one tips the bytes, and 32 that fit
    Set tip{"bytes before count", {}};
    for (int i = 0; i < 32; i++) tip.items.push_back(i == 20 ? Item{3840, 2160, rgb()} : Item{1500, 1000, rgba()});
    s.push_back(tip);
    Set screens{"512 x 512 screenshots", {}};
    for (int i = 0; i < 128; i++) screens.items.push_back(Item{512, 512, i % 3 ? paletted(16) : paletted(200)});
    s.push_back(screens);
    // more images than a chunk
    for (int n : {31, 32, 33, 64, 65, 70}) {
        Set many{"many " + std::to_string(n), {}};
        for (int i = 0; i < n; i++) many.items.push_back(Item{9 + i % 3, 5 + i % 2, kinds[i % 12]});
        s.push_back(many);
    }
    // photographs: a few per chunk by the byte cap
    Set photos{"4K photographs", {}};
    for (int i = 0; i < 9; i++) photos.items.push_back(Item{3840, 2160, i % 2 ? rgb() : rgba()});
    s.push_back(photos);
    Set between{"icons between photographs", {}};
    for (int i = 0; i < 40; i++) between.items.push_back(i % 5 == 4 ? Item{3840, 2160, rgb()} : Item{64, 64, paletted(16)});
    s.push_back(between);
    // an image whose worst case alone passes the byte cap: a chunk of its own, its neighbours in theirs
    s.push_back(Set{"one above the cap", {Item{64, 64, paletted(16)}, Item{64, 64, gray()}, Item{20000, 12000, rgba()}, Item{64, 64, rgb()}, Item{20000, 12000, paletted(200)},
                                          Item{20000, 12000, gray()}, Item{8, 8, rgba()}}});
    s.push_back(Set{"the largest image", {Item{65535, 65535, rgba()}}});
    for (int n : {1, 2}) {
        Set tiny{"tiny " + std::to_string(n), {}};
        for (int i = 0; i < n; i++) tiny.items.push_back(Item{1, 1, i ? rgba() : paletted(1)});
        s.push_back(tiny);
    }
    return s;
}

}  // namespace

int main()
{
    // the split reads nothing but the dimensions: its signature says so, and the variants above run every chunk under four
    // classifications.  The bound of a file is checked against the planner's own figures
    if (png_cb_worst_bytes(20000, 12000) <= FNX_PNG_COMPRESS_CHUNK_BYTES || png_cb_worst_bytes(3840, 2160) < (size_t(150) << 20) ||
        png_cb_worst_bytes(3840, 2160) > (size_t(300) << 20)) {
        std::printf("FAILED: the worst case of a 4K image is %zu bytes, of 20000 x 12000 %zu\n", png_cb_worst_bytes(3840, 2160), png_cb_worst_bytes(20000, 12000));
        return 1;
    }
    const std::vector<Set> all = sets();
    for (const Set &set : all) check_set(set);
    if (g_failures) {
        std::printf("%d of %zu sets FAILED\n", g_failures, all.size());
        return 1;
    }
    std::printf("%zu sets: ok\n", all.size());
    return 0;
}
