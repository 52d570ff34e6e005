// The host plan of fnx_png_compress_batch (png_compress_plan.cpp): how a list of images is cut into chunks, and what one chunk's
// launches work on once its images are classified.  Pure functions of their arguments in plain C++ -- no HIP call, no ctx --,
// so that the file builds alone (tools/png_compress_plan_host.cpp runs it under the sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "deflate_batch.hpp"

namespace fnx {

inline size_t align16(size_t v) { return (v + 15) & ~size_t(15); }

// what a workgroup of a batched kernel takes: rows [first, end) of an image of the chunk -- or, in the colours and plane passes,
// workgroup `first` of the `end` that share the image
struct PngCbUnit {
    uint32_t image, first, end;
};

// the row forms, in the order of the launches: png_filter_batch_kernel<RGB | RGBA | GRAY>, png_pack_batch_kernel<8 | 4 | 2 | 1>
enum PngCbForm { PNG_CB_RGB = 0, PNG_CB_RGBA, PNG_CB_GRAY, PNG_CB_PACK8, PNG_CB_PACK4, PNG_CB_PACK2, PNG_CB_PACK1, PNG_CB_FORMS };

// what classification said of an image: kind FNX_PNG_*; ncolors 1..256 for a paletted one; opaque 1 / 0 for FNX_PNG_NRGBA
struct PngCbClass {
    int kind, ncolors, opaque;
};

struct PngCbImage {
    int w, h, kind;
    int form;                            // PngCbForm
    int depth, color_type;               // IHDR's
    uint32_t rowbytes;                   // n: the raw bytes of a row; a row of the stream is 1 + n
    size_t stream_bytes;                 // h (1 + n)
    size_t stream_off;                   // in the chunk's stream area, a multiple of 16
    size_t plane_off;                    // in the chunk's plane area (paletted and gray images), a multiple of 16
    uint32_t plane_pitch;                // 0: no plane
    uint32_t chunk0, nchunks;            // its deflate units
};

struct PngCbDeflateUnit {
    size_t src_off;                      // in the stream area
    uint32_t len;
    int row;
    uint32_t last, image;
};

struct PngCbPlan {
    std::vector<PngCbImage> images;
    std::vector<PngCbUnit> rows[PNG_CB_FORMS];     // by form; an image's units in row order, the images in index order
    std::vector<PngCbDeflateUnit> deflate;         // the images in index order, an image's chunks in order
    size_t stream_bytes = 0, plane_bytes = 0;      // the two areas
    size_t tok_bytes = 0, slot_bytes = 0;          // deflate's token words (four bytes per chunk byte) and output slots + meta words
    size_t out_bytes = 0;                          // the sum of the streams' bounds
    size_t total() const { return stream_bytes + plane_bytes + tok_bytes + slot_bytes + out_bytes; }
};

// workgroups of the colours / plane pass of a w x h image: a function of the dimensions and of whether the image is walked as one
// tight row (stride 4w) -- at most PNG_CB_GRID
constexpr int PNG_CB_GRID = 256;
int png_cb_grid(int w, int h, bool tight);
// an image's share of the colours pass's work area at most: its result record and colour -> index table, PNG_CB_GRID lists of
// 256 (colour, first index) pairs and their counts (png_reduce.hip checks the figure against its own types)
constexpr size_t PNG_CB_WORK_BYTES = 1040 + 8192 + static_cast<size_t>(PNG_CB_GRID) * (4 + 8 * 256) + 16;
// rows a unit of the row stage (or of the flags scan) takes where a row has `rowbytes` bytes: 1 for all but short rows
int png_cb_unit_rows(size_t rowbytes);
// the device scratch an image can need at most, whatever it holds: RGBA rows, every array counted (stream, plane, colour lists
// and tables, deflate's token words, slots and meta words, the stream's bound)
size_t png_cb_worst_bytes(int w, int h);
// the chunks of a list of n images, from the dimensions alone: chunk c is images [first[c], first[c + 1]); at most
// FNX_PNG_COMPRESS_CHUNK images and FNX_PNG_COMPRESS_CHUNK_BYTES of worst-case scratch each, an image that alone passes the
// byte cap a chunk of its own
void png_cb_split(const int *ws, const int *hs, int n, std::vector<int> *first);
// one chunk of m classified images
void png_cb_plan(const int *ws, const int *hs, const PngCbClass *cls, int m, PngCbPlan *plan);
// the bit depth of a palette of ncolors entries, and the PLTE + tRNS chunks' bytes (ntrns: the alphas written, 0: no tRNS)
int png_palette_depth(int ncolors);
size_t png_palette_chunks(int ncolors, int ntrns);

}  // namespace fnx
