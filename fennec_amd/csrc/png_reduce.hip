// compressPNG's pixel stages (compress.go:90-153, convert.go:76-100) on gfx950: tryPalettize's colour set and index
// plane, and toGray's plane.  Integers only; the encoder (deflate, row filters) stays with the caller.
//
//  * png_colors_kernel: ONE read of the image.  Every workgroup keeps an open-addressed set in LDS -- 64-bit slots
//    (bit 32: occupied, so that 0x00000000 and 0xFFFFFFFF are colours like any other) and, per slot, the smallest
//    row-major pixel index at which the workgroup met the colour (atomicMin; w, h <= 65535 keep it in 32 bits).  A lane
//    skips a pixel equal to the one it handled last (few-colour images are long runs) and settles a colour already in the
//    set with two plain LDS reads.  A workgroup that holds more than max_colors colours on its own raises the global
//    "over" word and leaves; every wave polls that word every few trips, so a photograph is dropped after ~1000 pixels
//    per workgroup, as the reference drops it after max_colors + 1 colours.  Workgroups that finish write their set as a
//    compact list to their OWN slice of global memory (no shared global word: analyze.hip measured ~80 ns per contended
//    device-scope atomic).
//  * png_finish_kernel, one workgroup behind a kernel boundary: merges the lists into one LDS set (same slots, minimum of
//    the first indices), counts it exactly, ranks the <= 256 survivors by first index (256 x 256 compares) and writes the
//    palette in that order plus the colour -> index table of the mapping pass.
//  * png_plane_kernel: the index plane (table in LDS, four indices per lane as one 32-bit store where the destination
//    allows) or, in gray mode, toGray's plane (R of every pixel).  The index form is launched unconditionally behind the
//    finish and returns at once when the set overflowed: the common paths take ONE synchronisation.
//
//  * png_colors_batch_kernel, png_finish_batch_kernel, png_plane_batch_kernel (fnx_png_compress_batch): the three bodies over
//    a chunk of images in one launch each -- a unit is workgroup b of the G an image gets, the finish a workgroup per image,
//    every image with its own result record -- and png_flags_batch_kernel, which makes the two flags the single route fetches
//    separately.  No scratch; VGPRs 40, 24, 25 (their twins' figures) and 20; LDS 24848, 59664, 8192 and 256 bytes.
//
// Palette order: the reference ranges over a Go map (compress.go:134), whose order is random by specification -- every
// order is a reference answer.  This one is fixed: ascending row-major index of each colour's first occurrence, what an
// insertion-ordered map gives.  It does not depend on the grid or on timing: the first index of a colour is a minimum
// over all pixels that carry it, and the rank is a function of those minima alone.
#include "common.hpp"
#include "devutil.hpp"

#include <algorithm>

namespace fnx {

constexpr int PNG_T = 256;               // lanes per workgroup of the colours and plane passes
constexpr int PNG_WG_SLOTS = 2048;       // a workgroup's set: at most max_colors + PNG_T <= 512 entries (see png_insert)
constexpr int PNG_FIN_T = 1024;          // lanes of the finish workgroup
constexpr int PNG_FIN_SLOTS = 4096;      // its set: at most max_colors + PNG_FIN_T <= 1280 entries
constexpr int PNG_MAP_SLOTS = 1024;      // colour -> index table: <= 256 entries
constexpr int PNG_LIST = 256;            // entries of a workgroup's list (a workgroup with more has raised "over")
constexpr int PNG_POLL = 8;              // trips between two looks at the "over" word
constexpr uint32_t PNG_NO_LIST = 0xffffffffu;   // a workgroup's count when it left early or overflowed
constexpr unsigned long long PNG_OCC = 1ull << 32;

// what the passes leave for the host (the first 16 bytes are zeroed before the colours pass)
struct PngResult {
    uint32_t over;                       // more than max_colors colours
    uint32_t nongray;                    // (only with over) some visible pixel with r != g or g != b was seen on the way
    uint32_t ncolors;
    uint32_t pad;
    uint32_t palette[256];               // r | g << 8 | b << 16 | a << 24, in palette order
};

__device__ __forceinline__ uint32_t png_hash(uint32_t p)
{
    // two rounds: keys that differ in one byte only, or that are all multiples of a power of two, must not share slots
    uint32_t h = p * 0x9E3779B1u;
    h ^= h >> 15;
    h *= 0x85EBCA6Bu;
    return h ^ (h >> 13);
}

// Insert (p, first index idx) into an LDS set of `slots` slots (a power of two).  `count` is the set's size, `stop`
// becomes 1 once it exceeds max_colors.  A lane looks at `stop` before every insertion and at most one insertion per lane
// is under way behind that look, so the set never holds more than max_colors + (lanes of the workgroup) entries: less
// than half of the slots in both kernels -- every probe sequence ends at a free slot.
template <int SLOTS>
__device__ __forceinline__ void png_insert(unsigned long long *keys, uint32_t *first, uint32_t *count, uint32_t *stop, int max_colors,
                                           uint32_t p, uint32_t idx)
{
    if (__atomic_load_n(stop, __ATOMIC_RELAXED)) return;
    const unsigned long long key = PNG_OCC | p;
    uint32_t slot = png_hash(p) & (SLOTS - 1);
    for (int probes = 0; probes < SLOTS; probes++) {
        // a slot only ever goes 0 -> key: a plain read that shows this key settles the colour without an atomic
        unsigned long long old = __atomic_load_n(&keys[slot], __ATOMIC_RELAXED);
        if (old == 0ull) {
            old = atomicCAS(&keys[slot], 0ull, key);
            if (old == 0ull) {
                if (atomicAdd(count, 1u) + 1u > static_cast<uint32_t>(max_colors)) __atomic_store_n(stop, 1u, __ATOMIC_RELAXED);
                old = key;
            }
        }
        if (old == key) {
            // first[] only falls: a (possibly stale) read at or below idx means the true value is too
            if (__atomic_load_n(&first[slot], __ATOMIC_RELAXED) > idx) atomicMin(&first[slot], idx);
            return;
        }
        slot = (slot + 1) & (SLOTS - 1);
    }
    __atomic_store_n(stop, 1u, __ATOMIC_RELAXED);          // (not reached: the set is never more than half full)
}

// How the passes walk a w x h image.  Tight images (stride 4w, and a tight plane) are ONE row of w h pixels shared by all
// workgroups; pitched ones go a row per workgroup.  Either way a lane meets its pixels in ascending row-major order.
struct PngWalk {
    int rows;                            // 1 (tight) or h
    uint32_t row_px;                     // pixels per row of the walk: w h or w
    int by_row;                          // workgroup b takes rows b, b + G, ...; else all take row 0, lanes strided over the grid
    int vec;                             // 16-byte loads allowed (base and stride 16-byte aligned)
};

struct PngColorsArgs {
    const uint8_t *src;
    int sstride, w;
    PngWalk walk;
    int max_colors;
    PngResult *res;
    uint32_t *counts;                    // [G]
    uint2 *lists;                        // [G][PNG_LIST]: (colour, first index)
};

// workgroup b of the G that share the image `a` describes, every lane: both colours kernels are this body
__device__ __forceinline__ void png_colors_body(const PngColorsArgs &a, const int b, const int G)
{
    __shared__ unsigned long long s_keys[PNG_WG_SLOTS];
    __shared__ uint32_t s_first[PNG_WG_SLOTS];
    __shared__ uint32_t s_count, s_stop, s_n;
    const int tid = threadIdx.x;
    for (int i = tid; i < PNG_WG_SLOTS; i += PNG_T) { s_keys[i] = 0ull; s_first[i] = 0xffffffffu; }
    if (tid == 0) { s_count = 0; s_stop = 0; s_n = 0; }
    __syncthreads();

    const PngWalk k = a.walk;
    const uint32_t upr = (k.row_px + 3u) / 4u;                       // 4-px units per row
    const uint32_t u0 = k.by_row ? tid : static_cast<uint32_t>(b) * PNG_T + tid;
    const unsigned long long ustep = k.by_row ? PNG_T : static_cast<unsigned long long>(G) * PNG_T;
    uint32_t last = 0;
    bool have_last = false, nongray = false, left = false;
    int trips = 0;
    auto load = [&](const uint8_t *row, unsigned long long u, uint32_t v[4]) {
        const uint32_t x = 4u * static_cast<uint32_t>(u);
        const uint8_t *p = row + 4 * static_cast<size_t>(x);
        const int cnt = k.row_px - x >= 4u ? 4 : static_cast<int>(k.row_px - x);
        if (k.vec && cnt == 4) {
            const u32x4 q = ld16_stream(p);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
            for (int e = 0; e < cnt; e++) v[e] = *(g_u32 *)(p + 4 * e);
        }
        return cnt;
    };
    auto take = [&](const uint32_t v[4], int cnt, uint32_t idx0) {
        for (int e = 0; e < cnt; e++) {
            const uint32_t p = v[e];
            if (have_last && p == last) continue;                     // an earlier pixel of this lane: a smaller index
            nongray |= ((p ^ (p >> 8)) & 0xffffu) != 0u;              // R == G == B: bytes 0, 1 equal bytes 1, 2
            png_insert<PNG_WG_SLOTS>(s_keys, s_first, &s_count, &s_stop, a.max_colors, p, idx0 + e);
            last = p;
            have_last = true;
        }
    };
    for (int y = k.by_row ? b : 0; y < k.rows && !left; y += k.by_row ? G : 1) {
        const uint8_t *row = a.src + static_cast<size_t>(y) * a.sstride;
        const uint32_t base = static_cast<uint32_t>(y) * static_cast<uint32_t>(a.w);
        for (unsigned long long u = u0; u < upr; u += 2 * ustep) {   // two loads in flight per lane
            uint32_t v0[4], v1[4];
            const int c0 = load(row, u, v0);
            const bool two = u + ustep < upr;
            const int c1 = two ? load(row, u + ustep, v1) : 0;
            take(v0, c0, base + 4u * static_cast<uint32_t>(u));
            take(v1, c1, base + 4u * static_cast<uint32_t>(u + ustep));
            // wave-uniform in all but a row's last trips; a lane that stays behind only reads a little longer
            uint32_t over = __atomic_load_n(&s_stop, __ATOMIC_RELAXED);
            if (++trips % PNG_POLL == 0) over |= __hip_atomic_load(&a.res->over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (__any(over != 0u)) { left = true; break; }
        }
    }
    const int any_nongray = __syncthreads_or(nongray ? 1 : 0);        // (also: every insertion of the workgroup is done)
    const bool full = s_stop != 0u;
    const bool gone = __syncthreads_or(left ? 1 : 0) != 0;
    if (full || gone) {
        // the list of a workgroup that stopped is worth nothing; one word tells the finish
        if (tid == 0) {
            a.counts[b] = PNG_NO_LIST;
            if (full && __hip_atomic_load(&a.res->over, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atomicOr(&a.res->over, 1u);
            if (any_nongray && __hip_atomic_load(&a.res->nongray, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atomicOr(&a.res->nongray, 1u);
        }
        return;
    }
    uint2 *list = a.lists + static_cast<size_t>(b) * PNG_LIST;       // s_count <= max_colors <= PNG_LIST here
    for (int i = tid; i < PNG_WG_SLOTS; i += PNG_T) {
        if (s_keys[i] != 0ull) list[atomicAdd(&s_n, 1u)] = make_uint2(static_cast<uint32_t>(s_keys[i]), s_first[i]);
    }
    if (tid == 0) a.counts[b] = s_count;
}

__global__ __launch_bounds__(PNG_T) void png_colors_kernel(PngColorsArgs a)
{
    png_colors_body(a, blockIdx.x, gridDim.x);
}

struct PngFinishArgs {
    int G, max_colors;
    const uint32_t *counts;
    const uint2 *lists;
    PngResult *res;
    unsigned long long *map;             // [PNG_MAP_SLOTS]: 0, or bit 63 | index << 32 | colour
};

__device__ __forceinline__ void png_finish_body(const PngFinishArgs &a)
{
    __shared__ unsigned long long s_keys[PNG_FIN_SLOTS];             // 32 KB
    __shared__ uint32_t s_first[PNG_FIN_SLOTS];                      // 16 KB
    __shared__ unsigned long long s_map[PNG_MAP_SLOTS];              // 8 KB
    __shared__ uint2 s_list[PNG_LIST];
    __shared__ uint32_t s_count, s_stop, s_n;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int i = tid; i < PNG_FIN_SLOTS; i += PNG_FIN_T) { s_keys[i] = 0ull; s_first[i] = 0xffffffffu; }
    for (int i = tid; i < PNG_MAP_SLOTS; i += PNG_FIN_T) s_map[i] = 0ull;
    if (tid == 0) { s_count = 0; s_stop = 0; s_n = 0; }
    int stopped = 0;
    for (int g = tid; g < a.G; g += PNG_FIN_T) stopped |= a.counts[g] == PNG_NO_LIST;
    if (__syncthreads_or(stopped)) {                                 // some workgroup overflowed on its own, or left behind one
        if (tid == 0) { a.res->over = 1u; a.res->ncolors = 0u; }
        return;
    }
    // a wave per workgroup's list, its lanes across the entries
    for (int g = wave; g < a.G; g += PNG_FIN_T / 64) {
        const int n = static_cast<int>(a.counts[g]);
        const uint2 *list = a.lists + static_cast<size_t>(g) * PNG_LIST;
        for (int i = lane; i < n; i += 64) {
            const uint2 e = list[i];
            png_insert<PNG_FIN_SLOTS>(s_keys, s_first, &s_count, &s_stop, a.max_colors, e.x, e.y);
        }
    }
    __syncthreads();
    if (s_stop != 0u) {                                              // the union holds more than max_colors
        if (tid == 0) { a.res->over = 1u; a.res->ncolors = 0u; }
        return;
    }
    for (int i = tid; i < PNG_FIN_SLOTS; i += PNG_FIN_T) {
        if (s_keys[i] != 0ull) s_list[atomicAdd(&s_n, 1u)] = make_uint2(static_cast<uint32_t>(s_keys[i]), s_first[i]);
    }
    __syncthreads();
    const int n = static_cast<int>(s_n);                             // == s_count <= max_colors <= 256
    if (tid < n) {
        // distinct colours first occur at distinct pixels: the rank is a permutation of 0 .. n-1
        const uint2 me = s_list[tid];
        uint32_t rank = 0;
        for (int j = 0; j < n; j++) rank += s_list[j].y < me.y ? 1u : 0u;
        a.res->palette[rank] = me.x;
        const unsigned long long entry = (1ull << 63) | (static_cast<unsigned long long>(rank) << 32) | me.x;
        uint32_t slot = png_hash(me.x) & (PNG_MAP_SLOTS - 1);
        while (atomicCAS(&s_map[slot], 0ull, entry) != 0ull) slot = (slot + 1) & (PNG_MAP_SLOTS - 1);   // <= 256 of 1024 slots
    }
    __syncthreads();
    for (int i = tid; i < PNG_MAP_SLOTS; i += PNG_FIN_T) a.map[i] = s_map[i];
    if (tid == 0) a.res->ncolors = static_cast<uint32_t>(n);
}

__global__ __launch_bounds__(PNG_FIN_T) void png_finish_kernel(PngFinishArgs a)
{
    png_finish_body(a);
}

struct PngPlaneArgs {
    const uint8_t *src;
    int sstride, w;
    PngWalk walk;
    int gray;                            // toGray's plane; else the index plane, unless res->over
    const PngResult *res;
    const unsigned long long *map;
    uint8_t *plane;
    int pstride;
};

__device__ __forceinline__ void png_plane_body(const PngPlaneArgs &a, const int b, const int G)
{
    __shared__ unsigned long long s_map[PNG_MAP_SLOTS];
    const int tid = threadIdx.x;
    if (!a.gray) {
        if (a.res->over != 0u) return;                               // not paletted: nothing is written
        for (int i = tid; i < PNG_MAP_SLOTS; i += PNG_T) s_map[i] = a.map[i];
        __syncthreads();
    }
    const PngWalk k = a.walk;
    const uint32_t upr = (k.row_px + 3u) / 4u;
    const uint32_t u0 = k.by_row ? tid : static_cast<uint32_t>(b) * PNG_T + tid;
    const unsigned long long ustep = k.by_row ? PNG_T : static_cast<unsigned long long>(G) * PNG_T;
    uint32_t last = 0, last_i = 0;
    bool have_last = false;
    auto index_of = [&](uint32_t p) -> uint32_t {
        if (a.gray) return p & 0xffu;                                // convert.go:96: Pix[srcOff + x*4], alpha dropped
        if (have_last && p == last) return last_i;
        uint32_t slot = png_hash(p) & (PNG_MAP_SLOTS - 1), found = 0;
        for (int probes = 0; probes < PNG_MAP_SLOTS; probes++) {     // every pixel's colour is in the table
            const unsigned long long e = s_map[slot];
            if (static_cast<uint32_t>(e) == p && (e >> 63)) { found = static_cast<uint32_t>(e >> 32) & 0xffu; break; }
            if (e == 0ull) break;
            slot = (slot + 1) & (PNG_MAP_SLOTS - 1);
        }
        last = p; last_i = found; have_last = true;
        return found;
    };
    for (int y = k.by_row ? b : 0; y < k.rows; y += k.by_row ? G : 1) {
        const uint8_t *row = a.src + static_cast<size_t>(y) * a.sstride;
        uint8_t *out = a.plane + static_cast<size_t>(y) * a.pstride;
        for (unsigned long long u = u0; u < upr; u += ustep) {
            const uint32_t x = 4u * static_cast<uint32_t>(u);
            const uint8_t *p = row + 4 * static_cast<size_t>(x);
            const int cnt = k.row_px - x >= 4u ? 4 : static_cast<int>(k.row_px - x);
            uint32_t v[4] = {0, 0, 0, 0};
            if (k.vec && cnt == 4) {
                const u32x4 q = ld16_stream(p);
                v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
            } else {
                for (int e = 0; e < cnt; e++) v[e] = *(g_u32 *)(p + 4 * e);
            }
            uint32_t i4[4];
            for (int e = 0; e < cnt; e++) i4[e] = index_of(v[e]);
            uint8_t *d = out + x;
            if (cnt == 4 && (reinterpret_cast<uintptr_t>(d) & 3u) == 0) {
                *(g_u32w *)d = i4[0] | (i4[1] << 8) | (i4[2] << 16) | (i4[3] << 24);
            } else {
                for (int e = 0; e < cnt; e++) d[e] = static_cast<uint8_t>(i4[e]);
            }
        }
    }
}

__global__ __launch_bounds__(PNG_T) void png_plane_kernel(PngPlaneArgs a)
{
    png_plane_body(a, blockIdx.x, gridDim.x);
}

// ---- the compress batch: the same passes over a chunk of images in one launch each --------------------------------------------
// A unit {image, first, end} is workgroup `first` of the `end` that share the image; the unit and the image's record come
// through the scalar cache.  Every image has its own result words, so a photograph's "over" stops its own workgroups only.
struct PngCbClassify {
    PngColorsArgs c;
    int G;                               // the image's workgroups of the colours pass = its lists
    unsigned long long *map;
};

__global__ __launch_bounds__(PNG_T) void png_colors_batch_kernel(const PngCbUnit *__restrict__ units, const PngCbClassify *__restrict__ images)
{
    const PngCbUnit u = units[blockIdx.x];
    png_colors_body(images[u.image].c, static_cast<int>(u.first), static_cast<int>(u.end));
}

__global__ __launch_bounds__(PNG_FIN_T) void png_finish_batch_kernel(const PngCbClassify *__restrict__ images)
{
    const PngCbClassify &im = images[blockIdx.x];
    PngFinishArgs a;
    a.G = im.G; a.max_colors = im.c.max_colors; a.counts = im.c.counts; a.lists = im.c.lists; a.res = im.c.res; a.map = im.map;
    png_finish_body(a);
}

// The two flags the single route fetches one by one, for rows [first, end) of an image: bit 0 -- some VISIBLE pixel with
// alpha != 255 (image.NRGBA.Opaque, png_alpha_kernel's answer); bit 1 -- some pixel of the FLAT Pix walk, row padding included,
// with r != g or g != b (isGrayscale, convert.go:76-84: every row but the last is sstride / 4 pixels long there).  OR-ed into
// the image's fourth result word, which nothing else writes.
__global__ __launch_bounds__(PNG_T) void png_flags_batch_kernel(const PngCbUnit *__restrict__ units, const PngCbClassify *__restrict__ images)
{
    const PngCbUnit u = units[blockIdx.x];
    const PngColorsArgs &a = images[u.image].c;
    const int h = a.walk.by_row ? a.walk.rows : static_cast<int>(a.walk.row_px / static_cast<uint32_t>(a.w));
    uint32_t all = 0xff000000u, mixed = 0;
    for (int y = static_cast<int>(u.first); y < static_cast<int>(u.end); y++) {
        const uint8_t *row = a.src + static_cast<size_t>(y) * a.sstride;
        const int flat = y + 1 == h ? a.w : a.sstride >> 2;
        for (int x = threadIdx.x; x < flat; x += PNG_T) {
            const uint32_t p = ld_px(row, x);
            mixed |= (p ^ (p >> 8)) & 0xffffu;
            if (x < a.w) all &= p;
        }
    }
    const int translucent = __syncthreads_or((all >> 24) != 0xffu ? 1 : 0);
    const int nongray = __syncthreads_or(mixed != 0u ? 1 : 0);
    const uint32_t bits = (translucent ? 1u : 0u) | (nongray ? 2u : 0u);
    if (bits && threadIdx.x == 0) atomicOr(&a.res->pad, bits);
}

__global__ __launch_bounds__(PNG_T) void png_plane_batch_kernel(const PngCbUnit *__restrict__ units, const PngPlaneArgs *__restrict__ images)
{
    const PngCbUnit u = units[blockIdx.x];
    png_plane_body(images[u.image], static_cast<int>(u.first), static_cast<int>(u.end));
}

namespace {

PngWalk png_walk(const uint8_t *src, int sstride, int w, int h, bool tight)
{
    PngWalk k{};
    k.rows = tight ? 1 : h;
    k.row_px = tight ? static_cast<uint32_t>(w) * static_cast<uint32_t>(h) : static_cast<uint32_t>(w);
    k.by_row = tight ? 0 : 1;
    k.vec = (reinterpret_cast<uintptr_t>(src) & 15u) == 0 && (tight || (sstride & 15) == 0) ? 1 : 0;
    return k;
}

int png_grid(const fnx_ctx *ctx, const PngWalk &k)
{
    const long long units = k.by_row ? k.rows : (static_cast<long long>(k.row_px) + 3) / 4;
    const long long want = k.by_row ? units : (units + PNG_T - 1) / PNG_T;
    return static_cast<int>(std::max<long long>(1, std::min<long long>(want, 2LL * ctx->num_cus)));
}

}  // namespace

// The colours pass, the finish and (d_plane != nullptr) the index plane of a w x h device image, w, h in 1 .. 65535.
// (Under fnx_ctx_profile every launch of the call is bracketed, in launch order: colours, finish, plane.)
// *d_result: what the caller reads back once the stream has run -- words 0 over, 1 nongray, 2 ncolors, 3 unused, then
// 256 palette words (png_result_bytes() in all).  Nothing is waited for.
size_t png_result_bytes() { return sizeof(PngResult); }

int launch_png_palettize(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, int max_colors, uint8_t *d_plane, int pstride,
                         const void **d_result)
{
    const PngWalk k = png_walk(src, sstride, w, h, sstride == 4 * w);
    const int G = png_grid(ctx, k);
    void *lp = nullptr, *wp = nullptr;
    const size_t counts_bytes = (sizeof(uint32_t) * static_cast<size_t>(G) + 15) & ~size_t(15);
    FNX_TRY(scratch(ctx, SLOT_PARTIAL, counts_bytes + sizeof(uint2) * PNG_LIST * static_cast<size_t>(G), &lp));
    FNX_TRY(scratch(ctx, SLOT_PNG, sizeof(PngResult) + sizeof(unsigned long long) * PNG_MAP_SLOTS, &wp));
    PngResult *res = static_cast<PngResult *>(wp);
    *d_result = res;
    FNX_HIP(hipMemsetAsync(res, 0, 16, ctx->stream));

    PngColorsArgs ca{};
    ca.src = src; ca.sstride = sstride; ca.w = w; ca.walk = k; ca.max_colors = max_colors; ca.res = res;
    ca.counts = static_cast<uint32_t *>(lp);
    ca.lists = reinterpret_cast<uint2 *>(static_cast<char *>(lp) + counts_bytes);
    note_route(ctx, FNX_PROF_MAIN, "png_colors_kernel");
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(png_colors_kernel, dim3(G), dim3(PNG_T), 0, ctx->stream, ca);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));

    PngFinishArgs fa{};
    fa.G = G; fa.max_colors = max_colors; fa.counts = ca.counts; fa.lists = ca.lists; fa.res = res;
    fa.map = reinterpret_cast<unsigned long long *>(res + 1);
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(png_finish_kernel, dim3(1), dim3(PNG_FIN_T), 0, ctx->stream, fa);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    if (!d_plane) return FNX_OK;
    return launch_png_plane(ctx, src, sstride, w, h, false, d_plane, pstride);
}

// gray: toGray's plane (convert.go:86-100); else tryPalettize's index plane from what the last launch_png_palettize of
// the ctx left behind (nothing is written when its colour set overflowed)
int launch_png_plane(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, bool gray, uint8_t *d_plane, int pstride)
{
    PngPlaneArgs pa{};
    pa.src = src; pa.sstride = sstride; pa.w = w;
    pa.walk = png_walk(src, sstride, w, h, sstride == 4 * w && pstride == w);
    pa.gray = gray ? 1 : 0;
    pa.res = static_cast<const PngResult *>(ctx->slot[SLOT_PNG].p);
    pa.map = reinterpret_cast<const unsigned long long *>(pa.res + 1);
    pa.plane = d_plane; pa.pstride = pstride;
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(png_plane_kernel, dim3(png_grid(ctx, pa.walk)), dim3(PNG_T), 0, ctx->stream, pa);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    return FNX_OK;
}

// ---- the compress batch's launchers ------------------------------------------------------------------------------------------
namespace {

// SLOT_PNG_CB_WORK of a chunk of m images: the m results (what the host fetches: png_result_bytes() each), the m colour ->
// index tables, then per image its counts and lists
struct CbWork {
    std::vector<int> G;
    std::vector<size_t> lists_off;
    size_t maps_off = 0, total = 0;
};

static_assert(sizeof(PngResult) + sizeof(unsigned long long) * PNG_MAP_SLOTS + PNG_CB_GRID * (sizeof(uint32_t) + sizeof(uint2) * PNG_LIST) + 16 <=
                  PNG_CB_WORK_BYTES, "the planner counts an image's share of the work area");

CbWork cb_work(int m, const PngCbSrc *imgs)
{
    CbWork k;
    k.maps_off = sizeof(PngResult) * static_cast<size_t>(m);
    k.total = k.maps_off + sizeof(unsigned long long) * PNG_MAP_SLOTS * static_cast<size_t>(m);
    for (int i = 0; i < m; i++) {
        k.G.push_back(png_cb_grid(imgs[i].w, imgs[i].h, imgs[i].sstride == 4 * imgs[i].w));
        k.lists_off.push_back(k.total);
        k.total += ((sizeof(uint32_t) * static_cast<size_t>(k.G[i]) + 15) & ~size_t(15)) + sizeof(uint2) * PNG_LIST * static_cast<size_t>(k.G[i]);
    }
    return k;
}

}  // namespace

// tryPalettize's colour set of every image of a chunk (max_colors 256) and its two flags, nothing waited for.  *d_results: m
// records of png_result_bytes() -- words 0 over, 2 ncolors, 3 the flags (bit 0: a visible pixel is translucent, bit 1: the flat
// walk met a non-grey pixel), then the palette; word 1 is the single route's shortcut and means nothing here.
int launch_png_classify_batch(fnx_ctx *ctx, int m, const PngCbSrc *imgs, const void **d_results)
{
    const CbWork k = cb_work(m, imgs);
    void *wp = nullptr;
    FNX_TRY(scratch(ctx, SLOT_PNG_CB_WORK, k.total + 16, &wp));
    uint8_t *base = static_cast<uint8_t *>(wp);
    std::vector<PngCbClassify> tab(m);
    std::vector<PngCbUnit> cu, fu;
    for (int i = 0; i < m; i++) {
        const PngCbSrc &im = imgs[i];
        PngCbClassify &t = tab[i];
        std::memset(&t, 0, sizeof t);
        t.c.src = im.src; t.c.sstride = im.sstride; t.c.w = im.w;
        t.c.walk = png_walk(im.src, im.sstride, im.w, im.h, im.sstride == 4 * im.w);
        t.c.max_colors = 256;
        t.c.res = reinterpret_cast<PngResult *>(base) + i;
        t.c.counts = reinterpret_cast<uint32_t *>(base + k.lists_off[i]);
        t.c.lists = reinterpret_cast<uint2 *>(base + k.lists_off[i] + ((sizeof(uint32_t) * static_cast<size_t>(k.G[i]) + 15) & ~size_t(15)));
        t.G = k.G[i];
        t.map = reinterpret_cast<unsigned long long *>(base + k.maps_off) + static_cast<size_t>(PNG_MAP_SLOTS) * i;
        for (int b = 0; b < k.G[i]; b++) cu.push_back(PngCbUnit{static_cast<uint32_t>(i), static_cast<uint32_t>(b), static_cast<uint32_t>(k.G[i])});
        const int per = png_cb_unit_rows(4 * static_cast<size_t>(im.w));
        for (int y = 0; y < im.h; y += per)
            fu.push_back(PngCbUnit{static_cast<uint32_t>(i), static_cast<uint32_t>(y), static_cast<uint32_t>(std::min(im.h, y + per))});
    }
    const void *hosts[3] = {tab.data(), cu.data(), fu.data()};
    const size_t sizes[3] = {sizeof(PngCbClassify) * tab.size(), sizeof(PngCbUnit) * cu.size(), sizeof(PngCbUnit) * fu.size()};
    void *dp[3];
    FNX_TRY(upload_tables(ctx, SLOT_PNG_CB_TAB0, hosts, sizes, 3, dp));
    const PngCbClassify *d_tab = static_cast<const PngCbClassify *>(dp[0]);
    FNX_HIP(hipMemsetAsync(base, 0, sizeof(PngResult) * static_cast<size_t>(m), ctx->stream));
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(png_colors_batch_kernel, dim3(static_cast<unsigned>(cu.size())), dim3(PNG_T), 0, ctx->stream, static_cast<const PngCbUnit *>(dp[1]), d_tab);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(png_finish_batch_kernel, dim3(m), dim3(PNG_FIN_T), 0, ctx->stream, d_tab);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(png_flags_batch_kernel, dim3(static_cast<unsigned>(fu.size())), dim3(PNG_T), 0, ctx->stream, static_cast<const PngCbUnit *>(dp[2]), d_tab);
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    *d_results = base;
    return FNX_OK;
}

// The planes of the chunk's paletted (which[i] == 1: the index plane, from what launch_png_classify_batch left for the SAME
// images) and gray (2: toGray's plane) images in one launch; which[i] == 0: none.  planes[i] / pstrides[i]: DEVICE planes.
int launch_png_planes_batch(fnx_ctx *ctx, int m, const PngCbSrc *imgs, const int *which, uint8_t *const *planes, const int *pstrides)
{
    const CbWork k = cb_work(m, imgs);
    uint8_t *base = static_cast<uint8_t *>(ctx->slot[SLOT_PNG_CB_WORK].p);
    std::vector<PngPlaneArgs> tab(m);
    std::vector<PngCbUnit> pu;
    for (int i = 0; i < m; i++) {
        const PngCbSrc &im = imgs[i];
        PngPlaneArgs &t = tab[i];
        std::memset(&t, 0, sizeof t);
        if (!which[i]) continue;
        const bool tight = im.sstride == 4 * im.w && pstrides[i] == im.w;
        t.src = im.src; t.sstride = im.sstride; t.w = im.w;
        t.walk = png_walk(im.src, im.sstride, im.w, im.h, tight);
        t.gray = which[i] == 2 ? 1 : 0;
        t.res = reinterpret_cast<const PngResult *>(base) + i;
        t.map = reinterpret_cast<const unsigned long long *>(base + k.maps_off) + static_cast<size_t>(PNG_MAP_SLOTS) * i;
        t.plane = planes[i]; t.pstride = pstrides[i];
        const int G = png_cb_grid(im.w, im.h, tight);
        for (int b = 0; b < G; b++) pu.push_back(PngCbUnit{static_cast<uint32_t>(i), static_cast<uint32_t>(b), static_cast<uint32_t>(G)});
    }
    if (pu.empty()) return FNX_OK;
    const void *hosts[2] = {tab.data(), pu.data()};
    const size_t sizes[2] = {sizeof(PngPlaneArgs) * tab.size(), sizeof(PngCbUnit) * pu.size()};
    void *dp[2];
    FNX_TRY(upload_tables(ctx, SLOT_PNG_CB_TAB1, hosts, sizes, 2, dp));
    FNX_TRY(prof_begin(ctx));
    hipLaunchKernelGGL(png_plane_batch_kernel, dim3(static_cast<unsigned>(pu.size())), dim3(PNG_T), 0, ctx->stream, static_cast<const PngCbUnit *>(dp[1]),
                       static_cast<const PngPlaneArgs *>(dp[0]));
    FNX_HIP(hipGetLastError());
    FNX_TRY(prof_end(ctx));
    return FNX_OK;
}

}  // namespace fnx
