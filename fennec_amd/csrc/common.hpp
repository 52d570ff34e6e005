// Internal header of libfennec_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/fennec_hip.h"
#include "blur_plan.hpp"
#include "dev_env.hpp"
#include "png_compress_plan.hpp"

namespace fnx {

void set_error(const char *fmt, ...);

// ---- what steers the library from outside (r6: VERDICT r5 item 7) ------------------------------------------------------
// A release build reads FIVE environment names, each once, all listed in include/fennec_hip.h: FENNEC_HIP_DISABLE,
// FENNEC_HIP_DEVICES (runtime.cpp: which devices), FNX_ROCTX, FNX_POOL_TRACE, FNX_JPEG_TRACE (tracing; no effect on results
// or on which kernel runs).  Everything else:
//   * kernel FORMS the tests must be able to reach on any image (a fallback kernel that the product only takes for rare
//     tables, the two-pass twin of a fused launch ...) are a per-ctx selection, fnx_ctx_set_form (Form below) -- explicit,
//     per context, no process-wide state;
//   * development switches (tile sizes, priorities, thresholds, A/B of two correct kernels) exist in `make DEVELOP=1`
//     builds only: dev_env() (dev_env.hpp) is getenv there and a constant nullptr in a release build, so the compiler drops the branch.

enum Form {
    FORM_FX_STREAM = 0,      // "fx_stream":       "0" = effects.hip's tile kernel instead of the streaming one
    FORM_FX_PAIRS,           // "fx_pairs":        "0" = the tile kernel's one-row form
    FORM_FX_REF,             // "fx_ref":          "1" = the fp64 reference-order kernel (what tables outside the guard take)
    FORM_RESIZE_MFMA,        // "resize_mfma":     "0" never / "1" downscales (default) / "2" wherever the tables allow; read when a plan is built
    FORM_RESIZE_FP64,        // "resize_fp64":     "1" = the fp64 reference-order resize kernels (what tables outside the guard take)
    FORM_RESIZE_FUSED,       // "resize_fused":    "0" = the two-pass kernels (what windows wider than the fused tile take)
    FORM_MSSSIM_LEVELWISE,   // "msssim_levelwise":"1" = one SSIMFast + one halving per level
    FORM_MSSSIM_NOFUSE0,     // "msssim_nofuse0":  "1" = level 0's boxes and halving as two reads
    FORM_MSSSIM_FOLD,        // "msssim_fold":     "0" = a finish launch instead of the fold in the window kernel
    FORM_MSSSIM_BOXFLY,      // "msssim_boxfly":   "1" = levels 1..4's boxes taken on the fly
    FORM_PALETTE_GRID,       // "palette_grid":    "0" every image walks the whole palette / "1" every image takes the grid
    FORM_ANALYZE_STAGED,     // "analyze_staged":  "1" = analyze.hip's staged launches (what batches of more than 4096 images take) instead of the one-launch form
    FORM_RESIZE_BOX,         // "resize_box":      "1" = resize_box_kernel where its domain allows (default: the resize kernels, then the box kernel)
    FORM_JPEG_SIZE,          // "jpeg_size":       "1" = a size-only JPEG query counts the stuffed bytes from the strips, one wait (default: packed and stuffed as a file is)
    FORM_COUNT
};

#define FNX_HIP(expr)                                                                      \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess) {                                                           \
            fnx::set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, \
                           __LINE__);                                                      \
            return e__ == hipErrorOutOfMemory ? FNX_ERR_OOM : FNX_ERR_HIP;                 \
        }                                                                                  \
    } while (0)

#define FNX_TRY(expr)            \
    do {                         \
        int r__ = (expr);        \
        if (r__ < 0) return r__; \
    } while (0)

#define FNX_REQUIRE(cond, msg)                  \
    do {                                        \
        if (!(cond)) {                          \
            fnx::set_error("invalid argument: %s", msg); \
            return FNX_ERR_INVALID;             \
        }                                       \
    } while (0)

// Scratch slots of a ctx (device memory, grown on demand, reused across calls).
enum Slot {
    SLOT_IN_A = 0,   // staged host input a / src
    SLOT_IN_B,       // staged host input b
    SLOT_OUT,        // staged host output
    SLOT_TMP0,       // op intermediates (blur/resize uint8 tmp, downsampled planes ...)
    SLOT_TMP1,
    SLOT_TMP2,
    SLOT_TMP3,
    SLOT_TABLE0,     // weight tables
    SLOT_TABLE1,
    SLOT_TABLE_MFMA, // blur_mfma.hip: the weight matrices of the matrix-pipe blur
    SLOT_PARTIAL,    // reduction partials
    SLOT_RESULT,     // scalar results
    SLOT_PTRS,       // pointer arrays of batched ops
    SLOT_BOXMAP,     // source column/row -> box index tables (blur + SSIMFast in one pass)
    SLOT_SLABS,      // per-tile box partial sums of that pass (buffer 0)
    // second halves of the one-pass pipeline's double buffers, and its private plane / partial slots: its tail
    // (box_from_slabs, windowed SSIM, finish) runs on the ctx's second stream under the NEXT step's blur
    SLOT_SLABS1,
    SLOT_PLANES0,
    SLOT_PLANES1,
    SLOT_PART0,
    SLOT_PART1,
    // the JPEG quantisation round trip (jpeg.hip): unquantised planes, planes at a quality, decoded NRGBA, search reference
    SLOT_JPEG0,
    SLOT_JPEG1,
    SLOT_JPEG2,
    SLOT_JPEG3,
    SLOT_JPEG_ENC, SLOT_JPEG_ENC2, SLOT_JPEG_LUT, SLOT_JPEG_ECS,   // jpeg.hip's entropy coder
    SLOT_JPEG_FF,    // jpeg_ffcount_strips_kernel's 0xff total, zero between queries
    SLOT_JPEG_HUFF, SLOT_JPEG_HUFF_STD,   // jpeg.hip's optimised Huffman tables: the images' symbol histograms and look-up words; the standard tables for a table that takes them
    SLOT_FILE0, SLOT_FILE1, SLOT_FILE_SAMPLES,                     // host_api.cpp: fennec_CompressFileJPEG's images between its stages
    SLOT_JPEG_DEC, SLOT_JPEG_DEC_PLANES, SLOT_JPEG_DEC_IMG,        // jpeg_dec.hip: the decoder's work arrays, its planes, toNRGBARef's image
    SLOT_AN_HASH0, SLOT_AN_HASH1,   // analyze.hip: the colour-set tables of this call and the next (the launch that uses one zeroes the other)
    SLOT_TS_SCALED, SLOT_TS_UP,    // jpeg_api.cpp: fnx_jpeg_target_size's Lanczos-scaled image and its upscale back to the source's size
    SLOT_TS_PNG_PLANE, SLOT_TS_PNG_QUANT, SLOT_TS_PNG_BOX,   // the PNG legs: a level's index plane (the fallback's reduced plane), the winning level's quantized image, a scale step's box image
    SLOT_JPEG_QTAB, SLOT_JPEG_JOBS,  // fnx_jpeg_compress_batch: the quantiser tables of qualities 1..100, a search step's job list
    SLOT_RZBOX_TABLES, SLOT_RZBOX_SUMS,   // resize_box.hip: both tap tables + the box maps, the image-wide integer box sums
    SLOT_PNG,        // png_reduce.hip: the colour set's result (over, count, palette) and the colour -> index table of the plane pass
    SLOT_PNG_STREAM, // png_filter.hip: the filtered scanlines on their way to a host buffer
    SLOT_DEFLATE_TOK, SLOT_DEFLATE_SLOTS, SLOT_DEFLATE_OUT,   // deflate.hip: the chunks' tokens; the result word, the chunks' sizes and output slots; the stream on its way to a host buffer
    SLOT_DEFLATE_SIZE,   // deflate.hip's size-only form: the result word and the chunks' meta words (no slots, no stream)
    SLOT_PNG_DEC_STREAM, SLOT_PNG_DEC_ROWS, SLOT_PNG_DEC_TAB,   // png_decode.hip: the inflated stream, the reconstructed rows, the unit table + the palette's pixel values
    // fnx_png_compress_batch: the colours pass's work area (results, tables, lists), the chunk's planes, its filtered streams, the
    // unit and image tables of its four stages; fnx_png_recompress_batch: the decoded images of a span
    SLOT_PNG_CB_WORK, SLOT_PNG_CB_PLANES, SLOT_PNG_CB_STREAMS, SLOT_PNG_CB_TAB0, SLOT_PNG_CB_TAB1, SLOT_PNG_CB_TAB2, SLOT_PNG_CB_TAB3, SLOT_PNG_CB_IMG,
    SLOT_MEDIAN_CUT, SLOT_MEDIAN_CUT_TAB,   // median_cut.hip: both sample buffers and the palettes; palette.hip: apply_palette's tables made on the device from them
    SLOT_CRC, SLOT_CRC_TAB,   // crc32.hip: the pieces' words (and fnx_crc32's result word); the batch's unit and stream tables
    SLOT_DONE,       // workgroup counters of the kernels that finish their own reduction (ssim.hip), zero between launches
    SLOT_COUNT
};

struct Scratch {
    void *p = nullptr;
    size_t cap = 0;
};

// Cached copy of the last table uploaded into a table slot.
struct TableCache {
    std::vector<unsigned char> host;
    bool fresh = false;      // the last upload_tables() into this slot really uploaded (contents changed)
    int contig_taps = 0;     // resize tap tables: resize_contiguous_taps() of the cached table
};

// A CSR tap table of one resize pass (precomputeWeights, resize.go:164-197).  id != 0 marks an immutable
// table with a process-unique id (host_api.cpp's cache): plans are then looked up by id instead of content.
struct TapTable {
    const int32_t *off = nullptr, *idx = nullptr;
    const double *wt = nullptr;
    int nout = 0;
    uint64_t id = 0;
};

}  // namespace fnx

struct fnx_resize_plan;   // resize.hip: device tables of one (tap table, direction)

struct fnx_ctx {
    int device = 0;             // HIP device ordinal
    int logical_device = 0;     // its index in this library's device list (fnx_set_devices / FENNEC_HIP_DEVICES)
    hipStream_t stream = nullptr;       // where the ctx launches: its own stream, or one lent by the caller (fnx_ctx_use_stream)
    hipStream_t own_stream = nullptr;   // created with the ctx, destroyed with it
    hipEvent_t ev_switch = nullptr;
    // One-pass GaussianBlur + SSIMFast batches (api.cpp): the blur kernel of step s runs on `stream`, the
    // step's tail on `stream2`, ordered by ev_blur[p]; step s + 2 reuses buffer set p = s & 1 and waits for
    // ev_tail[p] first.  A caller that enqueues step s + 1 before fetching step s gets the tail for free.
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_blur[2] = {}, ev_tail[2] = {};
    hipEvent_t blur_done = nullptr;     // the stop event BOUND to the last one-pass blur dispatch (blur_bind_events)
    bool tail_pending[2] = {false, false};
    unsigned long long tail_gen[2] = {0, 0};   // uses of each buffer set so far
    int parity = 0;
    int ev_toggle = 0;           // fnx_ssim_enqueue alternates between the two hand-over events
    bool stream2_used = false;
    int partial_slot = -1;       // >= 0: launch_windowed_ssim takes its partial sums from this slot (one-pass tail)
    // fnx_gaussian_blur_batch with FNX_BLUR_KEEP_BOX_SUMS (api.cpp): the boxDownsample planes of the batch's sources and blurred
    // images, made by the blur's own pass, wait here for the fnx_ssim_fast_batch(_enqueue) that scores exactly these pairs --
    // the very next call on the ctx (op_seq) or nothing
    struct KeptBoxes {
        bool valid = false;
        unsigned long long seq = 0;
        int n = 0, sstride = 0, dstride = 0, w = 0, h = 0, nw = 0, nh = 0, parity = 0;
        std::vector<const uint8_t *> srcs, dsts;
        uint8_t *planes = nullptr;
        size_t plane = 0;
    } kept;
    unsigned long long op_seq = 0;     // exported calls bound to this ctx so far (bind)
    bool boxes_on_main = false;        // launch_blur_scored: box_from_slabs_kernel on `stream` instead of `stream2` (the kept form)
    fnx::Scratch slot[fnx::SLOT_COUNT];
    fnx::TableCache tcache[fnx::SLOT_COUNT];
    // pinned host ring: tables going up, scalars coming down
    unsigned char *pinned = nullptr;
    size_t pinned_cap = 0, pinned_off = 0;
    // fnx_png_decode_batch: the pinned home of a chunk's inflated streams, and the event behind the chunk's uploads -- the next
    // chunk (of this call or a later one) is inflated into the same bytes once that event has passed
    unsigned char *png_stage = nullptr;
    size_t png_stage_cap = 0;
    hipEvent_t png_stage_ev = nullptr;
    bool png_stage_busy = false;
    int num_cus = 256;
    // results of the *_enqueue calls not fetched yet, oldest first: each batch has its own pinned slots and
    // an event right behind its result kernels, so a fetch waits for THAT batch only and a caller may queue
    // the next batch before fetching this one (the stream never drains between steps)
    static constexpr int RES_DEPTH = 4;
    struct Pending {
        const double *pinned = nullptr;
        int n = 0;
        hipEvent_t ev = nullptr;
        // fnx_msssim_enqueue: the slots hold `nraw` per-level SSIMFast values and the fetch returns ONE number,
        // exp(sum weights[i] log(max(level i, 1e-10))) (ssim.go:344-352); nraw == 0: the values as they are
        int nraw = 0;
        int nimg = 1;          // fnx_msssim_batch_enqueue: that many images, five slots each, `nraw` of them written; the fetch returns nimg numbers
        double weights[5] = {0, 0, 0, 0, 0};
        int tail_parity = -1;  // one-pass batches: the buffer set (slabs, planes, partials) this batch's tail reads,
        unsigned long long tail_gen = 0;   // and which use of that set it was
    } res_q[RES_DEPTH];
    int res_head = 0, res_count = 0;
    struct ResBuf {            // pinned home of FIFO position i's results (api.cpp: result_slot_queued)
        double *p = nullptr;
        size_t cap = 0;
    } res_buf[RES_DEPTH];
    fnx::ScoreGeom score_geom;
    std::vector<fnx_resize_plan *> rplans;   // at most 8, least recently used evicted (resize.hip)
    uint32_t *rz_todo = nullptr;             // resize_mfma.hip -> resize_fused_kernel: tiles to redo, stamped with rz_gen
    size_t rz_todo_cap = 0;
    uint32_t rz_gen = 0;
    unsigned long long *rz_report = nullptr; // host-mapped: what resize_fused_sparse_kernel redid (gen << 32 | tiles)
    uint32_t rz_last_gen = 0;                // the last matrix launch whose report has not been read
    size_t rz_last_cells = 0;
    const fnx_resize_plan *rz_last_h = nullptr;
    uint32_t d21_gen = 0;                    // resize_dense21_kernel's launches (rz_report[1] holds the last one that met translucent content)
    // fnx_ctx_profile: event pairs around the profiled kernel launches, oldest unread first
    static constexpr int PROF_DEPTH = 32;
    int prof = 0;                 // bit mask of FNX_PROF_* kernel classes being bracketed (0: off)
    hipEvent_t prof_ev[PROF_DEPTH][2] = {};
    int prof_head = 0, prof_count = 0, prof_open = -1;
    // fnx_ctx_last_kernel: the kernel the last call of each class really launched (static strings), so that a report can
    // name the route the library took instead of inferring it from environment switches
    const char *route[8] = {"", "", "", "", "", "", "", ""};
    int png_adam7 = 0;           // fnx_ctx_set_png_adam7: 1 -- the PNG entries decode Adam7-interlaced files instead of refusing them
    int jpeg_huffman = 0;        // fnx_ctx_set_jpeg_huffman: FNX_JPEG_HUFFMAN_STANDARD / _OPTIMIZED -- the tables of every JPEG file (and size) this ctx makes
    int jpeg_subsampling = 0;    // fnx_ctx_set_jpeg_subsampling: FNX_JPEG_SUBSAMPLING_420 / _444 -- the single-image JPEG entries follow it, the others refuse 4:4:4
    int deflate_level = 0;       // fnx_ctx_set_deflate_level: FNX_DEFLATE_LEVEL_FAST / _DENSE -- which chunk kernels launch_deflate and launch_deflate_batch run
    int png_crc = 0;             // fnx_ctx_set_png_crc: FNX_PNG_CRC_HOST / _DEVICE -- where the IDAT CRC of this ctx's device-deflated PNG files comes from
    int ssim_mode = 0;           // fnx_ctx_set_ssim_mode: FNX_SSIM_EXACT (fp64 moments) / FNX_SSIM_FAST (fp32 moments for full-resolution planes)
    // fnx_ctx_set_form: the kernel forms this ctx was told to take ("" = the product's own choice)
    char form[fnx::FORM_COUNT][8] = {};
    // analyze.hip's single-launch form: which colour table the next call uses, and how many tables of each are not zero
    int an_cur = 0;
    int an_dirty[2] = {0, 0};
};

struct fnx_prepared {
    int w = 0, h = 0;      // original dims
    int pw = 0, ph = 0;    // dims SSIMFast compares at
    uint8_t *pix = nullptr;  // device, tight pw x ph NRGBA (downsampled or copied reference side)
};

namespace fnx {

int bind(fnx_ctx *ctx);
// the ctx's selection for a kernel form (fnx_ctx_set_form), else -- DEVELOP builds only -- the environment variable of the
// same name (FNX_ + upper case: the A/B scripts under tools/ and experiments/), else nullptr: the product's own choice
const char *form_value(const fnx_ctx *ctx, Form f);
int form_set(fnx_ctx *ctx, const char *name, const char *value);
// roctx range around an exported op (runtime.cpp: FNX_ROCTX=1 turns them on; off they cost a load and a branch)
class OpRange {
public:
    explicit OpRange(const char *name);
    ~OpRange();
    OpRange(const OpRange &) = delete;
    OpRange &operator=(const OpRange &) = delete;
private:
    bool on_;
};
#define FNX_ENTER(ctx)                  \
    fnx::OpRange fnx_op_range_(__func__); \
    FNX_TRY(bind(ctx))
// Device scratch of at least `bytes` in `slot` (contents undefined).
int scratch(fnx_ctx *ctx, Slot slot, size_t bytes, void **out);
// Pinned host bytes valid until the next fnx call on this ctx wraps the ring.
int pinned_alloc(fnx_ctx *ctx, size_t bytes, void **out);
// Upload a small host table into a table slot (skipped when identical to the cached one).
int upload_table(fnx_ctx *ctx, Slot slot, const void *host, size_t bytes, void **dptr);
// Upload several host arrays back to back into one slot (each 16-byte aligned).
int upload_tables(fnx_ctx *ctx, Slot slot, const void *const *hosts, const size_t *sizes, int n,
                  void **dptrs);

// staged / intermediate images are TIGHT (stride = 4*w), like image.NewNRGBA; 16-byte vector
// access is then available whenever w % 4 == 0 (every size the benchmarks and codecs produce).
inline int pitch16(int w) { return w * 4; }

// An input image resolved to device memory.
struct DevImg {
    const uint8_t *p = nullptr;
    int stride = 0;
};
struct DevOut {
    uint8_t *p = nullptr;
    int stride = 0;
    uint8_t *host = nullptr;  // non-null: copy back to here (hstride) at finish
    int hstride = 0, w = 0, h = 0;
};

int stage_in(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, Slot slot,
             DevImg *out);
// Same, but keeps the caller's stride and copies the flat Pix slice ((h-1)*stride + 4*w bytes):
// pixelSSIM walks the flat slice, row padding included (ssim.go:178).
int stage_in_flat(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, Slot slot,
                  DevImg *out);
// toNRGBA's copy (convert.go:12-19: copy(dst.Pix, nrgba.Pix) into a fresh tight image): the FIRST 4wh flat bytes of
// the Pix slice as a tight w x h image -- the image's rows only when its stride is 4w.  MSSSIM's pyramid starts
// from these copies (ssim.go:345-346).  Device sources are read in place with stride 4w.
int stage_in_front(fnx_ctx *ctx, int space, const uint8_t *src, int w, int h, Slot slot, DevImg *out);
int stage_out(fnx_ctx *ctx, int space, uint8_t *dst, int dstride, int w, int h, Slot slot,
              DevOut *out);
// Copy a staged output back (if host) and synchronise when `space` is host.
int finish(fnx_ctx *ctx, int space, DevOut *out);
int finish_enqueue(fnx_ctx *ctx, int space, DevOut *out);   // the copy back without the wait
// fnx_ctx_profile hooks: bracket the launch of a profiled kernel (no-ops when profiling is off)
// Events carried by ONE dispatch (hipExtLaunchKernelGGL's startEvent / stopEvent): they ride on the kernel packet's own
// completion signal, so neither costs a barrier packet on the stream.  hipEventRecord before and after a launch is two
// barrier packets, ~6-8 us each on this part: with the cross-stream hand-over event that was a 24 us bubble between
// consecutive one-pass blur launches (r3 kernel trace).  prof_bind reserves the profile FIFO's next pair when the
// class is being profiled (nulls otherwise); the launch must then really happen.
struct LaunchEvents {
    hipEvent_t start = nullptr, stop = nullptr;
};
int prof_bind(fnx_ctx *ctx, int cls, LaunchEvents *ev);
int prof_begin(fnx_ctx *ctx, int cls = FNX_PROF_MAIN);
inline void note_route(fnx_ctx *ctx, int cls, const char *kernel)      // cls: one FNX_PROF_* bit
{
    int i = 0;
    while (i < 7 && !((cls >> i) & 1)) i++;
    ctx->route[i] = kernel;
}
int prof_end(fnx_ctx *ctx);
// Fetch n doubles from device memory into host memory (synchronises).
int fetch_doubles(fnx_ctx *ctx, const double *dptr, double *host, int n);
int fetch_bytes(fnx_ctx *ctx, const void *dptr, void *host, size_t bytes);

inline bool aligned16(const void *p, int stride)
{
    return ((reinterpret_cast<uintptr_t>(p) | static_cast<uintptr_t>(stride)) & 15u) == 0;
}

// ---- api.cpp: what its entry points and jpeg_api.cpp's share ----
// argument checks: an image's pointer and stride (nothing to check when w or h <= 0); the space of an op with a scalar
// result (FNX_HOST, FNX_DEVICE) and of an image -> image op (those or FNX_DEVICE_SRC: device source, host destination)
int check_img(const void *p, int stride, int w, int h, const char *what);
int check_space(int space);
int check_space_io(int space);
// SSIMFast's dims (ssim.go:52-56): true when the w x h image is compared box-downsampled, at *nw x *nh (<= 512 px)
bool ssim_fast_dims(int w, int h, int *nw, int *nh);
// the 8 x 8 SSIM window (64 doubles, host) as the ctx's device table
int upload_window(fnx_ctx *ctx, const double *window, const double **d_window);
// n result doubles in pinned memory that the result kernels write (NaN until then), and the wait for them (-> out)
int result_slot(fnx_ctx *ctx, int n, double **d);
int result_wait(fnx_ctx *ctx, const double *pinned, double *out, int n);
// SSIMFast(prepared reference, device image b) -> *out; b_is_plane: b is already the candidate's tight pw x ph plane
int against_device(fnx_ctx *ctx, const fnx_prepared *ref, const uint8_t *b, int bstride, const double *window, double *out,
                   bool b_is_plane = false);
// the reference's own plane from the device image src into ref.pix (ref.w, ref.h, ref.pw, ref.ph as ssim_fast_dims set them)
int prepared_plane(fnx_ctx *ctx, const uint8_t *src, int sstride, const fnx_prepared &ref);

// n same-geometry w x h image pairs on the device, as the SSIM and boxDownsample launchers take them.  Image i of a side is
// ptrs[i] where ptrs (a DEVICE array) is given, else p + i * image_bytes.
struct ImgSide { const uint8_t *p = nullptr; const uint8_t *const *ptrs = nullptr; int stride = 0; size_t image_bytes = 0; };
struct ImgPairs { int n = 0, w = 0, h = 0; ImgSide a, b; };
// one pair; n pairs of tight planes, `plane` bytes apart on each side; n pairs by device pointer arrays
inline ImgPairs one_pair(const uint8_t *a, int astride, const uint8_t *b, int bstride, int w, int h) { return {1, w, h, {a, nullptr, astride, 0}, {b, nullptr, bstride, 0}}; }
inline ImgPairs plane_pairs(int n, const uint8_t *a, const uint8_t *b, size_t plane, int w, int h) { return {n, w, h, {a, nullptr, w * 4, plane}, {b, nullptr, w * 4, plane}}; }
inline ImgPairs pairs_by_pointer(int n, const uint8_t *const *d_as, int astride, const uint8_t *const *d_bs, int bstride, int w, int h)
{
    return {n, w, h, {nullptr, d_as, astride, 0}, {nullptr, d_bs, bstride, 0}};
}

// ---- kernel launchers (each enqueues on ctx->stream; device pointers only) ----
int launch_blur(fnx_ctx *ctx, int n, const uint8_t *src, const uint8_t *const *srcs, int sstride,
                int w, int h, const double *kernel, int radius, int flags, uint8_t *dst,
                uint8_t *const *dsts, int dstride);
// blur (fast, or with FNX_BLUR_EXACT the guarded bit-exact kernel) + both boxDownsample'd planes
// ([src 0..n-1][blurred 0..n-1], tight dstW x dstH) in one pass; FNX_NOOP (nothing launched) when the
// shape or the kernel is not covered.  srcs/dsts: device arrays.
int launch_blur_scored(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h,
                       const double *kernel, int radius, int flags, uint8_t *const *dsts, int dstride,
                       uint8_t *planes, size_t plane, int dstW, int dstH);
int launch_blur3x3(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, uint8_t *dst,
                   int dstride);
int launch_sharpen(fnx_ctx *ctx, bool adaptive, const uint8_t *src, int sstride, int w, int h,
                   double amount, uint8_t *dst, int dstride);
int launch_sharpen_batch(fnx_ctx *ctx, bool adaptive, int n, const uint8_t *src0, const uint8_t *const *d_srcs, int sstride, int w, int h,
                         double amount, uint8_t *dst0, uint8_t *const *d_dsts, int dstride);
// One pass of lanczosResize through the ctx's plan cache: guard-exact fp32 kernels where the table allows,
// the fp64 kernels otherwise.  vertical == false: dst is t.nout x srcH; true: dst is srcW x t.nout.
// `hint` (optional) carries the H pass's per-workgroup verdicts to the V pass of the same lanczosResize call: where
// most H waves found their rows dense with rounding-guard flags the V pass skips its fp32 form (resize.hip).
struct ResizeHint {
    uint32_t *cells = nullptr;     // device, `cap` words
    size_t cap = 0;
    int gx = 0, gy = 0, rows = 0;  // filled by the H pass
    bool valid = false;
};
int resize_pass(fnx_ctx *ctx, bool vertical, const TapTable &t, const uint8_t *src, int sstride, int srcW, int srcH,
                uint8_t *dst, int dstride, ResizeHint *hint = nullptr);
// both passes in one launch (the uint8 intermediate in LDS); FNX_NOOP when the tables are outside its reach
// nimg > 1: a batch of same-geometry images in one set of launches (blockIdx.z / .y = image); d_srcs / d_dsts are DEVICE arrays
// of their pointers (src / dst are then ignored)
int resize_fused(fnx_ctx *ctx, const TapTable &th, const TapTable &tv, const uint8_t *src, int sstride, int srcW, int srcH,
                 uint8_t *dst, int dstride, int nimg = 1, const uint8_t *const *d_srcs = nullptr, uint8_t *const *d_dsts = nullptr);
void free_resize_plans(fnx_ctx *ctx);
// resize_mfma.hip: lanczosResize on the i8 matrix pipe (opaque images, ratios up to ~2.3).  One tap table in matrix form:
struct RzMfTable {
    bool ok = false;
    int KH = 0;                    // H tables: 64-byte chunks of a group's window (1, 2)
    int NC = 0;                    // H tables: 16-byte chunks of a staged source row
    int ngroups = 0;               // H: groups of 4 outputs, 16 per 64-column strip; V: groups of 16 output rows
    int nmat = 0;                  // distinct matrices
    int S = 22;                    // fixed point of the weights: 2^22 or 2^23
    int seed = 0, thr = 0;         // rounding seed + G, 2 G (units of 2^-S)
    void *blob = nullptr;          // device: matrices | per-group records | per-strip source offsets
    const void *mats = nullptr;
    const int32_t *meta = nullptr, *sbase = nullptr;
    const void *ex = nullptr;      // per output: the operands of the fp64 fix-ups
};
bool resize_mfma_build(const fnx_ctx *ctx, const TapTable &t, int srcN, bool vertical, const double *inv, RzMfTable *out);
void resize_mfma_free(RzMfTable *t);
// Launches the matrix kernel; regions it gives up are marked todo[tile] = gen for resize_fused_kernel's tiles
// (old_tw x old_th output px, old_gx per row), which the caller launches next.
int resize_mfma_launch(fnx_ctx *ctx, const RzMfTable &h, const RzMfTable &v,
                       const uint8_t *src, int sstride, int srcW, int srcH, uint8_t *dst, int dstride, int dstW, int dstH,
                       uint32_t *todo, unsigned *gave_up, uint32_t gen, int old_tw, int old_th, int old_gx, int *workgroups,
                       int nimg = 1, const uint8_t *const *d_srcs = nullptr, uint8_t *const *d_dsts = nullptr, uint32_t todo_stride = 0);
// lanczosResize (resize.go:37-53) with both tables given: the body of fnx_lanczos_resize
int lanczos_resize_tables(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW, int srcH,
                          const TapTable &th, const TapTable &tv, uint8_t *dst, int dstride, int dstW, int dstH);
int lanczos_resize_tables_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int srcW, int srcH,
                                const TapTable &th, const TapTable &tv, uint8_t *const *dsts, int dstride, int dstW, int dstH);
// resize_box.hip: dst = boxDownsample(lanczosResize(src, midW, midH), dstW, dstH) in one pass, the midW x midH image never
// stored (device pointers); FNX_NOOP (nothing launched) for pairs outside the kernel's domain (see there)
int launch_resize_box(fnx_ctx *ctx, const uint8_t *src, int sstride, int srcW, int srcH, const TapTable &th, const TapTable &tv,
                      int midW, int midH, uint8_t *dst, int dstride, int dstW, int dstH);
bool resize_box_covers(const TapTable &th, const TapTable &tv, int srcW, int srcH, int midW, int midH, int dstW, int dstH,
                       std::vector<int32_t> *map = nullptr, int *maxbw = nullptr);
// the same for a device image: lanczosResize into `up_slot` and the box kernel, or the fused kernel where it applies and
// the ctx asks for it ("resize_box" "1")
int lanczos_box_device(fnx_ctx *ctx, const uint8_t *src, int sstride, int srcW, int srcH, const TapTable &th, const TapTable &tv,
                       int midW, int midH, uint8_t *dst, int dstride, int dstW, int dstH, Slot up_slot);
// computeSSIMNRGBA's tail (targetsize.go:563-568): SSIMFast(prepared reference, lanczosResize(b -> ref's dims)), b on the device
int ssim_fast_resized_device(fnx_ctx *ctx, const fnx_prepared *ref, const uint8_t *b, int bstride, int bw, int bh,
                             const TapTable &th, const TapTable &tv, const double *window, double *out);
// b (bw x bh in `space`) staged at its own size (SLOT_IN_B) and resized to w x h on the device into SLOT_TMP3 (ssim.go:31-33, 320-322)
int resize_b_device(fnx_ctx *ctx, int space, const uint8_t *b, int bstride, int bw, int bh, const TapTable &th, const TapTable &tv,
                    int w, int h, const uint8_t **out, int *ostride);
// the same with the tables of host_api.cpp's cache (make_taps), as fennec_lanczosResize takes them
int ssim_fast_resized_prepared(fnx_ctx *ctx, const fnx_prepared *ref, const uint8_t *b, int bstride, int bw, int bh,
                               const double *window, double *out);
// the bodies of fnx_ssim_fast_resized / fnx_ssim_resized / fnx_msssim_resized / fnx_lanczos_box_downsample: images in `space`,
// both tables given (an id != 0 keeps the plan look-up by id)
int ssim_fast_resized_tables(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah, const uint8_t *b, int bstride, int bw,
                             int bh, const TapTable &th, const TapTable &tv, const double *window, double *out);
int ssim_resized_tables(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah, const uint8_t *b, int bstride, int bw, int bh,
                        const TapTable &th, const TapTable &tv, const double *window, double *out);
int msssim_resized_tables(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah, const uint8_t *b, int bstride, int bw, int bh,
                          const TapTable &th, const TapTable &tv, const double *window, double *out, double *per_level);
int lanczos_box_tables(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW, int srcH, const TapTable &th, const TapTable &tv,
                       int midW, int midH, uint8_t *dst, int dstride, int dstW, int dstH);
// contig_taps: resize_contiguous_taps() of the (host) H table -- most taps of any output when every
// output's tap indices are consecutive, else 0
int launch_resize_h(fnx_ctx *ctx, const uint8_t *src, int sstride, int srcW, int srcH,
                    const int32_t *d_off, const int32_t *d_idx, const double *d_wt, uint8_t *dst,
                    int dstride, int dstW, int contig_taps);
int resize_contiguous_taps(const int32_t *off, const int32_t *idx, int nout);
int launch_resize_v(fnx_ctx *ctx, const uint8_t *src, int sstride, int srcW, int srcH,
                    const int32_t *d_off, const int32_t *d_idx, const double *d_wt, uint8_t *dst,
                    int dstride, int dstH, int contig_taps);
// n images: src either one pointer or device array; dst images are tight dstW x dstH, image i at
// dst + i*dst_image_bytes.
int launch_box_downsample(fnx_ctx *ctx, int n, const uint8_t *src, const uint8_t *const *srcs,
                          int sstride, int srcW, int srcH, uint8_t *dst, int dstride,
                          size_t dst_image_bytes, int dstW, int dstH);
// both sides of n SSIM comparisons in one launch: dst holds [a0..an-1][b0..bn-1] (src.b.p == src.b.ptrs == nullptr: a only)
int launch_box_downsample_pair(fnx_ctx *ctx, const ImgPairs &src, uint8_t *dst, int dstride, size_t dst_image_bytes, int dstW, int dstH);
// Windowed SSIM of n image pairs (tight or strided NRGBA, w x h >= 8); writes n doubles to d_out.
// Windowed-SSIM launches whose final means are taken later by ONE finish launch (MSSSIM: five levels,
// each finish is ~4.5 us of latency for a few hundred additions).  The caller reserves SLOT_PARTIAL
// for all of them first (SSIM_DEFER_DOUBLES) so that the partial pointers stay valid.
constexpr size_t SSIM_DEFER_DOUBLES = 64 * 1024;
struct SsimDeferred {
    int count = 0;
    size_t used = 0;                       // doubles of SLOT_PARTIAL handed out
    struct Item { size_t offset; int tiles; double windows; int out_index; } item[8];
};
struct SsimOpts {
    SsimDeferred *defer = nullptr;   // (n must be 1): no finish launch; d_out[defer_index] is written when
    int defer_index = 0;             // launch_ssim_finish_deferred runs
    bool select_as_one = false;      // kernel, tiling and reduction order of a call with n == 1
    static SsimOpts deferred(SsimDeferred *d, int index) { SsimOpts o; o.defer = d; o.defer_index = index; return o; }
    static SsimOpts as_one() { SsimOpts o; o.select_as_one = true; return o; }
};
int launch_windowed_ssim(fnx_ctx *ctx, const ImgPairs &im, const double *h_window, const double *d_window, double *d_out, const SsimOpts &opt = SsimOpts());
int launch_ssim_finish_deferred(fnx_ctx *ctx, const SsimDeferred &d, double *d_out, int nimg = 1, size_t part_img = 0, int out_img = 0);
// MSSSIM's levels in five launches (ssim.hip); FNX_NOOP (nothing launched) for shapes it does not cover.
// d_out[i] = SSIMFast of level i; *nlev = levels the reference's loop visits.
int launch_msssim_fused(fnx_ctx *ctx, const uint8_t *a, int astride, const uint8_t *b, int bstride, int w, int h,
                        int nweights, const double *h_window, double *d_out, int *nlev,
                        int nimg = 1, const uint8_t *const *d_as = nullptr, const uint8_t *const *d_bs = nullptr);
int launch_pixel_ssim(fnx_ctx *ctx, const uint8_t *a, const uint8_t *b, int w, int h,
                      size_t pix_len, double *d_out);
int launch_pixel_ssim_batch(fnx_ctx *ctx, int n, const uint8_t *const *d_as, const uint8_t *const *d_bs, int w, int h, size_t pix_len,
                            double *d_out);
// Analyze's device side (analyze.hip): n images -> d_res[n]; aligned16_ok: every base pointer is 16-byte aligned
int launch_analyze(fnx_ctx *ctx, int n, const uint8_t *src, const uint8_t *const *srcs, int sstride, int w, int h,
                   bool aligned16_ok, fnx_analysis *d_res);
// flat Pix scan: *d_flags bit 0 = some alpha != 255, bit 1 = some pixel with r != g or g != b
int launch_analyze_ready_words();
int launch_analyze_var_parts();
int launch_analyze_one(fnx_ctx *ctx, int n, const uint8_t *src, const uint8_t *const *srcs, int sstride, int w, int h,
                       bool aligned16_ok, fnx_analysis *res, double *var_part, uint32_t *ready);
int launch_scan_flags(fnx_ctx *ctx, const uint8_t *pix, size_t pix_len, uint32_t *d_flags);
// the same scan as ONE launch whose workgroups each write their flags (| 0x100) into their own word of host-visible memory
// (h_slots: pinned, launch_scan_flags_slots(ctx) words set to 0xffffffff by the caller, who watches the first *nslots of
// them change): no memset, no copy, no stream synchronisation
int launch_scan_flags_slots(const fnx_ctx *ctx);
int launch_scan_flags_direct(fnx_ctx *ctx, const uint8_t *pix, size_t pix_len, uint32_t *h_slots, int *nslots);
int ssim_done_counters(fnx_ctx *ctx, unsigned **out);   // ssim.hip: zeroed "workgroups finished" words (see there)
constexpr int DONE_SCAN = 2 * 4096 + 16;                // first of the 16 words of analyze.hip's scans
// analyzeFormat's samples: pixels at row-major indices 0, step, 2 step, ... (nsamples of them) as packed NRGBA words
int launch_sample_pixels(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, long long step, uint32_t *d_out, int nsamples);
// png_reduce.hip: compressPNG's pixel stages (compress.go:90-153).  launch_png_palettize: tryPalettize's colour set, palette
// and (d_plane != nullptr) index plane of a device image, w, h <= 65535; *d_result (device, png_result_bytes()): words
// 0 over (more than max_colors colours), 1 nongray (with over: a non-grey visible pixel was met on the way), 2 ncolors,
// 3 unused, then the palette words in first-occurrence order.  launch_png_plane: that index plane later, or toGray's plane.
size_t png_result_bytes();
int launch_png_palettize(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, int max_colors, uint8_t *d_plane, int pstride,
                         const void **d_result);
int launch_png_plane(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, bool gray, uint8_t *d_plane, int pstride);
// png_api.cpp: the body of fnx_png_reduce for a device image (flat Pix readable: (h-1) sstride + 4w bytes); d_plane: device, or
// nullptr (classify only).  Blocks; kind / palette / ncolors are host memory.
int png_reduce_device(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, int max_colors, uint8_t *d_plane, int pstride,
                      int *kind, uint8_t *palette, int *ncolors);
// png_filter.hip: the encoder's per-row stage (compress.go:94-107, targetsize.go:189, 342) -- rows of 1 + n bytes, the filter
// type and the filtered row, as zlib reads them.  Row forms: RGB / RGBA from an NRGBA image (4-byte aligned), GRAY from a
// byte plane, PALETTED from an index plane at `depth` 8, 4, 2 or 1 bits (type 0, packed MSB first; depth is ignored otherwise).
enum PngRowForm { PNG_ROW_RGB = 0, PNG_ROW_RGBA = 1, PNG_ROW_GRAY = 2, PNG_ROW_PALETTED = 3 };
int png_row_bytes(int form, int w, int depth);          // n
int launch_png_filter(fnx_ctx *ctx, int form, const uint8_t *src, int sstride, int w, int h, int depth, uint8_t *d_out);
// image.NRGBA.Opaque(): *d_flag = 1 when a visible pixel has alpha != 255, else 0
int launch_png_alpha(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, uint32_t *d_flag);
// png_api.cpp: the body of fnx_png_filter for a DEVICE image or plane; out: device (out_on_device) or host memory.  Blocks
// unless the opacity is stated and the stream stays on the device.
int png_filter_device(fnx_ctx *ctx, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque, bool out_on_device,
                      uint8_t *out, size_t cap, size_t *nbytes, int *color_type, int *bit_depth);
// deflate.hip: the zlib stream of n >= 1 device bytes into d_out (device, cap bytes; a larger stream writes nothing);
// *d_size: the device word that holds the stream's size once both kernels have run.  row: a match-distance hint, 0 for none.
// (deflate_chunks, deflate_bound: deflate_batch.hpp)
// (the 8 bytes behind *d_size are spare: png_encode_device's CRC word, fetched with the size)
int launch_deflate(fnx_ctx *ctx, const uint8_t *d_src, size_t n, int row, uint8_t *d_out, size_t cap, const unsigned long long **d_size);
// the size launch_deflate's stream would have under the ctx's level, and nothing else: the chunk kernels' size-only forms (the
// parse and the choice of form; no codes, no bits, no slots) and deflate_size_kernel.  *d_size: the device word with the size
int launch_deflate_size(fnx_ctx *ctx, const uint8_t *d_src, size_t n, int row, const unsigned long long **d_size);
// png_api.cpp: the body of fnx_deflate for device bytes (out: device or host memory), and of fnx_png_encode for a DEVICE image or
// plane (out: host memory; palette: host)
int deflate_device(fnx_ctx *ctx, const uint8_t *d_src, size_t n, int row, bool out_on_device, uint8_t *out, size_t cap, size_t *nbytes);
int png_encode_device(fnx_ctx *ctx, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque, const uint8_t *palette,
                      uint8_t *out, size_t cap, size_t *nbytes);
// the size png_encode_device's file would have, same arguments: the row stage into SLOT_PNG_STREAM, the size-only deflate, one
// fetch of 8 bytes.  palette (HOST) is read for the tRNS chunk's length alone
int png_size_device(fnx_ctx *ctx, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors, int opaque, const uint8_t *palette,
                    size_t *nbytes);
// the eight bytes a PNG file opens with, and image.Decode's test for them (io.go:65-88)
constexpr uint8_t PNG_SIG[8] = {0x89, 'P', 'N', 'G', '\r', '\n', 0x1a, '\n'};
inline bool png_signature(const uint8_t *data, size_t n) { return n >= 8 && std::memcmp(data, PNG_SIG, 8) == 0; }
// png_frame.cpp (host only): the file around a zlib stream -- signature, IHDR, PLTE + tRNS for colour type 3, one IDAT, IEND
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
uint8_t *png_frame_head(const PngFrame &f, uint8_t *out);
// the IDAT chunk whose zsize body bytes are in place, and IEND
void png_frame_tail(uint8_t *idat, size_t zsize);
// the same with the IDAT chunk's CRC given (the finished one, as the device's fold kernel writes it): no byte of the body is read
void png_frame_tail(uint8_t *idat, size_t zsize, uint32_t idat_crc);
// the CRC register after the four bytes "IDAT" from all ones: what the device's CRC of a chunk's body starts from
uint32_t png_idat_seed();
// ---- fnx_png_compress_batch: a chunk of images through one set of launches (png_compress_plan.hpp has the host plan) ----
struct PngCbSrc {                        // an image of the chunk: DEVICE, NRGBA, 4-byte aligned, the flat Pix readable
    const uint8_t *src;
    int sstride, w, h;
};
// png_reduce.hip: png_colors_batch_kernel, png_finish_batch_kernel, png_flags_batch_kernel -> *d_results, m records of
// png_result_bytes(): words 0 over, 2 ncolors, 3 flags (bit 0: a visible pixel is translucent, bit 1: the flat walk met a
// non-grey pixel), then the palette.  Nothing is waited for.  launch_png_planes_batch: png_plane_batch_kernel over the images
// with which[i] != 0 (1: the index plane from those results, 2: toGray's plane).
int launch_png_classify_batch(fnx_ctx *ctx, int m, const PngCbSrc *imgs, const void **d_results);
int launch_png_planes_batch(fnx_ctx *ctx, int m, const PngCbSrc *imgs, const int *which, uint8_t *const *planes, const int *pstrides);
// png_filter.hip: the row stage.  A record is what both single kernels take as their argument; d_units: the units of forms 0, 1,
// ... back to back, nunits[k] of form k
struct PngCbRows {
    const uint8_t *src;                  // the image, or its plane
    int sstride, w, h;
    int n;                               // raw bytes per row
    int al4;                             // png_cb_al4(src, sstride)
    uint8_t *out;                        // h rows of 1 + n bytes
};
int png_cb_al4(const uint8_t *src, int sstride);
int launch_png_rows_batch(fnx_ctx *ctx, const PngCbUnit *d_units, const int nunits[PNG_CB_FORMS], const PngCbRows *d_rows);
// deflate.hip: deflate_chunk_batch_kernel, deflate_gather_batch_kernel over DEVICE tables of nunits units and m streams;
// out_bytes: the sum of the streams' bounds.  *d_out: the zlib streams back to back at their true sizes, *d_sizes: the m sizes
// (*d_sizes + m, as words: room for the streams' CRCs -- launch_crc32_batch -- so that they come down with the sizes)
int launch_deflate_batch(fnx_ctx *ctx, const DeflateBatchUnit *d_units, const DeflateBatchImage *d_images, uint32_t nunits, uint32_t m,
                         size_t out_bytes, const uint8_t **d_out, const unsigned long long **d_sizes);
// crc32.hip: crc32_pieces_kernel, crc32_fold_kernel over the device bytes at d_src -> the finished CRC-32 in the device word
// *d_crc.  n_max: the bytes the grid covers; d_n: nullptr (the length is n_max) or the DEVICE word that holds the length once
// the kernels in front have run (held to n_max).  seed: the register the bytes start from (0xffffffff: a CRC of its own).
// Nothing is waited for.
int launch_crc32(fnx_ctx *ctx, const uint8_t *d_src, size_t n_max, const unsigned long long *d_n, uint32_t seed, uint32_t *d_crc);
// the batched twins over launch_deflate_batch's *d_out and *d_sizes: bounds[i] = deflate_bound of stream i (HOST, m of them),
// d_crcs: m device words
int launch_crc32_batch(fnx_ctx *ctx, const uint8_t *d_out, const unsigned long long *d_sizes, const size_t *bounds, uint32_t m, uint32_t seed,
                       uint32_t *d_crcs);
// jpeg_api.cpp: fnx_jpeg_decode_batch's body (the files' images into DEVICE dsts; per item fnx_jpeg_decode's answer)
int jpeg_decode_batch_device(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes, uint8_t *const *dsts, const int *dstrides,
                             int *ws, int *hs, int *status);
// applyPalette (+ palettedToNRGBA): palette = n x 4 host bytes (opaque); idx and/or quant may be null
int launch_apply_palette(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, const uint8_t *palette, int n,
                         uint8_t *idx, int istride, uint8_t *quant, int qstride);
// the same with the palette still on the device (fnx_quantize): d_palette = 256 words r | g << 8 | b << 16 | 255 << 24, *d_ncolors of
// them valid; pal_tables_kernel makes the tables the host makes above
int launch_apply_palette_device(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, const uint32_t *d_palette, const uint32_t *d_ncolors,
                                uint8_t *idx, int istride, uint8_t *quant, int qstride);
// median_cut.hip: medianCut's samples (targetsize.go:426-441) of an image of n pixels, and the palettes of a tight w x h image
// (w h >= 1) in `space` at nlevels strictly ascending sizes within 1 .. 256; *d_out (device): [nlevels][256] entries
// r | g << 8 | b << 16 | 255 << 24, then ncolors[nlevels].  Nothing is waited for.
void median_cut_samples(long long n, long long *step, long long *ns);
int launch_median_cut(fnx_ctx *ctx, int space, const uint8_t *src, int w, int h, int nlevels, const int *max_colors, const uint32_t **d_out);
// a level's entries from the kernel's words (HOST copies) into 256 x 4 bytes r, g, b, a; the rest of the 256 zeroed
inline int unpack_palette(const uint32_t *words, uint32_t n, uint8_t *palette)
{
    FNX_REQUIRE(n >= 1 && n <= 256, "median cut: the kernel's colour count");
    std::memset(palette, 0, 1024);
    for (uint32_t i = 0; i < n; i++)
        for (int c = 0; c < 4; c++) palette[4 * i + c] = static_cast<uint8_t>(words[i] >> (8 * c));
    return FNX_OK;
}
// image.YCbCr / image.Gray planes -> NRGBA (convert.hip); device pointers; cb == cr == nullptr: Gray
// boxDownsample(toNRGBARef(planes)) without the image (ssim.hip); *done = false: not its case, convert and downsample instead
int launch_box_downsample_ycc(fnx_ctx *ctx, const uint8_t *y, int ystride, const uint8_t *cb, const uint8_t *cr, int cstride,
                              int ratio, int srcW, int srcH, uint8_t *dst, int dstride, int dstW, int dstH, bool *done);
// four planes of equal geometry (a four-component JPEG, reader.go applyBlack) -> toNRGBARef's image; adobe: the APP14 transform
int launch_cmyk_to_nrgba(fnx_ctx *ctx, const uint8_t *const planes[4], int stride, int adobe, int w, int h, uint8_t *dst, int dstride);
int launch_ycbcr_to_nrgba(fnx_ctx *ctx, const uint8_t *y, int ystride, const uint8_t *cb, const uint8_t *cr,
                          int cstride, int ratio, int w, int h, uint8_t *dst, int dstride);
int launch_orient(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, int orient,
                  uint8_t *dst, int dstride);
// jpeg.hip: plane geometry of the round trip (Y: ys x yh, Cb / Cr: cs x ch), the quality-independent colour
// conversion + chroma averaging, and fdct / quantise / dequantise / idct of every block at `quality` (in -> out).
// mode: FNX_JPEG_SUBSAMPLING_420 / _444 (jpeg_layout.hpp); the single-image forms take it, the batched forms are 4:2:0
void jpeg_plane_dims(int w, int h, int *ys, int *yh, int *cs, int *ch, int mode = 0);
int launch_jpeg_ycc(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, uint8_t *yp, uint8_t *cbp, uint8_t *crp, int mode = 0);
int launch_jpeg_ycc_planes(fnx_ctx *ctx, const uint8_t *dy, int dys, const uint8_t *dcb, const uint8_t *dcr, int dcs, int ratio, int w, int h,
                           uint8_t *yp, uint8_t *cbp, uint8_t *crp);
// the planes of boxDownsample(src, dw, dh) straight from the w x h source, the downsampled image never written
int launch_jpeg_box_ycc(fnx_ctx *ctx, const uint8_t *src, int sstride, int w, int h, int dw, int dh, uint8_t *yp, uint8_t *cbp,
                        uint8_t *crp);
// a Huffman table's record as jpeg_hufftab_kernel leaves it (jpeg_hufftab.inc): [0] the number of values, [1] 1 when the table
// is the class's standard one (a code size above 32), then the DHT body's bytes in memory order: 16 counts, 256 values
constexpr int JPEG_HUFF_REC_WORDS = 70;
// rec: nullptr for the typical tables, else the file's four records (fnx_ctx_set_jpeg_huffman: FNX_JPEG_HUFFMAN_OPTIMIZED)
void jpeg_header(int w, int h, int quality, std::vector<uint8_t> &out, const uint32_t *rec = nullptr, int mode = 0);
int jpeg_entropy_code(fnx_ctx *ctx, int w, int h, int quality, const uint8_t *const planes[3], unsigned long long *totals,
                      uint32_t *rec = nullptr, int mode = 0);
// the kernels of the optimised tables on their own (fnx_jpeg_symbol_histogram, fnx_jpeg_huffman_tables): host results
int jpeg_symbol_hist_of(fnx_ctx *ctx, int w, int h, int quality, const uint8_t *const planes[3], uint32_t *hist, int mode = 0);
int jpeg_huffman_tables_of(fnx_ctx *ctx, const uint32_t *hist, uint32_t *lut, uint32_t *rec);
size_t jpeg_ecs_capacity(unsigned long long total_bits);
int jpeg_entropy_pack(fnx_ctx *ctx, int w, int h, unsigned long long total_bits, uint8_t *ecs, unsigned long long *totals, int mode = 0);
// behind jpeg_entropy_code on the same stream: totals[1] = the 0xff bytes of the string, counted from the blocks' strips (no packed string)
int jpeg_entropy_ffcount(fnx_ctx *ctx, int w, int h, unsigned long long *totals, int mode = 0);
int launch_jpeg_blocks(fnx_ctx *ctx, int w, int h, int quality, const uint8_t *const in[3], uint8_t *const out[3], int mode = 0);
// jpeg_api.cpp: the JPEG-writing entries that have no 4:4:4 form refuse a ctx set to FNX_JPEG_SUBSAMPLING_444 with this, first thing:
// FNX_ERR_UNSUPPORTED and a message that names `entry` and "4:4:4"; nothing launched, uploaded or written.  A NULL ctx passes
// (the entry's own checks answer for it)
int jpeg_refuse_444(const fnx_ctx *ctx, const char *entry);
// ---- batched forms (fnx_jpeg_compress_batch): n images of one geometry, the image index in grid x ----
constexpr int JPEG_QTAB_WORDS = 101 * 2 * 2 * 64;   // [quality 0..100][luma, chroma][step, magic][64]: the per-ctx quality table
void jpeg_qtab(uint32_t *tab);
// bytes per image of the unquantised / candidate planes (Y | Cb at *cb_off | Cr at *cr_off; 256-byte multiple)
size_t jpeg_batch_plane_bytes(int w, int h, size_t *cb_off, size_t *cr_off);
int launch_jpeg_ycc_batch(fnx_ctx *ctx, int n, const uint8_t *const *d_srcs, int sstride, int w, int h, uint8_t *planes);
// d_jobs: (image, quality) per job: image's planes at orig + image * plane bytes -> job j's at work + j * plane bytes
int launch_jpeg_blocks_batch(fnx_ctx *ctx, int njobs, int w, int h, const uint8_t *orig, uint8_t *work, const int2 *d_jobs,
                             const uint32_t *d_qtab);
int launch_copy_tight_batch(fnx_ctx *ctx, int n, const uint8_t *const *d_srcs, int sstride, int w, int h, uint8_t *dst, size_t dst_bytes);
int launch_ycbcr_to_nrgba_batch(fnx_ctx *ctx, int njobs, const uint8_t *planes, size_t plane_bytes, size_t cb_off, size_t cr_off,
                                int ystride, int cstride, int w, int h, uint8_t *dst, size_t dst_bytes);
// does launch_box_downsample_ycc take a w x h 4:2:0 candidate (jpeg_planes' aligned layout) to dstW x dstH?  (ssim.hip)
bool box_downsample_ycc_fused(int srcW, int srcH, int dstW, int dstH);
int launch_box_downsample_ycc_batch(fnx_ctx *ctx, int njobs, const uint8_t *planes, size_t plane_bytes, size_t cb_off, size_t cr_off,
                                    int ystride, int cstride, int srcW, int srcH, uint8_t *dst, size_t dst_bytes, int dstW, int dstH);
size_t jpeg_entropy_batch_bytes(int w, int h);
int jpeg_entropy_code_batch(fnx_ctx *ctx, int n, int w, int h, const uint8_t *planes, const int *d_quality, const uint32_t *d_qtab,
                            unsigned long long *tot, uint32_t *rec = nullptr);
int jpeg_entropy_pack_batch(fnx_ctx *ctx, int n, int w, int h, const unsigned long long *tbits, uint8_t **ecs, size_t *ecs_off,
                            unsigned long long *fftot);

// jpeg_dec.hip: Huffman decoding tables of one file (tables 0, 1: DC th 0, 1; 2, 3: AC th 0, 1) and what its segments say
constexpr int DEC_FAST_BITS = 11;                    // DecTables::fast is indexed by this many bits of the string
struct DecTables {                                   // tables 0, 1: DC (th 0, 1); 2, 3: AC (th 0, 1)
    uint16_t fast[4][1 << DEC_FAST_BITS];                          // by the next 11 bits: length << 8 | symbol; 0: a longer code
    uint32_t limit[4][18];                           // [L]: (largest code of length L + 1) << (16 - L)
    int32_t delta[4][18];                            // [L]: index of the first value of length L - its code
    uint8_t value[4][256];
};

// The synchronisation passes' form of the same tables: what a symbol DOES to the decoder's state, ready made -- ONE
// entry format for all four tables, so that a wave whose lanes stand in DC and in AC positions makes one LDS look-up per
// symbol instead of two divergent ones (r3: the loop is a chain of dependent LDS round trips, ~600 clocks per symbol).
//   st[t][prefix]   first symbol: bits consumed (code + value) | steps << 8 (DC: 1; AC: r + 1, or 64 for the end of block);
//                   AC tables: the first TWO symbols where the second one's code lies inside the prefix and the first
//                   does not end the block: total bits << 16 | total steps << 24 (else 0).  0: a longer code
struct DecSyncTables {
    uint32_t st[4][1 << DEC_FAST_BITS];
    uint32_t limit[4][18];
    int32_t delta[4][18];
    uint8_t value[4][256];
};

struct JpegFile {
    int w = 0, h = 0;
    int ncomp = 3;               // 3: image.YCbCr; 1: image.Gray; 4: image.CMYK (Adobe CMYK / YCbCrK, every component 1 x 1: the host route)
    int adobe = -1;              // the APP14 segment's transform byte (-1: no such segment)
    int ratio = 0;               // image.YCbCrSubsampleRatio: 0 4:4:4, 1 4:2:2, 2 4:2:0, 3 4:4:0, 4 4:1:1, 5 4:1:0; -1: one component
    int hy = 1, vy = 1;          // Y blocks per MCU across / down
    int nslots = 3;              // blocks per MCU
    int ri = 0;                  // MCUs per restart interval (DRI); 0: none
    int mx = 0, my = 0;          // MCUs per row / column
    uint64_t dcpack = 0, acpack = 0;   // Huffman table of MCU slot s: (pack >> 4 s) & 15 (up to 4 x 2 + 2 slots)
    uint16_t q[4][64];           // per component, natural order
    size_t scan = 0;             // offset of the entropy-coded segment in the file
    int rounds = 0;              // cross-workgroup synchronisation rounds the decode took
    bool progressive = false;    // the scans are entropy-decoded on the host (jpeg_prog.cpp: SOF2, SOF1, sequential scans the device has no form for), the image is made on the device
    // the frame header as jpeg_parse read and judged it: jpeg_prog.cpp takes the frame from HERE and never reads a SOF segment
    // itself (two readings of one file by two sets of marker rules was a heap overflow: ADVICE r5)
    bool sof_sequential = false; // SOF0 / SOF1 (true) or SOF2 (false)
    int comp_id[4] = {0, 0, 0, 0}, comp_h[4] = {1, 1, 1, 1}, comp_v[4] = {1, 1, 1, 1}, comp_q[4] = {0, 0, 0, 0};
    DecTables tab;
};
int jpeg_parse(const uint8_t *data, size_t n, JpegFile *f);
// a progressive file's coefficients over all its scans into coef (zeroed by the caller; [mx my nslots][64] int16, blocks in the
// order of an interleaved scan, natural order inside a block, DC as it is), the quantisation tables in force at EOI into f->q
int jpeg_progressive_coefficients(const uint8_t *data, size_t n, JpegFile *f, int16_t *coef);
// the host route's size limit (FNX_JPEG_HOST_MAX_BLOCKS in the header): a block costs 128 bytes of pinned host memory + 8 of
// mask before a single scan bit is validated, so a header may not promise more than this many (4 M blocks = 512 MB pinned:
// 16K x 8K at 4:2:0, 8K x 8K at 4:4:4); above it FNX_ERR_UNSUPPORTED -- the host codec's call
constexpr long long JPEG_HOST_MAX_BLOCKS = 1ll << 22;
int jpeg_unsupported(const char *what);     // set_error + FNX_ERR_UNSUPPORTED
int jpeg_corrupt(const char *what);         // set_error + FNX_ERR_INVALID
// the scan's bytes without the stuffing into dst (capacity: n - f.scan); *nbytes = what was written
// rst: the byte offsets (in dst) at which restart intervals 1, 2, ... start
int jpeg_unstuff(const uint8_t *data, size_t n, const JpegFile &f, uint8_t *dst, size_t *nbytes, std::vector<uint32_t> *rst);
int jpeg_decode_planes(fnx_ctx *ctx, const uint8_t *data, size_t n, JpegFile *f, uint8_t *planes[4], int *ystride, int *cstride);
// a chunk of BASELINE files (jpeg_parse'd, !progressive) through one set of launches: per item its status (what
// jpeg_decode_planes answers for the file) and, when that is FNX_OK, its planes in SLOT_JPEG_DEC_PLANES.  The return value is
// below 0 only where the chunk could not run at all.
struct JpegBatchItem {
    const uint8_t *data = nullptr;
    size_t n = 0;
    JpegFile f;
    int status = 0;
    uint8_t *planes[3] = {nullptr, nullptr, nullptr};
    int ystride = 0, cstride = 0;
};
size_t jpeg_decode_chunk_bytes(const JpegFile &f, size_t n);      // device scratch the file adds to a chunk (an upper estimate, from its bytes)
int jpeg_decode_planes_chunk(fnx_ctx *ctx, int m, JpegBatchItem *items);
// ---- PNG sources (png_parse.cpp: host only; png_decode.hip) ----
struct PngFile {
    int w = 0, h = 0, color_type = 0, depth = 0, interlace = 0;
    int channels = 1;
    int bpp = 1;                 // the filters' pixel distance: max(1, channels * depth / 8)
    size_t rowbytes = 0;         // ceil(w * channels * depth / 8): a row of the inflated stream is 1 + rowbytes
    int npal = 0, ntrns = 0;     // PLTE entries; tRNS alphas of a paletted file
    bool has_trns = false;
    uint8_t plte[768], trns[256];
    uint16_t trns16[3] = {0, 0, 0};   // the tRNS sample(s) of colour types 0 and 2
    std::vector<uint8_t> idat;   // the IDAT bodies back to back: one zlib stream
    // an accepted Adam7 file (interlace == 1, fnx_ctx_set_png_adam7): the seven passes as images of their own -- pw x ph pixels,
    // rows of 1 + prow bytes from poff of the inflated stream on; a pass without pixels has ph = 0 and no bytes
    int pw[7] = {0, 0, 0, 0, 0, 0, 0}, ph[7] = {0, 0, 0, 0, 0, 0, 0};
    size_t prow[7] = {0, 0, 0, 0, 0, 0, 0}, poff[7] = {0, 0, 0, 0, 0, 0, 0};
    size_t pstream = 0;          // the passes' bytes together
};
int png_corrupt(const char *what);          // set_error + FNX_ERR_INVALID
int png_unsupported(const char *what);      // set_error + FNX_ERR_UNSUPPORTED
// the signature and IHDR alone (CRC checked): the dimensions, and FNX_ERR_UNSUPPORTED for what the device does not take -- the
// file-level probe of host_api.cpp, which decodes next and so leaves the walk of the other chunks to that call
// adam7: the ctx's fnx_ctx_set_png_adam7 -- an Adam7 file passes, its pass geometry filled in, instead of being unsupported
int png_probe(const uint8_t *data, size_t n, PngFile *f, bool adam7 = false);
int png_parse(const uint8_t *data, size_t n, PngFile *f, bool adam7 = false);
// Adam7's pass geometry (the rule above fnx_png_decode): pass p holds the pixels (x0 + i dx, y0 + j dy); bits = channels * depth.
// A pass with pw == 0 or ph == 0 is absent: all three of its values are 0.  Returns the sum of ph (1 + rowbytes)
constexpr int ADAM7_X0[7] = {0, 4, 0, 2, 0, 1, 0}, ADAM7_Y0[7] = {0, 0, 4, 0, 2, 0, 1};
constexpr int ADAM7_DX[7] = {8, 8, 4, 4, 2, 2, 1}, ADAM7_DY[7] = {8, 8, 8, 4, 4, 2, 2};
size_t png_adam7_geometry(int w, int h, int bits, int pw[7], int ph[7], size_t rowbytes[7]);
// the zlib stream src[0 .. n) into out[0 .. cap); *nbytes: the bytes written.  A stream with more than cap bytes is refused
// with *nbytes = cap + 1
int png_inflate(const uint8_t *src, size_t n, uint8_t *out, size_t cap, size_t *nbytes);
// h * (1 + rowbytes) -- an Adam7 file: the sum of that over its passes --, the size the inflated stream must have
size_t png_stream_bytes(const PngFile &f);
// the same, refused when the file's IDAT bytes cannot hold that much
int png_stream_size(const PngFile &f, size_t *want);
// png_unfilter_kernel's work: a workgroup keeps PNG_DEC_ROWS rows in flight, one per lane.  The chain-segment table (a row of
// type None or Sub, and row 0, starts a segment; segments are independent) is cut into UNITS of whole segments, one workgroup
// each: a unit ends at the first segment boundary at which it holds PNG_UNIT_MIN_ROWS rows, so a long chain is one unit however
// long, and short segments share a workgroup instead of taking one each.  units: [first row, end row) pairs.  Refuses a
// filter type above 4.  An Adam7 file's passes are planned one by one, each as an image of its own: a pass's row 0 starts a
// segment, no unit spans two passes, the rows count from the pass's first, and passes (when asked for) gets each unit's pass.
constexpr int PNG_DEC_ROWS = FNX_PNG_DECODE_ROWS;
constexpr int PNG_UNIT_MIN_ROWS = 64;
int png_row_plan(const uint8_t *stream, const PngFile &f, std::vector<uint32_t> *units, std::vector<uint8_t> *passes = nullptr);
void png_palette_table(const PngFile &f, uint32_t table[256]);   // r | g << 8 | b << 16 | a << 24 of every index, toNRGBA applied
struct PngExpand {                          // what png_expand_kernel needs of the file
    int w, h, color_type, depth, has_trns;
    uint32_t key[3];                        // the tRNS sample(s)
};
size_t png_plane_pitch(const PngFile &f);   // bytes between the reconstructed rows: rowbytes rounded up to 16
// the reconstructed rows' bytes: h rows of png_plane_pitch -- an Adam7 file: a plane per present pass, ph rows of the pass's
// row bytes rounded up to 16, back to back (so every plane starts on a 16-byte boundary)
size_t png_planes_bytes(const PngFile &f);
// fnx_png_decode_batch's host side: everything fnx_png_decode does to a file before its first launch, for m files on up to
// `workers` threads (1: the calling thread alone, no thread started; more: the calling thread is one of them), handed out by
// an atomic index.  No HIP call, no ctx.  In: stream / cap, where the file's inflated stream goes (the batch's pinned staging;
// cap 0 for a file whose header promises more than its bytes can hold -- png_stream_size refuses it before the inflate).  Out:
// status, and for a refused file `what`, the static text png_corrupt / png_unsupported was called with (set_error is
// thread_local, so the caller re-issues the message: png_reissue).  Nothing depends on which thread took which file.
struct PngPrepared {
    uint8_t *stream = nullptr;
    size_t cap = 0;
    PngFile f;
    size_t want = 0;                        // the stream's bytes
    std::vector<uint32_t> units;            // png_row_plan
    std::vector<uint8_t> unit_pass;         // an Adam7 file: the pass each unit belongs to (empty otherwise)
    uint32_t table[256] = {};               // png_palette_table (colour type 3; zeros otherwise)
    int status = FNX_OK;
    const char *what = nullptr;
};
int png_workers(int workers, int m);        // the threads png_prepare_many runs m files on: 0 -> min(8, m), never above m
void png_prepare_many(const uint8_t *const *files, const size_t *sizes, int m, int workers, PngPrepared *items, bool adam7 = false);
int png_reissue(const PngPrepared &it);     // the item's set_error again, on this thread; returns its status
// a chunk of prepared files through one set of launches (png_decode.hip): per file what the two batched kernels read
struct PngBatchFile {
    const uint8_t *stream;                  // h rows of spitch = 1 + rowbytes bytes, 16 readable bytes on both sides
    size_t spitch;
    uint8_t *rows;                          // the reconstructed rows, ppitch (a multiple of 16) apart
    size_t ppitch;
    int rowbytes, npix;
    PngExpand e;
    const uint32_t *table;                  // colour type 3: the file's 256 pixel values
    uint8_t *dst;
    int dstride;
    uint32_t tile0;                         // png_expand_batch_kernel: the file's first workgroup (256 pixels of a row each)
};
struct PngBatchUnit {
    uint32_t file, r0, r1;                  // rows [r0, r1) of file `file` of the chunk
};
// an Adam7 file for png_expand_adam7_kernel (its argument) and png_expand_adam7_batch_kernel (a descriptor per file): the
// passes' reconstructed planes; e.w x e.h is the whole image.  An absent pass is never asked for (no pixel maps to it)
struct PngAdam7File {
    const uint8_t *plane[7];
    uint32_t ppitch[7];
    PngExpand e;
    const uint32_t *table;
    uint8_t *dst;
    int dstride;
    uint32_t tile0;                         // the batch kernel: the file's first workgroup
};
// png_parse.cpp: the file's PngExpand; and an accepted Adam7 file's passes as png_unfilter_batch_kernel's images, in pass order:
// passes[k], the k-th present pass -- its rows from stream + poff on, its plane (16-byte pitch) behind the planes before it from
// rows on, nothing else set --, a's planes and pitches, and slot[p] = first + k, the descriptor of pass p (0 for an absent pass).
// stream, rows: the DEVICE homes of the file's inflated stream and of its png_planes_bytes.  Returns the present passes' number
PngExpand png_expand_of(const PngFile &f);
int png_adam7_passes(const PngFile &f, const uint8_t *stream, uint8_t *rows, uint32_t first, PngBatchFile passes[7], PngAdam7File *a, uint32_t slot[7]);
// d_units: the chunk's units sorted by bpp, nunits[k] of them with bpp PNG_BPPS[k]; d_files: m descriptors; tiles: the sum of
// the files' workgroups of the expand kernel
constexpr int PNG_BPPS[6] = {1, 2, 3, 4, 6, 8};
// d_files[0 .. m) are the non-interlaced files (the expand kernel's); the Adam7 files' pass descriptors lie behind them, for the
// unfilter kernel alone.  d_adam7: ma descriptors and atiles workgroups of png_expand_adam7_batch_kernel (ma = 0: none)
int launch_png_decode_chunk(fnx_ctx *ctx, const PngBatchUnit *d_units, const int nunits[6], const PngBatchFile *d_files, int m, uint32_t tiles,
                            const PngAdam7File *d_adam7, int ma, uint32_t atiles);
// one Adam7 file: all passes' units in one launch of png_unfilter_batch_kernel<bpp>, then png_expand_adam7_kernel
int launch_png_adam7(fnx_ctx *ctx, int bpp, const PngBatchUnit *d_units, int nunits, const PngBatchFile *d_passes, const PngAdam7File &a);
int launch_png_unfilter(fnx_ctx *ctx, const uint8_t *d_stream, const PngFile &f, const uint32_t *d_units, int nunits, uint8_t *d_rows);
int launch_png_expand(fnx_ctx *ctx, const uint8_t *d_rows, const PngFile &f, const uint32_t *d_table, uint8_t *dst, int dstride);
int launch_scan(fnx_ctx *ctx, const uint32_t *in, unsigned long long *out, unsigned long long *totals, int n, unsigned long long *grand);

}  // namespace fnx
