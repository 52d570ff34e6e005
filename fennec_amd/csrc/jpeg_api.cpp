// fnx_jpeg_* entry points: the JPEG encoder's host flow (compress.go, targetsize.go) around jpeg.hip's kernels, and the
// decoder's around jpeg_dec.hip and jpeg_prog.cpp.
#include "common.hpp"
#include "jpeg_layout.hpp"

using namespace fnx;

namespace fnx {

int jpeg_refuse_444(const fnx_ctx *ctx, const char *entry)
{
    if (!ctx || ctx->jpeg_subsampling != FNX_JPEG_SUBSAMPLING_444) return FNX_OK;
    set_error("%s: not supported on a ctx set to 4:4:4 chroma (fnx_ctx_set_jpeg_subsampling): only fnx_jpeg_roundtrip, fnx_jpeg_quality_search, "
              "fnx_jpeg_encode, fnx_jpeg_compress, fnx_jpeg_size_search and fnx_jpeg_symbol_histogram follow the mode", entry);
    return FNX_ERR_UNSUPPORTED;
}

}  // namespace fnx

// ---- the JPEG quantisation round trip (compress.go:45-74; SURVEY 8(f)2, first slice: jpeg.hip) -------------
namespace {

// a JPEG file's dimensions are 16-bit
bool jpeg_dims(int w, int h) { return w >= 1 && w <= 65535 && h >= 1 && h <= 65535; }

struct JpegPlanes {
    uint8_t *p[3];
    int ys, yh, cs, ch;
    int mode;                   // FNX_JPEG_SUBSAMPLING_*: the layout these planes have, and with them every file made of them
};

// planes in the ctx's subsampling mode (the entries without a 4:4:4 form have refused such a ctx: theirs are 4:2:0)
int jpeg_planes(fnx_ctx *ctx, Slot slot, int w, int h, JpegPlanes *jp)
{
    jp->mode = ctx->jpeg_subsampling;
    jpeg_plane_dims(w, h, &jp->ys, &jp->yh, &jp->cs, &jp->ch, jp->mode);
    const size_t yb = static_cast<size_t>(jp->ys) * jp->yh, cb = static_cast<size_t>(jp->cs) * jp->ch;
    void *t = nullptr;
    FNX_TRY(scratch(ctx, slot, yb + 2 * cb + 16, &t));
    jp->p[0] = static_cast<uint8_t *>(t);
    jp->p[1] = jp->p[0] + yb;
    jp->p[2] = jp->p[1] + cb;
    return FNX_OK;
}

// the unquantised planes of the device image img in `slot`: what every encode of it starts from
int jpeg_ycc_planes(fnx_ctx *ctx, Slot slot, const uint8_t *img, int stride, int w, int h, JpegPlanes *pl)
{
    FNX_TRY(jpeg_planes(ctx, slot, w, h, pl));
    return launch_jpeg_ycc(ctx, img, stride, w, h, pl->p[0], pl->p[1], pl->p[2], pl->mode);
}

// planes at `quality` from the unquantised planes in SLOT_JPEG0, then the NRGBA image toNRGBARef makes of them
int jpeg_decode_at(fnx_ctx *ctx, const JpegPlanes &orig, int w, int h, int quality, uint8_t *dst, int dstride)
{
    JpegPlanes work;
    FNX_TRY(jpeg_planes(ctx, SLOT_JPEG1, w, h, &work));
    const uint8_t *in[3] = {orig.p[0], orig.p[1], orig.p[2]};
    FNX_TRY(launch_jpeg_blocks(ctx, w, h, quality, in, work.p, work.mode));
    return launch_ycbcr_to_nrgba(ctx, work.p[0], work.ys, work.p[1], work.p[2], work.cs, jpeg_ycbcr_ratio(work.mode), w, h, dst, dstride);
}

// the source side of every SSIMFast of a call (ssim.go:52-58), prepared once: its dims and its plane's buffer in SLOT_JPEG3
// (the plane: prepared_plane, or launch_box_downsample_ycc from a decoded file's planes)
int jpeg_prepared(fnx_ctx *ctx, int w, int h, fnx_prepared *ref)
{
    ref->w = w; ref->h = h;
    ssim_fast_dims(w, h, &ref->pw, &ref->ph);
    void *rp = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG3, static_cast<size_t>(ref->pw) * ref->ph * 4 + 16, &rp));
    ref->pix = static_cast<uint8_t *>(rp);
    return FNX_OK;
}

// compressJPEGOptimal's bisection (compress.go:24-74): a target >= 1 is 0.999, the lower bound comes from the target, and
// quality 100 (SSIM 1) stands when no quality reaches it
struct QualitySearch {
    double target;
    int lo = 1, hi = 100, best_q = 100, steps = 0;
    double best_ssim = 1.0;
    bool found = false;

    explicit QualitySearch(double t) : target(t >= 1.0 ? 0.999 : t)
    {
        if (target >= 0.99) lo = 75;
        else if (target >= 0.97) lo = 50;
        else if (target >= 0.94) lo = 30;
        else if (target >= 0.90) lo = 15;
    }
    bool done() const { return lo > hi; }
    int mid() const { return (lo + hi) / 2; }
    void record(int q, double ssim)
    {
        steps++;
        if (ssim >= target) {
            best_q = q; best_ssim = ssim; found = true;
            hi = q - 1;
        } else {
            lo = q + 1;
        }
    }
};

// compressJPEGOptimal's search over the unquantised planes `orig` of a w x h source whose prepared side is `ref`;
// FNX_NOOP: no quality reached the target
int jpeg_search_device(fnx_ctx *ctx, const fnx_prepared &ref, const JpegPlanes &orig, int w, int h, double target_ssim,
                       const double *window, int *quality, double *ssim, int *steps)
{
    void *dec = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG2, static_cast<size_t>(w) * h * 4 + 16, &dec));
    const bool ds = ref.pw != w || ref.ph != h;
    void *cand = nullptr;                                         // the candidate's SSIMFast plane
    if (ds) FNX_TRY(scratch(ctx, SLOT_TMP2, static_cast<size_t>(ref.pw) * ref.ph * 4 + 16, &cand));
    QualitySearch qs(target_ssim);
    while (!qs.done()) {
        const int mid = qs.mid();
        double v = 0;
        // the candidate: planes at quality `mid`; its <= 256 px plane straight from them where the image would only be
        // written to be box-summed (r3), else toNRGBARef's image
        JpegPlanes work;
        FNX_TRY(jpeg_planes(ctx, SLOT_JPEG1, w, h, &work));
        const uint8_t *in[3] = {orig.p[0], orig.p[1], orig.p[2]};
        FNX_TRY(launch_jpeg_blocks(ctx, w, h, mid, in, work.p, work.mode));
        const int ratio = jpeg_ycbcr_ratio(work.mode);
        bool fused = false;                                       // (a 4:4:4 candidate: "not fused" where the box sums have no form for it)
        if (ds) FNX_TRY(launch_box_downsample_ycc(ctx, work.p[0], work.ys, work.p[1], work.p[2], work.cs, ratio, w, h, static_cast<uint8_t *>(cand),
                                                  ref.pw * 4, ref.pw, ref.ph, &fused));
        if (fused) {
            FNX_TRY(against_device(ctx, &ref, static_cast<const uint8_t *>(cand), ref.pw * 4, window, &v, true));
        } else {
            FNX_TRY(launch_ycbcr_to_nrgba(ctx, work.p[0], work.ys, work.p[1], work.p[2], work.cs, ratio, w, h, static_cast<uint8_t *>(dec), w * 4));
            FNX_TRY(against_device(ctx, &ref, static_cast<const uint8_t *>(dec), w * 4, window, &v));
        }
        qs.record(mid, v);
    }
    *quality = qs.best_q;
    *ssim = qs.best_ssim;
    if (steps) *steps = qs.steps;
    return qs.found ? FNX_OK : FNX_NOOP;
}

// compressJPEGOptimal up to its file: src staged, its planes (-> *orig), the search
int jpeg_search_src(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, double target_ssim, const double *window,
                    JpegPlanes *orig, int *quality, double *ssim, int *steps)
{
    DevImg s;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    FNX_TRY(jpeg_ycc_planes(ctx, SLOT_JPEG0, s.p, s.stride, w, h, orig));
    fnx_prepared ref;
    FNX_TRY(jpeg_prepared(ctx, w, h, &ref));
    FNX_TRY(prepared_plane(ctx, s.p, s.stride, ref));
    return jpeg_search_device(ctx, ref, *orig, w, h, target_ssim, window, quality, ssim, steps);
}

// The file: header | entropy-coded segment | EOI.  The segment of a scan of `bits` bits with `ff` 0xff bytes in it is the bits
// padded to whole bytes plus the zero stuffed behind each 0xff.
size_t jpeg_ecs_bytes(unsigned long long bits, unsigned long long ff)
{
    return static_cast<size_t>((bits + 7) / 8) + static_cast<size_t>(bits ? ff : 0);
}

// -> the size of the file around a segment of `ecs` bytes; when it fits `cap`, its header and EOI go into out (the caller puts
// the segment at out + hdr.size())
size_t jpeg_file_frame(const std::vector<uint8_t> &hdr, size_t ecs, uint8_t *out, size_t cap)
{
    const size_t total = hdr.size() + ecs + 2;
    if (out == nullptr || cap < total) return total;
    std::memcpy(out, hdr.data(), hdr.size());
    out[total - 2] = 0xff;
    out[total - 1] = 0xd9;          // EOI
    return total;
}

// the "jpeg_size" form: "1" = a size-only query takes the one-wait route; "0" and unset = the file's two steps (opt-in: DESIGN.md
// 5.1 has the measurement and the rule it has to pass to become the default)
bool jpeg_size_one_wait(const fnx_ctx *ctx)
{
    const char *v = form_value(ctx, FORM_JPEG_SIZE);
    return v && v[0] == '1';
}

// the file of `orig`'s image at `quality` into host memory (see fnx_jpeg_encode)
int jpeg_file_from_planes(fnx_ctx *ctx, const JpegPlanes &orig, int w, int h, int quality, uint8_t *out, size_t cap, size_t *nbytes)
{
    // two u64 the kernels write and the host reads: bits of the scan's string, 0xff bytes in it; under
    // FNX_JPEG_HUFFMAN_OPTIMIZED the four tables' records (their DHT bodies) come back behind them, in the same wait
    const bool opt = ctx->jpeg_huffman == FNX_JPEG_HUFFMAN_OPTIMIZED;
    double *slot;
    FNX_TRY(result_slot(ctx, opt ? 2 + (4 * JPEG_HUFF_REC_WORDS + 1) / 2 : 2, &slot));
    unsigned long long *totals = reinterpret_cast<unsigned long long *>(slot);
    totals[0] = totals[1] = ~0ull;
    uint32_t *rec = opt ? reinterpret_cast<uint32_t *>(totals + 2) : nullptr;
    const uint8_t *planes[3] = {orig.p[0], orig.p[1], orig.p[2]};
    FNX_TRY(jpeg_entropy_code(ctx, w, h, quality, planes, totals, rec, orig.mode));
    if (out == nullptr && cap == 0 && jpeg_size_one_wait(ctx)) {
        // a size query never needs the packed string: the stuffed bytes are counted from the blocks' strips behind the scan,
        // and both totals come back in ONE wait (jpeg.hip: jpeg_ffcount_strips_kernel)
        FNX_TRY(jpeg_entropy_ffcount(ctx, w, h, totals, orig.mode));
        FNX_HIP(hipStreamSynchronize(ctx->stream));
        std::vector<uint8_t> hdr;
        jpeg_header(w, h, quality, hdr, rec, orig.mode);
        *nbytes = jpeg_file_frame(hdr, jpeg_ecs_bytes(totals[0], totals[1]), nullptr, 0);
        return FNX_OK;
    }
    FNX_HIP(hipStreamSynchronize(ctx->stream));
    const unsigned long long tbits = totals[0];
    void *ecs = nullptr;
    FNX_TRY(scratch(ctx, SLOT_JPEG_ECS, jpeg_ecs_capacity(tbits), &ecs));
    FNX_TRY(jpeg_entropy_pack(ctx, w, h, tbits, static_cast<uint8_t *>(ecs), totals, orig.mode));
    FNX_HIP(hipStreamSynchronize(ctx->stream));
    const size_t ecs_bytes = jpeg_ecs_bytes(tbits, totals[1]);
    std::vector<uint8_t> hdr;
    jpeg_header(w, h, quality, hdr, rec, orig.mode);
    const size_t total = jpeg_file_frame(hdr, ecs_bytes, out, cap);
    *nbytes = total;
    if (out == nullptr && cap == 0) return FNX_OK;       // size query: targetsize.go's searches need len(encoded) only
    if (out == nullptr || cap < total) {
        set_error("invalid argument: the file needs %zu bytes, the buffer holds %zu", total, cap);
        return FNX_ERR_INVALID;
    }
    if (ecs_bytes) FNX_HIP(hipMemcpy(out + hdr.size(), ecs, ecs_bytes, hipMemcpyDeviceToHost));
    return FNX_OK;
}

// jpegQualitySearchOpt's bisection (targetsize.go:129-165) over the planes of a w x h image, file sizes only: *q = the highest
// quality whose file fits `target` bytes (0: none), *sz its file's size; *n += the encodes it ran
int jpeg_size_bisect(fnx_ctx *ctx, const JpegPlanes &pl, int w, int h, long long target, int *q, size_t *sz, int *n)
{
    const double pixels = static_cast<double>(static_cast<long long>(w) * h);
    const double bpp = static_cast<double>(target * 8) / pixels;
    int lo = 1, hi = 100;
    if (bpp < 0.5) hi = 40;
    else if (bpp < 1.0) { lo = 10; hi = 70; }
    else if (bpp < 2.0) { lo = 30; hi = 90; }
    else if (bpp > 4.0) lo = 60;
    *q = 0; *sz = 0;
    while (lo <= hi) {
        const int mid = (lo + hi) / 2;
        size_t len = 0;
        FNX_TRY(jpeg_file_from_planes(ctx, pl, w, h, mid, nullptr, 0, &len));       // len(encoded) only
        ++*n;
        if (static_cast<long long>(len) <= target) {
            *q = mid; *sz = len;
            lo = mid + 1;
        } else {
            hi = mid - 1;
        }
    }
    return FNX_OK;
}

}  // namespace

extern "C" {

int fnx_jpeg_roundtrip(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int quality,
                       uint8_t *dst, int dstride)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    FNX_TRY(check_img(dst, dstride, w, h, "dst"));
    if (w <= 0 || h <= 0) return FNX_OK;
    DevImg s;
    DevOut d;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, w, h, SLOT_OUT, &d));
    JpegPlanes orig;
    FNX_TRY(jpeg_ycc_planes(ctx, SLOT_JPEG0, s.p, s.stride, w, h, &orig));
    FNX_TRY(jpeg_decode_at(ctx, orig, w, h, quality, d.p, d.stride));
    return finish(ctx, space, &d);
}

int fnx_jpeg_quality_search(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, double target_ssim,
                            const double *window, int *quality, double *ssim, int *steps)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(window && quality && ssim && w > 0 && h > 0, "search arguments");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    JpegPlanes orig;
    // FNX_NOOP: no quality reached the target (compress.go:82-86: encode at 100)
    return jpeg_search_src(ctx, space, src, sstride, w, h, target_ssim, window, &orig, quality, ssim, steps);
}

int fnx_jpeg_encode(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int quality, uint8_t *out, size_t cap,
                    size_t *nbytes)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(nbytes != nullptr && jpeg_dims(w, h), "encode arguments (JPEG dims are 16-bit)");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    *nbytes = 0;
    DevImg s;
    JpegPlanes orig;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    FNX_TRY(jpeg_ycc_planes(ctx, SLOT_JPEG0, s.p, s.stride, w, h, &orig));
    return jpeg_file_from_planes(ctx, orig, w, h, quality, out, cap, nbytes);
}

int fnx_jpeg_symbol_histogram(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int quality, uint32_t hist[4][256])
{
    if (!ctx || !src || !hist) { set_error("fnx_jpeg_symbol_histogram: null argument"); return FNX_ERR_INVALID; }
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(jpeg_dims(w, h), "symbol histogram arguments (JPEG dims are 16-bit)");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    DevImg s;
    JpegPlanes orig;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    FNX_TRY(jpeg_ycc_planes(ctx, SLOT_JPEG0, s.p, s.stride, w, h, &orig));
    const uint8_t *planes[3] = {orig.p[0], orig.p[1], orig.p[2]};
    return jpeg_symbol_hist_of(ctx, w, h, quality, planes, &hist[0][0], orig.mode);
}

int fnx_jpeg_huffman_tables(fnx_ctx *ctx, const uint32_t hist[4][256], uint8_t bits[4][16], uint8_t vals[4][256], int nvals[4],
                            uint32_t lut[4][256], int standard[4])
{
    // (the arguments first, the ctx last: what is wrong with a call does not depend on there being a device)
    if (!hist || !bits || !vals || !nvals || !lut || !standard) {
        set_error("fnx_jpeg_huffman_tables: null argument");
        return FNX_ERR_INVALID;
    }
    for (int t = 0; t < 4; t++) {
        bool any = false;
        for (int i = 0; i < 256; i++) any = any || hist[t][i] != 0;
        if (!any) {
            set_error("fnx_jpeg_huffman_tables: invalid argument: table %d's histogram is all zero", t);
            return FNX_ERR_INVALID;
        }
    }
    if (!ctx) { set_error("fnx_jpeg_huffman_tables: null ctx"); return FNX_ERR_INVALID; }
    FNX_ENTER(ctx);
    uint32_t rec[4 * JPEG_HUFF_REC_WORDS];
    FNX_TRY(jpeg_huffman_tables_of(ctx, &hist[0][0], &lut[0][0], rec));
    for (int t = 0; t < 4; t++) {
        const uint32_t *r = rec + t * JPEG_HUFF_REC_WORDS;
        FNX_REQUIRE(r[0] >= 1 && r[0] <= 256 && r[1] <= 1, "jpeg_hufftab_kernel left no table");
        const uint8_t *body = reinterpret_cast<const uint8_t *>(r + 2);
        nvals[t] = static_cast<int>(r[0]);
        standard[t] = static_cast<int>(r[1]);
        std::memcpy(bits[t], body, 16);
        std::memset(vals[t], 0, 256);
        std::memcpy(vals[t], body + 16, r[0]);
    }
    return FNX_OK;
}

int fnx_jpeg_size_search(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, long long target_bytes, int skip_ssim,
                         const double *window, uint8_t *out, size_t cap, size_t *nbytes, int *quality, double *ssim, int *steps)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(nbytes && quality && ssim && (skip_ssim || window) && jpeg_dims(w, h), "size search arguments");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    *nbytes = 0; *quality = 0; *ssim = 0.0;
    DevImg s;
    JpegPlanes orig;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    FNX_TRY(jpeg_ycc_planes(ctx, SLOT_JPEG0, s.p, s.stride, w, h, &orig));
    // targetsize.go:125-176
    int best_q = 0, n = 0;
    size_t sz = 0;
    FNX_TRY(jpeg_size_bisect(ctx, orig, w, h, target_bytes, &best_q, &sz, &n));
    if (steps) *steps = n;
    if (best_q == 0) return FNX_NOOP;                        // bestBuf == nil: nothing fits (the caller tries its next strategy)
    *quality = best_q;
    if (!skip_ssim) {
        // the SSIMFast the reference takes of every fitting candidate; the one that survives is the best quality's
        fnx_prepared ref;
        FNX_TRY(jpeg_prepared(ctx, w, h, &ref));
        FNX_TRY(prepared_plane(ctx, s.p, s.stride, ref));
        void *dec = nullptr;
        FNX_TRY(scratch(ctx, SLOT_JPEG2, static_cast<size_t>(w) * h * 4 + 16, &dec));
        FNX_TRY(jpeg_decode_at(ctx, orig, w, h, best_q, static_cast<uint8_t *>(dec), w * 4));
        FNX_TRY(against_device(ctx, &ref, static_cast<const uint8_t *>(dec), w * 4, window, ssim));
    }
    return jpeg_file_from_planes(ctx, orig, w, h, best_q, out, cap, nbytes);
}

int fnx_jpeg_compress(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, double target_ssim, const double *window,
                      uint8_t *out, size_t cap, size_t *nbytes, int *quality, double *ssim, int *steps)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(window && nbytes && quality && ssim && jpeg_dims(w, h), "compress arguments");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    *nbytes = 0;
    JpegPlanes orig;
    FNX_TRY(jpeg_search_src(ctx, space, src, sstride, w, h, target_ssim, window, &orig, quality, ssim, steps));
    // compress.go:76-86: the best candidate's bytes, or -- nothing reached the target -- an encode at bestQuality (100)
    return jpeg_file_from_planes(ctx, orig, w, h, *quality, out, cap, nbytes);
}

// ---- compressJPEGOptimal of n device images of one geometry in lockstep (fnx_jpeg_compress_batch) -------------------------
// Per item, jpeg_search_device's search and jpeg_file_from_planes' file.  The items still searching take ONE set of launches
// per step (each at its own mid) and ONE read-back of their scores; the winners are entropy-coded together with one read-back
// per phase.  Every kernel runs the single call's arithmetic on each item, and SSIMFast picks its kernel, tiling and
// reduction order as for one image: per item, the results are fnx_jpeg_compress's bit for bit.
namespace {

// device scratch a chunk of the batch may hold (orig + candidate planes, reference / candidate SSIMFast planes, decoded
// candidates where the route needs them, the entropy coder's per-block arrays); the entropy coder's bit strings and file
// bytes come on top (about 3 x the files' size)
constexpr size_t JPEG_BATCH_SCRATCH = size_t(1) << 30;

size_t al256(size_t v) { return (v + 255) & ~size_t(255); }

const uint32_t *jpeg_qtab_host()
{
    static const std::vector<uint32_t> t = [] {
        std::vector<uint32_t> v(JPEG_QTAB_WORDS);
        jpeg_qtab(v.data());
        return v;
    }();
    return t.data();
}

// the body of fnx_jpeg_compress_batch behind its argument checks (fnx_jpeg_recompress_batch: once per geometry of its files)
int jpeg_compress_group(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h, const double *target_ssim,
                        const double *window, uint8_t *const *outs, const size_t *caps, size_t *nbytes, int *quality, double *ssim,
                        int *steps, int *status);

}  // namespace

int fnx_jpeg_compress_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h, const double *target_ssim,
                            const double *window, uint8_t *const *outs, const size_t *caps, size_t *nbytes, int *quality, double *ssim,
                            int *steps, int *status)
{
    FNX_TRY(jpeg_refuse_444(ctx, "fnx_jpeg_compress_batch"));
    FNX_ENTER(ctx);
    FNX_REQUIRE(n >= 1 && n <= FNX_BATCH_MAX, "compress batch: n must be 1..FNX_BATCH_MAX (65535)");
    FNX_REQUIRE(srcs && target_ssim && outs && caps && nbytes && quality && ssim && status, "compress batch: NULL array");
    FNX_REQUIRE(window != nullptr, "compress batch: NULL window");
    FNX_REQUIRE(jpeg_dims(w, h), "compress batch: w and h must be 1..65535 (JPEG dims are 16-bit)");
    FNX_REQUIRE(sstride >= 4 * w && (sstride & 3) == 0, "compress batch: sstride must be a multiple of 4 and >= 4 * w");
    for (int i = 0; i < n; i++) {
        if (!srcs[i] || !outs[i]) {
            set_error("invalid argument: compress batch: srcs[%d] or outs[%d] is NULL", i, i);
            return FNX_ERR_INVALID;
        }
    }
    FNX_REQUIRE(ctx->res_count == 0, "enqueued batches are waiting for fnx_results_fetch: fetch them before a blocking batch call");
    return jpeg_compress_group(ctx, n, srcs, sstride, w, h, target_ssim, window, outs, caps, nbytes, quality, ssim, steps, status);
}

namespace {

int jpeg_compress_group(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h, const double *target_ssim,
                        const double *window, uint8_t *const *outs, const size_t *caps, size_t *nbytes, int *quality, double *ssim,
                        int *steps, int *status)
{
    // the route is the single call's for this geometry: tested once, taken for every item
    int pw, ph, ys, yh, cs, chh;
    const bool ds = ssim_fast_dims(w, h, &pw, &ph);
    const bool fused = ds && box_downsample_ycc_fused(w, h, pw, ph);     // candidate plane straight from its planes
    const bool pixel = pw < 8 || ph < 8;                                 // pixelSSIM instead of the windowed form
    jpeg_plane_dims(w, h, &ys, &yh, &cs, &chh);
    size_t cb_off = 0, cr_off = 0;
    const size_t PB = jpeg_batch_plane_bytes(w, h, &cb_off, &cr_off);
    const size_t RB = al256(static_cast<size_t>(pw) * ph * 4 + 16);     // a tight SSIMFast plane
    const size_t DB = al256(static_cast<size_t>(w) * h * 4 + 16);       // a decoded candidate (routes without the fused sums)
    const size_t per_item = 2 * PB + RB + (ds ? RB : 0) + (fused ? 0 : DB) + jpeg_entropy_batch_bytes(w, h);
    const size_t chunk_cap = JPEG_BATCH_SCRATCH / per_item;
    const int chunk = static_cast<int>(chunk_cap < 1 ? 1 : (chunk_cap > static_cast<size_t>(n) ? n : chunk_cap));

    const double *dwin = nullptr;
    void *dq = nullptr;
    FNX_TRY(upload_window(ctx, window, &dwin));
    FNX_TRY(upload_table(ctx, SLOT_JPEG_QTAB, jpeg_qtab_host(), sizeof(uint32_t) * JPEG_QTAB_WORDS, &dq));
    const uint32_t *d_qtab = static_cast<const uint32_t *>(dq);

    std::vector<QualitySearch> st;
    st.reserve(chunk);
    std::vector<int2> jobs(chunk);
    std::vector<const uint8_t *> pa(chunk), pb(chunk), pd(chunk);
    std::vector<int> qv(chunk), act(chunk);
    std::vector<double> vals(chunk);
    std::vector<unsigned long long> tbits(chunk);
    std::vector<size_t> ecs_off(chunk), ecs_len(chunk), host_off(chunk);
    std::vector<std::vector<uint8_t>> hdr(101);
    std::vector<uint32_t> recs;                          // FNX_JPEG_HUFFMAN_OPTIMIZED: the chunk's table records
    for (int c0 = 0; c0 < n; c0 += chunk) {
        const int m = n - c0 < chunk ? n - c0 : chunk;
        void *t = nullptr;
        FNX_TRY(upload_table(ctx, SLOT_PTRS, srcs + c0, sizeof(void *) * m, &t));
        const uint8_t *const *d_srcs = static_cast<const uint8_t *const *>(t);
        // the unquantised planes and the prepared reference planes of the chunk's sources, one launch each
        FNX_TRY(scratch(ctx, SLOT_JPEG0, PB * m, &t));
        uint8_t *orig = static_cast<uint8_t *>(t);
        FNX_TRY(launch_jpeg_ycc_batch(ctx, m, d_srcs, sstride, w, h, orig));
        FNX_TRY(scratch(ctx, SLOT_JPEG3, RB * m, &t));
        uint8_t *refs = static_cast<uint8_t *>(t);
        if (ds) {
            bool al = true;                                  // the single call's box kernel form depends on the source's alignment
            for (int i = 0; i < m; i++) al = al && aligned16(srcs[c0 + i], sstride);
            if (al) {
                FNX_TRY(launch_box_downsample(ctx, m, nullptr, d_srcs, sstride, w, h, refs, pw * 4, RB, pw, ph));
            } else {
                for (int i = 0; i < m; i++)
                    FNX_TRY(launch_box_downsample(ctx, 1, srcs[c0 + i], nullptr, sstride, w, h, refs + RB * i, pw * 4, 0, pw, ph));
            }
        } else {
            FNX_TRY(launch_copy_tight_batch(ctx, m, d_srcs, sstride, w, h, refs, RB));
        }
        uint8_t *work = nullptr, *cand = nullptr, *dec = nullptr;
        FNX_TRY(scratch(ctx, SLOT_JPEG1, PB * m, &t));
        work = static_cast<uint8_t *>(t);
        if (ds) {
            FNX_TRY(scratch(ctx, SLOT_TMP2, RB * m, &t));
            cand = static_cast<uint8_t *>(t);
        }
        if (!fused) {
            FNX_TRY(scratch(ctx, SLOT_JPEG2, DB * m, &t));
            dec = static_cast<uint8_t *>(t);
        }
        st.clear();
        for (int i = 0; i < m; i++) st.emplace_back(target_ssim[c0 + i]);
        for (;;) {
            int nj = 0;
            for (int i = 0; i < m; i++) {
                if (st[i].done()) continue;
                act[nj] = i;
                jobs[nj] = make_int2(i, st[i].mid());
                pa[nj] = refs + RB * i;
                pb[nj] = ds ? cand + RB * nj : dec + DB * nj;
                pd[nj] = fused ? nullptr : dec + DB * nj;
                nj++;
            }
            if (nj == 0) break;
            const void *hosts[4] = {jobs.data(), pa.data(), pb.data(), pd.data()};
            const size_t sizes[4] = {sizeof(int2) * nj, sizeof(void *) * nj, sizeof(void *) * nj, sizeof(void *) * nj};
            void *dp[4];
            FNX_TRY(upload_tables(ctx, SLOT_JPEG_JOBS, hosts, sizes, 4, dp));
            const uint8_t *const *d_as = static_cast<const uint8_t *const *>(dp[1]);
            const uint8_t *const *d_bs = static_cast<const uint8_t *const *>(dp[2]);
            FNX_TRY(launch_jpeg_blocks_batch(ctx, nj, w, h, orig, work, static_cast<const int2 *>(dp[0]), d_qtab));
            if (fused) {
                FNX_TRY(launch_box_downsample_ycc_batch(ctx, nj, work, PB, cb_off, cr_off, ys, cs, w, h, cand, RB, pw, ph));
            } else {
                FNX_TRY(launch_ycbcr_to_nrgba_batch(ctx, nj, work, PB, cb_off, cr_off, ys, cs, w, h, dec, DB));
                if (ds) FNX_TRY(launch_box_downsample(ctx, nj, nullptr, static_cast<const uint8_t *const *>(dp[3]), w * 4, w, h, cand,
                                                      pw * 4, RB, pw, ph));
            }
            double *dres;
            FNX_TRY(result_slot(ctx, nj, &dres));
            if (pixel) FNX_TRY(launch_pixel_ssim_batch(ctx, nj, d_as, d_bs, pw, ph, static_cast<size_t>(pw) * ph * 4, dres));
            else FNX_TRY(launch_windowed_ssim(ctx, pairs_by_pointer(nj, d_as, pw * 4, d_bs, pw * 4, pw, ph), window, dwin, dres, SsimOpts::as_one()));
            FNX_TRY(result_wait(ctx, dres, vals.data(), nj));
            for (int j = 0; j < nj; j++) st[act[j]].record(jobs[j].y, vals[j]);
        }
        // compress.go:76-86: every item's file at its best quality (100 when nothing reached the target), entropy-coded together
        for (int i = 0; i < m; i++) qv[i] = st[i].best_q;
        FNX_TRY(upload_table(ctx, SLOT_JPEG_JOBS, qv.data(), sizeof(int) * m, &t));
        // (FNX_JPEG_HUFFMAN_OPTIMIZED: every item's four table records behind the totals, in the same pinned read-back)
        const bool opt = ctx->jpeg_huffman == FNX_JPEG_HUFFMAN_OPTIMIZED;
        const size_t rec_words = opt ? static_cast<size_t>(4) * JPEG_HUFF_REC_WORDS * m : 0;
        void *pin = nullptr;
        FNX_TRY(pinned_alloc(ctx, sizeof(unsigned long long) * 2 * m + sizeof(uint32_t) * rec_words, &pin));
        unsigned long long *tot = static_cast<unsigned long long *>(pin);
        for (int i = 0; i < 2 * m; i++) tot[i] = ~0ull;
        uint32_t *rec = opt ? reinterpret_cast<uint32_t *>(tot + 2 * m) : nullptr;
        FNX_TRY(jpeg_entropy_code_batch(ctx, m, w, h, orig, static_cast<const int *>(t), d_qtab, tot, rec));
        FNX_HIP(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < m; i++) tbits[i] = tot[i];
        if (opt) recs.assign(rec, rec + rec_words);          // (the ring may wrap under the segments' staging below)
        uint8_t *ecs = nullptr;
        FNX_TRY(jpeg_entropy_pack_batch(ctx, m, w, h, tbits.data(), &ecs, ecs_off.data(), tot + m));
        FNX_HIP(hipStreamSynchronize(ctx->stream));
        size_t end = 0, exact = 0;
        for (int i = 0; i < m; i++) {
            ecs_len[i] = jpeg_ecs_bytes(tbits[i], tot[m + i]);
            end = ecs_off[i] + ecs_len[i] > end ? ecs_off[i] + ecs_len[i] : end;
            exact += ecs_len[i];
        }
        // the segments come down into pinned memory: each on its own (exact bytes) for a few items, the whole buffer with the
        // gaps its worst-case sizing leaves (~2x) for many small ones; one wait either way (tot is not read after this)
        const bool each = m <= 256;
        void *stage = nullptr;
        FNX_TRY(pinned_alloc(ctx, (each ? exact : end) + 64, &stage));
        uint8_t *hs = static_cast<uint8_t *>(stage);
        size_t o = 0;
        for (int i = 0; i < m; i++) {
            if (!each) {
                host_off[i] = ecs_off[i];
                continue;
            }
            host_off[i] = o;
            if (ecs_len[i]) FNX_HIP(hipMemcpyAsync(hs + o, ecs + ecs_off[i], ecs_len[i], hipMemcpyDeviceToHost, ctx->stream));
            o += ecs_len[i];
        }
        if (!each && end) FNX_HIP(hipMemcpyAsync(hs, ecs, end, hipMemcpyDeviceToHost, ctx->stream));
        FNX_HIP(hipStreamSynchronize(ctx->stream));
        for (int i = 0; i < m; i++) {
            const int k = c0 + i, q = st[i].best_q;
            if (opt) {                                       // the item's own tables: its own header
                hdr[q].clear();
                jpeg_header(w, h, q, hdr[q], recs.data() + static_cast<size_t>(i) * 4 * JPEG_HUFF_REC_WORDS);
            } else if (hdr[q].empty()) {
                jpeg_header(w, h, q, hdr[q]);
            }
            const size_t eb = ecs_len[i], total = jpeg_file_frame(hdr[q], eb, outs[k], caps[k]);
            nbytes[k] = total;
            quality[k] = q;
            ssim[k] = st[i].best_ssim;
            if (steps) steps[k] = st[i].steps;
            if (caps[k] < total) {
                status[k] = FNX_ERR_INVALID;
                continue;
            }
            if (eb) std::memcpy(outs[k] + hdr[q].size(), hs + host_off[i], eb);
            status[k] = FNX_OK;
        }
    }
    return FNX_OK;
}

}  // namespace

int fnx_jpeg_encode_scaled(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int dw, int dh, int quality,
                           uint8_t *out, size_t cap, size_t *nbytes)
{
    FNX_TRY(jpeg_refuse_444(ctx, "fnx_jpeg_encode_scaled"));
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(nbytes != nullptr && w > 0 && h > 0 && jpeg_dims(dw, dh), "encode_scaled arguments (JPEG dims are 16-bit)");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    *nbytes = 0;
    DevImg s;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    JpegPlanes pl;
    FNX_TRY(jpeg_planes(ctx, SLOT_JPEG1, dw, dh, &pl));
    FNX_TRY(launch_jpeg_box_ycc(ctx, s.p, s.stride, w, h, dw, dh, pl.p[0], pl.p[1], pl.p[2]));
    return jpeg_file_from_planes(ctx, pl, dw, dh, quality, out, cap, nbytes);
}

// ---- hitTargetSize's JPEG strategies (targetsize.go:26-357) in one call ---------------------------------------
// The source is staged once; every scale step's planes come from jpeg_box_ycc_kernel and only its file sizes (8 bytes
// a query) come back.  Slots: the source SLOT_IN_A, its planes SLOT_JPEG0, a scale step's planes SLOT_JPEG1, strategy 1's
// decoded winner SLOT_JPEG2, the prepared SSIMFast side of the source SLOT_JPEG3, the Lanczos-scaled image SLOT_TS_SCALED
// and -- unless the ctx runs resize_box_kernel ("resize_box" "1") -- its upscale for computeSSIMNRGBA SLOT_TS_UP.  At most one scaled
// candidate exists per call (strategy 4 runs only when strategy 3 found none), so SLOT_TS_SCALED still holds the winner's
// image at the end.
namespace {

constexpr int TS_MIN_QUALITY = 20;     // minJPEGQuality (targetsize.go:14)

struct TsRun {
    fnx_ctx *ctx;
    DevImg s;
    int w, h;
    long long target;
    const double *window;
    const volatile int *cancel;
    JpegPlanes orig{};      // SLOT_JPEG0 once orig_planes() has run
    fnx_prepared ref;       // SLOT_JPEG3 once prepared() has run

    bool cancelled() const { return cancel && *cancel != 0; }

    int orig_planes()
    {
        return orig.p[0] ? FNX_OK : jpeg_ycc_planes(ctx, SLOT_JPEG0, s.p, s.stride, w, h, &orig);
    }

    // SSIMFast's side of the source (ssim.go:52-58), once per call
    int prepared()
    {
        if (ref.pix) return FNX_OK;
        FNX_TRY(jpeg_prepared(ctx, w, h, &ref));
        return prepared_plane(ctx, s.p, s.stride, ref);
    }

    // computeSSIMNRGBA(src, b) (targetsize.go:534-539): b (device, bw x bh) Lanczos-resized to the source's size when the
    // dims differ, then SSIMFast against the prepared source
    int ssim_against(const uint8_t *b, int bstride, int bw, int bh, double *out)
    {
        FNX_TRY(prepared());
        return ssim_fast_resized_prepared(ctx, &ref, b, bstride, bw, bh, window, out);
    }

    // jpegQualitySearchFast(boxDownsample(src, dw, dh)) (targetsize.go:236, 260, 306): the scaled image never exists
    int scaled_query(int dw, int dh, int *q, size_t *sz, int *n)
    {
        JpegPlanes pl;
        FNX_TRY(jpeg_planes(ctx, SLOT_JPEG1, dw, dh, &pl));
        FNX_TRY(launch_jpeg_box_ycc(ctx, s.p, s.stride, w, h, dw, dh, pl.p[0], pl.p[1], pl.p[2]));
        return jpeg_size_bisect(ctx, pl, dw, dh, target, q, sz, n);
    }

    // lanczosResize(src, fw, fh) into SLOT_TS_SCALED and its planes into SLOT_JPEG1
    int lanczos_scaled(int fw, int fh, uint8_t **img, JpegPlanes *pl)
    {
        void *d = nullptr;
        FNX_TRY(scratch(ctx, SLOT_TS_SCALED, static_cast<size_t>(fw) * fh * 4 + 16, &d));
        *img = static_cast<uint8_t *>(d);
        FNX_TRY(fennec_lanczosResize(ctx, FNX_DEVICE, s.p, s.stride, w, h, *img, fw * 4, fw, fh));
        return jpeg_ycc_planes(ctx, SLOT_JPEG1, *img, fw * 4, fw, fh, pl);
    }

    // ---- strategy 1: jpegQualitySearch(src) (targetsize.go:33-37, 125-176) ----
    int quality(fnx_size_candidate *c)
    {
        FNX_TRY(orig_planes());
        int q = 0, n = 0;
        size_t sz = 0;
        FNX_TRY(jpeg_size_bisect(ctx, orig, w, h, target, &q, &sz, &n));
        c->steps = n;
        if (q < TS_MIN_QUALITY) return FNX_OK;           // nil, or below minJPEGQuality: not a candidate
        // computeSSIMNRGBA(src, decoded winner): the SSIM of every earlier fitting quality is overwritten by the reference
        void *dec = nullptr;
        FNX_TRY(scratch(ctx, SLOT_JPEG2, static_cast<size_t>(w) * h * 4 + 16, &dec));
        FNX_TRY(jpeg_decode_at(ctx, orig, w, h, q, static_cast<uint8_t *>(dec), w * 4));
        FNX_TRY(prepared());
        FNX_TRY(against_device(ctx, &ref, static_cast<const uint8_t *>(dec), w * 4, window, &c->ssim));
        c->strategy = FNX_TS_QUALITY; c->quality = q; c->final_w = w; c->final_h = h; c->nbytes = static_cast<int64_t>(sz);
        return FNX_OK;
    }

    // ---- strategy 3: jpegQualityScaleSearch (targetsize.go:210-283) ----
    int quality_scale(fnx_size_candidate *c)
    {
        int n = 0;
        bool have = false;
        double best = 0;
        double lo = 0.05, hi = 1.0;                      // findBestScaleBinary
        for (int i = 0; i < 10; i++) {
            if (cancelled()) break;
            const double mid = (lo + hi) / 2;
            const int nw = static_cast<int>(static_cast<double>(w) * mid), nh = static_cast<int>(static_cast<double>(h) * mid);
            if (nw < 8 || nh < 8) {
                lo = mid;
                continue;
            }
            int q = 0;
            size_t sz = 0;
            FNX_TRY(scaled_query(nw, nh, &q, &sz, &n));
            if (q != 0 && static_cast<long long>(sz) <= target && q >= TS_MIN_QUALITY) {
                have = true; best = mid;
                lo = mid;
            } else {
                hi = mid;
            }
        }
        static const double fixed[4] = {0.75, 0.50, 0.375, 0.25};   // findBestScaleFixed
        for (double scale : fixed) {
            if (cancelled()) break;
            const int nw = static_cast<int>(static_cast<double>(w) * scale), nh = static_cast<int>(static_cast<double>(h) * scale);
            if (nw < 8 || nh < 8) continue;
            int q = 0;
            size_t sz = 0;
            FNX_TRY(scaled_query(nw, nh, &q, &sz, &n));
            if (q != 0 && static_cast<long long>(sz) <= target && q >= TS_MIN_QUALITY && (!have || scale > best)) {
                have = true; best = scale;
            }
        }
        c->steps = n;
        if (!have) return FNX_OK;
        const int fw = static_cast<int>(static_cast<double>(w) * best), fh = static_cast<int>(static_cast<double>(h) * best);
        uint8_t *img = nullptr;
        JpegPlanes pl;
        FNX_TRY(lanczos_scaled(fw, fh, &img, &pl));
        int q = 0;
        size_t sz = 0;
        FNX_TRY(jpeg_size_bisect(ctx, pl, fw, fh, target, &q, &sz, &n));        // jpegQualitySearch(finalScaled): its SSIM is overwritten below
        c->steps = n;
        if (q < TS_MIN_QUALITY) return FNX_OK;
        FNX_TRY(ssim_against(img, fw * 4, fw, fh, &c->ssim));
        c->strategy = FNX_TS_QUALITY_SCALE; c->quality = q; c->final_w = fw; c->final_h = fh; c->nbytes = static_cast<int64_t>(sz);
        return FNX_OK;
    }

    // ---- strategy 4: scaleSearch(src, target, JPEG) (targetsize.go:285-357) ----
    int scale(fnx_size_candidate *c)
    {
        int n = 0, best_q = 0;
        double lo = 0.05, hi = 1.0, best = 0.0;
        for (int i = 0; i < 12; i++) {
            if (cancelled()) break;
            const double mid = (lo + hi) / 2;
            const int nw = static_cast<int>(static_cast<double>(w) * mid), nh = static_cast<int>(static_cast<double>(h) * mid);
            if (nw < 1 || nh < 1) {
                lo = mid;
                continue;
            }
            int q = 0;
            size_t sz = 0;
            FNX_TRY(scaled_query(nw, nh, &q, &sz, &n));
            if (q != 0 && static_cast<long long>(sz) <= target && q >= TS_MIN_QUALITY) {   // testScaleFits
                best = mid; best_q = q;
                lo = mid;
            } else {
                hi = mid;
            }
        }
        c->steps = n;
        if (best == 0.0) return FNX_OK;
        // executeFinalScaleEncode: jpegQualitySearchFast of the Lanczos image, else the file at bestQ (which may not fit)
        const int fw = static_cast<int>(static_cast<double>(w) * best), fh = static_cast<int>(static_cast<double>(h) * best);
        uint8_t *img = nullptr;
        JpegPlanes pl;
        FNX_TRY(lanczos_scaled(fw, fh, &img, &pl));
        int q = 0;
        size_t sz = 0;
        FNX_TRY(jpeg_size_bisect(ctx, pl, fw, fh, target, &q, &sz, &n));
        if (q == 0) {
            q = best_q;
            FNX_TRY(jpeg_file_from_planes(ctx, pl, fw, fh, q, nullptr, 0, &sz));
            n++;
        }
        c->steps = n;
        FNX_TRY(ssim_against(img, fw * 4, fw, fh, &c->ssim));
        c->strategy = FNX_TS_SCALE; c->quality = q; c->final_w = fw; c->final_h = fh; c->nbytes = static_cast<int64_t>(sz);
        return FNX_OK;
    }

    // ---- fallbackTargetSizeEncode's JPEG branch (targetsize.go:77-90) ----
    int fallback(fnx_size_candidate *c)
    {
        FNX_TRY(orig_planes());
        size_t sz = 0;
        FNX_TRY(jpeg_file_from_planes(ctx, orig, w, h, 1, nullptr, 0, &sz));
        FNX_TRY(ssim_against(s.p, s.stride, w, h, &c->ssim));     // computeSSIMNRGBA(original, original)
        c->strategy = FNX_TS_FALLBACK; c->quality = 1; c->final_w = w; c->final_h = h; c->steps = 1;
        c->nbytes = static_cast<int64_t>(sz);
        return FNX_OK;
    }
};

// betterFit (targetsize.go:92-115)
bool better_fit(const fnx_size_candidate &c, const fnx_size_candidate &b, long long t)
{
    const bool cu = c.nbytes <= t, bu = b.nbytes <= t;
    if (cu && !bu) return true;
    if (!cu && bu) return false;
    if (cu && bu) {
        if (c.ssim != b.ssim) return c.ssim > b.ssim;
        return c.quality > b.quality;
    }
    return c.nbytes < b.nbytes;
}

// ---- hitTargetSize's PNG legs (targetsize.go:39-43, 51-90, 180-206, 285-347) on the resident image of a TsRun ----
// Every "how many bytes?" is png_size_device (the row stage, the deflate kernels' size-only forms, 8 bytes back); a file is made
// once, for the call's winner (file()).  Slots: a level's index plane / the fallback's reduced plane SLOT_TS_PNG_PLANE, the
// winning level's quantized image SLOT_TS_PNG_QUANT, a scale step's box image SLOT_TS_PNG_BOX, the Lanczos image SLOT_TS_SCALED
// (free: the PNG scale leg runs only when no strategy produced a candidate); the palettes stay in SLOT_MEDIAN_CUT.
constexpr int TS_PNG_LEVELS[5] = {16, 32, 64, 128, 256};   // launch_median_cut's ascending order; the walk goes from 256 down

struct TsPng {
    TsRun &run;
    int plane_pitch = 0;
    // quantize's winner: its colour count and palette (HOST, r g b a)
    int q_ncolors = 0;
    uint8_t q_palette[1024];
    // the fallback's reduction
    int fb_kind = 0, fb_ncolors = 0;
    uint8_t fb_palette[1024];

    int plane(uint8_t **p)
    {
        plane_pitch = (run.w + 3) & ~3;
        void *t = nullptr;
        FNX_TRY(scratch(run.ctx, SLOT_TS_PNG_PLANE, static_cast<size_t>(plane_pitch) * run.h + 16, &t));
        *p = static_cast<uint8_t *>(t);
        return FNX_OK;
    }

    // ---- strategy 2: quantizeStrategy (targetsize.go:180-206) ----
    int quantize(fnx_size_candidate *c)
    {
        fnx_ctx *ctx = run.ctx;
        const int w = run.w, h = run.h;
        const uint32_t *d_pal = nullptr;                             // [5][256] entries, then the five colour counts
        FNX_TRY(launch_median_cut(ctx, FNX_DEVICE, run.s.p, w, h, 5, TS_PNG_LEVELS, &d_pal));
        std::vector<uint32_t> words(5 * 257);
        FNX_TRY(fetch_bytes(ctx, d_pal, words.data(), sizeof(uint32_t) * words.size()));
        uint8_t *idx = nullptr;
        FNX_TRY(plane(&idx));
        size_t prev = 0;
        int n = 0;
        for (int l = 4; l >= 0; l--) {
            const uint32_t nc = words[5 * 256 + l];
            size_t sz = prev;
            if (l == 4 || nc != words[5 * 256 + l + 1]) {            // else: the same palette, the same file
                FNX_TRY(unpack_palette(words.data() + 256 * l, nc, q_palette));
                FNX_TRY(launch_apply_palette_device(ctx, run.s.p, run.s.stride, w, h, d_pal + 256 * l, d_pal + 5 * 256 + l, idx, plane_pitch,
                                                    nullptr, 0));
                FNX_TRY(png_size_device(ctx, FNX_PNG_PALETTED, idx, plane_pitch, w, h, static_cast<int>(nc), 1, q_palette, &sz));
                n++;
            }
            c->steps = n;
            prev = sz;
            if (static_cast<long long>(sz) > run.target) continue;
            // the winner: palettedToNRGBA and computeSSIMNRGBA(src, quantized); the index plane stays for file()
            void *t = nullptr;
            FNX_TRY(scratch(ctx, SLOT_TS_PNG_QUANT, static_cast<size_t>(w) * h * 4 + 16, &t));
            FNX_TRY(launch_apply_palette_device(ctx, run.s.p, run.s.stride, w, h, d_pal + 256 * l, d_pal + 5 * 256 + l, nullptr, 0,
                                                static_cast<uint8_t *>(t), w * 4));
            FNX_TRY(run.ssim_against(static_cast<const uint8_t *>(t), w * 4, w, h, &c->ssim));
            q_ncolors = static_cast<int>(nc);
            c->strategy = FNX_TS_QUANTIZE; c->quality = 0; c->final_w = w; c->final_h = h; c->nbytes = static_cast<int64_t>(sz);
            return FNX_OK;
        }
        return FNX_OK;
    }

    // ---- strategy 4: scaleSearch(src, target, PNG) (targetsize.go:285-347) ----
    int scale(fnx_size_candidate *c)
    {
        fnx_ctx *ctx = run.ctx;
        const int w = run.w, h = run.h;
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_TS_PNG_BOX, static_cast<size_t>(w) * h * 4 + 16, &t));    // every step is smaller than the source
        uint8_t *box = static_cast<uint8_t *>(t);
        int n = 0;
        double lo = 0.05, hi = 1.0, best = 0.0;
        for (int i = 0; i < 12; i++) {
            if (run.cancelled()) break;
            const double mid = (lo + hi) / 2;
            const int nw = static_cast<int>(static_cast<double>(w) * mid), nh = static_cast<int>(static_cast<double>(h) * mid);
            if (nw < 1 || nh < 1) {
                lo = mid;
                continue;
            }
            size_t sz = 0;                                           // testScaleFits: png.Encode of the scaled image as it is
            FNX_TRY(launch_box_downsample(ctx, 1, run.s.p, nullptr, run.s.stride, w, h, box, nw * 4, 0, nw, nh));
            FNX_TRY(png_size_device(ctx, FNX_PNG_NRGBA, box, nw * 4, nw, nh, 0, -1, nullptr, &sz));
            n++;
            if (static_cast<long long>(sz) <= run.target) {
                best = mid;
                lo = mid;
            } else {
                hi = mid;
            }
        }
        c->steps = n;
        if (best == 0.0) return FNX_OK;
        // executeFinalScaleEncode: the Lanczos image's file, which may not fit
        const int fw = static_cast<int>(static_cast<double>(w) * best), fh = static_cast<int>(static_cast<double>(h) * best);
        FNX_TRY(scratch(ctx, SLOT_TS_SCALED, static_cast<size_t>(fw) * fh * 4 + 16, &t));
        uint8_t *img = static_cast<uint8_t *>(t);
        FNX_TRY(fennec_lanczosResize(ctx, FNX_DEVICE, run.s.p, run.s.stride, w, h, img, fw * 4, fw, fh));
        size_t sz = 0;
        FNX_TRY(png_size_device(ctx, FNX_PNG_NRGBA, img, fw * 4, fw, fh, 0, -1, nullptr, &sz));
        c->steps = n + 1;
        FNX_TRY(run.ssim_against(img, fw * 4, fw, fh, &c->ssim));
        c->strategy = FNX_TS_SCALE_PNG; c->quality = 0; c->final_w = fw; c->final_h = fh; c->nbytes = static_cast<int64_t>(sz);
        return FNX_OK;
    }

    // what the fallback's file is made from, after its reduction
    const uint8_t *fb_src() const { return fb_kind == FNX_PNG_NRGBA ? run.s.p : static_cast<const uint8_t *>(run.ctx->slot[SLOT_TS_PNG_PLANE].p); }
    int fb_stride() const { return fb_kind == FNX_PNG_NRGBA ? run.s.stride : plane_pitch; }

    // ---- fallbackTargetSizeEncode's PNG branch (targetsize.go:86-89): compressPNG(original), ssim 1.0 ----
    int fallback(fnx_size_candidate *c)
    {
        uint8_t *p = nullptr;
        FNX_TRY(plane(&p));
        FNX_TRY(png_reduce_device(run.ctx, run.s.p, run.s.stride, run.w, run.h, 256, p, plane_pitch, &fb_kind, fb_palette, &fb_ncolors));
        size_t sz = 0;
        FNX_TRY(png_size_device(run.ctx, fb_kind, fb_src(), fb_stride(), run.w, run.h, fb_ncolors, -1, fb_palette, &sz));
        c->strategy = FNX_TS_FALLBACK_PNG; c->quality = 0; c->final_w = run.w; c->final_h = run.h; c->steps = 1;
        c->nbytes = static_cast<int64_t>(sz);
        c->ssim = 1.0;
        return FNX_OK;
    }

    // the winner's image where it is not the source (device, tight), else nullptr
    const uint8_t *image(const fnx_size_candidate &c) const
    {
        if (c.strategy == FNX_TS_QUANTIZE) return static_cast<const uint8_t *>(run.ctx->slot[SLOT_TS_PNG_QUANT].p);
        if (c.strategy == FNX_TS_SCALE_PNG) return static_cast<const uint8_t *>(run.ctx->slot[SLOT_TS_SCALED].p);
        return nullptr;
    }

    // the winner's file: the single route's (png_encode_device) over what the leg left on the device
    int file(const fnx_size_candidate &c, uint8_t *out, size_t cap, size_t *nbytes)
    {
        fnx_ctx *ctx = run.ctx;
        if (c.strategy == FNX_TS_QUANTIZE)
            return png_encode_device(ctx, FNX_PNG_PALETTED, static_cast<const uint8_t *>(ctx->slot[SLOT_TS_PNG_PLANE].p), plane_pitch, run.w, run.h,
                                     q_ncolors, 1, q_palette, out, cap, nbytes);
        if (c.strategy == FNX_TS_SCALE_PNG)
            return png_encode_device(ctx, FNX_PNG_NRGBA, image(c), c.final_w * 4, c.final_w, c.final_h, 0, -1, nullptr, out, cap, nbytes);
        return png_encode_device(ctx, fb_kind, fb_src(), fb_stride(), run.w, run.h, fb_ncolors, -1, fb_palette, out, cap, nbytes);
    }
};

constexpr int TS_JPEG_BITS = FNX_TS_QUALITY | FNX_TS_QUALITY_SCALE | FNX_TS_SCALE | FNX_TS_FALLBACK;
constexpr int TS_PNG_BITS = FNX_TS_QUANTIZE | FNX_TS_SCALE_PNG | FNX_TS_FALLBACK_PNG;
constexpr int TS_AUTO = -1;            // ts_run's `strategies`: hitTargetSize under Format: Auto -- the source's opacity picks the legs

// hitTargetSize (targetsize.go:26-75) over the legs `strategies` names, behind the entries' argument checks.  cand[5]: strategy
// 1, quantize, strategy 3, strategy 4 (FNX_TS_SCALE or FNX_TS_SCALE_PNG; never both in one call), the fallback (likewise).
int ts_run(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, long long target_bytes, int strategies, const double *window,
           const volatile int *cancel, fnx_size_candidate cand[5], int *winner, uint8_t *out, size_t cap, size_t *nbytes, uint8_t *img, int istride)
{
    std::memset(cand, 0, sizeof(fnx_size_candidate) * 5);
    *winner = -1;
    *nbytes = 0;
    TsRun run{ctx, {}, w, h, target_bytes, window, cancel};
    TsPng png{run};
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &run.s));
    if (strategies == TS_AUTO) {
        // canUseJPEG = isOpaque(original) (convert.go:67-74: the flat Pix slice; the source is tight here, so the staged image is it)
        void *df = nullptr;
        FNX_TRY(scratch(ctx, SLOT_RESULT, 16, &df));
        FNX_TRY(launch_scan_flags(ctx, run.s.p, static_cast<size_t>(h - 1) * run.s.stride + static_cast<size_t>(w) * 4, static_cast<uint32_t *>(df)));
        uint32_t flags = 0;
        FNX_TRY(fetch_bytes(ctx, df, &flags, sizeof(flags)));
        strategies = FNX_TS_QUANTIZE | ((flags & 1u) ? FNX_TS_SCALE_PNG | FNX_TS_FALLBACK_PNG : TS_JPEG_BITS);
    }
    // the legs in the reference's order, ctx.Err() before each
    if ((strategies & FNX_TS_QUALITY) && !run.cancelled()) FNX_TRY(run.quality(&cand[0]));
    if ((strategies & FNX_TS_QUANTIZE) && !run.cancelled()) FNX_TRY(png.quantize(&cand[1]));
    if ((strategies & FNX_TS_QUALITY_SCALE) && !run.cancelled()) FNX_TRY(run.quality_scale(&cand[2]));
    auto none = [&] { return !cand[0].strategy && !cand[1].strategy && !cand[2].strategy && !cand[3].strategy; };
    if ((strategies & FNX_TS_SCALE) && none() && !run.cancelled()) FNX_TRY(run.scale(&cand[3]));
    if ((strategies & FNX_TS_SCALE_PNG) && none() && !run.cancelled()) FNX_TRY(png.scale(&cand[3]));
    if ((strategies & FNX_TS_FALLBACK) && none()) FNX_TRY(run.fallback(&cand[4]));       // also after a cancellation
    if ((strategies & FNX_TS_FALLBACK_PNG) && none()) FNX_TRY(png.fallback(&cand[4]));
    int best = -1;
    for (int i = 0; i < 5; i++)
        if (cand[i].strategy && (best < 0 || better_fit(cand[i], cand[best], target_bytes))) best = i;
    if (best < 0) return FNX_NOOP;
    *winner = best;
    const fnx_size_candidate &c = cand[best];
    const hipMemcpyKind down = space == FNX_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (c.strategy & TS_PNG_BITS) {
        if (img && png.image(c))
            FNX_HIP(hipMemcpy2DAsync(img, istride, png.image(c), size_t(c.final_w) * 4, size_t(c.final_w) * 4, c.final_h, down, ctx->stream));
        if (!out && cap == 0) *nbytes = static_cast<size_t>(c.nbytes);       // the size only: the leg's query was the file's
        else FNX_TRY(png.file(c, out, cap, nbytes));
        if (space == FNX_HOST) FNX_HIP(hipStreamSynchronize(ctx->stream));
        return FNX_OK;
    }
    JpegPlanes pl;
    if (best == 2 || best == 3) {
        // the winner's image (SLOT_TS_SCALED) and its planes once more: a later query may have used SLOT_JPEG1
        const uint8_t *scaled = static_cast<const uint8_t *>(ctx->slot[SLOT_TS_SCALED].p);
        FNX_TRY(jpeg_ycc_planes(ctx, SLOT_JPEG1, scaled, c.final_w * 4, c.final_w, c.final_h, &pl));
        if (img) FNX_HIP(hipMemcpy2DAsync(img, istride, scaled, size_t(c.final_w) * 4, size_t(c.final_w) * 4, c.final_h, down, ctx->stream));
    } else {
        FNX_TRY(run.orig_planes());
        pl = run.orig;
    }
    FNX_TRY(jpeg_file_from_planes(ctx, pl, c.final_w, c.final_h, c.quality, out, cap, nbytes));
    if (space == FNX_HOST) FNX_HIP(hipStreamSynchronize(ctx->stream));
    return FNX_OK;
}

// cand5's entries at[0 .. n) as the n candidates of an entry that runs a subset of the legs, the winner's index likewise
void ts_pick(const fnx_size_candidate cand5[5], int winner5, const int *at, int n, fnx_size_candidate *cand, int *winner)
{
    *winner = -1;
    for (int i = 0; i < n; i++) {
        cand[i] = cand5[at[i]];
        if (at[i] == winner5) *winner = i;
    }
}

}  // namespace

int fnx_jpeg_target_size(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, long long target_bytes, int strategies,
                         const double *window, const volatile int *cancel, fnx_size_candidate cand[4], int *winner, uint8_t *out,
                         size_t cap, size_t *nbytes, uint8_t *img, int istride)
{
    FNX_TRY(jpeg_refuse_444(ctx, "fnx_jpeg_target_size"));
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(cand && winner && nbytes, "target_size: cand, winner and nbytes are required");
    FNX_REQUIRE(window, "target_size: window is required");
    FNX_REQUIRE(jpeg_dims(w, h), "target_size: dimensions must be 1..65535 (JPEG dims are 16-bit)");
    FNX_REQUIRE(target_bytes > 0, "target_size: target_bytes must be > 0");
    FNX_REQUIRE(strategies > 0 && (strategies & ~TS_JPEG_BITS) == 0, "target_size: strategies must be a non-empty subset of bits 1, 2, 4, 8");
    FNX_REQUIRE(img == nullptr || istride >= 4 * w, "target_size: img needs a stride of at least 4 * w (the source's width)");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    fnx_size_candidate c5[5];
    int w5 = -1;
    const int rc = ts_run(ctx, space, src, sstride, w, h, target_bytes, strategies, window, cancel, c5, &w5, out, cap, nbytes, img, istride);
    static const int at[4] = {0, 2, 3, 4};
    ts_pick(c5, w5, at, 4, cand, winner);
    return rc;
}

int fnx_png_target_size(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, long long target_bytes, int strategies,
                        const double *window, const volatile int *cancel, fnx_size_candidate cand[3], int *winner, uint8_t *out, size_t cap,
                        size_t *nbytes, uint8_t *img, int istride)
{
    FNX_TRY(check_space(space));
    FNX_REQUIRE(cand && winner && nbytes, "png_target_size: cand, winner and nbytes are required");
    FNX_REQUIRE(window, "png_target_size: window is required");
    FNX_REQUIRE(jpeg_dims(w, h), "png_target_size: dimensions must be 1..65535");
    FNX_REQUIRE(target_bytes > 0, "png_target_size: target_bytes must be > 0");
    FNX_REQUIRE(strategies > 0 && (strategies & ~TS_PNG_BITS) == 0, "png_target_size: strategies must be a non-empty subset of bits 16, 32, 64");
    FNX_REQUIRE(out != nullptr || cap == 0, "png_target_size: out is null");
    FNX_REQUIRE(img == nullptr || istride >= 4 * w, "png_target_size: img needs a stride of at least 4 * w (the source's width)");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    FNX_REQUIRE(!(strategies & FNX_TS_QUANTIZE) || sstride == 4 * w,
                "png_target_size: quantize takes tight images only (sstride == 4*w): medianCut samples the flat Pix slice");
    FNX_REQUIRE(space == FNX_HOST || (reinterpret_cast<uintptr_t>(src) & 3u) == 0, "a device image is 4-byte aligned");
    FNX_ENTER(ctx);                                                  // every refusal above comes before the ctx is looked at
    fnx_size_candidate c5[5];
    int w5 = -1;
    const int rc = ts_run(ctx, space, src, sstride, w, h, target_bytes, strategies, window, cancel, c5, &w5, out, cap, nbytes, img, istride);
    static const int at[3] = {1, 3, 4};
    ts_pick(c5, w5, at, 3, cand, winner);
    return rc;
}

int fnx_hit_target_size(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, long long target_bytes, int format,
                        const double *window, const volatile int *cancel, fnx_size_candidate cand[5], int *winner, uint8_t *out, size_t cap,
                        size_t *nbytes, uint8_t *img, int istride)
{
    FNX_TRY(jpeg_refuse_444(ctx, "fnx_hit_target_size"));         // up front, whatever the format and the image would pick
    FNX_TRY(check_space(space));
    FNX_REQUIRE(cand && winner && nbytes, "hit_target_size: cand, winner and nbytes are required");
    FNX_REQUIRE(window, "hit_target_size: window is required");
    FNX_REQUIRE(jpeg_dims(w, h), "hit_target_size: dimensions must be 1..65535");
    FNX_REQUIRE(target_bytes > 0, "hit_target_size: target_bytes must be > 0");
    FNX_REQUIRE(format == FNX_FORMAT_AUTO || format == FNX_FORMAT_JPEG || format == FNX_FORMAT_PNG, "hit_target_size: format is 0 (Auto), 1 (JPEG) or 2 (PNG)");
    FNX_REQUIRE(img == nullptr || istride >= 4 * w, "hit_target_size: img needs a stride of at least 4 * w (the source's width)");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    if (format != FNX_FORMAT_JPEG) {
        FNX_REQUIRE(out != nullptr || cap == 0, "hit_target_size: out is null");
        FNX_REQUIRE(sstride == 4 * w, "hit_target_size: quantize takes tight images only (sstride == 4*w): medianCut samples the flat Pix slice");
        FNX_REQUIRE(space == FNX_HOST || (reinterpret_cast<uintptr_t>(src) & 3u) == 0, "a device image is 4-byte aligned");
    }
    FNX_ENTER(ctx);                                                  // every refusal above comes before the ctx is looked at
    const int strategies = format == FNX_FORMAT_JPEG ? TS_JPEG_BITS : (format == FNX_FORMAT_PNG ? TS_PNG_BITS : TS_AUTO);
    return ts_run(ctx, space, src, sstride, w, h, target_bytes, strategies, window, cancel, cand, winner, out, cap, nbytes, img, istride);
}

// ---- image.Decode of a baseline JPEG on the device (third slice: jpeg_dec.hip) ----------------
namespace {

// toNRGBARef's image of a decoded file's planes
int jpeg_planes_image(fnx_ctx *ctx, const JpegFile &f, const uint8_t *const pl[4], int ys, int cs, uint8_t *dst, int dstride)
{
    const bool grey = f.ncomp == 1;
    if (f.ncomp == 4) return launch_cmyk_to_nrgba(ctx, pl, ys, f.adobe, f.w, f.h, dst, dstride);
    return launch_ycbcr_to_nrgba(ctx, pl[0], ys, grey ? nullptr : pl[1], grey ? nullptr : pl[2], cs, grey ? 0 : f.ratio, f.w, f.h, dst, dstride);
}

// fnx_jpeg_decode behind its parse and its argument checks
int jpeg_decode_image(fnx_ctx *ctx, const uint8_t *data, size_t n, JpegFile *f, int space, uint8_t *dst, int dstride)
{
    DevOut d;
    FNX_TRY(stage_out(ctx, space, dst, dstride, f->w, f->h, SLOT_OUT, &d));
    uint8_t *pl[4] = {nullptr, nullptr, nullptr, nullptr};
    int ys = 0, cs = 0;
    FNX_TRY(jpeg_decode_planes(ctx, data, n, f, pl, &ys, &cs));
    FNX_TRY(jpeg_planes_image(ctx, *f, pl, ys, cs, d.p, d.stride));
    return finish(ctx, space, &d);
}

}  // namespace

int fnx_jpeg_decode(fnx_ctx *ctx, const uint8_t *data, size_t n, int space, uint8_t *dst, int dstride, int *w, int *h)
{
    FNX_REQUIRE(data != nullptr && w != nullptr && h != nullptr, "decode arguments");
    JpegFile f;
    if (dst == nullptr) {                        // jpeg.DecodeConfig: the dimensions only (and whether the device handles the file);
        FNX_TRY(jpeg_parse(data, n, &f));        // host work, no ctx needed
        *w = f.w; *h = f.h;
        return FNX_OK;
    }
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_TRY(jpeg_parse(data, n, &f));
    *w = f.w; *h = f.h;
    FNX_TRY(check_img(dst, dstride, f.w, f.h, "dst"));
    return jpeg_decode_image(ctx, data, n, &f, space, dst, dstride);
}

// ---- the same for a batch of files (fnx_jpeg_decode_batch; jpeg_dec.hip: jpeg_decode_planes_chunk) ------------------------
}  // extern "C"

namespace fnx {

// The files' images into dsts (DEVICE), per item what fnx_jpeg_decode(files[i], FNX_DEVICE, dsts[i]) gives.  Baseline files go
// through the decoder in chunks -- at most FNX_JPEG_DECODE_CHUNK files and JPEG_BATCH_SCRATCH of device scratch each (a file
// that alone needs more is a chunk of one) --, a refused file leaves its destination untouched (the images are made after the
// chunk's verdicts are in: launches, no wait); the host-route files follow one at a time.
int jpeg_decode_batch_device(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes, uint8_t *const *dsts, const int *dstrides,
                             int *ws, int *hs, int *status)
{
    std::vector<JpegBatchItem> chunk;
    std::vector<int> at, host;
    chunk.reserve(FNX_JPEG_DECODE_CHUNK);
    size_t bytes = 0;
    auto flush = [&]() -> int {
        if (chunk.empty()) return FNX_OK;
        FNX_TRY(jpeg_decode_planes_chunk(ctx, static_cast<int>(chunk.size()), chunk.data()));
        for (size_t j = 0; j < chunk.size(); j++) {
            const JpegBatchItem &it = chunk[j];
            const int k = at[j];
            status[k] = it.status;
            if (it.status != FNX_OK) continue;
            const uint8_t *pl[4] = {it.planes[0], it.planes[1], it.planes[2], nullptr};
            FNX_TRY(jpeg_planes_image(ctx, it.f, pl, it.ystride, it.cstride, dsts[k], dstrides[k]));
        }
        chunk.clear();
        at.clear();
        bytes = 0;
        return FNX_OK;
    };
    for (int i = 0; i < n; i++) {
        ws[i] = hs[i] = 0;
        status[i] = FNX_ERR_INVALID;
        if (!files[i]) {
            set_error("invalid argument: decode batch: files[%d] is NULL", i);
            continue;
        }
        JpegBatchItem it;
        it.data = files[i];
        it.n = sizes[i];
        const int rc = jpeg_parse(it.data, it.n, &it.f);
        if (rc < 0) {
            status[i] = rc;
            continue;
        }
        ws[i] = it.f.w; hs[i] = it.f.h;
        if (!dsts[i]) {
            set_error("invalid argument: decode batch: dsts[%d] is NULL", i);
            continue;
        }
        if (check_img(dsts[i], dstrides[i], it.f.w, it.f.h, "dst") < 0) continue;
        if (it.f.progressive) {
            host.push_back(i);
            continue;
        }
        const size_t cost = jpeg_decode_chunk_bytes(it.f, it.n);
        if (!chunk.empty() && (chunk.size() >= FNX_JPEG_DECODE_CHUNK || bytes + cost > JPEG_BATCH_SCRATCH)) FNX_TRY(flush());
        bytes += cost;
        chunk.push_back(it);
        at.push_back(i);
    }
    FNX_TRY(flush());
    for (int i : host) {
        JpegFile f;
        FNX_TRY(jpeg_parse(files[i], sizes[i], &f));
        status[i] = jpeg_decode_image(ctx, files[i], sizes[i], &f, FNX_DEVICE, dsts[i], dstrides[i]);
        if (status[i] == FNX_ERR_HIP || status[i] == FNX_ERR_OOM) return status[i];
    }
    return FNX_OK;
}

}  // namespace fnx

extern "C" {

int fnx_jpeg_decode_batch(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes, uint8_t *const *dsts, const int *dstrides,
                          int *ws, int *hs, int *status)
{
    FNX_ENTER(ctx);
    FNX_REQUIRE(n >= 1 && n <= FNX_BATCH_MAX, "decode batch: n must be 1..FNX_BATCH_MAX (65535)");
    FNX_REQUIRE(files && sizes && dsts && dstrides && ws && hs && status, "decode batch: NULL array");
    FNX_REQUIRE(ctx->res_count == 0, "enqueued batches are waiting for fnx_results_fetch: fetch them before a blocking batch call");
    return jpeg_decode_batch_device(ctx, n, files, sizes, dsts, dstrides, ws, hs, status);
}

// host only: jpeg_prog.cpp's output as the tests and the sanitizer runs read it
int fnx_jpeg_progressive_coefficients(const uint8_t *data, size_t n, int16_t *coef, size_t cap_blocks, size_t *blocks, int *w, int *h, int *ratio)
{
    FNX_REQUIRE(data != nullptr && blocks != nullptr && w != nullptr && h != nullptr && ratio != nullptr, "coefficient arguments");
    JpegFile f;
    FNX_TRY(jpeg_parse(data, n, &f));
    if (!f.progressive) return jpeg_unsupported("a baseline file here (its scan is decoded on the device)");
    const unsigned long long nblk = static_cast<unsigned long long>(f.mx) * f.my * f.nslots;
    *blocks = static_cast<size_t>(nblk);
    *w = f.w; *h = f.h; *ratio = f.ratio;
    if (nblk > static_cast<unsigned long long>(JPEG_HOST_MAX_BLOCKS)) return jpeg_unsupported("a host-decoded file of more than 4 M blocks (FNX_JPEG_HOST_MAX_BLOCKS)");
    if (coef == nullptr) return FNX_OK;
    FNX_REQUIRE(cap_blocks >= nblk, "coefficient capacity");
    if (8ull * n < nblk) return jpeg_corrupt("the file is too short for the image's blocks");       // (as fnx_jpeg_decode: before anything is sized by the header)
    std::memset(coef, 0, sizeof(int16_t) * 64 * static_cast<size_t>(nblk));
    return jpeg_progressive_coefficients(data, n, &f, coef);
}

int fnx_jpeg_recompress(fnx_ctx *ctx, const uint8_t *data, size_t n, double target_ssim, const double *window, uint8_t *out, size_t cap,
                        size_t *nbytes, int *quality, double *ssim, int *steps, int *w, int *h)
{
    FNX_TRY(jpeg_refuse_444(ctx, "fnx_jpeg_recompress"));
    FNX_ENTER(ctx);
    FNX_REQUIRE(data && window && nbytes && quality && ssim && w && h, "recompress arguments");
    *nbytes = 0;
    JpegFile f;
    uint8_t *pl[4] = {nullptr, nullptr, nullptr, nullptr};
    int ys = 0, cs = 0;
    FNX_TRY(jpeg_decode_planes(ctx, data, n, &f, pl, &ys, &cs));
    *w = f.w; *h = f.h;
    JpegPlanes orig;
    FNX_TRY(jpeg_planes(ctx, SLOT_JPEG0, f.w, f.h, &orig));
    fnx_prepared ref;
    bool from_planes = false;
    if (f.ncomp == 3) {
        // r3: toNRGBARef's image of the decoded planes (33 MB at 4K) was written for two readers only -- the encoder's colour
        // conversion and the reference plane's box sums; both take the planes themselves now (same per-pixel arithmetic), the
        // box sums where launch_box_downsample_ycc takes the planes' layout (else the image is made after all)
        FNX_TRY(launch_jpeg_ycc_planes(ctx, pl[0], ys, pl[1], pl[2], cs, f.ratio, f.w, f.h, orig.p[0], orig.p[1], orig.p[2]));
        FNX_TRY(jpeg_prepared(ctx, f.w, f.h, &ref));
        if (ref.pw != f.w || ref.ph != f.h)
            FNX_TRY(launch_box_downsample_ycc(ctx, pl[0], ys, pl[1], pl[2], cs, f.ratio, f.w, f.h, ref.pix, ref.pw * 4, ref.pw, ref.ph,
                                              &from_planes));
    }
    if (!from_planes) {
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_JPEG_DEC_IMG, static_cast<size_t>(f.w) * f.h * 4 + 16, &t));
        uint8_t *img = static_cast<uint8_t *>(t);
        const int istride = f.w * 4;
        const bool grey = f.ncomp == 1;
        if (f.ncomp == 4) FNX_TRY(launch_cmyk_to_nrgba(ctx, pl, ys, f.adobe, f.w, f.h, img, istride));
        else FNX_TRY(launch_ycbcr_to_nrgba(ctx, pl[0], ys, grey ? nullptr : pl[1], grey ? nullptr : pl[2], cs, grey ? 0 : f.ratio, f.w, f.h, img, istride));
        FNX_TRY(jpeg_ycc_planes(ctx, SLOT_JPEG0, img, istride, f.w, f.h, &orig));
        FNX_TRY(jpeg_prepared(ctx, f.w, f.h, &ref));
        FNX_TRY(prepared_plane(ctx, img, istride, ref));
    }
    FNX_TRY(jpeg_search_device(ctx, ref, orig, f.w, f.h, target_ssim, window, quality, ssim, steps));
    return jpeg_file_from_planes(ctx, orig, f.w, f.h, *quality, out, cap, nbytes);
}

// CompressBatch's item body for n JPEG files: fnx_jpeg_decode_batch into tight images in SLOT_JPEG_DEC_IMG, then
// fnx_jpeg_compress_batch's body once per geometry.  Per item the single call's results, by two equalities the tests pin:
// fnx_jpeg_recompress == fnx_jpeg_compress of the decoded image, and fnx_jpeg_compress_batch's item == fnx_jpeg_compress.
int fnx_jpeg_recompress_batch(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes, const double *target_ssim,
                              const double *window, uint8_t *const *outs, const size_t *caps, size_t *nbytes, int *quality, double *ssim,
                              int *steps, int *ws, int *hs, int *status)
{
    FNX_TRY(jpeg_refuse_444(ctx, "fnx_jpeg_recompress_batch"));
    FNX_ENTER(ctx);
    FNX_REQUIRE(n >= 1 && n <= FNX_BATCH_MAX, "recompress batch: n must be 1..FNX_BATCH_MAX (65535)");
    FNX_REQUIRE(files && sizes && target_ssim && outs && caps && nbytes && quality && ssim && ws && hs && status, "recompress batch: NULL array");
    FNX_REQUIRE(window != nullptr, "recompress batch: NULL window");
    for (int i = 0; i < n; i++) {
        if (!outs[i]) {
            set_error("invalid argument: recompress batch: outs[%d] is NULL", i);
            return FNX_ERR_INVALID;
        }
    }
    FNX_REQUIRE(ctx->res_count == 0, "enqueued batches are waiting for fnx_results_fetch: fetch them before a blocking batch call");
    std::vector<uint8_t *> dst;
    std::vector<int> dstride, idx;
    std::vector<size_t> off;
    std::vector<const uint8_t *> g_src;
    std::vector<uint8_t *> g_out;
    std::vector<double> g_target, g_ssim;
    std::vector<size_t> g_cap, g_nbytes;
    std::vector<int> g_quality, g_steps, g_status;
    // spans of the batch whose decoded images fit JPEG_BATCH_SCRATCH together (at least one file each)
    for (int s0 = 0; s0 < n;) {
        int s1 = s0;
        size_t total = 0;
        off.clear();
        for (; s1 < n; s1++) {
            int w = 0, h = 0;
            JpegFile f;
            if (files[s1] && jpeg_parse(files[s1], sizes[s1], &f) >= 0) { w = f.w; h = f.h; }
            const size_t b = al256(static_cast<size_t>(w) * h * 4 + 16);
            if (s1 > s0 && total + b > JPEG_BATCH_SCRATCH) break;
            off.push_back(total);
            total += b;
            ws[s1] = w; hs[s1] = h;
        }
        const int m = s1 - s0;
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_JPEG_DEC_IMG, total, &t));
        dst.assign(m, nullptr);
        dstride.assign(m, 0);
        for (int i = 0; i < m; i++) {
            nbytes[s0 + i] = 0;
            if (ws[s0 + i] <= 0) continue;                   // (the decoder answers for a file that does not parse)
            dst[i] = static_cast<uint8_t *>(t) + off[i];
            dstride[i] = ws[s0 + i] * 4;
        }
        FNX_TRY(jpeg_decode_batch_device(ctx, m, files + s0, sizes + s0, dst.data(), dstride.data(), ws + s0, hs + s0, status + s0));
        // every geometry's items that decoded, in the batch's order
        std::vector<char> taken(m, 0);
        for (int i = 0; i < m; i++) {
            if (taken[i] || status[s0 + i] != FNX_OK) continue;
            const int w = ws[s0 + i], h = hs[s0 + i];
            idx.clear();
            for (int j = i; j < m; j++)
                if (!taken[j] && status[s0 + j] == FNX_OK && ws[s0 + j] == w && hs[s0 + j] == h) {
                    taken[j] = 1;
                    idx.push_back(j);
                }
            const int g = static_cast<int>(idx.size());
            g_src.resize(g); g_out.resize(g); g_target.resize(g); g_ssim.resize(g); g_cap.resize(g); g_nbytes.resize(g);
            g_quality.resize(g); g_steps.resize(g); g_status.resize(g);
            for (int j = 0; j < g; j++) {
                const int k = s0 + idx[j];
                g_src[j] = dst[idx[j]]; g_out[j] = outs[k]; g_target[j] = target_ssim[k]; g_cap[j] = caps[k];
            }
            FNX_TRY(jpeg_compress_group(ctx, g, g_src.data(), w * 4, w, h, g_target.data(), window, g_out.data(), g_cap.data(), g_nbytes.data(),
                                        g_quality.data(), g_ssim.data(), g_steps.data(), g_status.data()));
            for (int j = 0; j < g; j++) {
                const int k = s0 + idx[j];
                nbytes[k] = g_nbytes[j]; quality[k] = g_quality[j]; ssim[k] = g_ssim[j]; status[k] = g_status[j];
                if (steps) steps[k] = g_steps[j];
            }
        }
        s0 = s1;
    }
    return FNX_OK;
}
}  // extern "C"
