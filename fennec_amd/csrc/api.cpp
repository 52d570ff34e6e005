// fnx_* entry points: argument checks, host<->device staging, table upload, kernel launches.
#include <algorithm>
#include <atomic>
#include <limits>
#include <cmath>

#include "common.hpp"

using namespace fnx;

namespace {

// Pix length of a w x h image with the given stride (Go: (h-1)*Stride + 4*w)
inline size_t pix_len(int w, int h, int stride)
{
    return (w > 0 && h > 0) ? static_cast<size_t>(h - 1) * stride + static_cast<size_t>(w) * 4 : 0;
}

// SSIMFast of n device image pairs -> d_out[n].  Image i of the single-pointer form lives at a.p + i*a.image_bytes (used by
// MSSSIM with n == 1).  opt.defer (n == 1 only): windowed paths leave their final mean to launch_ssim_finish_deferred, which
// writes d_out_base[defer_index]; d_out is then d_out_base + defer_index
int ssim_fast_device(fnx_ctx *ctx, const ImgPairs &im, const double *h_window, const double *d_window, double *d_out, const SsimOpts &opt = SsimOpts())
{
    const int n = im.n, w = im.w, h = im.h;
    double *d_base = opt.defer ? d_out - opt.defer_index : d_out;
    int nw, nh;
    if (ssim_fast_dims(w, h, &nw, &nh)) {
        // boxDownsample both sides (ssim.go:57-58) into tight planes: [a0..an-1][b0..bn-1]
        const size_t plane = static_cast<size_t>(nw) * nh * 4;
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_TMP2, plane * 2 * n + 16, &t));
        uint8_t *da = static_cast<uint8_t *>(t), *db = da + plane * n;
        FNX_TRY(launch_box_downsample_pair(ctx, im, da, nw * 4, plane, nw, nh));
        if (nw < 8 || nh < 8) {
            for (int i = 0; i < n; i++)
                FNX_TRY(launch_pixel_ssim(ctx, da + plane * i, db + plane * i, nw, nh, plane, d_out + i));
            return FNX_OK;
        }
        return launch_windowed_ssim(ctx, plane_pairs(n, da, db, plane, nw, nh), h_window, d_window, d_base, opt);
    }
    if (im.a.ptrs || im.b.ptrs) {
        set_error("batched SSIMFast needs images larger than 512 px (the downsample path)");
        return FNX_ERR_INVALID;
    }
    if (w < 8 || h < 8) return launch_pixel_ssim(ctx, im.a.p, im.b.p, w, h, pix_len(w, h, im.a.stride), d_out);
    return launch_windowed_ssim(ctx, one_pair(im.a.p, im.a.stride, im.b.p, im.b.stride, w, h), h_window, d_window, d_base, opt);
}

// Two host arrays of n device pointers each -> the ctx's device copies (batched launches index them by image)
template <typename Second>   // const uint8_t (both sides read) or uint8_t (sources, destinations)
int upload_ptr_pair(fnx_ctx *ctx, int n, const uint8_t *const *first, Second *const *second, const uint8_t *const **d_first, Second *const **d_second)
{
    const void *hosts[2] = {first, second};
    const size_t sizes[2] = {sizeof(void *) * size_t(n), sizeof(void *) * size_t(n)};
    void *dp[2];
    FNX_TRY(upload_tables(ctx, SLOT_PTRS, hosts, sizes, 2, dp));
    *d_first = static_cast<const uint8_t *const *>(dp[0]);
    *d_second = static_cast<Second *const *>(dp[1]);
    return FNX_OK;
}

bool all_aligned16(int n, const uint8_t *const *ptrs, int stride)
{
    bool al = true;
    for (int i = 0; i < n; i++) al = al && aligned16(ptrs[i], stride);
    return al;
}

// What the round 6 batch entry points ask of their arguments: the call's own conditions and the batch size, then -- once the
// caller has dealt with n == 0 and its dims -- every image of both arrays.  (The blur, SSIMFast and one-pass batches keep their
// older checks: they take n > FNX_BATCH_MAX and refuse null arrays at n == 0, so sharing these would change an answer.)
int check_batch(int n, bool arrays, bool args_ok = true)
{
    FNX_REQUIRE(n >= 0 && (n == 0 || arrays) && args_ok, "batch arguments");
    FNX_REQUIRE(n <= FNX_BATCH_MAX, "more than FNX_BATCH_MAX (65535) images in one batch call: the image is a grid dimension");
    return FNX_OK;
}

struct BatchSide { const uint8_t *const *p; int stride, w, h; const char *what; };
int check_batch_images(int n, const BatchSide &x, const BatchSide &y, const char *distinct_msg = nullptr)
{
    for (int i = 0; i < n; i++) {
        if (distinct_msg) FNX_REQUIRE(x.p[i] && y.p[i] && x.p[i] != y.p[i], distinct_msg);
        else FNX_REQUIRE(x.p[i] && y.p[i], "null image in batch");
        FNX_TRY(check_img(x.p[i], x.stride, x.w, x.h, x.what));
        FNX_TRY(check_img(y.p[i], y.stride, y.w, y.h, y.what));
    }
    return FNX_OK;
}

int check_pix_lens(int w, int h, int astride, int bstride)   // pixelSSIM walks a.Pix and indexes b.Pix with it (ssim.go:178)
{
    FNX_REQUIRE(pix_len(w, h, bstride) >= pix_len(w, h, astride), "b.Pix shorter than a.Pix (the reference would panic)");
    return FNX_OK;
}

// Both sides of a host- or device-space comparison on the device: `flat` (pixelSSIM's sizes) as the flat Pix slices they are,
// stride kept, else by rows
int stage_pair(fnx_ctx *ctx, int space, const uint8_t *a, int astride, const uint8_t *b, int bstride, int w, int h, bool flat, DevImg *da, DevImg *db)
{
    if (flat) FNX_TRY(check_pix_lens(w, h, astride, bstride));
    const auto stage = flat ? stage_in_flat : stage_in;
    FNX_TRY(stage(ctx, space, a, astride, w, h, SLOT_IN_A, da));
    return stage(ctx, space, b, bstride, w, h, SLOT_IN_B, db);
}

void nan_fill(double *d, int n) { std::fill_n(d, n, std::numeric_limits<double>::quiet_NaN()); }

// The FIFO position the next *_enqueue call fills (free while res_count < RES_DEPTH: can_enqueue)
int res_tail(const fnx_ctx *ctx) { return (ctx->res_head + ctx->res_count) % fnx_ctx::RES_DEPTH; }

// Result slots of an *_enqueue call: the batch's OWN pinned buffer (one per FIFO position), so that nothing
// a later call does to the pinned ring (growth frees it, wrap-around reuses it) can touch results that were
// enqueued and not fetched yet.  The position's buffer is free by construction: can_enqueue() has checked
// res_count < RES_DEPTH, and a fetched batch has been copied out.
int result_slot_queued(fnx_ctx *ctx, int n, double **d)
{
    fnx_ctx::ResBuf &rb = ctx->res_buf[res_tail(ctx)];
    const size_t need = sizeof(double) * static_cast<size_t>(n > 16 ? n : 16);
    if (need > rb.cap) {
        if (rb.p) FNX_HIP(hipHostFree(rb.p));
        rb.p = nullptr;
        rb.cap = 0;
        FNX_HIP(hipHostMalloc(reinterpret_cast<void **>(&rb.p), need * 2, hipHostMallocDefault));
        rb.cap = need * 2;
    }
    *d = rb.p;
    nan_fill(*d, n);
    return FNX_OK;
}

// Spin until ready() holds: on words in pinned host memory that the call's last kernel writes.  They arrive a PCIe write
// after the kernel stores them, while hipStreamSynchronize / hipEventSynchronize return 10-20 us later; the stream (or the
// event) is still queried now and then (done), which also ends the wait if the words never change or the GPU faulted.
template <typename Ready, typename Done>
int poll_until(Ready ready, Done done)
{
    for (unsigned spin = 1; !ready(); spin++) {
        if ((spin & 127u) == 0) {
            const hipError_t q = done();
            if (q == hipSuccess) break;
            if (q != hipErrorNotReady) FNX_HIP(q);
        }
        __builtin_ia32_pause();
    }
    std::atomic_thread_fence(std::memory_order_acquire);
    return FNX_OK;
}

// Wait until the n result slots hold values (a NaN slot is one not written yet, or a value that really is NaN)
template <typename Done>
int poll_results(const double *pinned, int n, Done done)
{
    const volatile double *v = pinned;
    return poll_until([=] {
        for (int i = 0; i < n; i++) {
            const double x = v[i];
            if (x != x) return false;
        }
        return true;
    }, done);
}

// ssim.go:344-352: exp(sum_i weights[i] * log(max(level_i, 1e-10)))
double msssim_combine(const double *lv, const double *weights, int nlev)
{
    double result = 0;
    for (int i = 0; i < nlev; i++) result += weights[i] * std::log(std::fmax(lv[i], 1e-10));   // ssim.go:351
    return std::exp(result);
}

int can_enqueue(fnx_ctx *ctx)
{
    if (ctx->res_count == fnx_ctx::RES_DEPTH) {
        set_error("invalid argument: %d enqueued batches are waiting for fnx_results_fetch on this ctx", ctx->res_count);
        return FNX_ERR_INVALID;
    }
    return FNX_OK;
}

// An event right behind the result kernels, and the batch joins the ctx's FIFO of unfetched results (*filled: its entry):
// fnx_results_fetch then never waits for work that was queued on this stream after the batch.
int publish_results(fnx_ctx *ctx, const double *pinned, int n, fnx_ctx::Pending **filled = nullptr)
{
    FNX_TRY(can_enqueue(ctx));
    fnx_ctx::Pending &q = ctx->res_q[res_tail(ctx)];
    if (!q.ev) FNX_HIP(hipEventCreateWithFlags(&q.ev, hipEventDisableTiming));
    FNX_HIP(hipEventRecord(q.ev, ctx->stream));
    q.pinned = pinned;
    q.n = n;
    q.nraw = 0;
    q.nimg = 1;
    q.tail_parity = -1;
    ctx->res_count++;
    if (filled) *filled = &q;
    return FNX_OK;
}

// MSSSIM's entry: five slots per image, `nlev` of them written; the fetch combines them with `weights` into nimg numbers
int publish_msssim(fnx_ctx *ctx, const double *pinned, int nimg, int nlev, const double (&weights)[5])
{
    fnx_ctx::Pending *q = nullptr;
    FNX_TRY(publish_results(ctx, pinned, nimg, &q));
    q->nraw = nlev;
    q->nimg = nimg;
    for (int i = 0; i < 5; i++) q->weights[i] = weights[i];
    return FNX_OK;
}

// While one lives, launch_windowed_ssim takes its partial sums from `partial_slot` (-1: the ctx's usual one) and, with
// on_tail, every launcher works on the ctx's second stream: the ctx is put back on every way out of the scope
class LaunchScope {
public:
    LaunchScope(fnx_ctx *ctx, int partial_slot, bool on_tail) : ctx_(ctx), main_(ctx->stream)
    {
        if (on_tail) ctx->stream = ctx->stream2;
        ctx->partial_slot = partial_slot;
    }
    ~LaunchScope() { ctx_->partial_slot = -1; ctx_->stream = main_; }
    LaunchScope(const LaunchScope &) = delete;
    LaunchScope &operator=(const LaunchScope &) = delete;
private:
    fnx_ctx *ctx_;
    hipStream_t main_;
};

// The tail stream waits for everything enqueued on `stream` so far (the one-pass batches' hand-over events, same use, in turn)
int tail_follows_main(fnx_ctx *ctx)
{
    hipEvent_t ev = ctx->ev_blur[ctx->ev_toggle];
    FNX_HIP(hipEventRecord(ev, ctx->stream));
    FNX_HIP(hipStreamWaitEvent(ctx->stream2, ev, 0));
    ctx->stream2_used = true;
    ctx->ev_toggle ^= 1;
    return FNX_OK;
}

// SSIM (ssim.go:35-42) of im.n device pairs into dres: pixelSSIM below 8 px, else toLuminance x2 + windowedSSIM at full resolution.
// as / bs: the HOST arrays of a batch's image pointers (uploaded for the windowed launch), or nullptr: the one pair im names.
// The values are left for result_wait (THEN_WAIT) or published as one FIFO entry.  THEN_PUBLISH_TAIL: the windowed SSIM runs on the
// ctx's second stream, behind everything enqueued so far (the images were produced on `stream`): what the caller enqueues next --
// the next image's AdaptiveSharpen in config 4 -- does not wait for it, so one kernel's last workgroups and the next one's first
// share the chip instead of each launch draining it (three launch boundaries per image, ~5 us each, at 8K).  The partial sums
// use the tail's own slot: other calls on `stream` may use SLOT_PARTIAL meanwhile.
enum SsimThen { THEN_WAIT, THEN_PUBLISH, THEN_PUBLISH_TAIL };
int ssim_pairs(fnx_ctx *ctx, ImgPairs im, const uint8_t *const *as, const uint8_t *const *bs, const double *window, const double *dwin, double *dres, SsimThen then)
{
    if (im.w < 8 || im.h < 8) {
        FNX_TRY(check_pix_lens(im.w, im.h, im.a.stride, im.b.stride));
        for (int i = 0; i < im.n; i++)
            FNX_TRY(launch_pixel_ssim(ctx, as ? as[i] : im.a.p, bs ? bs[i] : im.b.p, im.w, im.h, pix_len(im.w, im.h, im.a.stride), dres + i));
    } else {
        if (as) FNX_TRY(upload_ptr_pair(ctx, im.n, as, bs, &im.a.ptrs, &im.b.ptrs));
        if (then == THEN_PUBLISH_TAIL) {
            FNX_TRY(tail_follows_main(ctx));
            LaunchScope tail(ctx, SLOT_PART0, true);
            FNX_TRY(launch_windowed_ssim(ctx, im, window, dwin, dres));
            return publish_results(ctx, dres, im.n);          // the result's event: behind the score, on the second stream
        }
        FNX_TRY(launch_windowed_ssim(ctx, im, window, dwin, dres));
    }
    return then == THEN_WAIT ? FNX_OK : publish_results(ctx, dres, im.n);
}

}  // namespace

namespace fnx {

int check_img(const void *p, int stride, int w, int h, const char *what)
{
    if (w <= 0 || h <= 0) return FNX_OK;
    if (!p) {
        set_error("invalid argument: %s pixel pointer is null", what);
        return FNX_ERR_INVALID;
    }
    if (stride < w * 4 || (stride & 3)) {
        set_error("invalid argument: %s stride %d for width %d", what, stride, w);
        return FNX_ERR_INVALID;
    }
    return FNX_OK;
}

int check_space(int space)
{
    if (space != FNX_HOST && space != FNX_DEVICE) {
        set_error("invalid argument: space must be FNX_HOST or FNX_DEVICE");
        return FNX_ERR_INVALID;
    }
    return FNX_OK;
}

// image -> image ops also take FNX_DEVICE_SRC: device-resident source, host destination
int check_space_io(int space)
{
    if (space != FNX_HOST && space != FNX_DEVICE && space != FNX_DEVICE_SRC) {
        set_error("invalid argument: space must be FNX_HOST, FNX_DEVICE or FNX_DEVICE_SRC");
        return FNX_ERR_INVALID;
    }
    return FNX_OK;
}

// SSIMFast's dims (ssim.go:52-56)
bool ssim_fast_dims(int w, int h, int *nw, int *nh)
{
    *nw = w;
    *nh = h;
    const int maxDim = 512;
    if (w > maxDim || h > maxDim) {
        double scale = double(maxDim) / std::fmax(double(w), double(h));
        *nw = int(std::fmax(8, std::round(double(w) * scale)));
        *nh = int(std::fmax(8, std::round(double(h) * scale)));
        return true;
    }
    return false;
}

// n doubles the result kernels write into: pinned host memory mapped into the device's address
// space, so that a blocking entry point only has to wait for the stream (result_wait) -- no D2H copy
// The slots start out as NaN (no SSIM value is one: the denominators are >= C1*C2 > 0): the host can then
// watch them fill instead of waiting for the runtime's completion signal (poll_results).
int result_slot(fnx_ctx *ctx, int n, double **d)
{
    void *p = nullptr;
    FNX_TRY(pinned_alloc(ctx, sizeof(double) * static_cast<size_t>(n > 16 ? n : 16), &p));
    *d = static_cast<double *>(p);
    nan_fill(*d, n);
    return FNX_OK;
}

int upload_window(fnx_ctx *ctx, const double *window, const double **d_window)
{
    void *d = nullptr;
    FNX_TRY(upload_table(ctx, SLOT_TABLE0, window, sizeof(double) * 64, &d));
    *d_window = static_cast<const double *>(d);
    return FNX_OK;
}

int result_wait(fnx_ctx *ctx, const double *pinned, double *out, int n)
{
    FNX_TRY(poll_results(pinned, n, [&] { return hipStreamQuery(ctx->stream); }));
    std::memcpy(out, pinned, sizeof(double) * size_t(n));
    return FNX_OK;
}

// SSIMFast(prepared reference, device-resident candidate)
// b_is_plane: b is already the candidate's pw x ph plane (launch_box_downsample_ycc made it from the JPEG planes)
int against_device(fnx_ctx *ctx, const fnx_prepared *ref, const uint8_t *b, int bstride, const double *window,
                   double *out, bool b_is_plane)
{
    const int w = ref->w, h = ref->h, pw = ref->pw, ph = ref->ph;
    const double *dwin = nullptr;
    FNX_TRY(upload_window(ctx, window, &dwin));
    double *dres;
    FNX_TRY(result_slot(ctx, 1, &dres));
    const uint8_t *cb = b;
    int cbs = bstride;
    if (!b_is_plane && (pw != w || ph != h)) {
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_TMP2, static_cast<size_t>(pw) * ph * 4 + 16, &t));
        FNX_TRY(launch_box_downsample(ctx, 1, b, nullptr, bstride, w, h, static_cast<uint8_t *>(t), pw * 4, 0, pw, ph));
        cb = static_cast<const uint8_t *>(t);
        cbs = pw * 4;
    }
    if (pw < 8 || ph < 8) {
        // pixelSSIM walks both flat Pix slices; the prepared side is tight, so b must be too
        if (cbs != pw * 4) {
            void *t = nullptr;
            FNX_TRY(scratch(ctx, SLOT_TMP3, static_cast<size_t>(pw) * ph * 4 + 16, &t));
            FNX_HIP(hipMemcpy2DAsync(t, size_t(pw) * 4, cb, cbs, size_t(pw) * 4, ph, hipMemcpyDeviceToDevice, ctx->stream));
            cb = static_cast<const uint8_t *>(t);
        }
        FNX_TRY(launch_pixel_ssim(ctx, ref->pix, cb, pw, ph, static_cast<size_t>(pw) * ph * 4, dres));
    } else {
        FNX_TRY(launch_windowed_ssim(ctx, one_pair(ref->pix, pw * 4, cb, cbs, pw, ph), window, dwin, dres));
    }
    return result_wait(ctx, dres, out, 1);
}

// SSIMFast's side of a prepared reference (ssim.go:57): the device image src, ref.w x ref.h, box-downsampled into ref.pix
// when ssim_fast_dims shrank it, else copied there tight
int prepared_plane(fnx_ctx *ctx, const uint8_t *src, int sstride, const fnx_prepared &ref)
{
    const int w = ref.w, h = ref.h;
    if (ref.pw != w || ref.ph != h) return launch_box_downsample(ctx, 1, src, nullptr, sstride, w, h, ref.pix, ref.pw * 4, 0, ref.pw, ref.ph);
    FNX_HIP(hipMemcpy2DAsync(ref.pix, size_t(w) * 4, src, sstride, size_t(w) * 4, h, hipMemcpyDeviceToDevice, ctx->stream));
    return FNX_OK;
}

int lanczos_resize_tables(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW, int srcH,
                          const TapTable &th, const TapTable &tv, uint8_t *dst, int dstride, int dstW, int dstH)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    if (srcW <= 0 || srcH <= 0 || dstW <= 0 || dstH <= 0) return FNX_EMPTY;   // resize.go:41-43
    FNX_TRY(check_img(src, sstride, srcW, srcH, "src"));
    FNX_TRY(check_img(dst, dstride, dstW, dstH, "dst"));
    if (srcW == dstW && srcH == dstH) {   // flat copy of Pix (resize.go:45-49): no tables
        const size_t sl = pix_len(srcW, srcH, sstride), dl = pix_len(dstW, dstH, dstride);
        const size_t nbytes = sl < dl ? sl : dl;
        if (space == FNX_HOST) {
            std::memcpy(dst, src, nbytes);
        } else if (space == FNX_DEVICE_SRC) {
            FNX_HIP(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToHost, ctx->stream));
            FNX_HIP(hipStreamSynchronize(ctx->stream));
        } else {
            FNX_HIP(hipMemcpyAsync(dst, src, nbytes, hipMemcpyDeviceToDevice, ctx->stream));
        }
        return FNX_OK;
    }
    FNX_REQUIRE(th.off && th.idx && th.wt && tv.off && tv.idx && tv.wt, "tap table is null");
    DevImg s;
    DevOut d;
    FNX_TRY(stage_in(ctx, space, src, sstride, srcW, srcH, SLOT_IN_A, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, dstW, dstH, SLOT_OUT, &d));
    // both passes in one launch where the tables allow it (the uint8 intermediate stays in LDS)
    {
        const int rc = resize_fused(ctx, th, tv, s.p, s.stride, srcW, srcH, d.p, d.stride);
        if (rc < 0) return rc;
        if (rc != FNX_NOOP) return finish(ctx, space, &d);
    }
    // uint8 intermediate dstW x srcH (resize.go:51)
    const int tp = pitch16(dstW);
    void *tmp = nullptr;
    // ... followed by the H pass's verdict cells for the V pass (ResizeHint): at most one per 128 x 8 tmp pixels
    const size_t tmp_bytes = (static_cast<size_t>(tp) * srcH + 16 + 15) & ~size_t(15);
    ResizeHint hint;
    hint.cap = (static_cast<size_t>(dstW) / 128 + 2) * (static_cast<size_t>(srcH) / 8 + 2);
    FNX_TRY(scratch(ctx, SLOT_TMP0, tmp_bytes + sizeof(uint32_t) * hint.cap, &tmp));
    hint.cells = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(tmp) + tmp_bytes);
    FNX_TRY(resize_pass(ctx, false, th, s.p, s.stride, srcW, srcH, static_cast<uint8_t *>(tmp), tp, &hint));
    FNX_TRY(resize_pass(ctx, true, tv, static_cast<const uint8_t *>(tmp), tp, dstW, srcH, d.p, d.stride, &hint));
    return finish(ctx, space, &d);
}

// n same-geometry device images through ONE set of launches where resize_fused applies (every launch then holds n images'
// workgroups: a 4K call alone is 700 workgroups for 768-1024 slots -- one under-filled round), else image by image
int lanczos_resize_tables_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int srcW, int srcH,
                                const TapTable &th, const TapTable &tv, uint8_t *const *dsts, int dstride, int dstW, int dstH)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_batch(n, srcs && dsts));
    if (n == 0) return FNX_OK;
    if (srcW <= 0 || srcH <= 0 || dstW <= 0 || dstH <= 0) return FNX_EMPTY;   // resize.go:41-43
    FNX_REQUIRE((srcW == dstW && srcH == dstH) || (th.off && th.idx && th.wt && tv.off && tv.idx && tv.wt), "tap table is null");
    FNX_TRY(check_batch_images(n, {srcs, sstride, srcW, srcH, "src"}, {dsts, dstride, dstW, dstH, "dst"}));
    if (n > 1 && !(srcW == dstW && srcH == dstH)) {
        const uint8_t *const *d_srcs;
        uint8_t *const *d_dsts;
        FNX_TRY(upload_ptr_pair(ctx, n, srcs, dsts, &d_srcs, &d_dsts));
        const int rc = resize_fused(ctx, th, tv, srcs[0], sstride, srcW, srcH, dsts[0], dstride, n, d_srcs, d_dsts);
        if (rc < 0) return rc;
        if (rc != FNX_NOOP) return FNX_OK;
    }
    for (int i = 0; i < n; i++) {
        const int rc = lanczos_resize_tables(ctx, FNX_DEVICE, srcs[i], sstride, srcW, srcH, th, tv, dsts[i], dstride, dstW, dstH);
        if (rc < 0) return rc;
    }
    return FNX_OK;
}

// boxDownsample(lanczosResize(src, midW, midH), dstW, dstH) of a device image: lanczosResize into `up_slot` and the box
// kernel, or -- form "resize_box" "1", where it applies -- resize_box_kernel.  The fused kernel is not the default: it has
// not been timed against the resize kernels + box kernel it would replace (fp64 reference-order arithmetic against fp32 /
// matrix-pipe kernels plus a round trip of the image through memory)
int lanczos_box_device(fnx_ctx *ctx, const uint8_t *src, int sstride, int srcW, int srcH, const TapTable &th, const TapTable &tv,
                       int midW, int midH, uint8_t *dst, int dstride, int dstW, int dstH, Slot up_slot)
{
    const char *form = form_value(ctx, FORM_RESIZE_BOX);
    if (form && form[0] == '1' && !(srcW == midW && srcH == midH)) {
        const int rc = launch_resize_box(ctx, src, sstride, srcW, srcH, th, tv, midW, midH, dst, dstride, dstW, dstH);
        if (rc < 0) return rc;
        if (rc != FNX_NOOP) return FNX_OK;
    }
    void *up = nullptr;
    FNX_TRY(scratch(ctx, up_slot, static_cast<size_t>(midW) * midH * 4 + 16, &up));
    FNX_TRY(lanczos_resize_tables(ctx, FNX_DEVICE, src, sstride, srcW, srcH, th, tv, static_cast<uint8_t *>(up), midW * 4, midW, midH));
    return launch_box_downsample(ctx, 1, static_cast<const uint8_t *>(up), nullptr, midW * 4, midW, midH, dst, dstride, 0, dstW, dstH);
}

// computeSSIMNRGBA's tail (targetsize.go:563-568) against a prepared `a`: where SSIMFast downsamples, only the box plane of
// lanczosResize(b) is made (SLOT_TMP2, where against_device would put it); an `a` of at most 512 px is compared at full size
int ssim_fast_resized_device(fnx_ctx *ctx, const fnx_prepared *ref, const uint8_t *b, int bstride, int bw, int bh,
                             const TapTable &th, const TapTable &tv, const double *window, double *out)
{
    const int w = ref->w, h = ref->h, pw = ref->pw, ph = ref->ph;
    if (bw == w && bh == h) return against_device(ctx, ref, b, bstride, window, out);
    if (pw != w || ph != h) {
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_TMP2, static_cast<size_t>(pw) * ph * 4 + 16, &t));
        FNX_TRY(lanczos_box_device(ctx, b, bstride, bw, bh, th, tv, w, h, static_cast<uint8_t *>(t), pw * 4, pw, ph, SLOT_TS_UP));
        return against_device(ctx, ref, static_cast<const uint8_t *>(t), pw * 4, window, out, true);
    }
    void *up = nullptr;
    FNX_TRY(scratch(ctx, SLOT_TS_UP, static_cast<size_t>(w) * h * 4 + 16, &up));
    FNX_TRY(lanczos_resize_tables(ctx, FNX_DEVICE, b, bstride, bw, bh, th, tv, static_cast<uint8_t *>(up), w * 4, w, h));
    return against_device(ctx, ref, static_cast<const uint8_t *>(up), w * 4, window, out);
}

// What the *_resized entry points share before any work (ssim.go:31-33 with an empty side): *done = true with the call's
// status when there is nothing left to do
static int resized_guard(int space, int aw, int ah, int bw, int bh, const void *a, int astride, const void *b, int bstride,
                         const TapTable &th, const TapTable &tv, const char *what, bool *empty_a)
{
    FNX_TRY(check_space(space));
    *empty_a = aw <= 0 || ah <= 0;
    if (*empty_a) return FNX_OK;
    if (bw <= 0 || bh <= 0) {
        // lanczosResize hands back a 0x0 image; pixelSSIM / the windows then index past it for a non-empty `a`
        set_error("%s: second image is empty (the reference panics)", what);
        return FNX_ERR_INVALID;
    }
    FNX_TRY(check_img(a, astride, aw, ah, "a"));
    FNX_TRY(check_img(b, bstride, bw, bh, "b"));
    FNX_REQUIRE(th.off && th.idx && th.wt && tv.off && tv.idx && tv.wt, "tap table is null");
    return FNX_OK;
}

int resize_b_device(fnx_ctx *ctx, int space, const uint8_t *b, int bstride, int bw, int bh, const TapTable &th, const TapTable &tv,
                           int w, int h, const uint8_t **out, int *ostride)
{
    void *d = nullptr;
    FNX_TRY(scratch(ctx, SLOT_TMP3, static_cast<size_t>(w) * h * 4 + 16, &d));
    DevImg s;
    FNX_TRY(stage_in(ctx, space, b, bstride, bw, bh, SLOT_IN_B, &s));
    FNX_TRY(lanczos_resize_tables(ctx, FNX_DEVICE, s.p, s.stride, bw, bh, th, tv, static_cast<uint8_t *>(d), w * 4, w, h));
    *out = static_cast<const uint8_t *>(d);
    *ostride = w * 4;
    return FNX_OK;
}

int ssim_resized_tables(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah, const uint8_t *b, int bstride, int bw, int bh,
                        const TapTable &th, const TapTable &tv, const double *window, double *out)
{
    if (aw == bw && ah == bh) return fnx_ssim(ctx, space, a, astride, b, bstride, aw, ah, window, out);
    FNX_ENTER(ctx);
    FNX_REQUIRE(window && out, "window/out is null");
    bool empty_a;
    FNX_TRY(resized_guard(space, aw, ah, bw, bh, a, astride, b, bstride, th, tv, "SSIM", &empty_a));
    if (empty_a) { *out = 1.0; return FNX_OK; }     // pixelSSIM: n == 0 (ssim.go:172-175)
    const uint8_t *rb;
    int rbs;
    FNX_TRY(resize_b_device(ctx, space, b, bstride, bw, bh, th, tv, aw, ah, &rb, &rbs));
    DevImg da;
    FNX_TRY(stage_in(ctx, space, a, astride, aw, ah, SLOT_IN_A, &da));
    return fnx_ssim(ctx, FNX_DEVICE, da.p, da.stride, rb, rbs, aw, ah, window, out);
}

int msssim_resized_tables(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah, const uint8_t *b, int bstride, int bw, int bh,
                          const TapTable &th, const TapTable &tv, const double *window, double *out, double *per_level)
{
    if (aw == bw && ah == bh) return fnx_msssim(ctx, space, a, astride, b, bstride, aw, ah, window, out, per_level);
    FNX_ENTER(ctx);
    FNX_REQUIRE(window && out, "window/out is null");
    bool empty_a;
    FNX_TRY(resized_guard(space, aw, ah, bw, bh, a, astride, b, bstride, th, tv, "MSSSIM", &empty_a));
    if (empty_a) return fnx_msssim(ctx, space, a, astride, a, astride, aw, ah, window, out, per_level);
    const uint8_t *rb;
    int rbs;
    FNX_TRY(resize_b_device(ctx, space, b, bstride, bw, bh, th, tv, aw, ah, &rb, &rbs));
    DevImg da;
    FNX_TRY(stage_in_front(ctx, space, a, aw, ah, SLOT_IN_A, &da));      // toNRGBA(a): the flat front of a.Pix (ssim.go:345)
    return fnx_msssim(ctx, FNX_DEVICE, da.p, da.stride, rb, rbs, aw, ah, window, out, per_level);
}

int ssim_fast_resized_tables(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah, const uint8_t *b, int bstride, int bw,
                             int bh, const TapTable &th, const TapTable &tv, const double *window, double *out)
{
    if (aw == bw && ah == bh) return fnx_ssim_fast(ctx, space, a, astride, b, bstride, aw, ah, window, out);
    FNX_ENTER(ctx);
    FNX_REQUIRE(window && out, "window/out is null");
    bool empty_a;
    FNX_TRY(resized_guard(space, aw, ah, bw, bh, a, astride, b, bstride, th, tv, "computeSSIMNRGBA", &empty_a));
    if (empty_a) { *out = 1.0; return FNX_OK; }
    // pixelSSIM walks a's flat Pix slice and indexes the resized b (a fresh tight image) with it (ssim.go:178)
    FNX_REQUIRE((aw >= 8 && ah >= 8) || astride == aw * 4, "a under 8 px must be tight (the reference indexes past the resized image)");
    DevImg da, db;
    FNX_TRY(stage_in(ctx, space, a, astride, aw, ah, SLOT_IN_A, &da));
    FNX_TRY(stage_in(ctx, space, b, bstride, bw, bh, SLOT_IN_B, &db));
    fnx_prepared ref;
    ref.w = aw;
    ref.h = ah;
    ssim_fast_dims(aw, ah, &ref.pw, &ref.ph);
    void *rp = nullptr;
    FNX_TRY(scratch(ctx, SLOT_TMP1, static_cast<size_t>(ref.pw) * ref.ph * 4 + 16, &rp));
    ref.pix = static_cast<uint8_t *>(rp);
    FNX_TRY(prepared_plane(ctx, da.p, da.stride, ref));
    return ssim_fast_resized_device(ctx, &ref, db.p, db.stride, bw, bh, th, tv, window, out);
}

int lanczos_box_tables(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW, int srcH, const TapTable &th, const TapTable &tv,
                       int midW, int midH, uint8_t *dst, int dstride, int dstW, int dstH)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    if (srcW <= 0 || srcH <= 0 || midW <= 0 || midH <= 0 || dstW <= 0 || dstH <= 0) return FNX_EMPTY;   // resize.go:41-43, ssim.go:246-248
    FNX_TRY(check_img(src, sstride, srcW, srcH, "src"));
    FNX_TRY(check_img(dst, dstride, dstW, dstH, "dst"));
    FNX_REQUIRE((srcW == midW && srcH == midH) || (th.off && th.idx && th.wt && tv.off && tv.idx && tv.wt), "tap table is null");
    DevImg s;
    DevOut d;
    FNX_TRY(stage_in(ctx, space, src, sstride, srcW, srcH, SLOT_IN_A, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, dstW, dstH, SLOT_OUT, &d));
    FNX_TRY(lanczos_box_device(ctx, s.p, s.stride, srcW, srcH, th, tv, midW, midH, d.p, d.stride, dstW, dstH, SLOT_TS_UP));
    return finish(ctx, space, &d);
}

}  // namespace fnx

extern "C" {

static int blur_batch_body(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h, const double *kernel, int radius,
                           int flags, uint8_t *const *dsts, int dstride);

int fnx_gaussian_blur(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                      const double *kernel, int radius, int flags, uint8_t *dst, int dstride)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_REQUIRE(kernel != nullptr && radius >= 0, "blur kernel");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    FNX_TRY(check_img(dst, dstride, w, h, "dst"));
    if (w <= 0 || h <= 0) return FNX_OK;
    FNX_REQUIRE(space != FNX_DEVICE || src != dst, "dst aliases src (the blur is not in-place)");
    ctx->kept.valid = false;
    if ((flags & FNX_BLUR_KEEP_BOX_SUMS) && space == FNX_DEVICE && !(sstride & 3) && !(dstride & 3))   // a batch of one (fnx_ssim_fast consumes it)
        return blur_batch_body(ctx, 1, &src, sstride, w, h, kernel, radius, flags, &dst, dstride);
    flags &= ~FNX_BLUR_KEEP_BOX_SUMS;
    DevImg s;
    DevOut d;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, w, h, SLOT_OUT, &d));
    FNX_TRY(launch_blur(ctx, 1, s.p, nullptr, s.stride, w, h, kernel, radius, flags, d.p, nullptr, d.stride));
    return finish(ctx, space, &d);
}

int fnx_gaussian_blur_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w,
                            int h, const double *kernel, int radius, int flags,
                            uint8_t *const *dsts, int dstride)
{
    FNX_ENTER(ctx);
    return blur_batch_body(ctx, n, srcs, sstride, w, h, kernel, radius, flags, dsts, dstride);
}

static int blur_batch_body(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h, const double *kernel, int radius,
                           int flags, uint8_t *const *dsts, int dstride)
{
    FNX_REQUIRE(n >= 0 && srcs && dsts && kernel && radius >= 0, "batch arguments");
    if (n == 0 || w <= 0 || h <= 0) return FNX_OK;
    FNX_REQUIRE(sstride >= 4 * w && dstride >= 4 * w && !(sstride & 3) && !(dstride & 3), "stride");
    for (int i = 0; i < n; i++) FNX_REQUIRE(srcs[i] && dsts[i] && srcs[i] != dsts[i], "null image in batch, or dst aliases src (the blur is not in-place)");
    const uint8_t *const *d_srcs;
    uint8_t *const *d_dsts;
    FNX_TRY(upload_ptr_pair(ctx, n, srcs, dsts, &d_srcs, &d_dsts));
    const bool keep = (flags & FNX_BLUR_KEEP_BOX_SUMS) != 0;
    flags &= ~FNX_BLUR_KEEP_BOX_SUMS;
    ctx->kept.valid = false;
    int nw, nh;
    if (keep && ssim_fast_dims(w, h, &nw, &nh) && nw >= 8 && nh >= 8) {
        // the one-pass kernel (fnx_gaussian_blur_ssim_fast_batch's first half): the same blurred bytes, and the box planes of both
        // sides into buffer set p.  The set stays this batch's until the scoring call -- or, if none comes, until the next
        // one-pass launch on it (ordered behind this one on `stream`).
        const int p = ctx->parity;
        const size_t plane = static_cast<size_t>(nw) * nh * 4;
        void *t = nullptr;
        FNX_TRY(scratch(ctx, p ? SLOT_PLANES1 : SLOT_PLANES0, plane * 2 * n + 16, &t));
        if (ctx->tail_pending[p]) FNX_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_tail[p], 0));
        ctx->boxes_on_main = true;               // blur, box planes and (next call) the windowed SSIM back to back on `stream`
        const int st = launch_blur_scored(ctx, n, d_srcs, sstride, w, h, kernel, radius, flags, d_dsts, dstride,
                                          static_cast<uint8_t *>(t), plane, nw, nh);
        ctx->boxes_on_main = false;
        if (st < 0) return st;
        if (st == FNX_OK) {
            ctx->tail_pending[p] = false;        // whatever read set p before is in front of this blur on `stream`, and so is all that follows
            fnx_ctx::KeptBoxes &k = ctx->kept;
            k.srcs.assign(srcs, srcs + n);
            k.dsts.assign(dsts, dsts + n);
            k.n = n; k.sstride = sstride; k.dstride = dstride; k.w = w; k.h = h; k.nw = nw; k.nh = nh; k.parity = p;
            k.planes = static_cast<uint8_t *>(t); k.plane = plane;
            k.seq = ctx->op_seq;
            k.valid = true;
            return FNX_OK;
        }
        // FNX_NOOP: a shape the one-pass kernel is not built for -- the plain blur, nothing kept
    }
    return launch_blur(ctx, n, nullptr, d_srcs, sstride, w, h, kernel, radius, flags, nullptr, d_dsts, dstride);
}

// The effects read a SubImage (sstride != 4w) two ways: by rows, and as the flat front of its Pix slice
// (copy(dst.Pix, img.Pix), effects.go:68,120 -- see fx_flat_kernel): a host source of that kind goes up as the
// slice it is, stride kept, instead of being packed row by row.
static int stage_fx_src(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, DevImg *s)
{
    return sstride != w * 4 ? stage_in_flat(ctx, space, src, sstride, w, h, SLOT_IN_A, s)
                            : stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, s);
}

int fnx_blur3x3(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                uint8_t *dst, int dstride)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    FNX_TRY(check_img(dst, dstride, w, h, "dst"));
    if (w <= 0 || h <= 0) return FNX_OK;
    DevImg s;
    DevOut d;
    FNX_TRY(stage_fx_src(ctx, space, src, sstride, w, h, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, w, h, SLOT_OUT, &d));
    FNX_TRY(launch_blur3x3(ctx, s.p, s.stride, w, h, d.p, d.stride));
    return finish(ctx, space, &d);
}

static int sharpen_common(fnx_ctx *ctx, bool adaptive, int space, const uint8_t *src, int sstride,
                          int w, int h, double amount, uint8_t *dst, int dstride)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_REQUIRE(w >= 3 && h >= 3, "sharpen needs w,h >= 3 (the reference returns the input below that)");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    FNX_TRY(check_img(dst, dstride, w, h, "dst"));
    DevImg s;
    DevOut d;
    FNX_TRY(stage_fx_src(ctx, space, src, sstride, w, h, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, w, h, SLOT_OUT, &d));
    FNX_TRY(launch_sharpen(ctx, adaptive, s.p, s.stride, w, h, amount, d.p, d.stride));
    return finish(ctx, space, &d);
}

int fnx_sharpen(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                double amount, uint8_t *dst, int dstride)
{
    return sharpen_common(ctx, false, space, src, sstride, w, h, amount, dst, dstride);
}

int fnx_adaptive_sharpen(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                         double amount, uint8_t *dst, int dstride)
{
    return sharpen_common(ctx, true, space, src, sstride, w, h, amount, dst, dstride);
}

// n same-geometry device images in ONE launch of the streaming kernel (tight images); anything else image by image
static int sharpen_batch_common(fnx_ctx *ctx, bool adaptive, int n, const uint8_t *const *srcs, int sstride, int w, int h, double amount,
                                uint8_t *const *dsts, int dstride)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_batch(n, srcs && dsts));
    if (n == 0) return FNX_OK;
    FNX_REQUIRE(w >= 3 && h >= 3, "sharpen needs w,h >= 3 (the reference returns the input below that)");
    FNX_TRY(check_batch_images(n, {srcs, sstride, w, h, "src"}, {dsts, dstride, w, h, "dst"}, "null image in batch, or dst aliases src"));
    if (n > 1) {
        const uint8_t *const *d_srcs;
        uint8_t *const *d_dsts;
        FNX_TRY(upload_ptr_pair(ctx, n, srcs, dsts, &d_srcs, &d_dsts));
        const int rc = launch_sharpen_batch(ctx, adaptive, n, srcs[0], d_srcs, sstride, w, h, amount, dsts[0], d_dsts, dstride);
        if (rc < 0) return rc;
        if (rc != FNX_NOOP) return FNX_OK;
    }
    for (int i = 0; i < n; i++) FNX_TRY(launch_sharpen(ctx, adaptive, srcs[i], sstride, w, h, amount, dsts[i], dstride));
    return FNX_OK;
}

int fnx_sharpen_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h, double amount,
                      uint8_t *const *dsts, int dstride)
{
    return sharpen_batch_common(ctx, false, n, srcs, sstride, w, h, amount, dsts, dstride);
}

int fnx_adaptive_sharpen_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h, double amount,
                               uint8_t *const *dsts, int dstride)
{
    return sharpen_batch_common(ctx, true, n, srcs, sstride, w, h, amount, dsts, dstride);
}

// ---- resize ------------------------------------------------------------------------
int fnx_resize_h(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW, int srcH,
                 const int32_t *offset, const int32_t *index, const double *weight,
                 uint8_t *dst, int dstride, int dstW)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_REQUIRE(srcW > 0 && srcH > 0 && dstW > 0, "dims");
    FNX_REQUIRE(offset && index && weight, "tap table is null");
    FNX_TRY(check_img(src, sstride, srcW, srcH, "src"));
    FNX_TRY(check_img(dst, dstride, dstW, srcH, "dst"));
    DevImg s;
    DevOut d;
    FNX_TRY(stage_in(ctx, space, src, sstride, srcW, srcH, SLOT_IN_A, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, dstW, srcH, SLOT_OUT, &d));
    const TapTable t{offset, index, weight, dstW, 0};
    FNX_TRY(resize_pass(ctx, false, t, s.p, s.stride, srcW, srcH, d.p, d.stride));
    return finish(ctx, space, &d);
}

int fnx_resize_v(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW, int srcH,
                 const int32_t *offset, const int32_t *index, const double *weight,
                 uint8_t *dst, int dstride, int dstH)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_REQUIRE(srcW > 0 && srcH > 0 && dstH > 0, "dims");
    FNX_REQUIRE(offset && index && weight, "tap table is null");
    FNX_TRY(check_img(src, sstride, srcW, srcH, "src"));
    FNX_TRY(check_img(dst, dstride, srcW, dstH, "dst"));
    DevImg s;
    DevOut d;
    FNX_TRY(stage_in(ctx, space, src, sstride, srcW, srcH, SLOT_IN_A, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, srcW, dstH, SLOT_OUT, &d));
    const TapTable t{offset, index, weight, dstH, 0};
    FNX_TRY(resize_pass(ctx, true, t, s.p, s.stride, srcW, srcH, d.p, d.stride));
    return finish(ctx, space, &d);
}

int fnx_lanczos_resize(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW,
                       int srcH, const int32_t *offH, const int32_t *idxH, const double *wH,
                       const int32_t *offV, const int32_t *idxV, const double *wV,
                       uint8_t *dst, int dstride, int dstW, int dstH)
{
    const TapTable th{offH, idxH, wH, dstW, 0}, tv{offV, idxV, wV, dstH, 0};
    return fnx::lanczos_resize_tables(ctx, space, src, sstride, srcW, srcH, th, tv, dst, dstride, dstW, dstH);
}

int fnx_lanczos_resize_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int srcW, int srcH,
                             const int32_t *offH, const int32_t *idxH, const double *wH,
                             const int32_t *offV, const int32_t *idxV, const double *wV,
                             uint8_t *const *dsts, int dstride, int dstW, int dstH)
{
    const TapTable th{offH, idxH, wH, dstW, 0}, tv{offV, idxV, wV, dstH, 0};
    return fnx::lanczos_resize_tables_batch(ctx, n, srcs, sstride, srcW, srcH, th, tv, dsts, dstride, dstW, dstH);
}

// ---- ssim.go -----------------------------------------------------------------------
int fnx_box_downsample(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW,
                       int srcH, uint8_t *dst, int dstride, int dstW, int dstH)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    if (srcW <= 0 || srcH <= 0 || dstW <= 0 || dstH <= 0) return FNX_EMPTY;   // ssim.go:246-248
    FNX_TRY(check_img(src, sstride, srcW, srcH, "src"));
    FNX_TRY(check_img(dst, dstride, dstW, dstH, "dst"));
    DevImg s;
    DevOut d;
    FNX_TRY(stage_in(ctx, space, src, sstride, srcW, srcH, SLOT_IN_A, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, dstW, dstH, SLOT_OUT, &d));
    FNX_TRY(launch_box_downsample(ctx, 1, s.p, nullptr, s.stride, srcW, srcH, d.p, d.stride, 0, dstW, dstH));
    return finish(ctx, space, &d);
}

// the box planes a blur with FNX_BLUR_KEEP_BOX_SUMS left for exactly this scoring call?  (Either way they are gone afterwards.)
static bool kept_matches(fnx_ctx *ctx, int n, const uint8_t *const *as, int astride, const uint8_t *const *bs, int bstride, int w, int h)
{
    fnx_ctx::KeptBoxes &k = ctx->kept;
    bool use = k.valid && k.seq + 1 == ctx->op_seq && k.n == n && k.sstride == astride && k.dstride == bstride && k.w == w && k.h == h;
    for (int i = 0; use && i < n; i++) use = as[i] == k.srcs[i] && bs[i] == k.dsts[i];
    k.valid = false;
    return use;
}

// fnx_gaussian_blur_ssim_fast_batch's second half, on the main stream right behind the planes (the kept form's box_from_slabs_kernel
// ran there too): neither full-size image is read again
static int kept_score(fnx_ctx *ctx, int n, const double *window, const double *dwin, double *dres, bool batch_form)
{
    fnx_ctx::KeptBoxes &k = ctx->kept;
    {   // (the one-pass entry's arithmetic; a single call keeps its own)
        LaunchScope own(ctx, !batch_form ? -1 : k.parity ? SLOT_PART1 : SLOT_PART0, false);
        FNX_TRY(launch_windowed_ssim(ctx, plane_pairs(n, k.planes, k.planes + k.plane * n, k.plane, k.nw, k.nh), window, dwin, dres));
    }
    note_route(ctx, FNX_PROF_SSIM, "kept box planes + windowed SSIM");
    ctx->parity ^= 1;
    return FNX_OK;
}

int fnx_ssim_fast(fnx_ctx *ctx, int space, const uint8_t *a, int astride, const uint8_t *b,
                  int bstride, int w, int h, const double *window, double *out)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(window && out, "window/out is null");
    FNX_TRY(check_img(a, astride, w, h, "a"));
    FNX_TRY(check_img(b, bstride, w, h, "b"));
    if (w <= 0 || h <= 0) {   // pixelSSIM: n == 0 -> 1.0 (ssim.go:172-175)
        *out = 1.0;
        return FNX_OK;
    }
    const double *dwin = nullptr;
    FNX_TRY(upload_window(ctx, window, &dwin));
    if (kept_matches(ctx, 1, &a, astride, &b, bstride, w, h) && space == FNX_DEVICE) {
        double *dres;
        FNX_TRY(result_slot(ctx, 1, &dres));
        FNX_TRY(kept_score(ctx, 1, window, dwin, dres, false));
        return result_wait(ctx, dres, out, 1);
    }
    DevImg da, db;
    int nw, nh;
    const bool pixel = !ssim_fast_dims(w, h, &nw, &nh) && (w < 8 || h < 8);   // pixelSSIM on the inputs themselves
    FNX_TRY(stage_pair(ctx, space, a, astride, b, bstride, w, h, pixel, &da, &db));
    double *dres;
    FNX_TRY(result_slot(ctx, 1, &dres));
    FNX_TRY(ssim_fast_device(ctx, one_pair(da.p, da.stride, db.p, db.stride, w, h), window, dwin, dres));
    return result_wait(ctx, dres, out, 1);
}

int fnx_ssim_fast_batch(fnx_ctx *ctx, int n, const uint8_t *const *as, int astride,
                        const uint8_t *const *bs, int bstride, int w, int h,
                        const double *window, double *out)
{
    FNX_REQUIRE(out != nullptr, "out is null");
    FNX_REQUIRE(ctx && ctx->res_count == 0, "enqueued batches are waiting for fnx_results_fetch: fetch them before a blocking batch call");
    FNX_TRY(fnx_ssim_fast_batch_enqueue(ctx, n, as, astride, bs, bstride, w, h, window));
    return fnx_results_fetch(ctx, n, out);
}

int fnx_results_fetch(fnx_ctx *ctx, int n, double *out)
{
    FNX_ENTER(ctx);
    FNX_REQUIRE(n >= 0 && out, "fetch arguments");
    if (n == 0) return FNX_OK;
    FNX_REQUIRE(ctx->res_count > 0 && n <= ctx->res_q[ctx->res_head].n, "no enqueued results of that size on this ctx");
    fnx_ctx::Pending &q = ctx->res_q[ctx->res_head];            // oldest unfetched batch
    if (q.nraw > 0) {                                            // enqueued MSSSIMs: levels -> the weighted product, image by image
        for (int i = 0; i < n; i++) {
            FNX_TRY(poll_results(q.pinned + 5 * i, q.nraw, [&] { return hipEventQuery(q.ev); }));
            out[i] = msssim_combine(q.pinned + 5 * i, q.weights, q.nraw);
        }
    } else {
        FNX_TRY(poll_results(q.pinned, n, [&] { return hipEventQuery(q.ev); }));
        std::memcpy(out, q.pinned, sizeof(double) * size_t(n));
    }
    // a one-pass batch whose results have arrived has read its slabs / planes / partial sums for the last time: the
    // step that reuses the buffer set needs no stream-side wait for this tail (one barrier packet less per step)
    // -- only when ALL of the batch's results were polled: a partial fetch (n < q.n) has seen images 0..n-1 done while the
    // tail may still be reading the slabs and planes of the others (each image's last workgroup publishes its own mean)
    if (q.tail_parity >= 0 && q.tail_gen == ctx->tail_gen[q.tail_parity] && (q.nraw > 0 || n == q.n)) ctx->tail_pending[q.tail_parity] = false;
    ctx->res_head = (ctx->res_head + 1) % fnx_ctx::RES_DEPTH;
    ctx->res_count--;
    return FNX_OK;
}

int fnx_ssim_fast_batch_enqueue(fnx_ctx *ctx, int n, const uint8_t *const *as, int astride,
                                const uint8_t *const *bs, int bstride, int w, int h,
                                const double *window)
{
    FNX_ENTER(ctx);
    FNX_REQUIRE(n >= 0 && as && bs && window, "batch arguments");
    if (n == 0) return FNX_OK;
    FNX_REQUIRE(w > 0 && h > 0 && astride >= 4 * w && bstride >= 4 * w, "dims");
    FNX_TRY(can_enqueue(ctx));
    const double *dwin = nullptr;
    FNX_TRY(upload_window(ctx, window, &dwin));
    double *dres;
    FNX_TRY(result_slot_queued(ctx, n, &dres));
    if (kept_matches(ctx, n, as, astride, bs, bstride, w, h)) {
        FNX_TRY(kept_score(ctx, n, window, dwin, dres, true));
        return publish_results(ctx, dres, n);
    }
    int nw, nh;
    for (int i = 0; i < n; i++) FNX_REQUIRE(as[i] && bs[i], "null image in batch");
    if (ssim_fast_dims(w, h, &nw, &nh) && all_aligned16(n, as, astride) && all_aligned16(n, bs, bstride)) {
        const uint8_t *const *d_as, *const *d_bs;
        FNX_TRY(upload_ptr_pair(ctx, n, as, bs, &d_as, &d_bs));
        FNX_TRY(ssim_fast_device(ctx, pairs_by_pointer(n, d_as, astride, d_bs, bstride, w, h), window, dwin, dres));
    } else {
        for (int i = 0; i < n; i++)
            FNX_TRY(ssim_fast_device(ctx, one_pair(as[i], astride, bs[i], bstride, w, h), window, dwin, dres + i));
    }
    return publish_results(ctx, dres, n);
}

int fnx_gaussian_blur_ssim_fast_batch_enqueue(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride,
                                              int w, int h, const double *kernel, int radius, int flags,
                                              uint8_t *const *dsts, int dstride, const double *window)
{
    FNX_ENTER(ctx);
    FNX_REQUIRE(n >= 0 && srcs && dsts && kernel && radius >= 0 && window, "batch arguments");
    if (n == 0) return FNX_OK;
    FNX_REQUIRE(w > 0 && h > 0, "dims");
    FNX_REQUIRE(sstride >= 4 * w && dstride >= 4 * w && !(sstride & 3) && !(dstride & 3), "stride");
    for (int i = 0; i < n; i++) FNX_REQUIRE(srcs[i] && dsts[i] && srcs[i] != dsts[i], "null image in batch, or dst aliases src (the blur is not in-place)");
    FNX_TRY(can_enqueue(ctx));
    int nw, nh;
    const bool down = ssim_fast_dims(w, h, &nw, &nh);
    if (down && nw >= 8 && nh >= 8) {
        // one pass: the blur kernel also accumulates both boxDownsample planes.  Buffer set p (slabs, planes,
        // partial sums) belongs to this step; the blur waits for the tail that used it two steps ago, and the
        // step's own tail -- box_from_slabs, windowed SSIM, finish -- runs on the second stream, i.e. under the
        // blur of whatever step the caller enqueues next.
        const int p = ctx->parity;
        const uint8_t *const *d_srcs;
        uint8_t *const *d_dsts;
        FNX_TRY(upload_ptr_pair(ctx, n, srcs, dsts, &d_srcs, &d_dsts));
        const double *dwin = nullptr;
        FNX_TRY(upload_window(ctx, window, &dwin));   // before the blur: uploads ride on `stream`
        const size_t plane = static_cast<size_t>(nw) * nh * 4;
        void *t = nullptr;
        FNX_TRY(scratch(ctx, p ? SLOT_PLANES1 : SLOT_PLANES0, plane * 2 * n + 16, &t));
        uint8_t *planes = static_cast<uint8_t *>(t);
        if (ctx->tail_pending[p]) FNX_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_tail[p], 0));
        const int st = launch_blur_scored(ctx, n, d_srcs, sstride, w, h, kernel, radius, flags, d_dsts, dstride, planes, plane, nw, nh);
        if (st < 0) return st;
        if (st == FNX_OK) {
            double *dres;
            FNX_TRY(result_slot_queued(ctx, n, &dres));
            {
                LaunchScope tail(ctx, p ? SLOT_PART1 : SLOT_PART0, true);   // the windowed-SSIM launcher works on ctx->stream
                FNX_TRY(launch_windowed_ssim(ctx, plane_pairs(n, planes, planes + plane * n, plane, nw, nh), window, dwin, dres));
                fnx_ctx::Pending *q = nullptr;
                FNX_TRY(publish_results(ctx, dres, n, &q));      // the batch's event: behind the tail
                q->tail_parity = p;
                q->tail_gen = ++ctx->tail_gen[p];
                FNX_HIP(hipEventRecord(ctx->ev_tail[p], ctx->stream2));
            }
            ctx->tail_pending[p] = true;
            ctx->parity ^= 1;
            return FNX_OK;
        }
    }
    // shapes the one-pass kernel is not built for: the two ops back to back
    FNX_TRY(fnx_gaussian_blur_batch(ctx, n, srcs, sstride, w, h, kernel, radius, flags, dsts, dstride));
    return fnx_ssim_fast_batch_enqueue(ctx, n, srcs, sstride, const_cast<const uint8_t *const *>(dsts), dstride, w, h, window);
}

int fnx_gaussian_blur_ssim_fast_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w,
                                      int h, const double *kernel, int radius, int flags,
                                      uint8_t *const *dsts, int dstride, const double *window, double *out)
{
    FNX_REQUIRE(out != nullptr, "out is null");
    FNX_REQUIRE(ctx && ctx->res_count == 0, "enqueued batches are waiting for fnx_results_fetch: fetch them before a blocking batch call");
    FNX_TRY(fnx_gaussian_blur_ssim_fast_batch_enqueue(ctx, n, srcs, sstride, w, h, kernel, radius, flags, dsts,
                                                      dstride, window));
    return fnx_results_fetch(ctx, n, out);
}

// GaussianBlur + SSIMFast(src, blurred) of ONE image: what fnx_gaussian_blur followed by fnx_ssim_fast compute, with the image
// crossing PCIe once each way when it lives in host memory (the two calls upload the source twice and the blurred image once).
// The two kernels' launches back to back on the ctx's stream, on the staged copies: for one image the time is the link's (host
// space) or two launch latencies (device space), not HBM traffic -- the one-pass kernel and its second-stream tail are the
// BATCH entry's (a first version went through them: 82 us per device-space call against 53 for this form).
int fnx_gaussian_blur_ssim_fast(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, const double *kernel,
                                int radius, int flags, uint8_t *dst, int dstride, const double *window, double *ssim)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    FNX_REQUIRE(kernel != nullptr && radius >= 0 && window != nullptr && ssim != nullptr, "blur kernel / window / ssim");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    FNX_TRY(check_img(dst, dstride, w, h, "dst"));
    FNX_REQUIRE(w > 0 && h > 0, "dims");
    flags &= ~FNX_BLUR_KEEP_BOX_SUMS;
    ctx->kept.valid = false;
    int nw, nh;
    if (!ssim_fast_dims(w, h, &nw, &nh) && (w < 8 || h < 8)) {
        // pixelSSIM's sizes (ssim.go:61-63, the FLAT Pix slices): the two calls as they are
        FNX_TRY(fnx_gaussian_blur(ctx, space, src, sstride, w, h, kernel, radius, flags, dst, dstride));
        return fnx_ssim_fast(ctx, space, src, sstride, dst, dstride, w, h, window, ssim);
    }
    FNX_REQUIRE(space != FNX_DEVICE || src != dst, "dst aliases src (the blur is not in-place)");
    const double *dwin = nullptr;
    FNX_TRY(upload_window(ctx, window, &dwin));
    DevImg s;
    DevOut d;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, w, h, SLOT_OUT, &d));
    FNX_TRY(launch_blur(ctx, 1, s.p, nullptr, s.stride, w, h, kernel, radius, flags, d.p, nullptr, d.stride));
    double *dres;
    FNX_TRY(result_slot(ctx, 1, &dres));
    FNX_TRY(ssim_fast_device(ctx, one_pair(s.p, s.stride, d.p, d.stride, w, h), window, dwin, dres));
    FNX_TRY(finish_enqueue(ctx, space, &d));                     // the blurred image starts back behind the score's kernels
    FNX_TRY(result_wait(ctx, dres, ssim, 1));
    if (space != FNX_DEVICE) FNX_HIP(hipStreamSynchronize(ctx->stream));
    return FNX_OK;
}

int fnx_ssim(fnx_ctx *ctx, int space, const uint8_t *a, int astride, const uint8_t *b,
             int bstride, int w, int h, const double *window, double *out)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(window && out, "window/out is null");
    FNX_TRY(check_img(a, astride, w, h, "a"));
    FNX_TRY(check_img(b, bstride, w, h, "b"));
    if (w <= 0 || h <= 0) {
        *out = 1.0;
        return FNX_OK;
    }
    const double *dwin = nullptr;
    FNX_TRY(upload_window(ctx, window, &dwin));
    DevImg da, db;
    FNX_TRY(stage_pair(ctx, space, a, astride, b, bstride, w, h, w < 8 || h < 8, &da, &db));
    double *dres;
    FNX_TRY(result_slot(ctx, 1, &dres));
    FNX_TRY(ssim_pairs(ctx, one_pair(da.p, da.stride, db.p, db.stride, w, h), nullptr, nullptr, window, dwin, dres, THEN_WAIT));
    return result_wait(ctx, dres, out, 1);
}

int fnx_ssim_enqueue(fnx_ctx *ctx, const uint8_t *a, int astride, const uint8_t *b, int bstride, int w, int h,
                     const double *window)
{
    FNX_ENTER(ctx);
    FNX_REQUIRE(window != nullptr && w > 0 && h > 0, "enqueue arguments");
    FNX_TRY(check_img(a, astride, w, h, "a"));
    FNX_TRY(check_img(b, bstride, w, h, "b"));
    FNX_TRY(can_enqueue(ctx));
    const double *dwin = nullptr;
    FNX_TRY(upload_window(ctx, window, &dwin));
    double *dres;
    FNX_TRY(result_slot_queued(ctx, 1, &dres));
    // the score's kernels on the second stream (ssim_pairs); a and b stay the caller's until the fetch
    static const bool same_stream = [] { const char *e = dev_env("FNX_SSIM_ENQUEUE_INLINE"); return e && e[0] == '1'; }();
    return ssim_pairs(ctx, one_pair(a, astride, b, bstride, w, h), nullptr, nullptr, window, dwin, dres,
                      same_stream ? THEN_PUBLISH : THEN_PUBLISH_TAIL);
}

// MSSSIM's weights, trimmed while a level's min dim < 8 (ssim.go:324-342)
static int msssim_weights(int w, int h, double (&weights)[5])
{
    const double full[5] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
    for (int i = 0; i < 5; i++) weights[i] = full[i];
    int nweights = 5;
    int tw = w, th = h;
    for (int i = 0; i < 4; i++) {
        int minDim = int(std::fmin(double(tw), double(th)));
        if (minDim < 8) {
            nweights = i + 1;
            double sum = 0;
            for (int j = 0; j < nweights; j++) sum += weights[j];
            for (int j = 0; j < nweights; j++) weights[j] /= sum;
            break;
        }
        tw /= 2;
        th /= 2;
    }
    return nweights;
}

// Every level's SSIMFast of a device-resident pair into dres[0 .. *nlev) (ssim.go:344-362); nothing waits.
static int msssim_levels_device(fnx_ctx *ctx, const uint8_t *ap, int astride, const uint8_t *bp, int bstride, int w, int h,
                                int nweights, const double *window, double *dres, int *nlev_out)
{
    const double *dwin = nullptr;
    FNX_TRY(upload_window(ctx, window, &dwin));
    int nlev = 0;
    const int fused = launch_msssim_fused(ctx, ap, astride, bp, bstride, w, h, nweights, window, dres, &nlev);
    if (fused < 0) return fused;
    if (fused != FNX_OK) {
        // pyramid storage: levels 1.. of both images, ping-ponged in two slots per side
        const uint8_t *ca = ap, *cb = bp;
        int cas = astride, cbs = bstride, cw = w, ch = h;
        size_t lvl_bytes = static_cast<size_t>(w / 2) * (h / 2) * 4 + 16;
        void *pyr = nullptr;   // level k lives at (k&1)*2*lvl_bytes: [a][b]
        FNX_TRY(scratch(ctx, SLOT_TMP0, lvl_bytes * 4, &pyr));
        // the five levels' final means are taken by one launch at the end
        SsimDeferred defer;
        void *reserve = nullptr;
        FNX_TRY(scratch(ctx, SLOT_PARTIAL, sizeof(double) * SSIM_DEFER_DOUBLES, &reserve));
        for (int i = 0; i < nweights; i++) {
            const ImgPairs level = one_pair(ca, cas, cb, cbs, cw, ch);
            FNX_TRY(ssim_fast_device(ctx, level, window, dwin, dres + i, SsimOpts::deferred(&defer, i)));
            nlev = i + 1;
            if (i < nweights - 1) {
                const int nw = cw / 2, nh = ch / 2;
                if (nw < 8 || nh < 8) break;              // ssim.go:354-358
                uint8_t *na = static_cast<uint8_t *>(pyr) + (i & 1) * 2 * lvl_bytes;
                uint8_t *nb = na + lvl_bytes;
                FNX_TRY(launch_box_downsample_pair(ctx, level, na, nw * 4, lvl_bytes, nw, nh));
                ca = na; cb = nb; cas = cbs = nw * 4; cw = nw; ch = nh;
            }
        }
        FNX_TRY(launch_ssim_finish_deferred(ctx, defer, dres));
    }
    *nlev_out = nlev;
    return FNX_OK;
}

int fnx_pixel_ssim(fnx_ctx *ctx, int space, const uint8_t *a_pix, size_t a_pix_len, const uint8_t *b_pix,
                   size_t b_pix_len, int w, int h, double *out)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(out != nullptr && w >= 0 && h >= 0, "pixel_ssim arguments");
    if (static_cast<long long>(w) * h == 0) {      // ssim.go:172-175
        *out = 1.0;
        return FNX_OK;
    }
    const size_t walk = (a_pix_len + 3) & ~size_t(3);         // i < len(a.Pix), i += 4, reads [i, i+2]
    FNX_REQUIRE(a_pix_len == 0 || (a_pix && b_pix), "null Pix");
    FNX_REQUIRE(a_pix_len == 0 || (walk - 1 <= a_pix_len && walk - 1 <= b_pix_len),
                "a Pix slice ends inside the last pixel the loop reads, or b.Pix is shorter than a.Pix (the reference panics)");
    const uint8_t *da = a_pix, *db = b_pix;
    if (space == FNX_HOST && a_pix_len) {
        void *ta = nullptr, *tb = nullptr;
        FNX_TRY(scratch(ctx, SLOT_IN_A, walk + 16, &ta));
        FNX_TRY(scratch(ctx, SLOT_IN_B, walk + 16, &tb));
        FNX_HIP(hipMemsetAsync(static_cast<uint8_t *>(ta) + (walk - 4), 0, 4, ctx->stream));
        FNX_HIP(hipMemsetAsync(static_cast<uint8_t *>(tb) + (walk - 4), 0, 4, ctx->stream));
        FNX_HIP(hipMemcpyAsync(ta, a_pix, a_pix_len < walk ? a_pix_len : walk, hipMemcpyHostToDevice, ctx->stream));
        FNX_HIP(hipMemcpyAsync(tb, b_pix, b_pix_len < walk ? b_pix_len : walk, hipMemcpyHostToDevice, ctx->stream));
        da = static_cast<const uint8_t *>(ta);
        db = static_cast<const uint8_t *>(tb);
    }
    double *dres;
    FNX_TRY(result_slot(ctx, 1, &dres));
    FNX_TRY(launch_pixel_ssim(ctx, da, db, w, h, walk, dres));
    return result_wait(ctx, dres, out, 1);
}

int fnx_msssim(fnx_ctx *ctx, int space, const uint8_t *a, int astride, const uint8_t *b,
               int bstride, int w, int h, const double *window, double *out, double *per_level)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(window && out, "window/out is null");
    FNX_TRY(check_img(a, astride, w, h, "a"));
    FNX_TRY(check_img(b, bstride, w, h, "b"));
    double weights[5];
    const int nweights = msssim_weights(w, h, weights);
    double lv[5];
    for (double &v : lv) v = NAN;
    int nlev = 0;
    if (w <= 0 || h <= 0) {
        // SSIMFast of empty images: pixelSSIM n==0 -> 1.0; the halving loop then breaks (nw < 8)
        lv[0] = 1.0;
        nlev = 1;
    } else {
        DevImg da, db;
        // aCopy := toNRGBA(a), bCopy := toNRGBA(b) (ssim.go:345-346): flat copies -- the strides only vouch for the
        // slices' lengths (check_img above), the pyramid reads the first 4wh bytes of each as a tight image
        FNX_TRY(stage_in_front(ctx, space, a, w, h, SLOT_IN_A, &da));
        FNX_TRY(stage_in_front(ctx, space, b, w, h, SLOT_IN_B, &db));
        double *dres;
        FNX_TRY(result_slot(ctx, 5, &dres));
        FNX_TRY(msssim_levels_device(ctx, da.p, da.stride, db.p, db.stride, w, h, nweights, window, dres, &nlev));
        FNX_TRY(result_wait(ctx, dres, lv, nlev));
    }
    *out = msssim_combine(lv, weights, nlev);
    if (per_level)
        for (int i = 0; i < 5; i++) per_level[i] = i < nlev ? lv[i] : NAN;
    return FNX_OK;
}

// n checked same-geometry device pairs -> one FIFO entry of n MSSSIMs (fnx_msssim_enqueue: n == 1)
static int msssim_enqueue_body(fnx_ctx *ctx, int n, const uint8_t *const *as, const uint8_t *const *bs, int w, int h, const double *window)
{
    FNX_TRY(can_enqueue(ctx));
    double weights[5];
    const int nweights = msssim_weights(w, h, weights);
    double *dres;
    FNX_TRY(result_slot_queued(ctx, 5 * n, &dres));
    int nlev = 0;
    bool batched = false;
    // the five launches of the fused form with the image as a grid dimension of each (ssim.hip); shapes it does not cover
    // (odd dims, a pair that is not 16-byte aligned -- the pointers: the levels are read flat, stride 4w -- the non-default
    // forms) take the loop below
    if (n > 1 && all_aligned16(n, as, 0) && all_aligned16(n, bs, 0)) {
        const uint8_t *const *d_as, *const *d_bs;
        FNX_TRY(upload_ptr_pair(ctx, n, as, bs, &d_as, &d_bs));
        const double *dwin = nullptr;
        FNX_TRY(upload_window(ctx, window, &dwin));
        const int rc = launch_msssim_fused(ctx, as[0], w * 4, bs[0], w * 4, w, h, nweights, window, dres, &nlev, n, d_as, d_bs);
        if (rc < 0) return rc;
        batched = rc == FNX_OK;
    }
    for (int i = 0; i < n && !batched; i++)      // (every image has the same levels: the dims decide)
        FNX_TRY(msssim_levels_device(ctx, as[i], w * 4, bs[i], w * 4, w, h, nweights, window, dres + 5 * i, &nlev));   // toNRGBA: flat (see fnx_msssim)
    return publish_msssim(ctx, dres, n, nlev, weights);
}

int fnx_msssim_enqueue(fnx_ctx *ctx, const uint8_t *a, int astride, const uint8_t *b, int bstride, int w, int h,
                       const double *window)
{
    FNX_ENTER(ctx);
    FNX_REQUIRE(window != nullptr && w > 0 && h > 0, "enqueue arguments");
    FNX_TRY(check_img(a, astride, w, h, "a"));
    FNX_TRY(check_img(b, bstride, w, h, "b"));
    return msssim_enqueue_body(ctx, 1, &a, &b, w, h, window);
}

// n same-geometry device pairs scored by ONE launch of the window kernel (the image is its second grid dimension), on the
// ctx's second stream like fnx_ssim_enqueue; one FIFO entry of n values
int fnx_ssim_batch_enqueue(fnx_ctx *ctx, int n, const uint8_t *const *as, int astride, const uint8_t *const *bs, int bstride,
                           int w, int h, const double *window)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_batch(n, as && bs, window != nullptr && w > 0 && h > 0));
    if (n == 0) return FNX_OK;
    FNX_TRY(check_batch_images(n, {as, astride, w, h, "a"}, {bs, bstride, w, h, "b"}));
    FNX_TRY(can_enqueue(ctx));
    const double *dwin = nullptr;
    FNX_TRY(upload_window(ctx, window, &dwin));
    double *dres;
    FNX_TRY(result_slot_queued(ctx, n, &dres));
    ImgPairs im = one_pair(as[0], astride, bs[0], bstride, w, h);
    im.n = n;
    return ssim_pairs(ctx, im, as, bs, window, dwin, dres, THEN_PUBLISH_TAIL);
}

int fnx_msssim_batch_enqueue(fnx_ctx *ctx, int n, const uint8_t *const *as, int astride, const uint8_t *const *bs, int bstride,
                             int w, int h, const double *window)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_batch(n, as && bs, window != nullptr && w > 0 && h > 0));
    if (n == 0) return FNX_OK;
    FNX_TRY(check_batch_images(n, {as, astride, w, h, "a"}, {bs, bstride, w, h, "b"}));
    return msssim_enqueue_body(ctx, n, as, bs, w, h, window);
}

// ---- resize, then score (ssim.go:31-33, 320-322; targetsize.go:563-568): b goes up at its own size, nothing comes down ----
int fnx_lanczos_box_downsample(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW, int srcH,
                               const int32_t *offH, const int32_t *idxH, const double *wH,
                               const int32_t *offV, const int32_t *idxV, const double *wV,
                               int midW, int midH, uint8_t *dst, int dstride, int dstW, int dstH)
{
    const TapTable th{offH, idxH, wH, midW, 0}, tv{offV, idxV, wV, midH, 0};
    return fnx::lanczos_box_tables(ctx, space, src, sstride, srcW, srcH, th, tv, midW, midH, dst, dstride, dstW, dstH);
}

int fnx_lanczos_box_fused(int srcW, int srcH, const int32_t *offH, const int32_t *idxH, const double *wH,
                          const int32_t *offV, const int32_t *idxV, const double *wV, int midW, int midH, int dstW, int dstH)
{
    const TapTable th{offH, idxH, wH, midW, 0}, tv{offV, idxV, wV, midH, 0};
    return fnx::resize_box_covers(th, tv, srcW, srcH, midW, midH, dstW, dstH) ? 1 : 0;
}

int fnx_ssim_fast_resized(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah, const uint8_t *b, int bstride, int bw, int bh,
                          const int32_t *offH, const int32_t *idxH, const double *wH,
                          const int32_t *offV, const int32_t *idxV, const double *wV, const double *window, double *out)
{
    const TapTable th{offH, idxH, wH, aw, 0}, tv{offV, idxV, wV, ah, 0};
    return fnx::ssim_fast_resized_tables(ctx, space, a, astride, aw, ah, b, bstride, bw, bh, th, tv, window, out);
}

int fnx_ssim_resized(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah, const uint8_t *b, int bstride, int bw, int bh,
                     const int32_t *offH, const int32_t *idxH, const double *wH,
                     const int32_t *offV, const int32_t *idxV, const double *wV, const double *window, double *out)
{
    const TapTable th{offH, idxH, wH, aw, 0}, tv{offV, idxV, wV, ah, 0};
    return fnx::ssim_resized_tables(ctx, space, a, astride, aw, ah, b, bstride, bw, bh, th, tv, window, out);
}

int fnx_msssim_resized(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah, const uint8_t *b, int bstride, int bw, int bh,
                       const int32_t *offH, const int32_t *idxH, const double *wH,
                       const int32_t *offV, const int32_t *idxV, const double *wV, const double *window, double *out, double *per_level)
{
    const TapTable th{offH, idxH, wH, aw, 0}, tv{offV, idxV, wV, ah, 0};
    return fnx::msssim_resized_tables(ctx, space, a, astride, aw, ah, b, bstride, bw, bh, th, tv, window, out, per_level);
}

// ---- prepared reference ------------------------------------------------------------------
int fnx_ssim_fast_prepare(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int w, int h,
                          fnx_prepared **out)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(out != nullptr && w > 0 && h > 0, "prepare arguments");
    FNX_TRY(check_img(a, astride, w, h, "a"));
    *out = nullptr;
    fnx_prepared *p = new fnx_prepared();
    p->w = w;
    p->h = h;
    ssim_fast_dims(w, h, &p->pw, &p->ph);
    void *d = nullptr;
    hipError_t e = hipMalloc(&d, static_cast<size_t>(p->pw) * p->ph * 4 + 16);
    if (e != hipSuccess) {
        delete p;
        set_error("hipMalloc failed: %s", hipGetErrorString(e));
        return FNX_ERR_OOM;
    }
    p->pix = static_cast<uint8_t *>(d);
    DevImg da;
    int rc = stage_in(ctx, space, a, astride, w, h, SLOT_IN_A, &da);
    if (rc >= 0) rc = prepared_plane(ctx, da.p, da.stride, *p);
    if (rc >= 0 && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = FNX_ERR_HIP;
    if (rc < 0) {
        (void)hipFree(p->pix);
        delete p;
        return rc;
    }
    *out = p;
    return FNX_OK;
}

int fnx_ssim_fast_against(fnx_ctx *ctx, const fnx_prepared *ref, int space, const uint8_t *b,
                          int bstride, const double *window, double *out)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(ref && window && out, "against arguments");
    FNX_TRY(check_img(b, bstride, ref->w, ref->h, "b"));
    DevImg db;
    FNX_TRY(stage_in(ctx, space, b, bstride, ref->w, ref->h, SLOT_IN_B, &db));
    return against_device(ctx, ref, db.p, db.stride, window, out);
}

// ---- decoded JPEG planes (image.YCbCr / image.Gray) -> NRGBA: convert.go:22-64 ----------------
static int chroma_dims(int ratio, int w, int h, int *cw, int *ch)
{
    switch (ratio) {   // image.NewYCbCr's plane sizes for Rect.Min == (0,0)
    case 0: *cw = w; *ch = h; break;
    case 1: *cw = (w + 1) / 2; *ch = h; break;
    case 2: *cw = (w + 1) / 2; *ch = (h + 1) / 2; break;
    case 3: *cw = w; *ch = (h + 1) / 2; break;
    case 4: *cw = (w + 3) / 4; *ch = h; break;
    case 5: *cw = (w + 3) / 4; *ch = (h + 1) / 2; break;
    default: set_error("invalid argument: subsample ratio"); return FNX_ERR_INVALID;
    }
    return FNX_OK;
}

// planes -> tight device NRGBA in `slot`
static int ycbcr_stage_convert(fnx_ctx *ctx, int space, const uint8_t *y, int ystride, const uint8_t *cb,
                               const uint8_t *cr, int cstride, int ratio, int w, int h, uint8_t *dst, int dstride)
{
    const bool gray = !cb && !cr;
    FNX_REQUIRE(y != nullptr && ystride >= w, "Y plane");
    FNX_REQUIRE(gray || (cb && cr), "Cb and Cr must both be given (or both NULL for image.Gray)");
    int cw = 0, ch = 0;
    if (!gray) {
        FNX_TRY(chroma_dims(ratio, w, h, &cw, &ch));
        FNX_REQUIRE(cstride >= cw, "chroma stride");
    }
    const uint8_t *dy = y, *dcb = cb, *dcr = cr;
    int dys = ystride, dcs = cstride;
    if (space == FNX_HOST) {
        dys = (w + 15) & ~15;
        dcs = (cw + 15) & ~15;
        void *t = nullptr;
        const size_t ybytes = static_cast<size_t>(dys) * h, cbytes = gray ? 0 : static_cast<size_t>(dcs) * ch;
        FNX_TRY(scratch(ctx, SLOT_TMP1, ybytes + 2 * cbytes + 16, &t));
        uint8_t *base = static_cast<uint8_t *>(t);
        FNX_HIP(hipMemcpy2DAsync(base, dys, y, ystride, w, h, hipMemcpyHostToDevice, ctx->stream));
        dy = base;
        if (!gray) {
            FNX_HIP(hipMemcpy2DAsync(base + ybytes, dcs, cb, cstride, cw, ch, hipMemcpyHostToDevice, ctx->stream));
            FNX_HIP(hipMemcpy2DAsync(base + ybytes + cbytes, dcs, cr, cstride, cw, ch, hipMemcpyHostToDevice, ctx->stream));
            dcb = base + ybytes;
            dcr = base + ybytes + cbytes;
        }
    }
    return launch_ycbcr_to_nrgba(ctx, dy, dys, gray ? nullptr : dcb, gray ? nullptr : dcr, dcs, gray ? 0 : ratio, w, h, dst,
                                 dstride);
}

int fnx_ycbcr_to_nrgba(fnx_ctx *ctx, int space, const uint8_t *y, int ystride, const uint8_t *cb,
                       const uint8_t *cr, int cstride, int ratio, int w, int h, uint8_t *dst, int dstride)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_TRY(check_img(dst, dstride, w, h, "dst"));
    if (w <= 0 || h <= 0) return FNX_OK;
    DevOut d;
    FNX_TRY(stage_out(ctx, space, dst, dstride, w, h, SLOT_OUT, &d));
    FNX_TRY(ycbcr_stage_convert(ctx, space, y, ystride, cb, cr, cstride, ratio, w, h, d.p, d.stride));
    return finish(ctx, space, &d);
}

int fnx_ssim_fast_against_ycbcr(fnx_ctx *ctx, const fnx_prepared *ref, int space, const uint8_t *y, int ystride,
                                const uint8_t *cb, const uint8_t *cr, int cstride, int ratio,
                                const double *window, double *out)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(ref && window && out, "against arguments");
    const int w = ref->w, h = ref->h;
    FNX_REQUIRE(w > 0 && h > 0, "empty reference");
    void *t = nullptr;
    if (space == FNX_DEVICE && cb && cr && (ref->pw != w || ref->ph != h)) {
        // the candidate's plane straight from its planes: no NRGBA image (launch_box_downsample_ycc)
        FNX_REQUIRE(y != nullptr && ystride >= w, "Y plane");
        int cw = 0, ch = 0;
        FNX_TRY(chroma_dims(ratio, w, h, &cw, &ch));
        FNX_REQUIRE(cstride >= cw, "chroma stride");
        bool fused = false;
        FNX_TRY(scratch(ctx, SLOT_TMP2, static_cast<size_t>(ref->pw) * ref->ph * 4 + 16, &t));
        FNX_TRY(launch_box_downsample_ycc(ctx, y, ystride, cb, cr, cstride, ratio, w, h, static_cast<uint8_t *>(t), ref->pw * 4, ref->pw,
                                          ref->ph, &fused));
        if (fused) return against_device(ctx, ref, static_cast<const uint8_t *>(t), ref->pw * 4, window, out, true);
    }
    FNX_TRY(scratch(ctx, SLOT_IN_B, static_cast<size_t>(w) * h * 4 + 16, &t));
    FNX_TRY(ycbcr_stage_convert(ctx, space, y, ystride, cb, cr, cstride, ratio, w, h, static_cast<uint8_t *>(t), w * 4));
    return against_device(ctx, ref, static_cast<const uint8_t *>(t), w * 4, window, out);
}

void fnx_prepared_free(fnx_ctx *ctx, fnx_prepared *p)
{
    if (!p) return;
    if (ctx && bind(ctx) == FNX_OK) {
        // hipFree waits for the device's outstanding work itself; a lent stream (fnx_ctx_use_stream) is its owner's to drain
        if (ctx->stream == ctx->own_stream) (void)hipStreamSynchronize(ctx->stream);
        if (p->pix) (void)hipFree(p->pix);
    }
    delete p;
}

// ---- Analyze (analyze.go:26-124) and the flat scans (convert.go:66-84) --------------------
// One launch per call (analyze.hip: analyze_one_kernel): the results land in pinned host memory, each image's ready word
// after them; this thread watches the words.  Form "analyze_staged" = "1": the staged launches (launch_analyze) for every
// call -- what a batch of more than 4096 images takes -- for A/B and tests.
static bool analyze_staged(const fnx_ctx *ctx)
{
    const char *e = form_value(ctx, FORM_ANALYZE_STAGED);
    return e && e[0] == '1';
}

static int analyze_direct(fnx_ctx *ctx, int n, const uint8_t *src, const uint8_t *const *srcs, int sstride, int w, int h, bool al,
                          fnx_analysis *out)
{
    void *pin = nullptr;
    const size_t rbytes = (sizeof(fnx_analysis) * static_cast<size_t>(n) + 63) & ~size_t(63);
    const int nr = n * launch_analyze_ready_words(), nv = launch_analyze_var_parts();
    const size_t vbytes = (sizeof(double) * static_cast<size_t>(n) * nv + 63) & ~size_t(63);
    FNX_TRY(pinned_alloc(ctx, rbytes + vbytes + sizeof(uint32_t) * static_cast<size_t>(nr), &pin));
    fnx_analysis *hres = static_cast<fnx_analysis *>(pin);
    double *hvar = reinterpret_cast<double *>(static_cast<char *>(pin) + rbytes);
    volatile uint32_t *ready = reinterpret_cast<volatile uint32_t *>(static_cast<char *>(pin) + rbytes + vbytes);
    for (int i = 0; i < nr; i++) ready[i] = 0u;
    std::atomic_thread_fence(std::memory_order_release);
    FNX_TRY(launch_analyze_one(ctx, n, src, srcs, sstride, w, h, al, hres, hvar, const_cast<uint32_t *>(ready)));
    FNX_TRY(poll_until([=] {
        for (int i = 0; i < nr; i++)
            if (ready[i] != 1u) return false;
        return true;
    }, [&] { return hipStreamQuery(ctx->stream); }));           // (the stream is empty: the words are there)
    for (int i = 0; i < nr; i++) FNX_REQUIRE(ready[i] == 1u, "Analyze: the launch finished without a result");
    std::memcpy(out, hres, sizeof(fnx_analysis) * static_cast<size_t>(n));
    for (int i = 0; i < n; i++) {                                   // the contrast workgroups' sums, in order: bit-reproducible
        double v = 0.0;
        for (int k = 0; k < nv; k++) v += hvar[static_cast<size_t>(i) * nv + k];
        out[i].variance_sum = v;
    }
    return FNX_OK;
}

static void clamp_unique(fnx_analysis *a, int n)
{
    for (int i = 0; i < n; i++)
        if (a[i].unique_colors > 1024) a[i].unique_colors = 1024;   // len(colorSet) < 1024 gate, analyze.go:73
}

int fnx_analyze(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, fnx_analysis *out)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(out != nullptr, "out is null");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    std::memset(out, 0, sizeof(*out));
    if (w <= 0 || h <= 0) return FNX_EMPTY;      // Analyze returns the zero ImageStats (analyze.go:37-39)
    DevImg s;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    const bool al = (reinterpret_cast<uintptr_t>(s.p) & 15u) == 0;
    if (!analyze_staged(ctx)) {
        FNX_TRY(analyze_direct(ctx, 1, s.p, nullptr, s.stride, w, h, al, out));
    } else {
        void *dres = nullptr;
        FNX_TRY(scratch(ctx, SLOT_RESULT, sizeof(fnx_analysis), &dres));
        FNX_TRY(launch_analyze(ctx, 1, s.p, nullptr, s.stride, w, h, al, static_cast<fnx_analysis *>(dres)));
        FNX_TRY(fetch_bytes(ctx, dres, out, sizeof(fnx_analysis)));
    }
    clamp_unique(out, 1);
    return FNX_OK;
}

int fnx_analyze_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h,
                      fnx_analysis *out)
{
    FNX_ENTER(ctx);
    FNX_REQUIRE(n >= 0 && srcs && out, "batch arguments");
    if (n == 0) return FNX_OK;
    FNX_REQUIRE(w > 0 && h > 0 && sstride >= 4 * w && !(sstride & 3), "dims");
    for (int i = 0; i < n; i++) FNX_REQUIRE(srcs[i], "null image in batch");
    const bool al = all_aligned16(n, srcs, 0);
    void *dp = nullptr;
    FNX_TRY(upload_table(ctx, SLOT_PTRS, srcs, sizeof(void *) * size_t(n), &dp));
    if (!analyze_staged(ctx) && n <= 4096) {
        FNX_TRY(analyze_direct(ctx, n, nullptr, static_cast<const uint8_t *const *>(dp), sstride, w, h, al, out));
    } else {
        void *dres = nullptr;
        FNX_TRY(scratch(ctx, SLOT_RESULT, sizeof(fnx_analysis) * size_t(n), &dres));
        FNX_TRY(launch_analyze(ctx, n, nullptr, static_cast<const uint8_t *const *>(dp), sstride, w, h, al,
                               static_cast<fnx_analysis *>(dres)));
        FNX_TRY(fetch_bytes(ctx, dres, out, sizeof(fnx_analysis) * size_t(n)));
    }
    clamp_unique(out, n);
    return FNX_OK;
}

int fnx_scan_flags(fnx_ctx *ctx, int space, const uint8_t *pix, size_t pix_len, int *is_opaque, int *is_grayscale)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(pix != nullptr || pix_len == 0, "pix is null");
    uint32_t flags = 0;
    if (pix_len >= 4) {
        const uint8_t *d = pix;
        if (space == FNX_HOST) {
            void *t = nullptr;
            FNX_TRY(scratch(ctx, SLOT_IN_A, pix_len + 16, &t));
            FNX_HIP(hipMemcpyAsync(t, pix, pix_len, hipMemcpyHostToDevice, ctx->stream));
            d = static_cast<const uint8_t *>(t);
        }
        // one launch; its last workgroup writes the flags into pinned host memory, which this thread watches (the
        // memset + kernel + copy + stream synchronisation this replaces took 39 us for a 6 us scan of a 4K image)
        void *pin = nullptr;
        const int cap = launch_scan_flags_slots(ctx);
        FNX_TRY(pinned_alloc(ctx, sizeof(uint32_t) * static_cast<size_t>(cap), &pin));
        volatile uint32_t *hf = static_cast<volatile uint32_t *>(pin);
        for (int i = 0; i < cap; i++) hf[i] = 0xffffffffu;
        std::atomic_thread_fence(std::memory_order_release);
        int nslots = 0;
        FNX_TRY(launch_scan_flags_direct(ctx, d, pix_len, static_cast<uint32_t *>(pin), &nslots));
        int first = 0;                                             // slots below it have reported
        const auto drain = [&] {
            while (first < nslots && hf[first] != 0xffffffffu) { flags |= hf[first]; first++; }
            return first == nslots;
        };
        FNX_TRY(poll_until(drain, [&] { return hipStreamQuery(ctx->stream); }));
        FNX_REQUIRE(drain(), "scan_flags: the kernel finished without all of its results");   // (the stream is empty: every word is there)
        flags &= 3u;
    }
    if (is_opaque) *is_opaque = (flags & 1u) ? 0 : 1;
    if (is_grayscale) *is_grayscale = (flags & 2u) ? 0 : 1;
    return FNX_OK;
}

// ---- applyPalette + palettedToNRGBA (targetsize.go:488-546) ---------------------------------
int fnx_apply_palette(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                      const uint8_t *palette, int ncolors, uint8_t *indices, int istride,
                      uint8_t *quantized, int qstride)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space(space));
    FNX_REQUIRE(palette != nullptr && ncolors >= 1 && ncolors <= 256, "palette: 1..256 colours (image.Paletted indices are uint8)");
    for (int i = 0; i < ncolors; i++)
        FNX_REQUIRE(palette[4 * i + 3] == 255, "palette entries must be opaque (medianCut only emits A = 255, targetsize.go:407-410)");
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    FNX_REQUIRE(indices != nullptr || quantized != nullptr, "no output requested");
    if (indices) FNX_REQUIRE(istride >= w, "index stride");
    if (quantized) FNX_TRY(check_img(quantized, qstride, w, h, "quantized"));
    if (w <= 0 || h <= 0) return FNX_OK;
    DevImg s;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    DevOut q;
    if (quantized) FNX_TRY(stage_out(ctx, space, quantized, qstride, w, h, SLOT_OUT, &q));
    uint8_t *didx = indices;
    int dpitch = istride;
    if (indices && space == FNX_HOST) {
        dpitch = (w + 3) & ~3;
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_TMP0, static_cast<size_t>(dpitch) * h + 16, &t));
        didx = static_cast<uint8_t *>(t);
    }
    FNX_TRY(launch_apply_palette(ctx, s.p, s.stride, w, h, palette, ncolors, didx, dpitch,
                                 quantized ? q.p : nullptr, quantized ? q.stride : 0));
    if (indices && space == FNX_HOST)
        FNX_HIP(hipMemcpy2DAsync(indices, istride, didx, dpitch, w, h, hipMemcpyDeviceToHost, ctx->stream));
    if (quantized) return finish(ctx, space, &q);
    if (space == FNX_HOST) FNX_HIP(hipStreamSynchronize(ctx->stream));
    return FNX_OK;
}

// ---- medianCut (targetsize.go:422-486) and one iteration of quantizeStrategy (targetsize.go:183-205) ------------------------
// what both entries ask of the image and the levels, before the ctx is looked at
static int check_median_cut(int space, const uint8_t *src, int sstride, int w, int h, int nlevels, const int *max_colors)
{
    FNX_TRY(check_space(space));
    FNX_REQUIRE(w >= 0 && h >= 0, "negative dims");
    FNX_REQUIRE(max_colors != nullptr && nlevels >= 1, "max_colors: at least one level");
    for (int l = 0; l < nlevels; l++) {
        FNX_REQUIRE(max_colors[l] >= 1 && max_colors[l] <= 256, "a level outside 1..256");
        FNX_REQUIRE(l == 0 || max_colors[l] > max_colors[l - 1], "levels must be strictly ascending");
    }
    if (w > 0 && h > 0) {
        FNX_REQUIRE(src != nullptr, "src pixel pointer is null");
        // medianCut indexes the flat Pix slice (off := i*4, targetsize.go:437), not rows: a padded image's samples would be
        // taken from its padding
        FNX_REQUIRE(sstride == 4 * w, "median cut takes tight images only (sstride == 4*w): the reference samples the flat Pix slice");
    }
    return FNX_OK;
}

int fnx_median_cut(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int nlevels, const int *max_colors,
                   uint8_t *palettes, int *ncolors)
{
    FNX_TRY(check_median_cut(space, src, sstride, w, h, nlevels, max_colors));
    FNX_REQUIRE(palettes != nullptr && ncolors != nullptr, "palettes/ncolors is null");
    FNX_ENTER(ctx);
    if (w == 0 || h == 0) {   // targetsize.go:443-445
        std::memset(palettes, 0, static_cast<size_t>(nlevels) * 1024);
        for (int l = 0; l < nlevels; l++) { palettes[static_cast<size_t>(l) * 1024 + 3] = 255; ncolors[l] = 1; }
        return FNX_OK;
    }
    const uint32_t *d_out = nullptr;
    FNX_TRY(launch_median_cut(ctx, space, src, w, h, nlevels, max_colors, &d_out));
    std::vector<uint32_t> words(static_cast<size_t>(nlevels) * 257);
    FNX_TRY(fetch_bytes(ctx, d_out, words.data(), sizeof(uint32_t) * words.size()));
    for (int l = 0; l < nlevels; l++) {
        const uint32_t n = words[static_cast<size_t>(nlevels) * 256 + l];
        FNX_TRY(unpack_palette(words.data() + static_cast<size_t>(l) * 256, n, palettes + static_cast<size_t>(l) * 1024));
        ncolors[l] = static_cast<int>(n);
    }
    return FNX_OK;
}

int fnx_quantize(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int max_colors, uint8_t *palette, int *ncolors,
                 uint8_t *indices, int istride, uint8_t *quantized, int qstride, const double *window, double *ssim)
{
    FNX_TRY(check_median_cut(space, src, sstride, w, h, 1, &max_colors));
    FNX_REQUIRE(w > 0 && h > 0, "quantize: an empty image");
    FNX_REQUIRE(palette != nullptr && ncolors != nullptr, "palette/ncolors is null");
    FNX_REQUIRE(indices != nullptr || quantized != nullptr || ssim != nullptr, "no output requested");
    if (indices) FNX_REQUIRE(istride >= w, "index stride");
    if (quantized) FNX_TRY(check_img(quantized, qstride, w, h, "quantized"));
    FNX_REQUIRE(ssim == nullptr || window != nullptr, "window is null");
    FNX_ENTER(ctx);
    ctx->kept.valid = false;
    DevImg s;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));        // the image's one crossing
    const uint32_t *d_out = nullptr;
    FNX_TRY(launch_median_cut(ctx, FNX_DEVICE, s.p, w, h, 1, &max_colors, &d_out));
    // applyPalette with the palette where the kernel left it
    DevOut q;
    uint8_t *dq = nullptr;
    int dqs = 0;
    if (quantized) {
        FNX_TRY(stage_out(ctx, space, quantized, qstride, w, h, SLOT_OUT, &q));
        dq = q.p; dqs = q.stride;
    } else if (ssim) {
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_IN_B, static_cast<size_t>(w) * 4 * h + 16, &t));
        dq = static_cast<uint8_t *>(t); dqs = w * 4;
    }
    uint8_t *didx = indices;
    int dpitch = istride;
    if (indices && space == FNX_HOST) {
        dpitch = (w + 3) & ~3;
        void *t = nullptr;
        FNX_TRY(scratch(ctx, SLOT_TMP0, static_cast<size_t>(dpitch) * h + 16, &t));
        didx = static_cast<uint8_t *>(t);
    }
    FNX_TRY(launch_apply_palette_device(ctx, s.p, s.stride, w, h, d_out, d_out + 256, didx, dpitch, dq, dqs));
    if (indices && space == FNX_HOST)
        FNX_HIP(hipMemcpy2DAsync(indices, istride, didx, dpitch, w, h, hipMemcpyDeviceToHost, ctx->stream));
    if (quantized) FNX_TRY(finish_enqueue(ctx, space, &q));
    // computeSSIMNRGBA at equal dims = SSIMFast (targetsize.go:563-568), as fnx_ssim_fast runs it
    double *dres = nullptr;
    if (ssim) {
        const double *dwin = nullptr;
        FNX_TRY(upload_window(ctx, window, &dwin));
        int nw, nh;
        if (!ssim_fast_dims(w, h, &nw, &nh) && (w < 8 || h < 8)) FNX_TRY(check_pix_lens(w, h, s.stride, dqs));
        FNX_TRY(result_slot(ctx, 1, &dres));
        FNX_TRY(ssim_fast_device(ctx, one_pair(s.p, s.stride, dq, dqs, w, h), window, dwin, dres));
    }
    void *pin = nullptr;                                                      // (the ring's last allocation of the call)
    FNX_TRY(pinned_alloc(ctx, sizeof(uint32_t) * 257, &pin));
    FNX_HIP(hipMemcpyAsync(pin, d_out, sizeof(uint32_t) * 257, hipMemcpyDeviceToHost, ctx->stream));
    // the one wait
    if (ssim) FNX_TRY(result_wait(ctx, dres, ssim, 1));
    FNX_HIP(hipStreamSynchronize(ctx->stream));
    const uint32_t *words = static_cast<const uint32_t *>(pin);
    FNX_TRY(unpack_palette(words, words[256], palette));
    *ncolors = static_cast<int>(words[256]);
    return FNX_OK;
}

// ---- orientation -------------------------------------------------------------------------
int fnx_orient(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int orient,
               uint8_t *dst, int dstride)
{
    FNX_ENTER(ctx);
    FNX_TRY(check_space_io(space));
    if (orient < 2 || orient > 8) return FNX_NOOP;   // exif.go:180-181,200-201
    const bool swap = orient >= 5;
    const int ow = swap ? h : w, oh = swap ? w : h;
    FNX_TRY(check_img(src, sstride, w, h, "src"));
    FNX_TRY(check_img(dst, dstride, ow, oh, "dst"));
    if (w <= 0 || h <= 0) return FNX_OK;
    DevImg s;
    DevOut d;
    FNX_TRY(stage_in(ctx, space, src, sstride, w, h, SLOT_IN_A, &s));
    FNX_TRY(stage_out(ctx, space, dst, dstride, ow, oh, SLOT_OUT, &d));
    FNX_TRY(launch_orient(ctx, s.p, s.stride, w, h, orient, d.p, d.stride));
    return finish(ctx, space, &d);
}

}  // extern "C"
