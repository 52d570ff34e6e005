/*
 * fennec_hip.h -- C ABI of libfennec_hip.so: fennec's per-pixel hot path on
 * AMD Instinct MI355X (gfx950 / CDNA4), hand-written HIP kernels.
 *
 * The reference (shamspias/fennec, pure Go) has no FFI seam; the seam is the set
 * of Go functions whose BODIES a cgo shim replaces.  Every
 * entry point below names the reference function it replaces (file:line).
 * INTEGRATION.md shows the cgo binding.
 *
 * Two layers, both exported:
 *
 *   fnx_*     kernel level.  Takes weight tables (SSIM 8x8 window, blur 1-D
 *             kernel, Lanczos CSR taps) as INPUTS, so a Go caller passes tables
 *             computed with Go's own math.Exp / math.Sin and gets results
 *             identical to the reference's.  This is what cgo binds.
 *   fennec_*  the reference's exported/unexported function set mirrored in C++
 *             above fnx_* (guards, control flow, table generation with libm) --
 *             the host side as it exists where no Go toolchain is available;
 *             also what the Python test/bench harness binds.
 *
 * Conventions
 *   - Images are 8-bit non-premultiplied R,G,B,A ("NRGBA", Go image.NRGBA.Pix):
 *     pixel (x,y) lives at pix[y*stride + 4*x]; stride is in BYTES; Rect.Min is
 *     ignored exactly as the reference's kernels ignore it.
 *   - `space` says where image pointers live: FNX_HOST (the library stages
 *     through its own pinned/device buffers; call returns when dst is filled)
 *     or FNX_DEVICE (HIP device pointers of the ctx's device; the op is enqueued
 *     on the ctx stream and returns immediately unless it has a host scalar
 *     output).  Tables and scalar outputs are always HOST pointers.
 *   - Inputs are never written; C never retains a caller pointer past return
 *     (cgo rule), except device pointers of in-flight FNX_DEVICE ops until
 *     fnx_ctx_sync().
 *   - A fnx_ctx owns one device, one stream and its scratch.  It is NOT
 *     re-entrant: one ctx per worker thread (HIP's current device is per OS
 *     thread and goroutines migrate, so every call binds the ctx's device).
 *   - Return codes: FNX_OK; FNX_NOOP = the reference returns the SAME image
 *     (dst untouched); FNX_EMPTY = the reference returns a 0x0 image (dst
 *     untouched); negative = error, text via fnx_last_error().  There is NO
 *     CPU fallback inside this library: without a usable GPU every op fails
 *     with FNX_ERR_NO_DEVICE.
 *   - Environment: a release build reads exactly these names, each once --
 *       FENNEC_HIP_DISABLE=1    no device is used (fnx_device_count() == 0)
 *       FENNEC_HIP_DEVICES=0,2  which HIP devices, in which order
 *       FNX_ROCTX=1             a roctx range per exported call (tracing)
 *       FNX_POOL_TRACE=1        per-item wall times of the C++ batch pools on stderr
 *       FNX_JPEG_TRACE=1        the device decoder's pass counts on stderr
 *     None of them changes a result or the kernel a call takes.  Which kernel
 *     FORM a ctx takes where several compute the same bytes is a per-ctx
 *     selection (fnx_ctx_set_form); development switches exist only in
 *     `make DEVELOP=1` builds.
 */
#ifndef FENNEC_HIP_H
#define FENNEC_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default) /* the library itself is built with -fvisibility=hidden */
#endif

#define FNX_OK 0
#define FNX_NOOP 1
#define FNX_EMPTY 2
#define FNX_ERR_INVALID (-1)
#define FNX_ERR_NO_DEVICE (-2)
#define FNX_ERR_HIP (-3)
#define FNX_ERR_OOM (-4)
#define FNX_ERR_UNSUPPORTED (-5) /* fnx_jpeg_decode / fnx_jpeg_recompress / fnx_png_decode: a file the device decoder does not handle; decode it on the host */

/* most images one *_batch / *_batch_enqueue call of round 6 takes (the image is a grid dimension of the launch) */
#define FNX_BATCH_MAX 65535

#define FNX_HOST 0
#define FNX_DEVICE 1
/* image -> image ops only (blur, blur3x3, sharpen, resize, box downsample, orient): the source is device
 * memory (fnx_malloc + fnx_upload, or an earlier device result), the destination is host memory and the
 * call returns when it is filled.  For search loops over ONE resident source -- the scale searches of
 * targetsize.go:240-313 call boxDownsample(src, w, h) 10-12 times and encode each result on the host --
 * so that the source crosses PCIe once. */
#define FNX_DEVICE_SRC 2

/* fnx_gaussian_blur flags */
#define FNX_BLUR_FAST 0  /* fp32 FMA accumulation: <=1 LSB off the reference on <=0.1% of samples */
#define FNX_BLUR_EXACT 1 /* bit-exact: fp32 with a rounding guard, fp64 in the reference's tap order for every
                            sample the guard cannot decide (and for kernels with negative taps or gain > 1) */

/* fnx_gaussian_blur_batch (and fnx_gaussian_blur with FNX_DEVICE: a batch of one, scored by fnx_ssim_fast), OR-ed to either
 * mode: "the next call on this ctx is fnx_ssim_fast_batch(_enqueue) over exactly
 * these (srcs[i], dsts[i]) pairs, and nothing writes the images in between".  The blur then runs as the one-pass kernel of
 * fnx_gaussian_blur_ssim_fast_batch -- same blurred bytes -- which also takes SSIMFast's boxDownsample sums (ssim.go:244-309)
 * of both sides, and that scoring call reads neither full-size image again: the reference's two calls (effects.go:146, then
 * ssim.go:48) at the one-pass traffic of 2 S instead of 4 S.  Scores are those of fnx_gaussian_blur_ssim_fast_batch (integer
 * box sums, then the same code).  Any other call on the ctx (fnx_ctx_use_stream / _use_own_stream / _profile / _kernel_ms do not
 * count), other pointers, strides or dims: the sums are dropped and
 * SSIMFast reads the images as always; shapes the one-pass kernel does not take run the plain blur.  The promise about
 * writes is the caller's: the library cannot see a store to device memory it was only lent.  Pays from two 4K images per call
 * up (B = 2: 5 %, 8: 21 %, 32: 23 % less time for the pair of calls); one image per call: no gain (profiles/r05_time_twocall_keep.txt). */
#define FNX_BLUR_KEEP_BOX_SUMS 2

typedef struct fnx_ctx fnx_ctx;
typedef struct fnx_prepared fnx_prepared;

/* ---- runtime ---------------------------------------------------------- */
const char *fnx_version(void);
/* Number of devices this library uses (0 when there is none / no driver / switched off).  Default: every HIP device.
 * Environment, read once: FENNEC_HIP_DEVICES="0,2,3" picks and orders HIP ordinals (device index i below is then the
 * i-th of them), FENNEC_HIP_DISABLE=1 leaves none -- fnx_ctx_create then returns FNX_ERR_NO_DEVICE, the status on
 * which the cgo shim runs the reference's own Go bodies ("force CPU or pick devices"). */
int fnx_device_count(void);
/* The same choice from code (wins over the environment): the n HIP ordinals to use, in order; n == 0: none (force
 * off); (NULL, -1): back to the environment's / every device.  Contexts that exist keep their device. */
int fnx_set_devices(const int *hip_ordinals, int n);
/* Thread-local text of the last error returned on this thread. */
const char *fnx_last_error(void);
int fnx_ctx_create(int device, fnx_ctx **out);
void fnx_ctx_destroy(fnx_ctx *ctx);
int fnx_ctx_device(const fnx_ctx *ctx);
/* The ctx's hipStream_t (as void*), for callers that time or order work. */
void *fnx_ctx_stream(fnx_ctx *ctx);
/* Launch on a stream of the CALLER's (a framework's current stream, the NULL stream included) instead of the ctx's
 * own: FNX_DEVICE work is then ordered with the caller's other work on that stream by construction -- inputs the
 * caller produced there are complete before the kernels read them, outputs are ready for whatever the caller enqueues
 * next, and a stream-ordered allocator may recycle the tensors safely -- with no cross-stream event per call (each such
 * dependency costs ~25 us of idle GPU between two back-to-back calls).  The switch itself orders everything the ctx has
 * already enqueued before the new stream's work.  The ctx does not own a lent stream: keep it alive until the ctx has
 * been switched away from it (or destroyed after a sync).  fnx_ctx_use_own_stream returns to the ctx's stream. */
int fnx_ctx_use_stream(fnx_ctx *ctx, void *hip_stream);
int fnx_ctx_use_own_stream(fnx_ctx *ctx);
/* Block until everything enqueued on the ctx has finished. */
int fnx_ctx_sync(fnx_ctx *ctx);
/* Diagnostics for roofline reporting: while enabled, the ctx brackets every launch of the selected
 * kernel classes with a pair of HIP events on the stream the kernel is launched on.  `enable` is a bit
 * mask of FNX_PROF_* (0: off; 1 = FNX_PROF_MAIN keeps its round-1 meaning: blur_direct_kernel of the
 * GaussianBlur fast / one-pass path and analyze_pass_kernel).  fnx_ctx_kernel_ms waits for the OLDEST
 * bracketed launch not read yet and returns its duration in milliseconds -- one call per launch, in
 * launch order; the last 32 launches are kept (FNX_ERR_INVALID if none is unread).  Calling
 * fnx_ctx_profile with a non-zero mask also forgets the unread ones. */
#define FNX_PROF_MAIN 1    /* blur_direct_kernel, analyze_pass_kernel */
#define FNX_PROF_SSIM 2    /* windowed_ssim_march_kernel */
#define FNX_PROF_RESIZE 4  /* resize kernels: one launch per lanczosResize (fused H + V) or two (resizeH, resizeV) */
#define FNX_PROF_FX 8      /* fx kernels: gaussianBlur3x3 / Sharpen / AdaptiveSharpen */
#define FNX_PROF_JPEG 16   /* jpeg_block_kernel (fdct, quantise, dequantise, idct of every block) */
int fnx_ctx_profile(fnx_ctx *ctx, int enable);
int fnx_ctx_kernel_ms(fnx_ctx *ctx, float *ms);
/* The kernel the ctx's LAST call of one class (one FNX_PROF_* bit: MAIN = GaussianBlur, SSIM = the windowed kernel,
 * RESIZE = lanczosResize, FX = gaussianBlur3x3 / Sharpen / AdaptiveSharpen) really launched, as a static string ("" before
 * the first such call, NULL for a bad argument): which of the routes the dispatch took (matrix pipe, direct, generic;
 * fused, two-pass ...).  FX answers "fx_stream_kernel", "fx_march_kernel" (the tile kernel) or "fx_ref_kernel" (fp64, the
 * reference's operation order: amounts outside the guard's bound, Sharpen amounts with a near-tie product), with
 * " + fx_flat_kernel" behind it for a SubImage (stride != 4 w).  Reporting only: bench.py names its roofline kernel with
 * it.  No reference counterpart. */
const char *fnx_ctx_last_kernel(fnx_ctx *ctx, int prof_class);
/* Arithmetic of the windowed statistics of FULL-RESOLUTION SSIM (ssim.go:24-43, 110-148: planes of 4 M windows and more --
 * fnx_ssim, fnx_ssim_enqueue, fennec_SSIM on large images; SSIMFast / MSSSIM planes are <= 512 px and always exact):
 *   FNX_SSIM_EXACT (default)  fp64 moments, |result - reference| <= 1e-9 (measured ~1e-12)
 *   FNX_SSIM_FAST             fp32 moments of centred luminances in a cancellation-free form of the same expression,
 *                             |result - reference| <= 1e-6 (SURVEY.md Appendix A's tolerance for fp32-moment paths;
 *                             measured <= 3e-7), identical images still give exactly 1.  About 1.5 x the throughput.
 * The analogue of FNX_BLUR_FAST / FNX_BLUR_EXACT; a property of the ctx because the SSIM entry points keep the reference's
 * argument lists.  The Go shim leaves the default. */
#define FNX_SSIM_EXACT 0
#define FNX_SSIM_FAST 1
int fnx_ctx_set_ssim_mode(fnx_ctx *ctx, int mode);
/* Whether the PNG entries of ONE ctx decode Adam7-interlaced files: accept 0 (default) -- such a file is FNX_ERR_UNSUPPORTED,
 * as callers that route on that answer expect; 1 -- it is decoded on the device (the rule: above fnx_png_decode).  Holds for
 * every entry that takes this ctx and PNG bytes: fnx_png_decode (its dst == NULL probe too, when this ctx is passed; with
 * ctx == NULL the probe keeps the default's answer), fnx_png_decode_batch, fnx_png_recompress_batch, fennec_CompressFileJPEG /
 * PNG / PNGReduce / PNGStream.  The fennec_CompressBatch* pools create their own contexts and keep the default; fnx_png_info
 * and the limit of 65535 a dimension are untouched.  ctx == NULL or accept outside 0..1: FNX_ERR_INVALID.  A property of the
 * ctx for the reason fnx_ctx_set_ssim_mode is one; the Go shim leaves the default. */
int fnx_ctx_set_png_adam7(fnx_ctx *ctx, int accept);
/* Kernel-form selection of ONE ctx, for tests and A/B timing: every form computes the same bytes as the default, the
 * selection only says which kernel does it, so that a fallback the product takes for rare tables (the fp64
 * reference-order kernels, the two-pass twin of a fused launch ...) can be run on any image and compared.  name / value:
 *   "fx_stream" "0"        effects.hip's tile kernel instead of the streaming kernel
 *   "fx_pairs" "0"         the tile kernel's one-row form
 *   "fx_ref" "1"           the fp64 reference-order effects kernel
 *   "resize_mfma" "0|1|2"  matrix-pipe resize never / downscales (default) / wherever the tables allow (read when a plan is built)
 *   "resize_fp64" "1"      the fp64 reference-order resize kernels
 *   "resize_fused" "0"     the two-pass resize kernels
 *   "msssim_levelwise" "1", "msssim_nofuse0" "1", "msssim_fold" "0", "msssim_boxfly" "1"   MSSSIM's launch structure
 *   "palette_grid" "0|1"   applyPalette: whole-palette walk for every image / the candidate grid for every image
 *   "analyze_staged" "1"   fnx_analyze, fnx_analyze_batch: the staged launches (analyze_pass_kernel and the kernels after it) for
 *                          every call ("0" and the default: one launch, analyze_one_kernel, and the staged launches for a batch
 *                          of more than 4096 images).  fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) names the route's first kernel
 *   "resize_box" "1"       fnx_lanczos_box_downsample, fnx_ssim_fast_resized, target-size mode: resize_box_kernel where its
 *                          domain allows ("0" and the default: lanczosResize into scratch, then the box kernel)
 *   "jpeg_size" "1"        a size-only JPEG query (out == NULL with cap == 0 in fnx_jpeg_encode / _encode_scaled, every query of
 *                          fnx_jpeg_size_search, fnx_jpeg_target_size and fennec_CompressFileTargetSize): the stuffed bytes are
 *                          counted from the blocks' strips (jpeg_ffcount_strips_kernel) and the size comes back in one wait
 *                          ("0" and the default: the string is packed and stuffed as for a file, two waits; files always
 *                          are).  Opt-in: DESIGN.md 5.1 has the measurement.  fnx_ctx_last_kernel(ctx, FNX_PROF_JPEG) names
 *                          jpeg_ffcount_strips_kernel or jpeg_pack_kernel after such a query.  The fennec_CompressBatch* pools
 *                          create their own contexts and keep the default
 * value NULL: back to the default.  Unknown name or a value longer than 7 characters: FNX_ERR_INVALID.  No reference counterpart. */
int fnx_ctx_set_form(fnx_ctx *ctx, const char *name, const char *value);

/* Device memory on the ctx's device (for FNX_DEVICE callers). */
int fnx_malloc(fnx_ctx *ctx, size_t bytes, void **dptr);
int fnx_free(fnx_ctx *ctx, void *dptr);
/* 2-D copies host<->device, stream-ordered; both return after completion. */
int fnx_upload(fnx_ctx *ctx, void *dptr, int dstride, const void *host, int hstride, int w, int h);
int fnx_download(fnx_ctx *ctx, void *host, int hstride, const void *dptr, int dstride, int w, int h);

/* ---- effects.go ------------------------------------------------------- */
/* GaussianBlur body (effects.go:167-219): separable, clamp-to-edge, RGB only,
 * uint8 intermediate, alpha from the source.  kernel[2*radius+1] is the
 * normalised 1-D kernel of effects.go:153-165.  The sigma<=0 guard
 * (effects.go:147-149) belongs to the caller. */
int fnx_gaussian_blur(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                      const double *kernel, int radius, int flags, uint8_t *dst, int dstride);
/* A source with sstride != 4*w is a Go SubImage to fnx_blur3x3 / fnx_sharpen / fnx_adaptive_sharpen (and to fnx_msssim):
 * the reference copies borders and alpha -- and MSSSIM its whole pyramid base -- from the FIRST 4*w*h bytes of the flat
 * Pix slice (effects.go:68,120; convert.go:16; ssim.go:345), not row by row, and so do these entry points.  A caller
 * that passes an ordinary pitched or cropped view and wants row-wise semantics must hand over a tight copy.  dst must
 * not alias src (the flat-copy pass rewrites dst after the filter). */
/* The fixed-point form the matrix-pipe kernel (csrc/blur_mfma.hip) gives a GaussianBlur table (effects.go:153-165), for
 * callers and tests that want to reason about it: wq[k] = round(kernel[k] * 2^24) with the centre tap taking what is left
 * of 2^24 (so sum wq == 2^24 exactly), and *err255 = 255 * max(P, N), P / N the sums of the positive / negative differences
 * wq[k] - kernel[k] * 2^24 -- the largest distance, in units of 2^-24, between the integer sum sum wq[k] * p[k] and the real
 * sum sum kernel[k] * p[k] * 2^24 over bytes 0 <= p <= 255.  A sample
 * whose (sum + 2^23) mod 2^24 lies at least ceil(*err255) + 2 away from 0 and from 2^24 rounds to the same byte as the
 * reference's clampF of its fp64 chain; the others are recomputed in fp64 (FNX_BLUR_EXACT).  Host arithmetic only, no
 * device.  FNX_NOOP: the table is not the matrix kernels' (radius outside 1..62, a negative or >= 0.49 weight, sum != 1). */
int fnx_blur_fixed_point(const double *kernel, int radius, long long *wq /* 2*radius+1 */, double *err255);
/* gaussianBlur3x3 (effects.go:116-141). */
int fnx_blur3x3(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                uint8_t *dst, int dstride);
/* Sharpen body (effects.go:24-44), amount = 1+1.5*strength; requires w,h >= 3. */
int fnx_sharpen(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                double amount, uint8_t *dst, int dstride);
/* AdaptiveSharpen body (effects.go:63-89) incl. localEdgeStrength
 * (effects.go:93-112), amount = 1+2*strength; requires w,h >= 3. */
int fnx_adaptive_sharpen(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                         double amount, uint8_t *dst, int dstride);
/* Sharpen / AdaptiveSharpen bodies of n same-geometry DEVICE images (srcs / dsts: host arrays of device pointers, dst != src):
 * the bytes of n single calls, one launch of the streaming kernel for tight images (stride == 4 w; the image is its second
 * grid dimension), image by image otherwise.  Frames below 8K do not fill the machine alone (a 1080p image is 2 000 waves of
 * 12 rows each); enqueued, no wait. */
int fnx_sharpen_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h, double amount,
                      uint8_t *const *dsts, int dstride);
int fnx_adaptive_sharpen_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h, double amount,
                               uint8_t *const *dsts, int dstride);

/* ---- resize.go -------------------------------------------------------- */
/* Lanczos tap table in CSR form: taps of output d are
 * index[offset[d] .. offset[d+1]) with weight[...] (precomputeWeights,
 * resize.go:164-197).  offset has dst+1 entries. */
/* resizeH (resize.go:77-118): src srcW x srcH -> dst dstW x srcH. */
int fnx_resize_h(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW, int srcH,
                 const int32_t *offset, const int32_t *index, const double *weight,
                 uint8_t *dst, int dstride, int dstW);
/* resizeV (resize.go:121-161): src srcW x srcH -> dst srcW x dstH. */
int fnx_resize_v(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW, int srcH,
                 const int32_t *offset, const int32_t *index, const double *weight,
                 uint8_t *dst, int dstride, int dstH);
/* lanczosResize (resize.go:37-53): guards, equal-dims flat copy, H then V
 * through a uint8 intermediate.  Tables may be NULL when dims are equal. */
int fnx_lanczos_resize(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW,
                       int srcH, const int32_t *offH, const int32_t *idxH, const double *wH,
                       const int32_t *offV, const int32_t *idxV, const double *wV,
                       uint8_t *dst, int dstride, int dstW, int dstH);
/* The fixed-point form the matrix-pipe resize kernel (csrc/resize_mfma.hip: resize_mfma_kernel) gives ONE tap table of
 * nout outputs over srcN source px, for callers and tests that want to reason about it -- the very arithmetic the plan
 * builder runs (one function serves both), as under fnx_ctx_set_form(ctx, "resize_mfma", "2"):
 *   *S            the weights' binary point, 22 or 23 (23 where every |W_k| 2^23 <= 8355000; W_k = fl(255 w_k) * inv, inv =
 *                 1.0 / a, a = the sum of fl(255 w_k) in tap order)
 *   *G            the rounding guard in units of 2^-S: ceil(255 max(P, N)) + 2, P / N the largest sums of the positive /
 *                 negative differences Wq_k - W_k 2^S of one output
 *   first[d], count[d], wq[16 d .. 16 d + count[d])   output d's first source index, taps (<= 16) and integer weights, whose
 *                 sum is 2^S exactly (zeros behind the taps)
 * With u = sum_k Wq_k (R_k - 128) + (192 << S) + 2^(S-1) + G, an exact uint32, the kernel writes clamp((u >> S) - 64, 0, 255)
 * unless u mod 2^S < 2 G: such a sample is recomputed in fp64 in the reference's own order (resize.go:95-112).
 * Host arithmetic only: no ctx, no device.  FNX_NOOP: the table is not the kernel's (nout or srcN below 16, an output with
 * more than 16 taps or a gap in its indices, a outside [254.5, 255.5), negative lobes beyond 63 / 255, a weight three signed
 * base-256 digits do not reach) -- nothing is written.  FNX_ERR_INVALID: a NULL pointer, decreasing offsets, an index
 * outside the source.  What a plan adds for the H or V direction (window widths of a 16-output group) is not covered here.
 * No reference counterpart. */
int fnx_resize_fixed_point(const int32_t *offset, const int32_t *index, const double *weight, int nout, int srcN,
                           int *S, int *G, int32_t *first /* nout */, int32_t *count /* nout */, int32_t *wq /* 16*nout */);
/* What became of the workgroups of the ctx's most recent resize call that launched resize_mfma_kernel (a batch counts as
 * one call), to be asked after fnx_ctx_sync: *workgroups = how many it launched, *gave_up = how many of them handed their
 * region back to resize_fused_sparse_kernel (translucent pixels, a set dense with flagged samples).  *workgroups == 0: no
 * such call is on record (none yet, or a later resize call has taken the count for its cool-down decision).  Reporting
 * only, as fnx_ctx_last_kernel: reading it changes nothing, the cool-down reads the same word at the next call.  NULL ctx or
 * outputs, or a call still running: FNX_ERR_INVALID.  No reference counterpart. */
int fnx_ctx_resize_mfma_report(fnx_ctx *ctx, unsigned *gave_up, unsigned *workgroups);
/* lanczosResize of n same-geometry DEVICE images (srcs / dsts: host arrays of device pointers) with one tap-table pair: the
 * bytes of n fnx_lanczos_resize calls, enqueued as ONE set of launches where the one-launch kernels apply (a 4K resize
 * alone is ~700 workgroups on 768-1024 resident slots: one under-filled round; a batch fills the machine and pays the
 * launch, the plan look-up and the tails once).  Other tables (windows wider than the fused tile, tables outside the
 * rounding guard) run image by image.  CompressBatch workers that resize many same-sized frames (fennec.go:127-129). */
int fnx_lanczos_resize_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int srcW, int srcH,
                             const int32_t *offH, const int32_t *idxH, const double *wH,
                             const int32_t *offV, const int32_t *idxV, const double *wV,
                             uint8_t *const *dsts, int dstride, int dstW, int dstH);

/* ---- ssim.go ---------------------------------------------------------- */
/* boxDownsample (ssim.go:244-309). */
int fnx_box_downsample(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW,
                       int srcH, uint8_t *dst, int dstride, int dstW, int dstH);
/* SSIMFast (ssim.go:48-70); window = gaussianKernel(8,1.5) (ssim.go:223-241),
 * 64 doubles.  Both images are w x h (the reference does not check). */
int fnx_ssim_fast(fnx_ctx *ctx, int space, const uint8_t *a, int astride, const uint8_t *b,
                  int bstride, int w, int h, const double *window, double *out);
/* pixelSSIM (ssim.go:169-204), the branch SSIM / SSIMFast take when w < 8 || h < 8, with the slices' REAL
 * lengths: the reference walks `for i := 0; i < len(a.Pix); i += 4` over both flat Pix slices, and for a
 * SubImage len(Pix) runs to the end of the PARENT's buffer (image.NRGBA.SubImage: Pix = p.Pix[i:]), not just to
 * the sub-image's last pixel.  fnx_ssim / fnx_ssim_fast only know (h-1)*stride + 4w -- the shortest slice a
 * w x h image can have, which is what image.NewNRGBA and every image in this path's own pipeline has; a caller
 * holding a true SubImage under 8 px passes len(a.Pix), len(b.Pix) here.  b_pix_len < a_pix_len is
 * FNX_ERR_INVALID (the reference panics: index out of range).  a_pix_len is rounded up to a multiple of 4 the way
 * the loop's last iteration reads it (and must then fit).  Divides by w*h like the reference; w*h == 0 -> 1.0. */
int fnx_pixel_ssim(fnx_ctx *ctx, int space, const uint8_t *a_pix, size_t a_pix_len, const uint8_t *b_pix,
                   size_t b_pix_len, int w, int h, double *out);
/* SSIM (ssim.go:24-43) for equal dims (differing dims: fnx_ssim_resized;
 * fennec_SSIM routes both). */
int fnx_ssim(fnx_ctx *ctx, int space, const uint8_t *a, int astride, const uint8_t *b,
             int bstride, int w, int h, const double *window, double *out);
/* MSSSIM (ssim.go:313-365) for equal dims; per_level (NULL or 5 doubles)
 * receives each level's SSIMFast, NaN where the reference stops early.  Strides are NOT honoured for the pyramid base:
 * toNRGBA copies the first 4*w*h flat bytes (convert.go:16, ssim.go:345) -- see the SubImage note at fnx_blur3x3. */
int fnx_msssim(fnx_ctx *ctx, int space, const uint8_t *a, int astride, const uint8_t *b,
               int bstride, int w, int h, const double *window, double *out, double *per_level);

/* ---- resize, then score: the pairs of steps the reference makes when two images differ in size ----
 * Tables as fnx_lanczos_resize takes them: offH / idxH / wH for bw -> aw, offV / idxV / wV for bh -> ah; they may be NULL
 * when the dims are equal (the call is then exactly the plain entry point's).  Guards as fennec_SSIM: an empty `a` scores
 * 1.0, an empty `b` beside a non-empty `a` is FNX_ERR_INVALID (the reference panics), differing dims with a NULL table are
 * FNX_ERR_INVALID.  All of them block and return a scalar, so they follow the other blocking forms' rules about the
 * result FIFO.  In either space each image crosses PCIe once -- `a` at its size, `b` at ITS OWN size -- and nothing comes
 * back but the score: the resized image lives and dies in the ctx's scratch memory. */
/* boxDownsample(lanczosResize(src, midW, midH), dstW, dstH) (resize.go:37-53, then ssim.go:244-309), bit-exact.  On the
 * fused route (form "resize_box" "1"; csrc/resize_box.hip: resize_box_kernel, reported by fnx_ctx_last_kernel(ctx, FNX_PROF_RESIZE)) the
 * midW x midH image never exists in memory: a workgroup resizes a tile into registers and adds its bytes to integer box
 * sums.  Fused domain: an upscale or equal size on both axes whose tables have contiguous tap indices and at most 8 taps
 * per output (every precomputeWeights table for src <= mid), dst <= mid on both axes with boxes at most 32 px wide -- every
 * pair target-size mode makes (b = int(aw s) x int(ah s), 0.05 <= s < 1, both dims >= 8, a's long side from 513 to beyond
 * 8192 px).  Everything else -- a downscale on either axis, tables with gaps, dst above mid -- is composed from
 * fnx_lanczos_resize into scratch and fnx_box_downsample, same bytes.  The fused route is OPT-IN, fnx_ctx_set_form(ctx,
 * "resize_box", "1"): it has not been timed against the composed one (tools/time_ssim_resized.py is the script; no table
 * is committed), so the default stays with the kernels target-size mode has run so far. */
int fnx_lanczos_box_downsample(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW, int srcH,
                               const int32_t *offH, const int32_t *idxH, const double *wH,
                               const int32_t *offV, const int32_t *idxV, const double *wV,
                               int midW, int midH, uint8_t *dst, int dstride, int dstW, int dstH);
/* Would fnx_lanczos_box_downsample take the fused route for these tables and dims under "resize_box" "1" (the domain above)?  1 / 0.  Host arithmetic
 * only, no device, no ctx: what the library itself asks before every such call.  No reference counterpart. */
int fnx_lanczos_box_fused(int srcW, int srcH, const int32_t *offH, const int32_t *idxH, const double *wH,
                          const int32_t *offV, const int32_t *idxV, const double *wV, int midW, int midH, int dstW, int dstH);
/* computeSSIMNRGBA(a, b) (targetsize.go:563-568): SSIMFast(a, lanczosResize(b, aw, ah)).  Where SSIMFast downsamples (a's
 * long side above 512 px) only the box plane of the resized b is needed: fnx_lanczos_box_downsample's routes make it; a smaller `a`
 * is compared against the whole resized image.  An `a` under 8 px (pixelSSIM) must be tight. */
int fnx_ssim_fast_resized(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah,
                          const uint8_t *b, int bstride, int bw, int bh,
                          const int32_t *offH, const int32_t *idxH, const double *wH,
                          const int32_t *offV, const int32_t *idxV, const double *wV, const double *window, double *out);
/* SSIM with differing dims (ssim.go:24-43, the resize of lines 31-33 included): b is resized on the device into scratch
 * and scored there at full resolution. */
int fnx_ssim_resized(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah,
                     const uint8_t *b, int bstride, int bw, int bh,
                     const int32_t *offH, const int32_t *idxH, const double *wH,
                     const int32_t *offV, const int32_t *idxV, const double *wV, const double *window, double *out);
/* MSSSIM with differing dims (ssim.go:313-365, the resize of lines 320-322 included); per_level as fnx_msssim's. */
int fnx_msssim_resized(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah,
                       const uint8_t *b, int bstride, int bw, int bh,
                       const int32_t *offH, const int32_t *idxH, const double *wH,
                       const int32_t *offV, const int32_t *idxV, const double *wV, const double *window, double *out,
                       double *per_level);

/* Binary-search form of SSIMFast (compress.go:45-74 calls SSIMFast(src, decoded)
 * with the same src every iteration): downsample + luminance of the reference
 * side once, then compare candidates against it. */
int fnx_ssim_fast_prepare(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int w, int h,
                          fnx_prepared **out);
int fnx_ssim_fast_against(fnx_ctx *ctx, const fnx_prepared *ref, int space, const uint8_t *b,
                          int bstride, const double *window, double *out);
void fnx_prepared_free(fnx_ctx *ctx, fnx_prepared *p);

/* SURVEY 8(f)2, first slice -- the JPEG quantisation round trip on the device.  dst = toNRGBARef(jpeg.Decode(
 * jpeg.Encode(src, Options{Quality: quality}))) as far as the PIXELS go (compress.go:50-58 via io.go:157-169): baseline
 * 4:2:0, Go's colour equations, integer FDCT / IDCT and quantiser scaling, no entropy coding (it is lossless).  The
 * arithmetic restates Go's standard library, which is not part of the reference tree: parity with Go is unpinned twice
 * over; against the oracle's restatement it is bit-exact.  4:4:4 on a ctx set so: fnx_ctx_set_jpeg_subsampling. */
int fnx_jpeg_roundtrip(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int quality,
                       uint8_t *dst, int dstride);
/* compressJPEGOptimal's binary search (compress.go:21-74) with every candidate quality round-tripped and scored on the
 * device: *quality = lowest quality whose SSIMFast(src, round trip) >= target_ssim (the reference's lower bounds by
 * target, target >= 1 -> 0.999), *ssim its score, *steps the candidates tried.  FNX_NOOP: none reached the target
 * (*quality = 100, *ssim = 1.0, as the reference's fallback).  The caller encodes ONCE, at *quality, with the real codec. */
/* jpeg.Encode(src, &jpeg.Options{Quality: quality}) (io.go:157-169) on the device: the complete file -- baseline, 4:2:0,
 * the typical Huffman tables, writer.go's segment order -- into host memory `out` (capacity cap); *nbytes = its size.
 * FNX_ERR_INVALID with *nbytes set when cap is too small (call again); out == NULL with cap == 0 asks for the size
 * only (what targetsize.go's searches look at) and copies nothing.  Decoding the file gives exactly
 * fnx_jpeg_roundtrip's pixels (the entropy coder is lossless).  Restated from ITU T.81 and Go's file layout, not from
 * Go's source: byte parity with jpeg.Encode is unpinned; libjpeg-turbo decodes the files.
 * The file's Huffman tables follow fnx_ctx_set_jpeg_huffman, its chroma subsampling fnx_ctx_set_jpeg_subsampling. */
int fnx_jpeg_encode(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int quality, uint8_t *out, size_t cap,
                    size_t *nbytes);
/* jpegQualitySearchOpt (targetsize.go:125-176): the HIGHEST quality whose file fits target_bytes -- the bisection over
 * [lo, hi] the reference picks from the bits per pixel, every candidate's size from the device's entropy coder
 * (nothing is copied for a candidate), then the winner's file into `out` and, unless skip_ssim, its SSIMFast against the
 * source (the reference's computeSSIMNRGBA of the decoded winner).  FNX_NOOP: no quality fits (bestBuf == nil).
 * FNX_ERR_INVALID with *nbytes set when cap is too small. The file's Huffman tables follow fnx_ctx_set_jpeg_huffman, its chroma
 * subsampling fnx_ctx_set_jpeg_subsampling. */
int fnx_jpeg_size_search(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, long long target_bytes, int skip_ssim,
                         const double *window /* 64; may be NULL with skip_ssim */, uint8_t *out, size_t cap, size_t *nbytes,
                         int *quality, double *ssim, int *steps /* may be NULL */);
/* compressJPEGOptimal (compress.go:21-87) for one image in one call: the quality search of fnx_jpeg_quality_search, then
 * the file at the quality it found (100 when nothing reached the target) as fnx_jpeg_encode writes it -- one upload of
 * the source, no host codec.  *ssim is the winning candidate's SSIMFast (1.0 when none won, as the reference reports).
 * The file's Huffman tables follow fnx_ctx_set_jpeg_huffman; the search and the file follow fnx_ctx_set_jpeg_subsampling. */
int fnx_jpeg_compress(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, double target_ssim,
                      const double *window /* 64 */, uint8_t *out, size_t cap, size_t *nbytes, int *quality, double *ssim,
                      int *steps /* may be NULL */);
int fnx_jpeg_quality_search(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, double target_ssim,
                            const double *window /* 64 */, int *quality, double *ssim, int *steps);
/* jpeg.Encode(boxDownsample(src, dw, dh), quality) (ssim.go:244, io.go:157): the scaled image is never materialised --
 * the box sums go straight into the encoder's YCbCr planes (jpeg.hip: jpeg_box_ycc_kernel).  src is w x h in `space`,
 * dw x dh anything from 1 x 1 up to 65535 (also above w x h, as boxDownsample allows).  out / cap / *nbytes as
 * fnx_jpeg_encode: out == NULL with cap == 0: the size only (testScaleFits / findBestScale*'s question).
 * The file's Huffman tables follow fnx_ctx_set_jpeg_huffman. */
int fnx_jpeg_encode_scaled(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int dw, int dh,
                           int quality, uint8_t *out, size_t cap, size_t *nbytes);
/* The Huffman tables of the JPEG files a ctx writes.  FNX_JPEG_HUFFMAN_STANDARD (the default) is what the library always
 * wrote: the four typical tables of ITU T.81 Annex K.3.3, byte for byte.  FNX_JPEG_HUFFMAN_OPTIMIZED builds the four tables
 * (luminance DC, luminance AC, chrominance DC, chrominance AC; Y against Cb + Cr as before) from the symbols this file's own
 * scan codes -- what jpegtran -optimize does.  No coefficient changes, so no pixel and no SSIM score does: the same image
 * costs fewer bytes (types.go:146-153 and io.go:151-158 reserve their options for such an encoder).  The tables, exactly:
 *  - symbols: per block the category of its DC difference (predictions per component in scan order) and its (run, size)
 *    pairs, ZRL and EOB as the coder emits them; a symbol that does not occur gets no code and is not listed.
 *  - code sizes: T.81 Annex K.2, figures K.1 to K.4, over slots 0..255 (the symbols) and slot 256, a reserved symbol of
 *    frequency 1.  V1 is the slot of least non-zero frequency, V2 the slot of least non-zero frequency among the others; among
 *    equal frequencies the LARGEST slot index wins, both times.  V2 is merged into V1's slot.  Figure K.3 runs from length 32
 *    down to 17; the reserved symbol is then taken from the longest length in use.  HUFFVAL is ordered by (unlimited code
 *    size, symbol value); codes are canonical (Annex C).  (libjpeg's order: Pillow's optimize=True tables are these.)
 *  - a table whose unlimited code sizes exceed 32 is the standard table of its class, complete (a safety stop that real
 *    images do not reach).
 * The file keeps ONE DHT segment with the four tables in the same order; its length is 2 + sum(17 + symbols).
 * Followed by every entry that makes a JPEG file, or asks for its size, with this ctx -- fnx_jpeg_encode, fnx_jpeg_encode_scaled,
 * fnx_jpeg_size_search, fnx_jpeg_compress, fnx_jpeg_target_size, fnx_hit_target_size's JPEG legs, fnx_jpeg_recompress,
 * fennec_CompressFileJPEG, fennec_CompressFileTargetSize, fennec_CompressFileHitTargetSize, both size-query routes (the packed
 * string and form "jpeg_size" "1") -- and by fnx_jpeg_compress_batch and fnx_jpeg_recompress_batch, tables per image: a batch's
 * files stay byte for byte the single call's on the same ctx.  No host wait is added anywhere: the tables are built on the
 * device (csrc/jpeg.hip: jpeg_symhist_kernel, jpeg_hufftab_kernel; tools/jpeg_hufftab_hostsim runs the latter's text on the
 * CPU) and their DHT bodies come back with the totals.  The fennec_CompressBatch* pools and the Go shim create their own
 * contexts and keep the default.  The quality search's round trip never codes symbols and is untouched.  DESIGN.md 5.16.
 * ctx == NULL or any other mode: FNX_ERR_INVALID, nothing changed. */
#define FNX_JPEG_HUFFMAN_STANDARD  0
#define FNX_JPEG_HUFFMAN_OPTIMIZED 1
int fnx_ctx_set_jpeg_huffman(fnx_ctx *ctx, int mode);
/* What jpeg_symhist_kernel counts for this image at this quality: hist[t][s] = how often the scan of fnx_jpeg_encode(src,
 * quality) codes symbol s with table t (0 luminance DC, 1 luminance AC, 2 chrominance DC, 3 chrominance AC).  Independent of
 * the ctx's Huffman mode; the scan is the ctx's subsampling mode's (fnx_ctx_set_jpeg_subsampling).  NULL ctx, src or hist:
 * FNX_ERR_INVALID. */
int fnx_jpeg_symbol_histogram(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int quality,
                              uint32_t hist[4][256]);
/* jpeg_hufftab_kernel on the caller's four histograms (HOST; the tables are independent of each other): per table the DHT
 * body -- bits[t][L - 1] codes of length L, the nvals[t] values vals[t][..] in code order (the rest zero) -- the code look-up
 * words the coder reads, lut[t][s] = length << 24 | code (0: no code), and standard[t] = 1 when the table is the standard
 * table of its class (see above).  A NULL pointer or a table whose histogram is all zero: FNX_ERR_INVALID. */
int fnx_jpeg_huffman_tables(fnx_ctx *ctx, const uint32_t hist[4][256], uint8_t bits[4][16], uint8_t vals[4][256], int nvals[4],
                            uint32_t lut[4][256], int standard[4]);
/* The chroma subsampling of the JPEG files a ctx writes from ONE resident image.  FNX_JPEG_SUBSAMPLING_420 (the default) is
 * what the library always wrote.  FNX_JPEG_SUBSAMPLING_444 keeps the chroma at full resolution: the option the reference
 * reserves for "a custom encoder" (Options.Subsample, types.go:146-153; encodeJPEG drops it, io.go:151-158).  The file,
 * exactly -- writer.go's with every component at sampling 1 x 1:
 *  - padding: mx = (w + 7) / 8, my = (h + 7) / 8 MCUs of 8 x 8 px.
 *  - scan order: blocks in raster order; the MCU is three blocks, Y Cb Cr.
 *  - pixels of a block: block (bx, by) takes pixels min(8 bx + i, w - 1), min(8 by + j, h - 1) (toYCbCr's clamp).
 *  - colour: a pixel goes through color.RGBToYCbCr of its (for alpha < 255: premultiplied) RGB, as at 4:2:0; no averaging.
 *  - DCT and quantiser: unchanged (fdct, div(b, 8 q); table 0 for Y, table 1 for Cb and Cr).
 *  - DC prediction: per component, from the component's previous block, three scan positions back; 0 at the first MCU.
 *  - Huffman classes: luminance for Y, chrominance for Cb and Cr, as at 4:2:0.
 *  - header: byte for byte the 4:2:0 header of the same w, h, quality and Huffman mode, except the Y component's sampling byte
 *    in SOF0: 0x11 instead of 0x22.
 *  - decoding: the file decodes to an image.YCbCr of ratio 4:4:4; toNRGBARef of it is what fnx_jpeg_roundtrip returns.
 * FOLLOWED by fnx_jpeg_roundtrip, fnx_jpeg_quality_search, fnx_jpeg_encode, fnx_jpeg_compress, fnx_jpeg_size_search and
 * fnx_jpeg_symbol_histogram (compressJPEGOptimal and jpegQualitySearch on a resident image), in both Huffman modes and on both
 * size-query routes; no host wait is added.  REFUSED on a ctx set to 4:4:4, with FNX_ERR_UNSUPPORTED before anything is
 * launched, uploaded or written and a message naming the entry and "4:4:4": fnx_jpeg_encode_scaled, fnx_jpeg_target_size,
 * fnx_hit_target_size (whatever its format), fnx_jpeg_recompress, fnx_jpeg_compress_batch, fnx_jpeg_recompress_batch,
 * fennec_CompressFileJPEG, fennec_CompressFileTargetSize, fennec_CompressFileHitTargetSize.  The decoders, the PNG entries and
 * everything else ignore the mode; the fennec_CompressBatch* pools and the Go shim create their own contexts and keep 4:2:0.
 * csrc/jpeg_layout.hpp states the two layouts once for host and device code; csrc/jpeg.hip: jpeg_ycc444_kernel.  DESIGN.md 5.18.
 * ctx == NULL or any other mode: FNX_ERR_INVALID, nothing changed. */
#define FNX_JPEG_SUBSAMPLING_420 0   /* default: what the library always wrote */
#define FNX_JPEG_SUBSAMPLING_444 1
int fnx_ctx_set_jpeg_subsampling(fnx_ctx *ctx, int mode);
/* hitTargetSize's JPEG strategies (targetsize.go:26-357) in one call, the source staged once and every scale step's
 * file size taken on the device (fnx_jpeg_encode_scaled's planes; 8 bytes come back per size query).  `strategies`: */
#define FNX_TS_QUALITY 1       /* strategy 1: jpegQualitySearch(src)                        targetsize.go:33-37, 117-176 */
#define FNX_TS_QUALITY_SCALE 2 /* strategy 3: jpegQualityScaleSearch                        targetsize.go:45-49, 210-283 */
#define FNX_TS_SCALE 4         /* strategy 4: scaleSearch(src, target, JPEG); runs only when no
                                  strategy of this call produced a candidate                targetsize.go:51-62, 285-357 */
#define FNX_TS_FALLBACK 8      /* fallbackTargetSizeEncode's JPEG branch: quality 1 at full size,
                                  ssim = computeSSIMNRGBA(src, src); only when nothing else  targetsize.go:64-90 */
typedef struct fnx_size_candidate {
    int32_t strategy;        /* the FNX_TS_* bit; 0: not run or no candidate */
    int32_t quality, final_w, final_h;
    int32_t steps;           /* encodes this strategy ran (size queries, plus strategy 4's encode at bestQ when its final
                                search finds nothing; the fallback's one) -- also when it produced no candidate */
    int32_t reserved;
    int64_t nbytes;          /* len(data) */
    double ssim;             /* sizeResult.ssim exactly as the reference sets it */
} fnx_size_candidate;
/* cand[i]: strategy bit i's result (cand[0] FNX_TS_QUALITY ... cand[3] FNX_TS_FALLBACK); *winner: the index betterFit
 * (targetsize.go:92-115) picks over them in the reference's order, a tie keeping the earlier one.  `out` gets the
 * winner's file (out == NULL with cap == 0: *nbytes only); `img` (may be NULL; in `space`, stride istride >= 4 w) the
 * winner's final_w x final_h Lanczos image when it is strategy 3's or 4's -- left untouched otherwise (the image is then
 * the source).  *cancel != 0 (may be NULL) is looked at where the reference checks ctx.Err(): before each strategy and
 * each scale step; the fallback runs also after a cancellation, as the reference's does.  FNX_OK: there is a winner;
 * FNX_NOOP: no candidate; FNX_ERR_INVALID: bad arguments, or cap too small -- then *nbytes, cand, *winner and img are
 * filled and fnx_jpeg_encode(img or src, cand[*winner].quality) gives the file without searching again.
 * The file's Huffman tables follow fnx_ctx_set_jpeg_huffman. */
int fnx_jpeg_target_size(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, long long target_bytes,
                         int strategies, const double *window /* 64 */, const volatile int *cancel /* may be NULL */,
                         fnx_size_candidate cand[4], int *winner, uint8_t *out, size_t cap, size_t *nbytes, uint8_t *img,
                         int istride);
/* hitTargetSize's PNG legs (targetsize.go:39-43, 51-90, 180-206, 285-347) in one call on a resident image, the sibling of
 * fnx_jpeg_target_size: every "how many bytes?" is fnx_png_encoded_size's question (the deflate kernels' size-only forms, 8
 * bytes back), a file is made once, for the winner.  `strategies`: a non-empty subset of */
#define FNX_TS_QUANTIZE     16  /* strategy 2: quantizeStrategy                      targetsize.go:39-43, 180-206 */
#define FNX_TS_SCALE_PNG    32  /* strategy 4 with format PNG: scaleSearch/testScaleFits/executeFinalScaleEncode
                                   targetsize.go:51-62, 285-347; only when no strategy of this call produced a candidate */
#define FNX_TS_FALLBACK_PNG  64 /* fallbackTargetSizeEncode's PNG branch: compressPNG(original), ssim 1.0; only when nothing else
                                   targetsize.go:64-90 */
/* (fnx_jpeg_target_size and fennec_CompressFileTargetSize refuse these bits, this entry refuses the four JPEG bits.)
 * Quantize: medianCut ONCE at the levels 16, 32, 64, 128, 256 (the palettes are prefixes of one run; they stay on the device),
 * then the levels from 256 down: applyPalette's index plane, the size of its paletted file (bit depth by the level's colour
 * count as fnx_png_filter's table says, no tRNS), the first level at or under the target wins; only for it palettedToNRGBA and
 * SSIMFast run.  A level whose colour count equals the level's before it (the run stopped early) takes that level's size.
 * Scale: the reference's twelve bisection steps, per step boxDownsample and the size of the scaled NRGBA image's file (RGB rows
 * when it is Opaque(); no tryPalettize, no toGray: testScaleFits hands png.Encode the image as it is), then lanczosResize at the
 * best scale and its file's size -- which may be over the target, as in the reference.  Fallback: fnx_png_reduce(256) and the
 * reduced image's file, ssim exactly 1.0.  quality is 0 in every candidate.
 * WHAT "FITS" MEANS: every size is the size of THIS library's file under the ctx's deflate level, not the size Go's
 * compress/flate would give (the same opt-in fennec_CompressFilePNG asks for).  A winner reported at or under the target IS a
 * file at or under the target; which level or scale wins can differ from the reference's for targets between the two encoders'
 * sizes.  FNX_DEFLATE_LEVEL_DENSE is recommended here: its sizes are the nearer to png.BestCompression's.
 * cand[0] quantize, cand[1] scale, cand[2] fallback; steps: the size queries the leg ran (the final Lanczos file's and the
 * fallback's one included; a level that took its neighbour's size ran none).  *winner, out / cap / *nbytes, cancel (looked at
 * before each leg and each scale step; the fallback runs also after a cancellation), the return codes and the cap-too-small
 * protocol (FNX_ERR_INVALID with *nbytes, cand, *winner and img filled) are fnx_jpeg_target_size's.  img (may be NULL; in
 * `space`, stride istride >= 4 w): the quantize winner's w x h quantized image or the scale winner's final_w x final_h Lanczos
 * image; untouched for the fallback (the image is the source).  FNX_ERR_INVALID before any device work also for a padded
 * source (sstride != 4 w) with FNX_TS_QUANTIZE: medianCut samples the flat Pix slice (fnx_median_cut). */
int fnx_png_target_size(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, long long target_bytes,
                        int strategies /* subset of the three */, const double *window /* 64 */, const volatile int *cancel /* may be NULL */,
                        fnx_size_candidate cand[3], int *winner, uint8_t *out, size_t cap, size_t *nbytes, uint8_t *img, int istride);
/* All of hitTargetSize (targetsize.go:26-75) in one call, the source staged once, SSIMFast's prepared side of it shared by
 * every leg.  format: Options.Format (types.go:35-42): */
#define FNX_FORMAT_AUTO 0
#define FNX_FORMAT_JPEG 1
#define FNX_FORMAT_PNG  2
/* canUseJPEG = format != PNG && isOpaque(src) (the flat scan of fennec_isOpaque).  cand[0]: strategy 1 and cand[2]: strategy 3
 * (when canUseJPEG or format == JPEG); cand[1]: quantize (format != JPEG); cand[3]: strategy 4 when nothing before it produced
 * a candidate, in the format the reference picks -- its `strategy` says which, FNX_TS_SCALE or FNX_TS_SCALE_PNG; cand[4]: the
 * fallback when there is still none, FNX_TS_FALLBACK or FNX_TS_FALLBACK_PNG.  *winner: betterFit over the candidates in that
 * order, a tie keeping the earlier one; the output's format is read off cand[*winner].strategy (a PNG leg's bit: a PNG file).
 * With format == FNX_FORMAT_JPEG the call IS fnx_jpeg_target_size with all four bits: the same fields (cand[0], [2], [3], [4])
 * and the same bytes.  The PNG legs' sizes are this library's (see fnx_png_target_size).  Everything else -- cancel, out / cap
 * / *nbytes, img, the return codes -- as fnx_jpeg_target_size; a padded source is refused unless format == FNX_FORMAT_JPEG.
 * The file's Huffman tables follow fnx_ctx_set_jpeg_huffman. */
int fnx_hit_target_size(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, long long target_bytes, int format,
                        const double *window /* 64 */, const volatile int *cancel /* may be NULL */, fnx_size_candidate cand[5], int *winner,
                        uint8_t *out, size_t cap, size_t *nbytes, uint8_t *img, int istride);
/* SURVEY 8(f)2, third slice -- image.Decode of a JPEG source (batch.go:88-101 via io.go:60-95) on the device:
 * dst = toNRGBARef(jpeg.Decode(data)), *w x *h.  `data` is HOST memory (the file); dst is in `space`.  dst == NULL:
 * only the dimensions (jpeg.DecodeConfig) -- and whether the device decoder takes the file at all (host work: ctx may be
 * NULL and no device is touched).  Handled: 8 bit, three components (4:4:4, 4:2:2, 4:2:0, 4:4:0, 4:1:1, 4:1:0), one
 * (image.Gray) or four (image.CMYK: Adobe CMYK / YCbCrK with every component 1 x 1, reader.go applyBlack), with or without restart
 * intervals: baseline (SOF0), extended sequential (SOF1) and progressive (SOF2) frames in
 * any number of scans; anything else (12 bit, arithmetic coding, lossless) returns
 * FNX_ERR_UNSUPPORTED and the caller decodes on the host (an explicit answer, not a fallback inside the library).
 * FNX_ERR_INVALID: a scan that ends early or holds a code outside its Huffman table.  Baseline: Huffman decoding is parallel
 * over 1024-bit spans of the scan that synchronise with their neighbours (jpeg_dec.hip); the result does not depend on how
 * many rounds that takes.  Progressive (r5): a refinement scan's bits depend on the coefficients of the scans before it, so
 * the scans are entropy-decoded on the host (jpeg_prog.cpp) and the coefficients go up at 2 bytes each -- as are the sequential
 * files that decoder has no form for (SOF1, components in scans of their own, a table that assigns the all-ones code); dequantisation, IDCT
 * and colour conversion are the device's as for baseline.  Restated from ITU T.81 and Go's documented behaviour (scan.go's
 * refine / reconstructProgressiveImage): bit-exact against the tests' CPU restatement, parity with Go unpinned.
 * The host route sizes 136 bytes of host memory per block from the frame header alone, so it takes at most
 * FNX_JPEG_HOST_MAX_BLOCKS blocks (16K x 8K at 4:2:0); a header that promises more is FNX_ERR_UNSUPPORTED (the host codec's). */
#define FNX_JPEG_HOST_MAX_BLOCKS (1 << 22)
int fnx_jpeg_decode(fnx_ctx *ctx, const uint8_t *data, size_t n, int space, uint8_t *dst, int dstride, int *w, int *h);
/* Host only (no ctx, no device): what fnx_jpeg_decode hands the device for a progressive (SOF2) file -- the quantised
 * coefficients over all its scans (scan.go processSOS / refine as published).  coef: [*blocks][64] int16, blocks MCU by MCU
 * in the order of an interleaved scan (Y blocks of the MCU row by row, then Cb, then Cr), natural (row-major) order inside a
 * block, DC as it is.  *blocks, *w, *h, *ratio (image.YCbCrSubsampleRatio 0..5; -1: one component; -2: four) are set whenever the
 * frame parses; coef == NULL or cap_blocks < *blocks: nothing is decoded (FNX_OK / FNX_ERR_INVALID).  A baseline file:
 * FNX_ERR_UNSUPPORTED (its scan is decoded on the device).  Exists for the CPU-side parity tests and the sanitizer runs. */
int fnx_jpeg_progressive_coefficients(const uint8_t *data, size_t n, int16_t *coef, size_t cap_blocks, size_t *blocks, int *w, int *h,
                                      int *ratio);
/* CompressBatch's per-item body for a JPEG source in one call (batch.go:88-122 -> compress.go:21-87): decode `data`
 * on the device, run compressJPEGOptimal's quality search there and write the winner's file into `out` -- the file
 * bytes go up, the new file's bytes come down, no host codec.  Arguments as fnx_jpeg_compress; *w, *h: the image's
 * dimensions.  FNX_ERR_UNSUPPORTED as fnx_jpeg_decode. The file's Huffman tables follow fnx_ctx_set_jpeg_huffman. */
int fnx_jpeg_recompress(fnx_ctx *ctx, const uint8_t *data, size_t n, double target_ssim, const double *window /* 64 */, uint8_t *out,
                        size_t cap, size_t *nbytes, int *quality, double *ssim, int *steps /* may be NULL */, int *w, int *h);

/* ---- convert.go / exif.go --------------------------------------------- */
/* ApplyOrientation (exif.go:178-203 over convert.go:186-256).  orient 2..8;
 * dst is w x h for 2,3,4 and h x w for 5,6,7,8.  0, 1 and unknown values
 * return FNX_NOOP. */
int fnx_orient(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int orient,
               uint8_t *dst, int dstride);

/* ---- batched forms (FNX_DEVICE only) ------------------------------------ */
/* n independent images of identical geometry in ONE launch per stage
 * (CompressBatch items never interact, batch.go:88-122).  srcs/dsts/as/bs are
 * HOST arrays of n device pointers.  Image outputs are bit-identical to the per-image calls; SSIM
 * scalars may differ from them in the last bits (the window statistics are tiled differently when
 * there are many windows in flight) -- both stay within the 1e-9 bar and are run-to-run reproducible. */
int fnx_gaussian_blur_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w,
                            int h, const double *kernel, int radius, int flags,
                            uint8_t *const *dsts, int dstride);
int fnx_ssim_fast_batch(fnx_ctx *ctx, int n, const uint8_t *const *as, int astride,
                        const uint8_t *const *bs, int bstride, int w, int h,
                        const double *window, double *out /* n, host */);
/* The same split in two, so that one host thread can keep several contexts (= streams) busy, or keep
 * ONE stream from draining between batches: _enqueue only queues the kernels; the n results land in
 * pinned host memory and wait in the ctx's FIFO (up to 4 batches) until fnx_results_fetch takes the
 * OLDEST one (it waits for that batch only, not for work queued behind it).  Enqueueing batch s+1 before
 * fetching batch s is the intended use; the kernels of a ctx still run in order.  The blocking forms
 * require an empty FIFO. */
int fnx_ssim_fast_batch_enqueue(fnx_ctx *ctx, int n, const uint8_t *const *as, int astride,
                                const uint8_t *const *bs, int bstride, int w, int h,
                                const double *window);
int fnx_results_fetch(fnx_ctx *ctx, int n, double *out /* n, host */);
/* SSIM (ssim.go:24-43, equal dims) of ONE device-resident pair, enqueued like the batches above: the value joins the
 * ctx's FIFO and fnx_results_fetch(ctx, 1, &v) returns it later -- a worker that scores a stream of large images
 * (config 4: AdaptiveSharpen + SSIM per 8K image) keeps the next image's kernels queued while this one's result
 * crosses to the host instead of draining the stream at every call. */
int fnx_ssim_enqueue(fnx_ctx *ctx, const uint8_t *a, int astride, const uint8_t *b, int bstride, int w, int h,
                     const double *window /* 64 */);
/* SSIM of n device-resident pairs of ONE geometry: one launch of the window kernel with the image as a grid dimension,
 * one FIFO entry of n values (fnx_results_fetch(ctx, n, v)).  For frames smaller than 8K, where one pair does not fill the
 * machine (a 1080p pair is 500 waves).  Honours fnx_ctx_set_ssim_mode like fnx_ssim_enqueue. */
int fnx_ssim_batch_enqueue(fnx_ctx *ctx, int n, const uint8_t *const *as, int astride, const uint8_t *const *bs, int bstride,
                           int w, int h, const double *window /* 64 */);
/* MSSSIM (ssim.go:313-365, equal dims) of ONE device-resident pair, enqueued the same way: the per-level values wait in
 * the FIFO and fnx_results_fetch(ctx, 1, &v) combines them (exp of the weighted log sum, on the host as in fnx_msssim). */
int fnx_msssim_enqueue(fnx_ctx *ctx, const uint8_t *a, int astride, const uint8_t *b, int bstride, int w, int h,
                       const double *window /* 64 */);
/* n such pairs of ONE geometry as one FIFO entry: fnx_results_fetch(ctx, n, v) returns the n values in order (any k <= n of
 * them; the entry is consumed either way).  What a worker scoring a batch of frames calls instead of n enqueues: one FIFO
 * slot, one result event, and -- through fennec_MSSSIM_batch_enqueue -- ONE batched resize for the pairs whose dims differ. */
int fnx_msssim_batch_enqueue(fnx_ctx *ctx, int n, const uint8_t *const *as, int astride, const uint8_t *const *bs, int bstride,
                             int w, int h, const double *window /* 64 */);
/* compressJPEGOptimal (compress.go:21-87) of n device images of ONE geometry: item i is searched against target_ssim[i]
 * and its file goes to outs[i] (capacity caps[i], host memory).  Per item, (file bytes, *quality, *ssim, *steps) are
 * those fnx_jpeg_compress returns for the same image and target, byte for byte and bit for bit.  status[i]: FNX_OK, or
 * FNX_ERR_INVALID when caps[i] is too small -- nbytes[i] and quality[i] are then set, and fnx_jpeg_encode at quality[i]
 * gives the file without searching again.  Returns FNX_OK when the batch ran (per-item outcomes in status), an error
 * for bad arguments before anything is launched.  Blocking; like the other blocking forms, it needs an empty result FIFO.
 * Every item's Huffman tables follow fnx_ctx_set_jpeg_huffman (tables per image). */
int fnx_jpeg_compress_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h,
                            const double *target_ssim /* n */, const double *window /* 64 */,
                            uint8_t *const *outs, const size_t *caps, size_t *nbytes /* n */, int *quality /* n */,
                            double *ssim /* n */, int *steps /* n, may be NULL */, int *status /* n */);
/* image.Decode + toNRGBA of n JPEG files in host memory (the loadImage of CompressBatch's items, batch.go:88-122 ->
 * io.go:60-95) in one call: dsts[i] (DEVICE, stride dstrides[i]) and status[i] are what fnx_jpeg_decode(ctx, files[i], sizes[i],
 * FNX_DEVICE, dsts[i], dstrides[i], ..) gives, byte for byte, FNX_ERR_UNSUPPORTED / FNX_ERR_INVALID included (a refused file
 * leaves its destination untouched); ws[i] / hs[i] are set whenever the frame parses (else 0).  The files may differ in every
 * respect.  Baseline files share ONE set of launches per chunk of at most FNX_JPEG_DECODE_CHUNK files (fewer where their
 * scratch would pass 1 GiB): every synchronisation round, prefix sum, write pass and IDCT runs once for the chunk, and the
 * host waits once per pair of repair rounds and once for the chunk's verdicts -- where fnx_jpeg_decode waits at least twice
 * per file.  Files of the host route (progressive, SOF1, a component per scan, four components) follow one at a time.
 * dsts[i] == NULL or a stride fnx_jpeg_decode refuses: FNX_ERR_INVALID for that item only.  Returns FNX_OK when the batch ran,
 * an error for bad arguments (n outside 1..FNX_BATCH_MAX, a NULL array) before anything is launched.  Blocking; needs an empty
 * result FIFO.  The images are enqueued on the ctx's stream when it returns (as fnx_jpeg_decode with FNX_DEVICE). */
#define FNX_JPEG_DECODE_CHUNK 32   /* files per set of launches, at most */
int fnx_jpeg_decode_batch(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes, uint8_t *const *dsts,
                          const int *dstrides, int *ws /* n */, int *hs /* n */, int *status /* n */);
/* CompressBatch's item body (fnx_jpeg_recompress; batch.go:88-122 -> compress.go:21-87) for n JPEG files in host memory:
 * fnx_jpeg_decode_batch into images that stay on the device, then fnx_jpeg_compress_batch's search and files once per
 * geometry among them.  Per item, (file bytes, quality, ssim, steps, w, h) are fnx_jpeg_recompress's for the same file and
 * target.  status[i]: FNX_OK; the decoder's answer for a file it refused (nbytes[i] = 0); FNX_ERR_INVALID when caps[i] is too
 * small, with nbytes[i] and quality[i] set as in fnx_jpeg_compress_batch.  Return value as fnx_jpeg_decode_batch.
 * Every item's Huffman tables follow fnx_ctx_set_jpeg_huffman (tables per image). */
int fnx_jpeg_recompress_batch(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes,
                              const double *target_ssim /* n */, const double *window /* 64 */, uint8_t *const *outs,
                              const size_t *caps, size_t *nbytes /* n */, int *quality /* n */, double *ssim /* n */,
                              int *steps /* n, may be NULL */, int *ws /* n */, int *hs /* n */, int *status /* n */);

/* dsts[i] = GaussianBlur(srcs[i]) AND out[i] = SSIMFast(srcs[i], dsts[i]) -- the pair of calls
 * the reference makes whenever it scores a processed image against its source (effects.go:146
 * then ssim.go:48; the headline benchmark's step) -- with ONE pass over the pixels: the blur
 * kernel already holds every source and every blurred pixel, so it also accumulates the integer
 * channel sums of boxDownsample (ssim.go:244-309) for both, and SSIMFast never re-reads either
 * full-size image (HBM traffic 2*S instead of 4*S).  Results are identical to the two separate
 * calls: the box sums are integers, everything after them is the same code.  Shapes the one-pass
 * kernel is not built for or does not win on (radius > 24, no downsample, a box-downsample ratio below
 * 3.6 or boxes above 256 px: long side under ~1850 px or over 8192 px; with FNX_BLUR_EXACT also a kernel
 * with negative taps or gain > 1) run the two ops back to back.  With FNX_BLUR_EXACT the blurred images
 * are bit-exact and the scores are computed from exactly those images.  The _enqueue form pairs with fnx_results_fetch. */
/* The same for ONE image in either space: dst = GaussianBlur(src) and *ssim = SSIMFast(src, dst) -- bytes and score those of
 * fnx_gaussian_blur followed by fnx_ssim_fast.  With FNX_HOST the image crosses PCIe ONCE each way (source up, blurred
 * image down: 2 x 33 MB at 4K); the two separate calls upload the source twice and the blurred image once more
 * (4 x 33 MB), and PCIe is all a host-space call costs (0.6 ms per 33 MB against 40 us of kernels).  What the cgo
 * shim's GaussianBlurScored calls.  Blocking (the two kernels back to back on the ctx's stream; batches of device images
 * take fnx_gaussian_blur_ssim_fast_batch, whose one-pass kernel also halves the HBM traffic). */
int fnx_gaussian_blur_ssim_fast(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                                const double *kernel, int radius, int flags, uint8_t *dst, int dstride,
                                const double *window /* 64 */, double *ssim);
int fnx_gaussian_blur_ssim_fast_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride,
                                      int w, int h, const double *kernel, int radius, int flags,
                                      uint8_t *const *dsts, int dstride, const double *window,
                                      double *out /* n, host */);
int fnx_gaussian_blur_ssim_fast_batch_enqueue(fnx_ctx *ctx, int n, const uint8_t *const *srcs,
                                              int sstride, int w, int h, const double *kernel,
                                              int radius, int flags, uint8_t *const *dsts,
                                              int dstride, const double *window);

/* ---- Analyze (analyze.go:26-124), SURVEY 8(f) item 3 ---------------------- */
/* What the device computes: every statistic that needs the pixels.  The float
 * epilogue (computeEntropy, sqrt, the recommend* rules, analyze.go:87-230) is a
 * few hundred flops on these numbers and stays with the caller -- Go computes it
 * with its own math.Log2, fennec_Analyze below with libm. */
typedef struct fnx_analysis {
    uint64_t histogram[256]; /* luminance histogram, bin int(lum + 0.5), all pixels: exact */
    double bright_sum;       /* sum of luminance over all pixels (summation order differs from
                                the reference's serial loop: <= 1e-12 relative) */
    double variance_sum;     /* sum (lum - mean)^2 over the <=100x100 contrast grid (same remark) */
    int64_t sample_count;    /* points of that grid */
    int64_t edge_count;      /* Sobel magnitude > 30 on the sampled grid: exact */
    int64_t edge_total;
    int32_t unique_colors;   /* len(colorSet): distinct colours among every step-th pixel, capped 1024 */
    int32_t has_alpha;       /* some alpha < 255 */
    int32_t is_grayscale;    /* every pixel r == g == b */
    int32_t pad;
} fnx_analysis;
int fnx_analyze(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                fnx_analysis *out /* host */);
/* n same-sized device images (HOST array of device pointers), one launch per stage. */
int fnx_analyze_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int w, int h,
                      fnx_analysis *out /* n, host */);
/* isOpaque / isGrayscale (convert.go:66-84): both walk the FLAT Pix slice (pix_len bytes, row
 * padding included), one pass answers both. */
int fnx_scan_flags(fnx_ctx *ctx, int space, const uint8_t *pix, size_t pix_len, int *is_opaque,
                   int *is_grayscale);

/* ---- toNRGBARef of a decoded JPEG (convert.go:22-64), SURVEY 8(f) item 1 ------------------- */
/* Go's image/jpeg returns *image.YCbCr (or *image.Gray): the reference converts it with a
 * per-pixel At().RGBA() loop on the host (convertToNRGBA, convert.go:34-64) and SSIMFast then
 * uploads 4 bytes per pixel.  These take the decoder's planes as they are (Rect.Min == (0,0)):
 * Y: w x h, stride ystride; Cb, Cr: the subsampled planes of image.NewYCbCr, stride cstride;
 * ratio = image.YCbCrSubsampleRatio (0 4:4:4, 1 4:2:2, 2 4:2:0, 3 4:4:0, 4 4:1:1, 5 4:1:0);
 * cb == cr == NULL: image.Gray.  Arithmetic: image.YCbCr.COffset + color.YCbCr.RGBA() of the Go
 * standard library (go.mod:3 pins go 1.25.5), then convert.go:48-53's uint8(c >> 8) -- integer,
 * bit-exact against the restatement in oracle/ (which states its provenance). */
int fnx_ycbcr_to_nrgba(fnx_ctx *ctx, int space, const uint8_t *y, int ystride, const uint8_t *cb,
                       const uint8_t *cr, int cstride, int ratio, int w, int h, uint8_t *dst,
                       int dstride);
/* SSIMFast(prepared reference, toNRGBARef(decoded planes)) for the quality binary search
 * (compress.go:45-74): 1.5 bytes per pixel cross PCIe at 4:2:0 instead of 4. */
int fnx_ssim_fast_against_ycbcr(fnx_ctx *ctx, const fnx_prepared *ref, int space, const uint8_t *y,
                                int ystride, const uint8_t *cb, const uint8_t *cr, int cstride,
                                int ratio, const double *window, double *out);

/* ---- applyPalette + palettedToNRGBA (targetsize.go:488-546), SURVEY 8(f) item 4 ---------- */
/* Nearest palette entry per pixel by squared RGB distance, first minimum wins (targetsize.go:
 * 505-517); `indices` = image.Paletted.Pix (w x h bytes, stride istride), `quantized` =
 * palettedToNRGBA of it (NRGBA, alpha 255).  Either output may be NULL.  palette: ncolors x 4
 * HOST bytes r,g,b,a with a == 255 (what medianCut emits: fnx_median_cut below, or the
 * caller's own).  Integer arithmetic: bit-exact.  The route the call took -- "apply_palette_grid_kernel"
 * (images of 256 k pixels and more, or the form palette_grid = "1") or "apply_palette_kernel" -- is
 * fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) after the call; fnx_quantize's applyPalette step notes its route the
 * same way (it is the call's last note of that class when ssim == NULL). */
int fnx_apply_palette(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                      const uint8_t *palette, int ncolors, uint8_t *indices, int istride,
                      uint8_t *quantized, int qstride);

/* ---- medianCut (targetsize.go:352-486): the palettes of quantizeStrategy (targetsize.go:180-206) --------------------- */
/* The rule -- the arithmetic of targetsize.go:352-486 restated, with ONE tie order fixed:
 *   Samples (targetsize.go:426-441).  n = w*h in 64 bits; step = n / 100000 when n > 100000, else 1.  Sample j is the R, G, B of
 *     the flat 4-byte group at byte 4*j*step, for j*step < n; alpha is not looked at.  1 .. 199 999 samples (447 x 447: 199 809
 *     at step 1; 448 x 447: 100 128 at step 2).  The reference indexes the flat Pix slice (`off := i*4`, :437), not rows, so a
 *     padded image's samples would come out of its padding: this entry takes TIGHT images only, sstride != 4*w is
 *     FNX_ERR_INVALID.
 *   Boxes (targetsize.go:352-385, 447).  A box is a set of samples with its per-channel minima and maxima; the run starts with
 *     one box holding every sample.
 *   Split loop (targetsize.go:449-479), while there are fewer boxes than max_colors: among the boxes with two samples or more
 *     take the FIRST one of the largest score (rMax-rMin+1)*(gMax-gMin+1)*(bMax-bMin+1) * count (:452-461; 64 bits here: a
 *     64 x 64 noise image already scores 2^36); stop when no box has two samples (:462-464).  Axis (:387-398): R when rRange >=
 *     gRange and rRange >= bRange, else G when gRange >= bRange, else B.  Order the box by (value on the axis, sample number j)
 *     -- THIS IS THE LIBRARY'S TIE RULE: the reference's sort.Slice (:469-471) is pdqsort, which leaves tied samples in an
 *     order of its own, so ANY tie order is a reference answer (as with fnx_png_reduce's palette order) and this library fixes
 *     one; it makes every split a function of sets, so launch geometry cannot reach the bytes.  mid = count / 2 (:473): the
 *     first mid samples replace the box in place, the rest become a new box appended at the end (:474-478).  A box of
 *     identical samples still splits (volume 1, score = count).
 *   Palette (targetsize.go:400-414, 481-485).  Per box in list order (rSum / count, gSum / count, bSum / count, 255), truncating.
 *   Levels.  max_colors[0 .. nlevels) is strictly ascending, each in 1 .. 256.  The split sequence does not depend on max_colors,
 *     so medianCut(img, 16)'s boxes are medianCut(img, 256)'s after 15 splits: level l's palette is the box list when it first
 *     has max_colors[l] boxes, or the final list when the loop stopped earlier -- what medianCut(img, max_colors[l]) returns.
 *     ncolors[l] is that list's length; palettes + l*1024 holds its entries, the rest of the 256 zeroed.
 *   Empty image (targetsize.go:443-445).  w*h == 0: one entry (0,0,0,255) at every level, FNX_OK, no device work.
 * space FNX_DEVICE gathers the samples from the resident image on the device; FNX_HOST gathers them on the host and uploads
 * only them (<= 800 KB instead of the image); both return the same bytes.  FNX_ERR_INVALID before any device work: NULL ctx,
 * src (with w*h > 0), max_colors, palettes or ncolors; nlevels < 1; a level outside 1 .. 256 or a list that does not ascend;
 * sstride != 4*w; negative dims.  Kernel: csrc/median_cut.hip, one workgroup for the whole run (median_cut_kernel in
 * fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN); tools/median_cut_hostsim runs the same text on the CPU).  Integers: two calls
 * return identical bytes. */
int fnx_median_cut(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                   int nlevels, const int *max_colors,
                   uint8_t *palettes /* HOST, nlevels x 256 x 4 */, int *ncolors /* nlevels */);
/* One iteration of quantizeStrategy's loop (targetsize.go:183-205) without its PNG size test: fnx_median_cut at one level,
 * fnx_apply_palette with that palette into `indices` and / or `quantized` (either may be NULL), and -- ssim != NULL --
 * fnx_ssim_fast(src, quantized, window) (computeSSIMNRGBA at equal dims; the quantized image goes to scratch when the caller did
 * not ask for it).  The palette never leaves the device between the three; a host image crosses the link once; one wait at the
 * end.  Every output equals the three calls composed.  src is tight (sstride == 4*w) and w*h > 0. */
int fnx_quantize(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int max_colors,
                 uint8_t *palette /* HOST, 256 x 4 */, int *ncolors,
                 uint8_t *indices, int istride, uint8_t *quantized, int qstride,
                 const double *window, double *ssim);

/* ---- compressPNG's pixel stages (compress.go:90-153, convert.go:76-100) ------------------- */
/* What compressPNG decides and builds before png.Encoder sees a byte, for an NRGBA w x h image (w, h <= 65535):
 *   FNX_PNG_PALETTED  at most max_colors distinct (r,g,b,a) among the w visible pixels of the h rows (alpha is part of the
 *                     key, row padding is not visited: compress.go:116-128; the count is exact).  palette[0 .. *ncolors)
 *                     holds them, plane[y*pstride + x] the palette position of pixel (x, y) (compress.go:141-150).
 *   FNX_PNG_GRAY      else, when isGrayscale says so -- the flat walk of convert.go:76-84 over (h-1)*sstride + 4w bytes,
 *                     row padding INCLUDED, which must be readable: plane[y*pstride + x] = R(x, y), alpha dropped as
 *                     toGray drops it (convert.go:86-100).  An opaque grey image never gets here (at most 256 greys
 *                     always palettise); a translucent one with more than max_colors (v, a) pairs does -- the reference's
 *                     behaviour, kept.
 *   FNX_PNG_NRGBA     else: the image as it is; plane is not written.
 * Palette order: the reference builds its palette by ranging over a Go map (compress.go:134-138), an order the language
 * leaves random, so ANY order is a reference answer and parity is palette[plane] == source with a duplicate-free
 * palette.  This library fixes one: ascending row-major index of each colour's first occurrence (what an insertion-
 * ordered map would give) -- independent of launch geometry and timing, so two calls return identical bytes.
 * space: FNX_HOST, FNX_DEVICE, or FNX_DEVICE_SRC (device source, host plane).  *ncolors: the palette's length when
 * PALETTED, else 0.  plane == NULL: classify only (kind, palette, ncolors).  The encoder -- deflate, row filters -- stays
 * the caller's.  Kernels: csrc/png_reduce.hip (png_colors_kernel / png_plane_kernel in fnx_ctx_last_kernel(ctx,
 * FNX_PROF_MAIN)).  Integers: bit-exact. */
#define FNX_PNG_PALETTED 1   /* tryPalettize(img, max_colors) != nil     compress.go:92-96, 112-153 */
#define FNX_PNG_GRAY     2   /* else isGrayscale(img): toGray(img)       compress.go:98-103, convert.go:76-100 */
#define FNX_PNG_NRGBA    3   /* else the image as it is                  compress.go:105-107 */
int fnx_png_reduce(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int max_colors /* 1..256 */,
                   int *kind, uint8_t *palette /* HOST, 256 x 4: r,g,b,a */, int *ncolors,
                   uint8_t *plane /* w x h bytes, stride pstride >= w; may be NULL: classify only */, int pstride);

/* ---- the PNG encoder's per-row stage: pack, five filters, smallest sum (compress.go:94-107, targetsize.go:189, 342) ---- */
/* What png.Encoder{CompressionLevel: png.BestCompression} does to every row of the image it is handed, before zlib sees a
 * byte -- by compressPNG (compress.go:94-107), the quantize strategy (targetsize.go:189) and scaleSearch (targetsize.go:342).
 * Go's image/png/writer.go is not part of the reference tree, so the rule is restated here and parity with
 * Go is unpinned in the sense of DESIGN.md section 1; a numpy restatement of exactly this text is the tests' reference.
 *   kind, input                          colour type / depth   raw row of n bytes                              bpp
 *   FNX_PNG_NRGBA, every visible a==255  2 (RGB)  / 8          r,g,b per pixel, n = 3w                         3
 *   FNX_PNG_NRGBA otherwise              6 (RGBA) / 8          the 4w bytes as stored (non-premultiplied)      4
 *   FNX_PNG_GRAY (toGray's plane)        0        / 8          the w bytes                                     1
 *   FNX_PNG_PALETTED, ncolors > 16       3        / 8          the w bytes                                     -
 *   FNX_PNG_PALETTED, ncolors <= 16/4/2  3        / 4, 2, 1    indices packed MSB first, the last partial byte
 *                                                              shifted left to fill; n = ceil(w*depth / 8)     -
 * "Opaque" is image.NRGBA.Opaque(): the w visible pixels of the h rows; row padding is not looked at (unlike convert.go's
 * flat isOpaque).  opaque = 1 / 0 states it, -1 asks this call to decide that way first.
 * out: h rows of 1 + n bytes -- the filter type, then the filtered row -- exactly the stream zlib is fed.
 * Paletted rows always get type 0 and the raw bytes.  Otherwise, with cur the raw row, prev the RAW row above (zeros for
 * row 0), left[i] = cur[i-bpp] and ul[i] = prev[i-bpp] (both 0 for i < bpp), all arithmetic mod 256:
 *   0 None     cur[i]
 *   1 Sub      cur[i] - left[i]
 *   2 Up       cur[i] - prev[i]
 *   3 Average  cur[i] - ((left[i] + prev[i]) >> 1), the sum in at least 9 bits
 *   4 Paeth    cur[i] - paeth(left[i], prev[i], ul[i]);  p = a + b - c, pa = |p-a|, pb = |p-b|, pc = |p-c|:
 *              a if pa <= pb && pa <= pc, else b if pb <= pc, else c
 * The cost of a filter is the sum over the row of abs8(residual), abs8(d) = d < 128 ? d : 256 - d (abs8(128) = 128).  The
 * filters are tried in the order Up, Paeth, None, Sub, Average and a later one replaces the best only when its sum is
 * strictly smaller.  (Go leaves a filter's loop once its running sum reaches the best so far: that only abandons a filter
 * that can no longer win, full sums give the same choice.  Sums fit 32 bits: n <= 262 140, times 128.)
 * space: FNX_HOST, FNX_DEVICE, or FNX_DEVICE_SRC (device image, host stream: the product route).  src: the NRGBA image
 * (sstride >= 4w, a multiple of 4, the pointer 4-byte aligned in the device spaces) or the byte plane (sstride >= w, any
 * alignment).  w, h: 1..65535.  ncolors: 1..256 for FNX_PNG_PALETTED, ignored otherwise; opaque: ignored for planes.
 * *nbytes = h * (1 + n), *color_type and *bit_depth are set whenever the arguments are good; cap < *nbytes:
 * FNX_ERR_INVALID with the three set (call again), nothing written.  Bad arguments are refused before anything is
 * launched.  Integers: bit-exact, independent of launch geometry.  Deflate stays the caller's.  Kernels:
 * csrc/png_filter.hip (png_filter_kernel / png_pack_kernel in fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN)). */
int fnx_png_filter(fnx_ctx *ctx, int space, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors /* paletted: 1..256 */,
                   int opaque /* 1, 0, or -1: decide as Opaque() does */, uint8_t *out, size_t cap, size_t *nbytes,
                   int *color_type, int *bit_depth);

/* ---- deflate on the device: zlib streams and whole PNG files (RFC 1950 / 1951) ------------------------------- */
/* A chunk-parallel deflate (csrc/deflate.hip).  The input is cut into independent chunks of FNX_DEFLATE_CHUNK bytes, one
 * workgroup and ONE deflate block each (dynamic, fixed or stored, whichever is smallest); no match reaches behind its chunk's
 * start, and every chunk but the last ends with an empty stored block, so the chunks' outputs are whole bytes and are
 * concatenated behind the two zlib header bytes, the Adler-32 of the input behind them.  Inside a chunk every lane parses a
 * sub-chunk of FNX_DEFLATE_SUB bytes greedily: the candidates of a position are the distances 1, 2, 3, 4, 6, 8 and `row`
 * and one hash candidate, the longest match wins, the smaller distance on ties.  Every pick is deterministic: the bytes are
 * a function of (src, n, row) alone, never of the launch geometry or of timing.  Any inflate reads the stream back; it is
 * NOT the stream another encoder (zlib, Go's compress/flate) would write -- expect a size near zlib level 1 over the same
 * chunks (DESIGN.md section 5.7 has the measured figures). */
#define FNX_DEFLATE_CHUNK 32768   /* bytes per chunk = per workgroup = per deflate block */
#define FNX_DEFLATE_SUB   128     /* bytes per lane: tokens are cut at multiples of it */
/* The largest stream fnx_deflate returns for n bytes: every chunk stored (5 bytes of block header), every chunk's closing
 * empty stored block (5), header and Adler-32 (6).  Pure; no context.  Monotonic in n, at least n + 6. */
size_t fnx_deflate_bound(size_t n);
/* The zlib stream of src[0 .. n), n >= 1.  space: FNX_HOST (src and out in host memory), FNX_DEVICE (both device memory)
 * or FNX_DEVICE_SRC (device source, host stream).  row: the length of a row of the stream (1 + n of fnx_png_filter) as a
 * match-distance hint, 0 for none; values outside 1 .. FNX_DEFLATE_CHUNK - 1 are taken as none.  *nbytes is the stream's
 * size whenever the arguments are good; cap < *nbytes: FNX_ERR_INVALID with *nbytes set (call again; fnx_deflate_bound(n)
 * always suffices), nothing written.  Bytes of out behind *nbytes are never touched.  Bad arguments are refused before
 * anything is launched.  One host wait for the size (a second one behind the copy when the stream goes to host memory).
 * Kernels: deflate_chunk_kernel (the one fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) names), deflate_gather_kernel. */
int fnx_deflate(fnx_ctx *ctx, int space, const uint8_t *src, size_t n, int row, uint8_t *out, size_t cap, size_t *nbytes);
/* The deflate LEVEL of ONE ctx.  FNX_DEFLATE_LEVEL_FAST (default): the stream described above, byte for byte what the library
 * gave before the setting existed.  FNX_DEFLATE_LEVEL_DENSE: the same layout -- ceil(n / FNX_DEFLATE_CHUNK) data blocks, block c
 * yields exactly chunk c's bytes and starts on a byte, an empty stored block behind each but the last, BFINAL on the last, header
 * 78 01, the Adler-32 behind; each block the smallest of dynamic, fixed and stored; the same Huffman construction -- so
 * fnx_deflate_bound and fnx_png_file_bound hold unchanged.  What differs is the parse:
 *  - matches: 3 <= length <= 258, never past the chunk's end; distance <= min(p, 32768) with p the position in the STREAM: a
 *    match may reach into the previous chunk (an empty stored block does not reset inflate's window), never in front of the
 *    stream, never further than 32768.  A 3-byte match further than 4096 back is not taken.  No cut at multiples of
 *    FNX_DEFLATE_SUB.
 *  - candidates of a position: the distances 1, 2, 3, 4, 6, 8 and `row`, and up to FNX_DEFLATE_DENSE_DEPTH positions of its hash
 *    chain, nearest first.  The hash is ((b0 | b1 << 8 | b2 << 16) * 0x9e3779b1 mod 2^32) >> 20 of the position's three bytes.
 *    Chains are laid over the window -- the previous chunk from its first byte, then the own chunk: a position's link goes to
 *    the LARGEST EARLIER position of the window with its hash (none when that is further than 32768 back), so a chain visits,
 *    nearest first, every earlier position of the window that hashes alike, foreign three-byte words included.  (The kernel
 *    builds the links in segments of 256 positions -- against the earlier segments through a table, inside the segment by a
 *    search -- and the result does not depend on that.)  The longest
 *    match wins, the smaller distance on ties.  The set is a function of (src, n, row) alone.
 *  - parse: with (L, D) the best match of every position (L clipped to the chunk's end), from the chunk's first byte:
 *      at p: l = L[p];  l >= 3, p + 1 inside the chunk and L[p + 1] > l: the literal at p, go to p + 1;
 *            else l >= 3: the match (l, D[p]), go to p + l;   else: the literal, go to p + 1
 *    -- one step of lazy evaluation.  The tokens are those of this serial walk, however the kernel finds them.
 * Expect a size within a few per cent of zlib level 9 on photographic content (DESIGN.md section 5.12 has the measured
 * figures).  Followed by every entry that deflates on the device with this ctx: fnx_deflate, fnx_png_encode,
 * fennec_CompressFilePNG, fnx_png_compress_batch, fnx_png_recompress_batch -- the batch's files stay byte for byte the single
 * route's on the same ctx.  The fennec_CompressBatch* pools, the host's deflate and the Go shim are untouched.  After a dense
 * fnx_deflate fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) names deflate_dense_chunk_kernel; the batch's twin is
 * deflate_dense_chunk_batch_kernel.  ctx == NULL or any other level: FNX_ERR_INVALID, nothing changed. */
#define FNX_DEFLATE_LEVEL_FAST  0
#define FNX_DEFLATE_LEVEL_DENSE 1
#define FNX_DEFLATE_DENSE_DEPTH 32   /* the most chain candidates a position tries */
int fnx_ctx_set_deflate_level(fnx_ctx *ctx, int level);
/* fnx_png_filter's row stage and fnx_deflate in one call: the complete PNG file of a resident (or host) image, the filtered
 * stream never leaving the device.  kind, src, sstride, w, h, ncolors, opaque: as fnx_png_filter's; palette: HOST,
 * ncolors x 4 bytes r,g,b,a, for FNX_PNG_PALETTED (ignored otherwise).  space: FNX_HOST, FNX_DEVICE or FNX_DEVICE_SRC say
 * where src lives; out is ALWAYS host memory.  The file: signature, IHDR, for colour type 3 PLTE (3 bytes per entry) and
 * tRNS (the alphas up to and including the last entry whose alpha != 255; omitted when there is none), one IDAT holding the
 * zlib stream, IEND -- the chunk layout of the Python binding's png_file.  The chunk CRCs are computed on the host over
 * bytes that are there anyway -- on a ctx at FNX_PNG_CRC_DEVICE (fnx_ctx_set_png_crc) the IDAT chunk's alone comes from the
 * device, and fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) then names "deflate_chunk_kernel, crc32_pieces_kernel" (the dense
 * level: its chunk kernel).  *nbytes: the file's size; cap < *nbytes: FNX_ERR_INVALID with *nbytes set, nothing
 * written.  Decodes to the source's pixels; differs from the reference's file in the deflate bytes only. */
int fnx_png_encode(fnx_ctx *ctx, int space, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors /* paletted: 1..256 */,
                   int opaque /* 1, 0, or -1: decide as Opaque() does */, const uint8_t *palette, uint8_t *out, size_t cap, size_t *nbytes);
/* The size fnx_png_encode's file would have under this ctx's deflate level, same arguments, nothing but 8 bytes crossing
 * back: the row stage, then the chunk kernels' SIZE-ONLY forms -- the same parse and the same choice among dynamic, fixed
 * and stored, stopped where the block's bit count is known: no codes, no bits, no output slots, no gather, no file -- and
 * deflate_size_kernel, which adds the chunks' byte counts.  *nbytes == the *nbytes fnx_png_encode reports for the same
 * arguments on the same ctx, for every image.  palette: REQUIRED for FNX_PNG_PALETTED, as fnx_png_encode requires it (its
 * alphas decide the tRNS chunk's length; the colours are not read); ignored otherwise.  One host wait (a second one in front
 * of it when opaque == -1).  fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) names deflate_chunk_size_kernel, at
 * FNX_DEFLATE_LEVEL_DENSE deflate_dense_chunk_size_kernel. */
int fnx_png_encoded_size(fnx_ctx *ctx, int space, int kind, const uint8_t *src, int sstride, int w, int h, int ncolors /* paletted: 1..256 */,
                         int opaque /* 1, 0, or -1 */, const uint8_t *palette, size_t *nbytes);

/* ---- CRC-32 on the device (csrc/crc32.hip) ---------------------------------------------------------------------------- */
/* PNG's and zlib's CRC-32 (reflected polynomial 0xedb88320, register from all ones, inverted at the end).  The bytes are cut
 * into pieces of FNX_CRC_PIECE bytes, one workgroup each, a lane a contiguous run of FNX_CRC_RUN bytes (slice-by-4 from tables
 * in shared memory); the lanes' remainders are folded inside the workgroup, and a second kernel folds the pieces' words and
 * the seed into the answer -- a CRC is as combinable as deflate's Adler-32: with R(M) the register after M from 0,
 * R(A B) = R(A) x^(8 |B|) xor R(B) mod the polynomial.  No workgroup waits for another; the result is a function of the bytes.
 * DESIGN.md section 5.17. */
#define FNX_CRC_RUN   64      /* bytes per lane */
#define FNX_CRC_PIECE 16384   /* bytes per workgroup = 256 runs */
/* *out = zlib.crc32(src[0 .. n), crc): crc is the finished CRC of what came before, 0 for none.  space: FNX_HOST (src is
 * uploaded first) or FNX_DEVICE (resident bytes, any alignment).  n == 0: *out = crc, nothing launched.  Bad arguments are
 * refused before anything is launched.  One host wait.  Kernels: crc32_pieces_kernel (the one fnx_ctx_last_kernel(ctx,
 * FNX_PROF_MAIN) names), crc32_fold_kernel. */
int fnx_crc32(fnx_ctx *ctx, int space, const uint8_t *src, size_t n, uint32_t crc, uint32_t *out);
/* Where the IDAT chunk's CRC of the PNG files ONE ctx makes from a device deflate comes from.  FNX_PNG_CRC_HOST (default): the
 * host walks the chunk's bytes once they have come down, as before the setting existed.  FNX_PNG_CRC_DEVICE: the CRC kernels
 * above read the gathered zlib stream where deflate_gather_kernel / deflate_gather_batch_kernel left it (grid sized by
 * fnx_deflate_bound, the stream's length read on the device from the gather's size word, the batch's streams found by the
 * gather's size words; seed: the register after "IDAT"), and the CRC word comes down with a copy the route makes anyway -- the
 * size fetch of the single route, the sizes of the batch's second wait: no further host wait.  The files are byte for byte the
 * host mode's, at either deflate level.  Followed by every entry that makes a PNG file from a device deflate with this ctx:
 * fnx_png_encode, fennec_CompressFilePNG, fnx_hit_target_size's winner file, fennec_CompressFileHitTargetSize,
 * fnx_png_compress_batch, fnx_png_recompress_batch; their kernel list in fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) then also
 * names crc32_pieces_kernel (the batch: crc32_pieces_batch_kernel).  The small chunks (IHDR, PLTE, tRNS, IEND) keep the host's
 * CRC.  Routes whose deflate runs on the host ignore the setting: fennec_CompressFilePNGStream, the Python binding's
 * compress_png without device_deflate, the fennec_CompressBatch* pools, the Go shim.  ctx == NULL or any other mode:
 * FNX_ERR_INVALID, nothing changed. */
#define FNX_PNG_CRC_HOST   0
#define FNX_PNG_CRC_DEVICE 1
int fnx_ctx_set_png_crc(fnx_ctx *ctx, int mode);

/* ---- PNG sources: loadImage's image.Decode + toNRGBA for a .png (io.go:65-88 -> convert.go:12-64) --------------------- */
/* The zlib stream src[0 .. n) (RFC 1950: CM 8, CINFO <= 7, FCHECK; a preset dictionary is refused) of stored, fixed and dynamic
 * deflate blocks (RFC 1951) into out[0 .. cap).  Pure host code: no context, no device, no zlib.  Refused (FNX_ERR_INVALID):
 * a bad header, block type 3, LEN != ~NLEN, an over-subscribed code, an incomplete code (except, as zlib's and Go's
 * inflaters allow, a literal/length or distance code with no code at all or a single one-bit code), a bit pattern outside a
 * code, a distance that reaches before the start of the output, a stream that ends early, a wrong Adler-32 -- and a stream
 * of more than cap bytes: that one alone leaves *nbytes = cap + 1 (call again with more room; a deflate stream grows at most
 * 1032-fold, so 1032 * n always suffices), every other refusal *nbytes <= cap.  Bytes behind the Adler-32 are not looked at.
 * *nbytes: the output's size. */
int fnx_inflate(const uint8_t *src, size_t n, uint8_t *out, size_t cap, size_t *nbytes);
/* What a PNG file's signature and IHDR say (CRC checked): FNX_OK for every well-formed header -- also the interlaced and
 * oversized ones fnx_png_decode answers FNX_ERR_UNSUPPORTED to -- else FNX_ERR_INVALID.  Pure host code, no context. */
int fnx_png_info(const uint8_t *data, size_t n, int *w, int *h, int *color_type, int *bit_depth, int *interlace);
/* Adam7's pass geometry for a w x h image (1..65535 each) of one of the 15 colour type / bit depth pairs, else
 * FNX_ERR_INVALID.  Pass p = 1..7 starts at (x0, y0) and steps by (dx, dy) =
 *   (0,0,8,8)  (4,0,8,8)  (0,4,4,8)  (2,0,4,4)  (0,2,2,4)  (1,0,2,2)  (0,1,1,2)
 * pw[p-1] = ceil((w - x0) / dx), ph[p-1] = ceil((h - y0) / dy), 0 where that is not positive; a pass with pw == 0 or ph == 0 is
 * ABSENT: pw, ph and rowbytes are all 0 for it and it contributes no byte, not even filter bytes.  rowbytes = ceil(pw *
 * channels * depth / 8); *stream_bytes = the sum of ph * (1 + rowbytes) over the present passes, the size the inflated IDAT
 * stream must have.  Pure host code, no context. */
int fnx_png_adam7_passes(int w, int h, int color_type, int depth, int pw[7], int ph[7], size_t rowbytes[7], size_t *stream_bytes);
/* dst = toNRGBA(image.Decode(data)) for a PNG file, *w x *h.  The contract is fnx_jpeg_decode's: `data` is HOST memory, dst is
 * in `space` (FNX_HOST or FNX_DEVICE; a device dst is 4-byte aligned); dst == NULL: the dimensions only and whether the device
 * takes the file (host work: ctx may be NULL; `space` is checked there too).  Bad arguments and damaged files are refused
 * before anything is launched.
 * Go's image/png is not part of the reference tree, so the rule is restated here and parity with Go is unpinned in the sense
 * of DESIGN.md section 1; tests/png_decode_ref.py restates exactly this text.
 * Host (csrc/png_parse.cpp): the signature and every chunk's CRC-32; IHDR first (w, h >= 1, one of the 15 colour type / bit
 * depth pairs, compression 0, filter 0); PLTE once, before tRNS and IDAT, 1..256 entries (at most 2^depth for colour type 3,
 * none for types 0 and 4), mandatory for type 3; tRNS once, before IDAT, after PLTE: <= 256 alphas for type 3, one 16-bit sample for
 * type 0, three for type 2, illegal for 4 and 6; consecutive IDATs concatenated; IEND ends the file; every other chunk is
 * skipped after its CRC.  A violation is FNX_ERR_INVALID.  The IDAT stream goes through fnx_inflate's code and must yield
 * exactly h * (1 + rowbytes) bytes, rowbytes = ceil(w * channels * depth / 8); each row's first byte is its filter type, above
 * 4: FNX_ERR_INVALID.  FNX_ERR_UNSUPPORTED (decode it on the host): Adam7-interlaced files (unless the ctx accepts them, below),
 * w or h above 65535.
 * Reconstruction (png_unfilter_kernel), the inverse of fnx_png_filter's table: with bpp = max(1, channels * depth / 8),
 * a = the reconstructed byte bpp to the left (0 for i < bpp), b = the byte above (0 for row 0), c = the byte above-left (0
 * for i < bpp or row 0), f the stream's byte, mod 256:
 *   0 None f    1 Sub f + a    2 Up f + b    3 Average f + ((a + b) >> 1), the sum in 9 bits    4 Paeth f + paeth(a, b, c),
 *   p = a + b - c, pa = |p-a|, pb = |p-b|, pc = |p-c|: a if pa <= pb && pa <= pc, else b if pb <= pc, else c.
 * Rows of type None and Sub, and row 0, do not read the row above: they cut the image into independent chain segments.  A
 * workgroup keeps FNX_PNG_DECODE_ROWS rows of a chain in flight, one lane a row, each one pixel behind the row above, and
 * marches a longer chain band by band itself; no workgroup waits for another.  Bit-exact, independent of launch geometry.
 * Pixels (png_expand_kernel).  Samples of depth 1, 2, 4 are unpacked MSB first, grey values scaled by 0xff, 0x55, 0x11; 16-bit
 * samples are big-endian.  A tRNS match compares, at depth <= 8, the raw sample(s) with the LOW BYTE of the tRNS sample(s), at
 * depth 16 the full samples.
 *   source                                Go's type            toNRGBA's pixel
 *   type 6 / 8                            *image.NRGBA         the stored bytes (convert.go:13-17 copies)
 *   type 4 / 8                            *image.NRGBA         (y, y, y, a)
 *   type 0, depth <= 8, tRNS              *image.NRGBA         (y, y, y, 0) for a match, else (y, y, y, 255): the colour is KEPT
 *   type 2 / 8, tRNS                      *image.NRGBA         (r, g, b, 0) for a match, else (r, g, b, 255): the colour is KEPT
 *   type 0, depth <= 8                    *image.Gray          (y, y, y, 255)
 *   type 2 / 8                            *image.RGBA          (r, g, b, 255)
 *   type 0 / 16                           *image.Gray16        (hi, hi, hi, 255), hi = the sample's high byte
 *   type 2 / 16                           *image.RGBA64        the high bytes, 255
 *   types 0 / 16 and 2 / 16 with tRNS (A = 0 for a match, else 0xffff), 4 / 16, 6 / 16: *image.NRGBA64 through convertToNRGBA
 *     (convert.go:34-64), in exact uint32 on the 16-bit R, G, B, A: A == 0 -> (0, 0, 0, 0), the colour ZEROED; A == 0xffff ->
 *     (R >> 8, G >> 8, B >> 8, 255); else r' = R * A / 0xffff and the pixel is ((r' * 0xffff / A) >> 8, ..., A >> 8)
 *   type 3                                *image.Paletted      entry i is (r, g, b, t), t = tRNS[i] or 255, as a color.NRGBA; with
 *     A16 = t * 0x101: t == 255 -> (r, g, b, 255); t == 0 -> (0, 0, 0, 0); else r' = (r * 0x101) * t / 0xff and the pixel is
 *     ((r' * 0xffff / A16) >> 8, ..., t) -- lossy on purpose, it is the reference's round trip.  An index behind the palette's
 *     end reads as opaque black (under tRNS[i] where tRNS is longer than PLTE).  The 256 pixel values are made on the host.
 * Adam7 (interlace method 1), on a ctx after fnx_ctx_set_png_adam7(ctx, 1); restated like the rest.  The inflated IDAT stream
 * is the PRESENT passes back to back in pass order (fnx_png_adam7_passes: geometry, and which passes are present).  Each pass
 * is an image of pw x ph pixels with its own packed rows -- samples of depth 1, 2, 4 are packed per PASS row, MSB first -- and
 * each pass row carries its own filter byte; the row above a pass's first row is all zeros, bpp is the file's.  The stream
 * must hold exactly stream_bytes: fewer or more is FNX_ERR_INVALID, and so is a filter type above 4 in any pass, refused before
 * anything is launched.  Pass pixel (i, j) is image pixel (x0 + i * dx, y0 + j * dy).  The pixel model -- tRNS, 16-bit samples,
 * the palette's table, indices behind the palette's end -- is the non-interlaced one, and Go returns the same image type, so
 * the table above applies unchanged.  On the device the passes are seven small images of one bpp: ONE launch of
 * png_unfilter_batch_kernel reconstructs all of them (a pass's row 0 starts a chain, no unit spans two passes) into a plane
 * per pass, and png_expand_adam7_kernel writes the image, a thread per OUTPUT pixel that finds its pass from (x & 7, y & 7).
 * Inflate is one serial bit stream and stays on the host; the stream goes up as it is, 1/8 to 8 bytes a pixel.
 * Kernels: csrc/png_decode.hip; fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) answers "png_unfilter_kernel, png_expand_kernel", for
 * an Adam7 file "png_unfilter_batch_kernel, png_expand_adam7_kernel". */
#define FNX_PNG_DECODE_ROWS 1024   /* rows a workgroup of png_unfilter_kernel keeps in flight */
int fnx_png_decode(fnx_ctx *ctx, const uint8_t *data, size_t n, int space, uint8_t *dst, int dstride, int *w, int *h);
/* image.Decode + toNRGBA of n PNG files in host memory (the loadImage of CompressBatch's items, batch.go:88-122 ->
 * io.go:65-88 -> convert.go:12-64) in one call.  The contract is fnx_jpeg_decode_batch's: files[i] is HOST memory, dsts[i]
 * DEVICE memory (4-byte aligned, stride dstrides[i]); dsts[i] and status[i] are what fnx_png_decode(ctx, files[i], sizes[i],
 * FNX_DEVICE, dsts[i], dstrides[i], ..) gives, byte for byte, FNX_ERR_INVALID (a damaged file) and FNX_ERR_UNSUPPORTED (Adam7,
 * a dimension above 65535) included; a refused item leaves its destination untouched.  ws[i] / hs[i] are set whenever the
 * IHDR parses -- also for the unsupported files, as fnx_png_info would -- else 0.  files[i] == NULL, dsts[i] == NULL, or a
 * stride or alignment fnx_png_decode refuses: FNX_ERR_INVALID for that item only.  The files may differ in every respect
 * (size, colour type, depth, number of chains).
 * A chunk is at most FNX_PNG_DECODE_CHUNK files, fewer where their inflated streams and reconstructed planes would pass
 * FNX_PNG_DECODE_CHUNK_BYTES of device scratch (a file that alone needs more is a chunk of its own).  Per chunk, the host
 * side of fnx_png_decode -- chunk walk, inflate, row plan, palette table -- runs on `workers` host threads, handed out file
 * by file; the threads make no HIP call.  workers == 1: the calling thread alone, no thread is started; more: the calling
 * thread is one of them; 0: min(8, files in the chunk).  Then the chunk's streams go up from a pinned staging area and ALL
 * its chains go through one set of launches: png_unfilter_batch_kernel once per pixel size (bpp) present, one workgroup per
 * unit of any file, and png_expand_batch_kernel once -- where a loop of fnx_png_decode runs a single-chain file on one compute
 * unit, n times in a row.  The staging area is written again only after an event behind the chunk's uploads; the device is
 * never synchronised as a whole.
 * Neither the bytes, nor the statuses, nor fnx_last_error's text -- the message of the LOWEST-indexed refused item -- depend
 * on `workers` or on which thread finished first.  Returns FNX_OK when the batch ran; an error for bad arguments (n outside
 * 1..FNX_BATCH_MAX, a NULL array, workers outside 0..64) before anything is launched or any thread is started.  When it
 * returns, the images are enqueued on the ctx's stream (as fnx_png_decode with FNX_DEVICE).
 * On a ctx that accepts Adam7 files (fnx_ctx_set_png_adam7) they take part like the others: their passes' units join the
 * unfilter launch of their bpp, and png_expand_adam7_batch_kernel runs once over the chunk's Adam7 files; a chunk without one
 * runs the launches above and nothing else.
 * fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) answers "png_unfilter_batch_kernel, png_expand_batch_kernel", with
 * ", png_expand_adam7_batch_kernel" behind it for a chunk that holds Adam7 files. */
#define FNX_PNG_DECODE_CHUNK 32   /* files per set of launches, at most */
#define FNX_PNG_DECODE_CHUNK_BYTES ((size_t)1 << 30)   /* device scratch of a chunk's streams + planes, at most (as the JPEG batch's) */
int fnx_png_decode_batch(fnx_ctx *ctx, int n, const uint8_t *const *files, const size_t *sizes, uint8_t *const *dsts,
                         const int *dstrides, int workers, int *ws /* n */, int *hs /* n */, int *status /* n */);

/* ---- compressPNG for a list of images or files in one call (compress.go:90-153 per item of batch.go:88-122) -------------- */
/* The largest file fnx_png_encode, fnx_png_compress_batch and fnx_png_recompress_batch can return for a w x h image, whatever
 * it holds: the signature, IHDR, IDAT's and IEND's twelve bytes each, and the larger of an RGBA stream's bound
 * (fnx_deflate_bound(h * (4w + 1))) and a paletted image's layout -- a PLTE of 256 entries, a tRNS of 256 alphas,
 * fnx_deflate_bound(h * (w + 1)).  Pure; no context.  Monotonic in w and in h; 0 for a dimension outside 1..65535. */
size_t fnx_png_file_bound(int w, int h);
/* compressPNG (compress.go:90-108) of n resident images in one call.  srcs[i]: DEVICE memory, NRGBA, 4-byte aligned, stride
 * sstrides[i] >= 4 ws[i] and a multiple of 4, the flat Pix -- (h - 1) stride + 4w bytes -- readable; the images may differ in
 * every respect (size, stride, content).  outs[i]: HOST memory of caps[i] bytes.  Item i's file is the one
 * fnx_png_reduce(max_colors 256) followed by fnx_png_encode(kind, the image or its plane, ncolors, opaque = -1, palette)
 * returns for the same image, BYTE FOR BYTE, and kinds[i] is that kind (FNX_PNG_PALETTED, FNX_PNG_GRAY or FNX_PNG_NRGBA);
 * nbytes[i] its size.  Every stage is a function of the image alone -- the palette in first-occurrence order, the bit-exact row
 * stage, a deflate whose bytes depend on (src, n, row) only --, so neither the batch, nor an image's place in it, nor the
 * launch geometry shows in a file.
 * Refused, that item alone, outs[i] untouched, status[i] = FNX_ERR_INVALID: srcs[i] NULL; outs[i] NULL with a cap that is not
 * 0; ws[i] or hs[i] outside 1..65535; a stride below 4w or not a multiple of 4; a pointer that is not 4-byte aligned
 * (nbytes[i] = kinds[i] = 0 for these); caps[i] below the file's size (nbytes[i] and kinds[i] set: call again;
 * fnx_png_file_bound(w, h) always suffices).  fnx_last_error has the message of the lowest-indexed refused item.
 * The list is cut into chunks of at most FNX_PNG_COMPRESS_CHUNK images and FNX_PNG_COMPRESS_CHUNK_BYTES of device scratch --
 * counted for the worst case (RGBA rows: planes, streams, deflate's token words, slots, bounds: about 200 MB for a 4K image)
 * from the DIMENSIONS alone, before anything is classified, so the cut never depends on content; an image that alone passes
 * the byte cap is a chunk of its own.  Per chunk ONE set of launches with a workgroup per unit of any image --
 * png_colors_batch_kernel, png_finish_batch_kernel (the colour sets, an "over" word per image), png_flags_batch_kernel
 * (image.NRGBA.Opaque over the visible pixels; isGrayscale's flat walk, row padding included), png_plane_batch_kernel,
 * png_filter_batch_kernel / png_pack_batch_kernel once per row form present, deflate_chunk_batch_kernel,
 * deflate_gather_batch_kernel -- and THREE host waits whatever the number of images: the classification words, the streams'
 * sizes, the streams' own bytes (back to back at their true sizes, one copy); one more where the ctx's pinned ring, which
 * the fetches and the table uploads use, grows or wraps.  The chunks of the file and their CRCs are made
 * on the host, as fnx_png_encode's.  Blocking.  Returns FNX_OK when the batch ran; an error for n outside 1..FNX_BATCH_MAX or a
 * NULL array before anything is launched (and before the ctx is looked at).
 * fnx_ctx_last_kernel(ctx, FNX_PROF_MAIN) names the batch kernels after a call that ran a chunk. */
#define FNX_PNG_COMPRESS_CHUNK 32                       /* images per set of launches, at most */
#define FNX_PNG_COMPRESS_CHUNK_BYTES ((size_t)1 << 30)  /* device scratch of a chunk, at most */
int fnx_png_compress_batch(fnx_ctx *ctx, int n, const uint8_t *const *srcs /* DEVICE, NRGBA */, const int *sstrides, const int *ws,
                           const int *hs, uint8_t *const *outs /* HOST */, const size_t *caps, size_t *nbytes /* n */, int *kinds /* n */,
                           int *status /* n */);
/* CompressBatch's item body (batch.go:88-122) for n files in host memory that end as PNG: loadImage (io.go:65-88) and
 * compressPNG.  A file that opens with the eight PNG signature bytes is decoded by fnx_png_decode_batch's chunk path (`workers`
 * as there), every other file by fnx_jpeg_decode_batch's -- the sniff fennec_CompressFilePNG makes --, into images that stay
 * on the device; then the compress batch above.  Per item the file's bytes, kinds[i], ws[i] and hs[i] equal decoding files[i]
 * with fnx_png_decode / fnx_jpeg_decode and compressing the image with fnx_png_reduce + fnx_png_encode.  status[i] is the
 * decoder's answer for a file it refused (nbytes[i] = 0; Adam7 stays FNX_ERR_UNSUPPORTED), FNX_ERR_OOM for a file whose image
 * alone the device has no room for, else as above.  Nothing depends on
 * `workers` or on thread timing.  No options (orientation, resize): those are fennec_CompressFilePNG's.  Returns FNX_OK when
 * the batch ran; an error for n outside 1..FNX_BATCH_MAX, a NULL array or workers outside 0..64 before anything else. */
int fnx_png_recompress_batch(fnx_ctx *ctx, int n, const uint8_t *const *files /* HOST */, const size_t *sizes, int workers,
                             uint8_t *const *outs /* HOST */, const size_t *caps, size_t *nbytes /* n */, int *kinds /* n */,
                             int *ws /* n */, int *hs /* n */, int *status /* n */);

/* ======================================================================= */
/* fennec_* : the reference's function set (names and argument meaning as in
 * the Go source), mirrored above fnx_*.                                     */
/* ======================================================================= */

/* ImageStats (analyze.go:9-22); Format: 1 JPEG, 2 PNG (types.go:35-42); Quality: 0 Balanced,
 * 3 High, 4 Aggressive (types.go:59-72). */
typedef struct fennec_ImageStats {
    int32_t Width, Height;
    int32_t HasAlpha, IsGrayscale, UniqueColors;
    int32_t RecommendedFormat, RecommendedQuality, pad;
    double Entropy, EdgeDensity, MeanBrightness, Contrast, EstimatedCompression;
} fennec_ImageStats;
/* Analyze (analyze.go:26-124). */
int fennec_Analyze(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                   fennec_ImageStats *out);
/* The float epilogue alone: computeEntropy, contrast, edge density, recommendFormat,
 * recommendQuality, estimateCompression (analyze.go:87-230) from the device's numbers. */
void fennec_statsFromAnalysis(const fnx_analysis *a, int w, int h, fennec_ImageStats *out);
/* isOpaque / isGrayscale (convert.go:66-84) of an image (flat Pix: (h-1)*stride + 4*w bytes). */
int fennec_isOpaque(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int *out);
int fennec_isGrayscale(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h, int *out);

/* gaussianKernel(size, sigma) (ssim.go:223-241): size*size doubles. */
void fennec_gaussianKernel(int size, double sigma, double *kernel);
/* GaussianBlur's radius/kernel (effects.go:153-165); kernel may be NULL. */
int fennec_blurKernel(double sigma, double *kernel);
/* lanczosKernel (resize.go:57-69). */
double fennec_lanczosKernel(double x);
/* precomputeWeights (resize.go:164-197) with ratio/support derived as
 * resizeH/resizeV do; returns the tap count; index/weight may be NULL to size. */
int fennec_precomputeWeights(int dstSize, int srcSize, int32_t *offset, int32_t *index,
                             double *weight);
/* smartResize's dims (resize.go:12-32): returns 0 if the image already fits (negative: a NULL out pointer). */
int fennec_smartResizeDims(int srcW, int srcH, int maxW, int maxH, int *dstW, int *dstH);
/* SSIMFast's downsample dims (ssim.go:52-56): returns 1 if it downsamples (negative: a NULL out pointer). */
int fennec_ssimFastDims(int w, int h, int *newW, int *newH);

int fennec_SSIM(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah,
                const uint8_t *b, int bstride, int bw, int bh, double *out);     /* ssim.go:24 */
int fennec_SSIMFast(fnx_ctx *ctx, int space, const uint8_t *a, int astride, const uint8_t *b,
                    int bstride, int w, int h, double *out);                      /* ssim.go:48 */
int fennec_MSSSIM(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah,
                  const uint8_t *b, int bstride, int bw, int bh, double *out);   /* ssim.go:313 */
/* computeSSIMNRGBA (targetsize.go:563-568): fnx_ssim_fast_resized with precomputeWeights' tables and the 8 x 8 window. */
int fennec_computeSSIMNRGBA(fnx_ctx *ctx, int space, const uint8_t *a, int astride, int aw, int ah,
                            const uint8_t *b, int bstride, int bw, int bh, double *out);
/* MSSSIM of a device-resident pair through the ctx's result FIFO (fnx_msssim_enqueue), img2 resized to img1's
 * dims first when they differ (ssim.go:320-322); fnx_results_fetch(ctx, 1, &v) returns the value. */
int fennec_MSSSIM_enqueue(fnx_ctx *ctx, const uint8_t *a, int astride, int aw, int ah, const uint8_t *b, int bstride,
                          int bw, int bh);
/* ... of n device pairs (every a of aw x ah, every b of bw x bh): the b's are resized to the a's dims by ONE batched
 * lanczosResize (fnx_lanczos_resize_batch) when the dims differ, ssim.go:320-322; results as fnx_msssim_batch_enqueue's. */
int fennec_MSSSIM_batch_enqueue(fnx_ctx *ctx, int n, const uint8_t *const *as, int astride, int aw, int ah,
                                const uint8_t *const *bs, int bstride, int bw, int bh);
int fennec_GaussianBlur(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                        double sigma, uint8_t *dst, int dstride);                 /* effects.go:146;
                        FNX_HOST: FNX_BLUR_EXACT (bit-exact; the call is PCIe-bound anyway),
                        FNX_DEVICE: FNX_BLUR_FAST */
int fennec_Sharpen(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                   double strength, uint8_t *dst, int dstride);                   /* effects.go:10 */
int fennec_AdaptiveSharpen(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w, int h,
                           double strength, uint8_t *dst, int dstride);           /* effects.go:49 */
int fennec_ApplyOrientation(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int w,
                            int h, int orient, uint8_t *dst, int dstride);        /* exif.go:178 */
int fennec_lanczosResize(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW,
                         int srcH, uint8_t *dst, int dstride, int dstW, int dstH); /* resize.go:37 */
int fennec_lanczosResizeBatch(fnx_ctx *ctx, int n, const uint8_t *const *srcs, int sstride, int srcW, int srcH,
                              uint8_t *const *dsts, int dstride, int dstW, int dstH);   /* resize.go:37 x n (device images) */
int fennec_boxDownsample(fnx_ctx *ctx, int space, const uint8_t *src, int sstride, int srcW,
                         int srcH, uint8_t *dst, int dstride, int dstW, int dstH); /* ssim.go:244 */

/* CompressBatch (batch.go:58-128) over decoded NRGBA items with compressJPEGOptimal (compress.go:21-87) as the per-item
 * work, all of it on the device (fnx_jpeg_compress): `workers` threads, ONE closed queue of indices (an atomic counter:
 * the channel of batch.go:72-81), one fnx_ctx per worker on `device`, results stored by index, `on_item(completed,
 * total, user)` serialised as OnItem is, `*cancel != 0` checked before each item (ctx.Done(), batch.go:90-99).  Item i's
 * file goes to outs[i] (capacity caps[i]); a result with failed != 0 carries the FNX_* status in `status`.
 * Returns FNX_OK when the pool ran (per-item failures are in the results), an error when no worker could start. */
typedef struct fennec_BatchResult {
    int32_t index, failed, has_result, quality, steps, status;
    int64_t original_size, compressed_size;
    double ssim;
    int32_t device;      /* index (in this library's device list) of the device whose worker took the item; -1: nobody did */
    int32_t reserved;
} fennec_BatchResult;
typedef void (*fennec_on_item)(int completed, int total, void *user);
int fennec_CompressBatchNRGBA(int device, int workers, int n, int space, const uint8_t *const *srcs, const int *strides,
                              const int *widths, const int *heights, const int64_t *original_sizes, double target_ssim,
                              uint8_t *const *outs, const size_t *caps, fennec_BatchResult *results,
                              const volatile int *cancel /* may be NULL */, fennec_on_item on_item /* may be NULL */, void *user);
/* The same pool over the NODE's devices (batch.go:63-126 with g GPUs): `workers` threads (0: NumCPU, capped at
 * n), worker i bound to a context on devices[i mod ndev], ONE queue of indices for all of them, results by index with the
 * device that served each item.  A device may be listed more than once (more workers' contexts on it).  Device-resident
 * items (space FNX_DEVICE) live on one device, so a list of several distinct devices takes host-space items only. */
int fennec_CompressBatchNRGBADevices(const int *devices, int ndev, int workers, int n, int space, const uint8_t *const *srcs,
                                     const int *strides, const int *widths, const int *heights, const int64_t *original_sizes,
                                     double target_ssim, uint8_t *const *outs, const size_t *caps, fennec_BatchResult *results,
                                     const volatile int *cancel /* may be NULL */, fennec_on_item on_item /* may be NULL */, void *user);
/* CompressFile for a JPEG or PNG source in standard mode (fennec.go:30-76 -> compressImageInternal :107-141 -> handleStandardMode
 * :162-205) from the file's bytes with every pixel stage on the device: image.Decode + toNRGBA (a file that opens with the
 * eight PNG signature bytes goes to fnx_png_decode, every other one to fnx_jpeg_decode; the same holds for the three
 * fennec_CompressFilePNG* entries below and for the items of fennec_CompressBatchJPEGOpts),
 * ApplyOrientation when opts->orient is 2..8 (Options.AutoOrient; the caller reads the tag as exif.go does),
 * smartResize when max_w or max_h > 0 (Options.MaxWidth / MaxHeight), analyzeFormat when auto_format (Format: Auto),
 * compressJPEGOptimal at target_ssim.  dims = {OriginalDimensions (after orientation), FinalDimensions}.
 * FNX_NOOP: analyzeFormat chose PNG (a translucent sampled pixel, which only a PNG source can have, or fewer than 256 sampled
 * colours) -- the caller's compressPNG takes the item, dims are set.  FNX_ERR_UNSUPPORTED as fnx_jpeg_decode / fnx_png_decode.  Target-size mode
 * (Options.TargetSize) has a file entry of its own, fennec_CompressFileTargetSize below, and its pool,
 * fennec_CompressBatchTargetSize. */
typedef struct fennec_FileOptions {
    int32_t orient;      /* EXIF orientation 1..8; <= 1: none */
    int32_t max_w, max_h;
    int32_t auto_format; /* != 0: Format Auto */
    double target_ssim;  /* Options.Quality.targetSSIM() or Options.TargetSSIM */
} fennec_FileOptions;
/* (The file's Huffman tables follow fnx_ctx_set_jpeg_huffman.) */
int fennec_CompressFileJPEG(fnx_ctx *ctx, const uint8_t *data, size_t n, const fennec_FileOptions *opts, uint8_t *out, size_t cap,
                            size_t *nbytes, int *quality, double *ssim, int *steps /* may be NULL */, int dims[4]);
/* CompressFile's PNG branch for a JPEG source, up to the encoder (fennec.go:107-141 -> compressPNG, compress.go:90-153 with
 * convert.go:76-100): decode, ApplyOrientation and smartResize staged exactly as fennec_CompressFileJPEG stages them, then
 * fnx_png_reduce (max_colors 256) on the resident image -- for the item that came back FNX_NOOP there, or under Format:
 * PNG, without a second decode on the host.  opts->target_ssim and opts->auto_format are ignored: the caller has decided.
 * out: the tight reduced image the caller hands to png.Encoder -- w*h bytes (image.Paletted.Pix with `palette` in this
 * library's first-occurrence order, or image.Gray.Pix) or w*h*4 NRGBA bytes; *nbytes its size; dims as
 * fennec_CompressFileJPEG's.  cap too small: FNX_ERR_INVALID with *nbytes, *kind, *ncolors and dims set (call again).
 * FNX_ERR_UNSUPPORTED as fnx_jpeg_decode. */
int fennec_CompressFilePNGReduce(fnx_ctx *ctx, const uint8_t *data, size_t n, const fennec_FileOptions *opts,
                                 int *kind, uint8_t *palette /* 256 x 4 */, int *ncolors,
                                 uint8_t *out, size_t cap, size_t *nbytes, int dims[4]);
/* CompressFile's PNG branch for a JPEG source up to the bytes deflate reads (fennec.go:107-141 -> compressPNG,
 * compress.go:90-153 with convert.go:76-100, then the encoder's row stage, compress.go:94-107): fennec_CompressFilePNGReduce's
 * stages, then fnx_png_filter (opacity decided as Opaque() does) on the resident reduced image.  out: the h rows of 1 + n bytes
 * zlib is fed; *nbytes their size; *kind, palette, *ncolors as fennec_CompressFilePNGReduce's; *color_type, *bit_depth for
 * IHDR; dims as fennec_CompressFileJPEG's (dims[2], dims[3]: the PNG's width and height).  What is left to the caller:
 * zlib at BestCompression and the chunks (IHDR, PLTE from `palette`, tRNS from its alphas, IDAT, IEND).  cap too small:
 * FNX_ERR_INVALID with every result but the stream set (call again).  FNX_ERR_UNSUPPORTED as fnx_jpeg_decode. */
int fennec_CompressFilePNGStream(fnx_ctx *ctx, const uint8_t *data, size_t n, const fennec_FileOptions *opts,
                                 int *kind, uint8_t *palette /* 256 x 4 */, int *ncolors, int *color_type, int *bit_depth,
                                 uint8_t *out, size_t cap, size_t *nbytes, int dims[4]);

/* CompressFile's PNG branch for a JPEG source, whole: fennec_CompressFilePNGStream's stages (decode, ApplyOrientation,
 * smartResize, compressPNG's reduction, the encoder's row stage, compress.go:94-107), then fnx_deflate on the resident stream
 * and the file's chunks as fnx_png_encode writes them -- JPEG bytes in, PNG bytes out, no pixel and no scanline on the host.
 * out: HOST; *nbytes the file's size (cap too small: FNX_ERR_INVALID with *nbytes set); dims as fennec_CompressFileJPEG's;
 * *kind as fennec_CompressFilePNGReduce's.  Opt-in: the file is larger than png.BestCompression's. */
int fennec_CompressFilePNG(fnx_ctx *ctx, const uint8_t *data, size_t n, const fennec_FileOptions *opts,
                           uint8_t *out, size_t cap, size_t *nbytes, int dims[4], int *kind);
/* The same pool over JPEG FILES in host memory (what CompressBatch reads for a .jpg item, batch.go:88-101): per item
 * fnx_jpeg_recompress -- decoder, search and encoder on the device, no host codec.  A file the device decoder does not
 * take comes back with failed != 0 and status == FNX_ERR_UNSUPPORTED: the caller decodes it on the host and sends it
 * through fennec_CompressBatchNRGBA.  original_size = sizes[i]. */
int fennec_CompressBatchJPEG(int device, int workers, int n, const uint8_t *const *files, const size_t *sizes, double target_ssim,
                             uint8_t *const *outs, const size_t *caps, fennec_BatchResult *results,
                             const volatile int *cancel /* may be NULL */, fennec_on_item on_item /* may be NULL */, void *user);
/* ... over a device list, as fennec_CompressBatchNRGBADevices: CompressBatch of .jpg items on all GPUs of the node from one
 * process (file bytes are host memory, so any device may take any item). */
int fennec_CompressBatchJPEGDevices(const int *devices, int ndev, int workers, int n, const uint8_t *const *files, const size_t *sizes,
                                    double target_ssim, uint8_t *const *outs, const size_t *caps, fennec_BatchResult *results,
                                    const volatile int *cancel /* may be NULL */, fennec_on_item on_item /* may be NULL */, void *user);
/* ... with CompressFile's options: per item fennec_CompressFileJPEG under item_opts[i] when that is not NULL, else under
 * *default_opts (batch.go:101-105: item.Opts over BatchOptions.DefaultOpts).  dims (may be NULL): 4 ints per item, as
 * fennec_CompressFileJPEG's.  An item analyzeFormat sends to PNG comes back failed with status FNX_NOOP. */
int fennec_CompressBatchJPEGOpts(int device, int workers, int n, const uint8_t *const *files, const size_t *sizes,
                                 const fennec_FileOptions *default_opts, const fennec_FileOptions *const *item_opts /* may be NULL */,
                                 uint8_t *const *outs, const size_t *caps, fennec_BatchResult *results, int *dims /* may be NULL */,
                                 const volatile int *cancel /* may be NULL */, fennec_on_item on_item /* may be NULL */, void *user);
/* CompressFile for a JPEG or PNG source in target-size mode (fennec.go:107-160 with Options.TargetSize > 0) from the file's
 * bytes, every pixel stage on the device: image.Decode + toNRGBA, ApplyOrientation and smartResize staged exactly as
 * fennec_CompressFileJPEG stages them (opts->file; its auto_format and target_ssim are ignored), then ONE
 * fnx_jpeg_target_size on the resident image with the library's SSIM window: cand, *winner, out / cap / *nbytes and cancel are
 * that call's.  `strategies` with all four bits is hitTargetSize under Format: JPEG (targetsize.go:26-75 with wantJPEG).
 * Format: Auto and Format: PNG (quantizeStrategy between strategies 1 and 3, the PNG scale search, the PNG fallback, betterFit
 * over everything) are fennec_CompressFileHitTargetSize below; go/fennec_hip.go's hitTargetSize still composes them itself
 * over decoded images.
 * dims[0..1] = OriginalDimensions (after orientation); dims[2..3] = the winner's final_w x final_h (fennec.go:153 overwrites
 * FinalDimensions with the size result's) -- the staged image's size when there is no winner.
 * FNX_OK: a winner, its file in out.  FNX_NOOP: no candidate (possible only without FNX_TS_FALLBACK).  FNX_ERR_UNSUPPORTED
 * as fnx_jpeg_decode / fnx_png_decode.  FNX_ERR_INVALID before any device work: a NULL among ctx, data, opts, cand, winner,
 * nbytes, dims (out may be NULL with cap == 0: the size only), target_bytes <= 0, strategies not a non-empty subset of the
 * four bits, reserved != 0.  FNX_ERR_INVALID with *nbytes, cand, *winner and dims filled: cap is below the file's size -- call
 * again with *nbytes.  A winner that fits the target fits a buffer of target_bytes, so this happens only for winners OVER the
 * target: the fallback's file, and strategy 4's encode at bestQ. */
typedef struct fennec_TargetOptions {
    fennec_FileOptions file; /* orient, max_w, max_h as for fennec_CompressFileJPEG; auto_format and target_ssim ignored */
    int64_t target_bytes;    /* Options.TargetSize, > 0 */
    int32_t strategies;      /* FNX_TS_* mask; all four bits = Format: JPEG */
    int32_t reserved;        /* 0 */
} fennec_TargetOptions;      /* 40 bytes */
/* (The file's Huffman tables follow fnx_ctx_set_jpeg_huffman.) */
int fennec_CompressFileTargetSize(fnx_ctx *ctx, const uint8_t *data, size_t n, const fennec_TargetOptions *opts,
                                  const volatile int *cancel /* may be NULL */, fnx_size_candidate cand[4], int *winner,
                                  uint8_t *out, size_t cap, size_t *nbytes, int dims[4]);
/* The same from a file's bytes under any Options.Format: fennec_CompressFileTargetSize's staging exactly (decode a JPEG or PNG
 * source, orientation, smartResize: `file`), then ONE fnx_hit_target_size on the resident image with the library's SSIM window.
 * cand, *winner, out / cap / *nbytes, cancel: that call's; dims as fennec_CompressFileTargetSize's.  FNX_ERR_INVALID before any
 * device work: a NULL among ctx, data, file, cand, winner, nbytes, dims (out may be NULL with cap == 0), target_bytes <= 0, a
 * format outside 0..2.  The pool over files (fennec_CompressBatchTargetSize) stays on the JPEG legs.
 * The file's Huffman tables follow fnx_ctx_set_jpeg_huffman. */
int fennec_CompressFileHitTargetSize(fnx_ctx *ctx, const uint8_t *data, size_t n, const fennec_FileOptions *file, long long target_bytes,
                                     int format, const volatile int *cancel /* may be NULL */, fnx_size_candidate cand[5], int *winner,
                                     uint8_t *out, size_t cap, size_t *nbytes, int dims[4]);
/* The pool of fennec_CompressBatchJPEGOpts over files in target-size mode: per item fennec_CompressFileTargetSize under
 * item_opts[i] when that is not NULL, else under *default_opts (batch.go:101-105); `cancel` is the pool's (checked before each
 * item) and each item's (checked where hitTargetSize checks ctx.Err()).  Per result: quality and ssim the winner's,
 * compressed_size = the file's size, steps = the four candidates' steps added up, original_size = sizes[i], status the
 * item call's status, failed for anything but FNX_OK (an item whose buffer was too small comes back FNX_ERR_INVALID with
 * compressed_size set).  cands (may be NULL): 4 per item; dims (may be NULL): 4 ints per item.  FNX_ERR_INVALID before the
 * pool starts: a NULL array, or *default_opts refused as above. */
int fennec_CompressBatchTargetSize(int device, int workers, int n, const uint8_t *const *files, const size_t *sizes,
                                   const fennec_TargetOptions *default_opts, const fennec_TargetOptions *const *item_opts /* may be NULL */,
                                   uint8_t *const *outs, const size_t *caps, fennec_BatchResult *results,
                                   fnx_size_candidate *cands /* 4 per item, may be NULL */, int *dims /* 4 per item, may be NULL */,
                                   const volatile int *cancel /* may be NULL */, fennec_on_item on_item /* may be NULL */, void *user);
/* The pool's idle worker contexts (kept between batches, per device) are destroyed. */
void fennec_pool_release(void);
/* Summarize (batch.go:140-158) of such results: out4 = {Total, Succeeded, Failed, TotalSaved}; returns AvgSSIM. */
double fennec_SummarizeResults(int n, const fennec_BatchResult *results, int64_t out4[4]);

/* Summarize (batch.go:140-158) over parallel arrays; out4 = {Total, Succeeded,
 * Failed, TotalSaved}; returns AvgSSIM.  Pure host arithmetic in index order. */
double fennec_Summarize(int n, const int32_t *failed, const int32_t *has_result,
                        const int64_t *original_size, const int64_t *compressed_size,
                        const double *ssim, int64_t out4[4]);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* FENNEC_HIP_H */
