// What blur.hip and blur_mfma.hip share to launch a plan (blur_plan.hpp): the images of a call, the one-pass form's tables, the
// launch's events, and blur_mfma.hip's one entry.  Private to the two files.
#pragma once
#include "common.hpp"

namespace fnx {

// blur_mfma.hip: plan p's matrix kernel (BLUR_MFMA, BLUR_MFMA_WIDE); score: its one-pass form (launch_blur_scored's tables)
struct BlurImages {       // n same-geometry images by pointer (src / dst, n == 1) or by device pointer arrays
    const uint8_t *src; const uint8_t *const *srcs; uint8_t *dst; uint8_t *const *dsts;
    int sstride, dstride, w, h;
};
template <typename Args> void set_images(Args &k, const BlurImages &im)
{
    k.src = im.src; k.srcs = im.srcs; k.dst = im.dst; k.dsts = im.dsts;
    k.sstride = im.sstride; k.dstride = im.dstride; k.w = im.w; k.h = im.h;
}
struct BlurScore {
    const int32_t *bx, *by;             // box column / row of each source column / row
    const uint32_t *coltab, *rowtab;    // blur_mfma_kernel: build_score_geom's ready-made set-up of its column and row look-ups
    unsigned long long *slabs;
    int nbx, nby;
    int seg;                            // the form's rows per workgroup (ScoreGeom::th)
};
int launch_blur_mfma(fnx_ctx *ctx, int n, const BlurPlan &p, const BlurImages &im, const double *kernel, const BlurScore *score);
// The events of a blur launch ride on its own packet (LaunchEvents): the profile pair when this class is profiled, and for a
// SCORE launch always a stop event -- the step's tail on the ctx's second stream waits for it (launch_blur_scored)
inline int blur_bind_events(fnx_ctx *ctx, bool score, LaunchEvents *ev)
{
    FNX_TRY(prof_bind(ctx, FNX_PROF_MAIN, ev));
    if (score) {
        if (!ev->stop) ev->stop = ctx->ev_blur[ctx->parity];
        ctx->blur_done = ev->stop;
    }
    return FNX_OK;
}

}  // namespace fnx
