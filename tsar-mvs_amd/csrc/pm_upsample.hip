// pm_upsample.hip — the plane-upsampling kernel (pm_upsample_impl.h) in the configurations of the every-pixel kernel
// (pm_init.hip): both go through pm_dispatch.h, so the same tap loop is chosen for the same context and a candidate's score is
// tsar_pm_cost_planes's.
// MERGE = the merge form of tsar_upsample_merge (each instantiation also with the geometric-consistency term, pm_upsample_impl.h launch_up_g).
#include "pm_upsample_impl.h"

template <bool MERGE>
static int launch_up(tsar_ctx* ctx, const float4* coarse, int cw, int ch) {
    if (every_pixel_takes_lut(ctx)) return launch_pm_upsample_lut(ctx, MERGE, coarse, cw, ch);   // pm_upsample_lut.hip
    return with_tap_config(ctx, [&](auto cfg) { return launch_up_g<decltype(cfg), MERGE>(cfg, ctx, coarse, cw, ch); });
}

int launch_pm_upsample(tsar_ctx* ctx, const float4* coarse, int cw, int ch) { return launch_up<false>(ctx, coarse, cw, ch); }
int launch_pm_upsample_merge(tsar_ctx* ctx, const float4* coarse, int cw, int ch) { return launch_up<true>(ctx, coarse, cw, ch); }
