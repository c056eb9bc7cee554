// pm_upsample_lut.hip — the plane-upsampling kernel (pm_upsample_impl.h) for every window other than box 11 on 8-bit imagery:
// the general-window loop, chosen like pm_init_lut.hip's (pm_dispatch.h); merge = the merge form of tsar_upsample_merge (with and
// without the term).
#include "pm_upsample_impl.h"

int launch_pm_upsample_lut(tsar_ctx* ctx, bool merge, const float4* coarse, int cw, int ch) {
    return with_lut_config(ctx, [&](auto cfg) {
        return merge ? launch_up_g<decltype(cfg), true>(cfg, ctx, coarse, cw, ch) : launch_up_g<decltype(cfg), false>(cfg, ctx, coarse, cw, ch);
    });
}
