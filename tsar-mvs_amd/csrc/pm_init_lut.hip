// pm_init_lut.hip — the every-pixel kernel (pm_init_impl.h) for every window other than the scripts' box 11, on 8-bit imagery
// (pm_core_lut.h): random initialisation, the scoring of caller-supplied planes and tsar_pm_rescore's form (init && redraw).
#include "pm_init_impl.h"

int launch_pm_full_lut(tsar_ctx* ctx, bool init, bool redraw, const float4* planes, float* c, float4* n, int32_t* bv, float* rt) {
    return with_lut_config(ctx, [&](auto cfg) {
        using Cfg = decltype(cfg);
        if (!init) return launch_full_g<Cfg, false>(cfg, ctx, planes, c, n, bv, rt);
        return redraw ? launch_full_g<Cfg, true, true>(cfg, ctx, planes, c, n, bv, rt) : launch_full_g<Cfg, true>(cfg, ctx, planes, c, n, bv, rt);
    });
}
