// pm_init.hip — random plane initialisation (gipuma_init_cu2, reference gipuma.cu:678-729) and the
// diagnostic "score these planes" kernel (pmCostMultiview_cu over a caller-supplied plane map).
// Both visit every pixel: region 32 x 8 per 256-thread workgroup.  The tap loop is pm_dispatch.h's choice for the context.
#include "pm_init_impl.h"

// REDRAW (tsar_pm_rescore): the initialising form that keeps the given plane where it is a valid hypothesis (variant bit 25)
template <bool INIT, bool REDRAW = false>
static int launch_full(tsar_ctx* ctx, const float4* planes, float* c, float4* n, int32_t* bv, float* rt) {
    if (every_pixel_takes_lut(ctx)) return launch_pm_full_lut(ctx, INIT, REDRAW, planes, c, n, bv, rt);   // pm_init_lut.hip
    return with_tap_config(ctx, [&](auto cfg) { return launch_full_g<decltype(cfg), INIT, REDRAW>(cfg, ctx, planes, c, n, bv, rt); });
}

// The initialisation of the plain fast box-11 configuration — pm_dispatch.h's choice is TapConfig<2, 5, false, true, 250> and no term
// is installed — runs the paired-gather kernel of pm_pair.hip (TSAR_PAIR bit 0).  Decided on the configuration with_tap_config
// hands over, not on a second copy of its rule.
int launch_pm_init(tsar_ctx* ctx) {
    float* const c = ctx->buf[0].c;
    float4* const n = ctx->buf[0].n4;
    if (every_pixel_takes_lut(ctx)) return launch_pm_full_lut(ctx, true, false, nullptr, c, n, nullptr, nullptr);   // pm_init_lut.hip
    return with_tap_config(ctx, [&](auto cfg) {
        typedef decltype(cfg) Cfg;
        if constexpr (Cfg::NB == 2 && Cfg::HR == 5 && !Cfg::STRICT && Cfg::QUAD && Cfg::V == 250)
            if ((ctx->pair & 1) && !scene_has_terms(ctx->hscene)) return launch_pm_init_pair(ctx);
        return launch_full_g<Cfg, true, false>(cfg, ctx, nullptr, c, n, nullptr, nullptr);
    });
}
int launch_pm_cost_planes(tsar_ctx* ctx, const float4* planes, float* cost, int32_t* beview, float* ratio) {
    return launch_full<false>(ctx, planes, cost, nullptr, beview, ratio);
}
int launch_pm_rescore(tsar_ctx* ctx, const float4* planes, float* cost, float4* n, int32_t* beview, float* ratio) {
    return launch_full<true, true>(ctx, planes, cost, n, beview, ratio);
}
