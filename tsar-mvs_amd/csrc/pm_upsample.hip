// pm_upsample.hip — the plane-upsampling kernel (pm_upsample_impl.h) in the configurations of the every-pixel kernel
// (pm_init.hip launch_full): the same tap loop is chosen for the same context, so a candidate's score is tsar_pm_cost_planes's.
// MERGE = the merge form of tsar_upsample_merge (each instantiation also with the geometric-consistency term, pm_upsample_impl.h launch_up_g).
#include "pm_upsample_impl.h"

template <int NB, int HR, bool MERGE>
static int launch_up_nh(tsar_ctx* ctx, const float4* coarse, int cw, int ch) {
    const bool strict = ctx->hscene.flags & TSAR_FLAG_STRICT_DIV, quad = ctx->hscene.use_quad;
    const bool production = !(ctx->hscene.flags & TSAR_FLAG_TEX_FILTER_8BIT);
    if (production && quad && NB == 2 && HR == 5 && ctx->variant == 250 && !strict) return launch_up_g<2, 5, false, true, 250, MERGE>(ctx, coarse, cw, ch);
    if (production && quad && NB == 2 && HR == 5 && (ctx->variant == 250 || ctx->variant == 122 || ctx->variant == 114)) {
        if (strict) return ctx->variant != 114 ? launch_up_g<2, 5, true, true, 122, MERGE>(ctx, coarse, cw, ch) : launch_up_g<2, 5, true, true, 114, MERGE>(ctx, coarse, cw, ch);
        return ctx->variant == 122 ? launch_up_g<2, 5, false, true, 122, MERGE>(ctx, coarse, cw, ch) : launch_up_g<2, 5, false, true, 114, MERGE>(ctx, coarse, cw, ch);
    }
    if (strict) return quad ? launch_up_g<NB, HR, true, true, 0, MERGE>(ctx, coarse, cw, ch) : launch_up_g<NB, HR, true, false, 0, MERGE>(ctx, coarse, cw, ch);
    return quad ? launch_up_g<NB, HR, false, true, 0, MERGE>(ctx, coarse, cw, ch) : launch_up_g<NB, HR, false, false, 0, MERGE>(ctx, coarse, cw, ch);
}

template <bool MERGE>
static int launch_up(tsar_ctx* ctx, const float4* coarse, int cw, int ch) {
    const DevScene& hs = ctx->hscene;
    const int need = hs.cost_comb == TSAR_COMB_BEST_N ? (hs.n_best < hs.n_sel ? hs.n_best : hs.n_sel) : hs.n_sel;
    const bool r5 = hs.hrad == 5 && hs.vrad == 5;
    if (lut_path_applies(ctx) && (!(r5 && need <= 2) || (hs.flags & TSAR_FLAG_TEX_FILTER_8BIT) || lut_path_forced(ctx))) return launch_pm_upsample_lut(ctx, need, MERGE, coarse, cw, ch);   // pm_upsample_lut.hip
    if (need <= 2) return r5 ? launch_up_nh<2, 5, MERGE>(ctx, coarse, cw, ch) : launch_up_nh<2, 0, MERGE>(ctx, coarse, cw, ch);
    return r5 ? launch_up_nh<32, 5, MERGE>(ctx, coarse, cw, ch) : launch_up_nh<32, 0, MERGE>(ctx, coarse, cw, ch);
}

int launch_pm_upsample(tsar_ctx* ctx, const float4* coarse, int cw, int ch) { return launch_up<false>(ctx, coarse, cw, ch); }
int launch_pm_upsample_merge(tsar_ctx* ctx, const float4* coarse, int cw, int ch) { return launch_up<true>(ctx, coarse, cw, ch); }
