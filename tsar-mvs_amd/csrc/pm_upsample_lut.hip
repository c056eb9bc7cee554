// pm_upsample_lut.hip — the plane-upsampling kernel (pm_upsample_impl.h) for every window other than box 11 on 8-bit imagery:
// the general-window loop, dispatched like pm_init_lut.hip; MERGE = the merge form of tsar_upsample_merge (with and without the term).
#include "pm_upsample_impl.h"

#define LUT_V(ch) (1024 | ((ch) << 11))

template <int NB, bool STRICT, bool MERGE>
static int launch_up_lut_nsm(tsar_ctx* ctx, int chunk, const float4* coarse, int cw, int ch) {
    switch (chunk) {
        case 4: return launch_up_g<NB, 0, STRICT, true, LUT_V(4), MERGE>(ctx, coarse, cw, ch);
        case 5: return launch_up_g<NB, 0, STRICT, true, LUT_V(5), MERGE>(ctx, coarse, cw, ch);
        default: return launch_up_g<NB, 0, STRICT, true, LUT_V(6), MERGE>(ctx, coarse, cw, ch);
    }
}
template <int NB, bool STRICT>
static int launch_up_lut_ns(tsar_ctx* ctx, int chunk, bool merge, const float4* coarse, int cw, int ch) {
    return merge ? launch_up_lut_nsm<NB, STRICT, true>(ctx, chunk, coarse, cw, ch) : launch_up_lut_nsm<NB, STRICT, false>(ctx, chunk, coarse, cw, ch);
}

int launch_pm_upsample_lut(tsar_ctx* ctx, int need, bool merge, const float4* coarse, int cw, int ch) {
    const bool strict = ctx->hscene.flags & TSAR_FLAG_STRICT_DIV;
    const int chunk = ctx->hscene.lut_chunk;
    if (need <= 2) return strict ? launch_up_lut_ns<2, true>(ctx, chunk, merge, coarse, cw, ch) : launch_up_lut_ns<2, false>(ctx, chunk, merge, coarse, cw, ch);
    if (need <= 4) return strict ? launch_up_lut_ns<4, true>(ctx, chunk, merge, coarse, cw, ch) : launch_up_lut_ns<4, false>(ctx, chunk, merge, coarse, cw, ch);
    return strict ? launch_up_lut_ns<32, true>(ctx, chunk, merge, coarse, cw, ch) : launch_up_lut_ns<32, false>(ctx, chunk, merge, coarse, cw, ch);
}
