// pm_sweep_lut.hip — the sweep kernel (pm_sweep_impl.h) for every window other than the scripts' box 11, on 8-bit imagery:
// runtime radius, weights from the shared table, lines walked in chunks of 4 / 5 / 6 taps (pm_core_lut.h).
#include "pm_sweep_impl.h"

// Taps per chunk for a line of T taps: the fewest padding slots, the longer chunk on a tie (more gathers in flight per wave).
int lut_chunk_taps(int T) {
    int best = 6, waste = (6 - T % 6) % 6;
    for (int ch = 5; ch >= 4; ch--) {
        const int wst = (ch - T % ch) % ch;
        if (wst < waste) { waste = wst; best = ch; }
    }
    return best;
}

// The configuration is pm_dispatch.h's; on top of it, in fast mode only (strict mode instantiates neither): from sweep
// ctx->buffer_from of a run on the gathers are structured buffer loads (TSAR_V_BUF, see pm_sweep.hip), then on the half-float
// difference texture (TSAR_V_MIX, pm_tap_r5.h MIX) when tsar_set_views built it.
int launch_pm_sweep_lut(tsar_ctx* ctx, int colour, const PlaneBuf& same_in, const PlaneBuf& other, const PlaneBuf& same_out, uint32_t stream_id,
                        int do_prop, int do_refine) {
    const DevScene& hs = ctx->hscene;
    const bool buf = ctx->buffer_gather && ctx->sweeps_done >= ctx->buffer_from;
    const bool mix = hs.n_sel > 0 && hs.view[hs.sel[0]].dquad != nullptr;
    return with_lut_config(ctx, [&](auto cfg) {
        constexpr int NB = decltype(cfg)::NB, V = decltype(cfg)::V;
        constexpr bool STRICT = decltype(cfg)::STRICT;
        if constexpr (!STRICT) {
            if (buf && mix) return launch_sweep_g<NB, 0, false, true, V | TSAR_V_BUF | TSAR_V_MIX>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
            if (buf) return launch_sweep_g<NB, 0, false, true, V | TSAR_V_BUF>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
        }
        return launch_sweep_g<NB, 0, STRICT, true, V>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
    });
}
