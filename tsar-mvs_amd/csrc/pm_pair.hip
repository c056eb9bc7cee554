// pm_pair.hip — the random-plane launches' kernels with the paired tap loop (pm_tap_r5.h PAIR, variant bit TSAR_V_PAIR): one
// 16-byte gather per pair of row taps.  The initialisation and the first sweep of a view score planes that are unrelated between
// neighbouring lanes, so every lane's gather lands on its own cache line and the kernels are bound by the texture addresser's
// look-ups, not by VALU issue (profiles/r05 section 4, profiles/pair_gather).  The plain fast configuration only: box 11, best two
// views in registers, global loads on the byte texture, no geometric or prior term, no pruning; no packed form.  The launchers of
// pm_init.hip and pm_sweep.hip call in here where their choice is that configuration and TSAR_PAIR allows it.
#include "pm_init_impl.h"
#include "pm_sweep_impl.h"

int launch_pm_init_pair(tsar_ctx* ctx) {
    return launch_full_t<2, 5, false, true, true, 250 | TSAR_V_PAIR>(ctx, nullptr, ctx->buf[0].c, ctx->buf[0].n4, nullptr, nullptr);
}

int launch_pm_sweep_pair(tsar_ctx* ctx, int block, int colour, const PlaneBuf& same_in, const PlaneBuf& other, const PlaneBuf& same_out,
                         uint32_t stream_id, int do_prop, int do_refine) {
    if (block == 128) return launch_sweep_t<2, 5, false, true, 250 | TSAR_V_PAIR, 128>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
    return launch_sweep_t<2, 5, false, true, 250 | TSAR_V_PAIR, PM_BLOCK>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
}
