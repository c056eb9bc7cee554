// pm_ring.hip — the difference-texture sweep kernels with the ring form of the unrolled clamp-free walk (pm_tap_r5.h RING, variant
// bit TSAR_V_RING): six gathers in flight across a view's six lines instead of six per line.  The fast box-11 configuration only:
// best two views in registers, buffer loads on the half-float difference texture, no geometric or prior term; with and without the
// partial-window checks (TSAR_V_PRUNE), both workgroup shapes, rolled and packed.  The launcher of pm_sweep.hip calls in here where
// its choice is that configuration and TSAR_RING allows it; every kernel of pm_sweep.hip stays as it is.
#include "pm_sweep_impl.h"

int launch_pm_sweep_ring(tsar_ctx* ctx, int block, bool prune, int colour, const PlaneBuf& same_in, const PlaneBuf& other, const PlaneBuf& same_out,
                         uint32_t stream_id, int do_prop, int do_refine) {
    constexpr int V = 250 | TSAR_V_BUF | TSAR_V_MIX | TSAR_V_RING;
    if (prune) {
        if (block == 128) return launch_sweep_t<2, 5, false, true, V | TSAR_V_PRUNE, 128>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
        return launch_sweep_t<2, 5, false, true, V | TSAR_V_PRUNE, PM_BLOCK>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
    }
    if (block == 128) return launch_sweep_t<2, 5, false, true, V, 128>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
    return launch_sweep_t<2, 5, false, true, V, PM_BLOCK>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
}
