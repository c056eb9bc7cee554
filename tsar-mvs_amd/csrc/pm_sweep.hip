// pm_sweep.hip — one red/black half-iteration of PatchMatch: spatial propagation + plane refinement
// of every pixel of one checkerboard colour, fused into ONE launch.
//
// Replaces gipuma_{black,red}_spatialProp_cu + gipuma_{black,red}_planeRefine_cu
// (reference gipuma.cu:846-1138; host loop :1744-1754 issues 4 launches + 4 device syncs per
// iteration, here 2 launches and no sync).  Refinement touches only the thread's own pixel, so fusing
// it behind propagation does not change any value.
//
// Determinism: neighbours are read from the launch-start state.  Opposite-colour pixels are not
// written by this launch; same-colour pixels (the six "V" taps of each near arm,
// gipuma.cu:958-1034) are read from `same_in` while results go to `same_out` (ping-pong), where the
// reference reads and writes the same array concurrently.
#include "pm_sweep_impl.h"

// Variant bit 3 of the fast tap loop relies on D16 LDS loads writing the whole destination register (zeros in the
// half that is not loaded), which is how gfx950 behaves with SRAM ECC enabled.  Checked once per context.
__global__ void d16_probe_kernel(uint32_t* out) {
    __shared__ unsigned short t[64];
    t[threadIdx.x] = (unsigned short)(0x4300u + threadIdx.x);
    __syncthreads();
    uint32_t r = 0xffffffffu;
    const uint32_t addr = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned short*)(t + threadIdx.x);
    asm volatile("ds_read_u16_d16_hi %0, %1\n\ts_waitcnt lgkmcnt(0)" : "+v"(r) : "v"(addr));
    out[threadIdx.x] = r;
}
bool probe_d16_hi_zeroes(tsar_ctx* ctx) {
    CallFrame f(ctx, "d16 probe", nullptr, /*grow_arena=*/false);   // (tsar_create has made the stream; the arena is still empty and stays so)
    uint32_t h[64];
    uint32_t* d = f.out(h, 64, TSAR_MEM_HOST);
    if (f.ok()) {
        hipLaunchKernelGGL(d16_probe_kernel, dim3(1), dim3(64), 0, ctx->stream, d);
        f.launched();
    }
    bool ok = f.finish() == TSAR_OK;
    for (int i = 0; ok && i < 64; i++) ok = h[i] == ((0x4300u + i) << 16);
    return ok;
}

template <int NB, int HR>
static int launch_sweep_nh(tsar_ctx* ctx, int colour, const PlaneBuf& a, const PlaneBuf& b, const PlaneBuf& c, uint32_t sid, int dp, int dr) {
    const bool strict = ctx->hscene.flags & TSAR_FLAG_STRICT_DIV, quad = ctx->hscene.use_quad;
    // structured buffer loads for the gathers (pm_tap_r5.h BUF) from the third sweep of a run on: measured per launch
    // (tools/launch_series.sh) they take 0.6 ms off a converged launch (37.6 -> 37.0) and add 4 ms to the first sweep after the
    // random initialisation (55.1 -> 59.1), where neighbouring lanes' footprints are unrelated, and 0.3 ms to the second (41.0 -> 41.3).
    // Fast mode on the difference texture (round 4: its cheaper blend outweighs the doubled footprint already on the SECOND
    // sweep, -1.7 ms per view; on the first it costs 28 ms): from sweep ctx->buffer_from = 1 on.
    const bool buf = ctx->buffer_gather && ctx->sweeps_done >= (strict ? (ctx->buffer_from > 2 ? ctx->buffer_from : 2) : ctx->buffer_from);
    // The production configuration (8-bit quad textures, box 11, <= 4 best views) runs the hand-scheduled tap loop of pm_tap_r5.h in
    // both arithmetic modes: variant 250 in fast mode (row-wise walk), 122 in strict mode (the oracle's column order; also the
    // column-order fast loop, TSAR_VARIANT=122), 114 where the D16 probe fails; + TSAR_V_BUF with buffer loads.
    const int v = ctx->variant;
    if constexpr ((NB == 2 || NB == 4) && HR == 5)
    if (quad && !(ctx->hscene.flags & TSAR_FLAG_TEX_FILTER_8BIT) && (v == 250 || v == 122 || (v == 114 && NB == 2))) {   // (the 8-bit filter mode runs the general-window loop)
#define SWEEP_R5(S, V, B) (buf ? launch_sweep_g<NB, 5, S, true, (V) | TSAR_V_BUF, B>(ctx, colour, a, b, c, sid, dp, dr) : launch_sweep_g<NB, 5, S, true, V, B>(ctx, colour, a, b, c, sid, dp, dr))
        // fast mode, buffer-load launches: the half-float difference texture (pm_tap_r5.h MIX) when tsar_set_views built it
        const bool mix = buf && !strict && v == 250 && ctx->hscene.n_sel > 0 && ctx->hscene.view[ctx->hscene.sel[0]].dquad != nullptr;
#define SWEEP_R5_FAST250_ALL(B) (mix ? launch_sweep_g<NB, 5, false, true, 250 | TSAR_V_BUF | TSAR_V_MIX, B>(ctx, colour, a, b, c, sid, dp, dr) : SWEEP_R5(false, 250, B))
        // ... and, where a hypothesis's cost is its best view's alone (best-N combination, n_best 1, no geometric or prior term), the
        // same three forms with the partial-window check of the wide refinement steps (TSAR_V_PRUNE; TSAR_PRUNE=0: never)
        // Only in the launches that check (from launch TSAR_PRUNE_FROM of a call on): the pruning instantiation of the global-load
        // form, which the first sweep of a view runs, is 5.8 ms slower than the plain one with its checks idle (profiles/prune).
        const bool prune = NB == 2 && !strict && v == 250 && ctx->prune && ctx->prune_steps > 0 && dr && ctx->call_launch >= ctx->prune_from &&
                           ctx->hscene.cost_comb == TSAR_COMB_BEST_N && ctx->hscene.n_best == 1 && !scene_has_terms(ctx->hscene);
#define SWEEP_R5_PRUNE(B) (mix ? launch_sweep_t<2, 5, false, true, 250 | TSAR_V_BUF | TSAR_V_MIX | TSAR_V_PRUNE, B>(ctx, colour, a, b, c, sid, dp, dr) \
                           : buf ? launch_sweep_t<2, 5, false, true, 250 | TSAR_V_BUF | TSAR_V_PRUNE, B>(ctx, colour, a, b, c, sid, dp, dr)              \
                                 : launch_sweep_t<2, 5, false, true, 250 | TSAR_V_PRUNE, B>(ctx, colour, a, b, c, sid, dp, dr))
        // ... and where the choice is the plain global-load kernel <2, 5, false, true, 250, B> (the first sweep of a run: random planes,
        // every lane on its own cache line), the paired-gather kernel of pm_pair.hip (TSAR_PAIR bit 1)
        const bool pair = NB == 2 && !strict && v == 250 && !buf && !prune && (ctx->pair & 2) && !scene_has_terms(ctx->hscene);
        // ... and where it is a difference-texture kernel of the best-two-views form without terms, plain or checking, the ring kernel
        // of pm_ring.hip, from sweep TSAR_RING of a run on (the same counter as TSAR_BUFFER_FROM)
        const bool ring = NB == 2 && mix && ctx->ring > 0 && ctx->sweeps_done >= ctx->ring && !scene_has_terms(ctx->hscene);
#define SWEEP_R5_FAST250(B) (ring ? launch_pm_sweep_ring(ctx, B, prune, colour, a, b, c, sid, dp, dr) : prune ? SWEEP_R5_PRUNE(B) : pair ? launch_pm_sweep_pair(ctx, B, colour, a, b, c, sid, dp, dr) : SWEEP_R5_FAST250_ALL(B))
        if constexpr (NB == 2) {
            // small images: 128-thread workgroups (see SWEEP_SMALL_IMAGE_TILES); TSAR_BLOCK=128|256 forces a shape (A/B runs)
            const int tiles256 = ((ctx->hscene.w + PM_RW - 1) / PM_RW) * ((ctx->hscene.h + 15) / 16);
            bool small = tiles256 < SWEEP_SMALL_IMAGE_TILES;
            if (ctx->force_block) small = ctx->force_block == 128;
            if (small && v != 114) {
                if (strict) return SWEEP_R5(true, 122, 128);
                return v == 250 ? SWEEP_R5_FAST250(128) : launch_sweep_g<2, 5, false, true, 122, 128>(ctx, colour, a, b, c, sid, dp, dr);
            }
            if (v == 114) return strict ? launch_sweep_g<2, 5, true, true, 114>(ctx, colour, a, b, c, sid, dp, dr) : launch_sweep_g<2, 5, false, true, 114>(ctx, colour, a, b, c, sid, dp, dr);
        }
        if (strict) return SWEEP_R5(true, 122, PM_BLOCK);
        return v == 250 ? SWEEP_R5_FAST250(PM_BLOCK) : launch_sweep_g<NB, 5, false, true, 122>(ctx, colour, a, b, c, sid, dp, dr);
#undef SWEEP_R5_FAST250
#undef SWEEP_R5_PRUNE
#undef SWEEP_R5_FAST250_ALL
#undef SWEEP_R5
    }
    constexpr int NBG = NB == 4 ? 32 : NB;      // the one-tap-at-a-time kernels exist for 2 and 32 best views
    if (strict) return quad ? launch_sweep_g<NBG, HR, true, true>(ctx, colour, a, b, c, sid, dp, dr) : launch_sweep_g<NBG, HR, true, false>(ctx, colour, a, b, c, sid, dp, dr);
    return quad ? launch_sweep_g<NBG, HR, false, true>(ctx, colour, a, b, c, sid, dp, dr) : launch_sweep_g<NBG, HR, false, false>(ctx, colour, a, b, c, sid, dp, dr);
}

int launch_pm_sweep(tsar_ctx* ctx, int colour, const PlaneBuf& same_in, const PlaneBuf& other, const PlaneBuf& same_out, uint32_t stream_id,
                    int do_prop, int do_refine) {
    const DevScene& hs = ctx->hscene;
#ifdef TSAR_EXPERIMENTS
    // measured-and-rejected / diagnostic forms (pm_sweep_experiments.hip: TSAR_VARIANT / TSAR_VARIANT_NOW); they have no form with the
    // geometric-consistency term, so while one is installed the production kernels run (with it) instead
    if (!scene_has_terms(hs)) {
        int launched = 0;
        const int rc = launch_pm_sweep_experiment(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine, &launched);
        if (rc != TSAR_OK || launched) return rc;
    }
#endif
    const int need = views_in_cost(hs);
    const bool r5 = hs.hrad == 5 && hs.vrad == 5;
    // 8-bit imagery, any window but the box-11 / two-best-views configuration (which has its own tap loop): shared weight
    // table, chunked lines (pm_sweep_lut.hip)
    // (the box-11 loop filters with exact fp32 weights only: the 8-bit filter mode takes the general-window loop at box 11 too)
    const bool own_loop = r5 && need <= 4 && (need <= 2 || ctx->variant == 250 || ctx->variant == 122) && !(hs.flags & TSAR_FLAG_TEX_FILTER_8BIT);   // (TSAR_VARIANT=0 or an experiment: the generic loop below)
    if (lut_path_applies(ctx) && (!own_loop || lut_path_forced(ctx))) return launch_pm_sweep_lut(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
    if (need <= 4 && need > 2 && r5) return launch_sweep_nh<4, 5>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
    if (need <= 2) return r5 ? launch_sweep_nh<2, 5>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine)
                             : launch_sweep_nh<2, 0>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
    return r5 ? launch_sweep_nh<32, 5>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine)
              : launch_sweep_nh<32, 0>(ctx, colour, same_in, other, same_out, stream_id, do_prop, do_refine);
}
