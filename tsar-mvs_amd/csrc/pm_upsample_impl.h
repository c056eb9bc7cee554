// pm_upsample_impl.h — plane upsampling of the coarse-to-fine mode (tsar_upsample_planes): every fine pixel scores the planes of
// its four nearest coarse pixels with the context's own multi-view cost and keeps the cheapest.  The every-pixel kernel of
// pm_init_impl.h with four hypotheses instead of one: the reference window is staged and hoisted once per pixel and the four
// candidates run the same tap loop (box-11 loop / general-window loop / one-tap loop) as tsar_pm_cost_planes, so each candidate's
// cost, best view and ratio are bit for bit what that call returns for it.
// The merge form (MERGE, tsar_upsample_merge) scores the pixel's own current plane first, as a fifth candidate ahead of the four, so a
// coarse plane replaces it only where it scores lower; with a geometric-consistency term installed it runs with variant bit 24.
#pragma once
#include "pm_dispatch.h"

#define UP_RH 8

// coarse: [ch][cw] plane map of the coarse level.  Candidates of fine pixel (x, y): coarse (x / 2 + i, y / 2 + j), i, j in {0, 1},
// clamped to the coarse image, in the order (0,0), (1,0), (0,1), (1,1); the lowest cost wins, the first on a tie.  Writes the
// winner's plane to n_out and keep_out (the context's resize4), its cost / best view / ratio to c_out / beview_out / ratio_out.
// MERGE: candidate 0 is own_in[p] (the fine state's plane), the four coarse ones follow; keep_out is not written.  own_in and n_out are
// different buffers (the launcher writes the context's other ping-pong buffer).
template <int NB, int HR, bool STRICT, bool QUAD, int V = 0, bool MERGE = false>
__global__ __launch_bounds__(PM_BLOCK) void pm_upsample_kernel(const DevScene* __restrict__ sc, const float4* __restrict__ own_in,
                                                               const float4* __restrict__ coarse, int cw, int ch,
                                                               float* __restrict__ c_out, float4* __restrict__ n_out, float4* __restrict__ keep_out,
                                                               int32_t* __restrict__ beview_out, float* __restrict__ ratio_out, int tiles_x,
                                                               int n_tiles, int strip_w) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    typedef typename TileOf<QUAD>::type TileT;
    const int hr = HR > 0 ? HR : sc->hrad, vr = HR > 0 ? HR : sc->vrad;
    const int tw = PM_RW + 2 * hr, th = UP_RH + 2 * vr;
    constexpr bool LUTW = (V & TSAR_V_LUT) != 0;
    const size_t lut_bytes = LUTW ? (size_t)(sc->lut_classes + 1) * 1024 : 0;
    TileT* tile = (TileT*)(lds_raw + lut_bytes);
    float* wts = LUTW ? (float*)lds_raw : (float*)(lds_raw + tile_bytes<QUAD>(tw, th)) + threadIdx.x;
    if constexpr (LUTW) build_weight_lut<PM_BLOCK>(sc, wts);
    const int t = xcd_tile(blockIdx.x, n_tiles);
    int tix, tiy;
    strip_tile(t, tiles_x, n_tiles / tiles_x, strip_w, tix, tiy);
    const int ty0 = tiy * UP_RH, tx0 = tix * PM_RW;
    stage_ref_tile<UP_RH, TileT>(sc, tile, tx0, ty0, hr, vr, LUTW ? LUT_TILE_PAD_ROWS : 0);
    __syncthreads();
    const int ly = threadIdx.x >> 5, lx = threadIdx.x & 31;
    const int x = tx0 + lx, y = ty0 + ly;
    const int w = sc->w, h = sc->h;
    if (x >= w || y >= h) return;
    const int p = y * w + x;
    const int own = (ly + vr) * tw + lx + hr;

    const int cx0 = min(x >> 1, cw - 1), cy0 = min(y >> 1, ch - 1);
    const int cx1 = min(cx0 + 1, cw - 1), cy1 = min(cy0 + 1, ch - 1);

    PixelRef pr;
    if constexpr (LUTW) pr = hoist_reference_lut(sc, tile, tw, own, wts);
    else pr = hoist_reference<HR, TileT>(tile, tw, own, wts, hr, vr);
    // candidates are loaded where they are scored and the winner is kept as its coarse index, -1 = the pixel's own plane (an array of
    // the candidate planes, indexed in the rolled loop, would live in scratch; one rolled loop keeps one copy of the tap loop)
    int best_q = MERGE ? -1 : cy0 * cw + cx0;
    float best_c = TSAR_MAXCOST, best_rt = 0.f;
    int best_bv = -1;
    if (pr.textured) {      // an untextured reference window scores MAXCOST / -1 / 0 for every plane: the first candidate wins
        best_c = __builtin_inff();
#pragma unroll 1
        for (int k = MERGE ? -1 : 0; k < 4; k++) {
            const int q = k < 0 ? -1 : ((k & 2) ? cy1 : cy0) * cw + ((k & 1) ? cx1 : cx0);
            int bv = -1;
            float rt = 0.f;
            const float c = multiview_cost<NB, HR, STRICT, QUAD, V>(sc, tile, tw, own, wts, pr, x, y, (MERGE && q < 0) ? own_in[p] : coarse[q], bv, rt);
            if (c < best_c) { best_c = c; best_q = q; best_bv = bv; best_rt = rt; }
        }
    }
    const float4 best_n = (MERGE && best_q < 0) ? own_in[p] : coarse[best_q];
    n_out[p] = best_n;
    if constexpr (!MERGE) keep_out[p] = best_n;
    c_out[p] = best_c;
    beview_out[p] = best_bv;
    ratio_out[p] = best_rt;
}

// MERGE (tsar_upsample_merge): reads the state in buf[0], writes buf[1] (the caller swaps them); the plain form writes buf[0] and
// resize4.  Timed as "pm_upsample_merge" / "pm_upsample".
template <int NB, int HR, bool STRICT, bool QUAD, int V = 0, bool MERGE = false>
static int launch_up_t(tsar_ctx* ctx, const float4* coarse, int cw, int ch) {
    auto kern = pm_upsample_kernel<NB, HR, STRICT, QUAD, V, MERGE>;
    TapGrid g;
    if (const int rc = tap_grid(ctx, kern, UP_RH, PM_BLOCK, QUAD, V, 0, g)) return rc;
    const PlaneBuf& out = ctx->buf[MERGE ? 1 : 0];
    {
        ScopedKernelTimer tm(ctx, MERGE ? "pm_upsample_merge" : "pm_upsample");
        hipLaunchKernelGGL(kern, dim3(g.n_tiles), dim3(PM_BLOCK), g.lds, ctx->stream, ctx->dscene, MERGE ? ctx->buf[0].n4 : nullptr, coarse, cw, ch, out.c,
                           out.n4, MERGE ? nullptr : ctx->resize4, ctx->beview, ctx->ratio, g.tiles_x, g.n_tiles, strip_width(ctx->strip_w, g.tiles_x));
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    return TSAR_OK;
}

// The launchers' entry, for a configuration of pm_dispatch.h: the merge form carries the geometric-consistency term (variant bit 24)
// while one, or a plane prior, is installed; the plain form never runs with either (tsar_upsample_planes refuses them).
template <class Cfg, bool MERGE>
static int launch_up_g(Cfg, tsar_ctx* ctx, const float4* coarse, int cw, int ch) {
    constexpr int NB = Cfg::NB, HR = Cfg::HR, V = Cfg::V;
    constexpr bool STRICT = Cfg::STRICT, QUAD = Cfg::QUAD;
    if constexpr (MERGE)
        if (scene_has_terms(ctx->hscene)) return launch_up_t<NB, HR, STRICT, QUAD, V | TSAR_V_GEOM, true>(ctx, coarse, cw, ch);
    return launch_up_t<NB, HR, STRICT, QUAD, V, MERGE>(ctx, coarse, cw, ch);
}
