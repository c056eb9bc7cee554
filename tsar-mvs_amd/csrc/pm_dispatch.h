// pm_dispatch.h — the one place where a context becomes a tap-loop configuration.  The every-pixel operators (tsar_pm_init,
// tsar_pm_cost_planes, tsar_pm_rescore, tsar_upsample_planes, tsar_upsample_merge) all take their kernel's template arguments from
// with_tap_config / with_lut_config, so the same tap loop is chosen for the same context by construction and a candidate's score is
// tsar_pm_cost_planes's (tests/test_kernel_configs.py holds the instantiated sets to that).  Host code only; the selectors are
// templates, so each translation unit instantiates the kernels of its own operator and nothing else.
#pragma once
#include "pm_core.h"

// What names a tap loop: best views kept in registers (2 / 4 / 32), the compile-time radius (5 = box 11, 0 = runtime), the
// arithmetic mode, the quad-texture gathers of 8-bit imagery and the variant number (tsar_dev.h TSAR_V_*, pm_tap_r5.h).
template <int NB_, int HR_, bool STRICT_, bool QUAD_, int V_>
struct TapConfig {
    static constexpr int NB = NB_, HR = HR_, V = V_;
    static constexpr bool STRICT = STRICT_, QUAD = QUAD_;
};
#define LUT_V(ch) (TSAR_V_LUT | ((ch) << 11))      // the general-window loop walking its lines in chunks of ch taps

// how many views enter a hypothesis's cost
static inline int views_in_cost(const DevScene& hs) {
    return hs.cost_comb == TSAR_COMB_BEST_N ? (hs.n_best < hs.n_sel ? hs.n_best : hs.n_sel) : hs.n_sel;
}

// The every-pixel kernels run the general-window loop (with_lut_config) wherever it applies, except in the box-11 / two-best-views
// configuration, which has its own tap loop — unless the 8-bit filter mode (that loop filters with exact fp32 weights only) or
// TSAR_LUT=2 sends that one through it too.
static inline bool every_pixel_takes_lut(const tsar_ctx* ctx) {
    const DevScene& hs = ctx->hscene;
    const bool own_loop = hs.hrad == 5 && hs.vrad == 5 && views_in_cost(hs) <= 2 && !(hs.flags & TSAR_FLAG_TEX_FILTER_8BIT);
    return lut_path_applies(ctx) && (!own_loop || lut_path_forced(ctx));
}

// a runtime flag as a compile-time one: f(std::true_type) or f(std::false_type)
template <class F>
static int with_flag(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// Calls f(TapConfig{}) for the box-11 / float-imagery configuration of the context (every_pixel_takes_lut is false).  The production
// configuration (8-bit quad textures, box 11, <= 2 best views, exact filter weights) runs the sweep's tap loop (pm_tap_r5.h) in both
// arithmetic modes: variant 250 (fast) / 122 (strict, or TSAR_VARIANT=122) / 114 (the D16 probe failed); everything else the
// generic one-tap loop (variant 0) with 2 or 32 best views and, at box 11, the radius at compile time.
template <class F>
static int with_tap_config(const tsar_ctx* ctx, F&& f) {
    const DevScene& hs = ctx->hscene;
    const bool strict = hs.flags & TSAR_FLAG_STRICT_DIV, quad = hs.use_quad;
    const bool r5 = hs.hrad == 5 && hs.vrad == 5, few = views_in_cost(hs) <= 2;
    const int v = ctx->variant;
    if (few && r5 && quad && !(hs.flags & TSAR_FLAG_TEX_FILTER_8BIT) && (v == 250 || v == 122 || v == 114)) {
        if (strict) return v != 114 ? f(TapConfig<2, 5, true, true, 122>{}) : f(TapConfig<2, 5, true, true, 114>{});
        return v == 250 ? f(TapConfig<2, 5, false, true, 250>{}) : v == 122 ? f(TapConfig<2, 5, false, true, 122>{}) : f(TapConfig<2, 5, false, true, 114>{});
    }
    return with_flag(few, [&](auto few_c) { return with_flag(r5, [&](auto r5_c) { return with_flag(strict, [&](auto strict_c) { return with_flag(quad, [&](auto quad_c) {
        return f(TapConfig<decltype(few_c)::value ? 2 : 32, decltype(r5_c)::value ? 5 : 0, decltype(strict_c)::value, decltype(quad_c)::value, 0>{});
    }); }); }); });
}

// Calls f(TapConfig{}) for the general-window configuration of the context: selection in two / four registers or the general one,
// the arithmetic mode, and the chunk length the scene was laid out for (lut_chunk_taps).
template <class F>
static int with_lut_config(const tsar_ctx* ctx, F&& f) {
    const DevScene& hs = ctx->hscene;
    auto chunked = [&](auto nb, auto strict_c) {
        constexpr int NB = decltype(nb)::value;
        constexpr bool STRICT = decltype(strict_c)::value;
        switch (hs.lut_chunk) {
            case 4: return f(TapConfig<NB, 0, STRICT, true, LUT_V(4)>{});
            case 5: return f(TapConfig<NB, 0, STRICT, true, LUT_V(5)>{});
            default: return f(TapConfig<NB, 0, STRICT, true, LUT_V(6)>{});
        }
    };
    const int need = views_in_cost(hs);
    return with_flag(hs.flags & TSAR_FLAG_STRICT_DIV, [&](auto strict_c) {
        if (need <= 2) return chunked(std::integral_constant<int, 2>{}, strict_c);
        if (need <= 4) return chunked(std::integral_constant<int, 4>{}, strict_c);
        return chunked(std::integral_constant<int, 32>{}, strict_c);
    });
}

// Dynamic LDS of a tap-loop kernel whose workgroup of `block` threads owns region_rows rows of PM_RW pixels: the reference window
// (region + halo; one padding row for the general-window loop) and either the shared weight table or the per-thread weights.
static inline size_t tap_loop_lds_bytes(const DevScene& hs, int region_rows, int block, bool quad, int v) {
    const bool lut = (v & TSAR_V_LUT) != 0;
    const int tw = PM_RW + 2 * hs.hrad, th = region_rows + 2 * hs.vrad + (lut ? LUT_TILE_PAD_ROWS : 0);
    return (quad ? tile_bytes<true>(tw, th) : tile_bytes<false>(tw, th)) +
           (lut ? (size_t)(hs.lut_classes + 1) * 1024 : sizeof(float) * (size_t)(hs.hrad + 1) * (hs.vrad + 1) * block);
}

// The launch shape of a tap-loop kernel: the tile grid of the image, the dynamic LDS (+ extra_lds the caller adds behind it), and
// the kernel's limit raised where that exceeds the 64 KiB a kernel may use unasked.
struct TapGrid { int tiles_x, n_tiles; size_t lds; };
template <class K>
static int tap_grid(tsar_ctx* ctx, K kern, int region_rows, int block, bool quad, int v, size_t extra_lds, TapGrid& g) {
    const DevScene& hs = ctx->hscene;
    g.tiles_x = (hs.w + PM_RW - 1) / PM_RW;
    g.n_tiles = g.tiles_x * ((hs.h + region_rows - 1) / region_rows);
    g.lds = tap_loop_lds_bytes(hs, region_rows, block, quad, v) + extra_lds;
    if (g.lds > 64 * 1024) TSAR_HIP_TRY(ctx, hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds));
    return TSAR_OK;
}
