// pm_core.h — the matching cost and the per-pixel PatchMatch step, shared by the init / sweep / upsampling /
// cost-evaluation kernels (pm_init_impl.h, pm_sweep_impl.h, pm_upsample_impl.h).  The cost of one view is one of three tap loops —
// view_cost_generic here, view_cost_r5 (pm_tap_r5.h), view_cost_lut (pm_core_lut.h) — built from the per-tap pieces of
// pm_tap_common.h; multiview_cost combines the views.
//
// Mapping (MI355X-first): one thread owns one pixel and walks its hypotheses; a
// 256-thread workgroup owns a 32-wide pixel region.  Per workgroup, once per launch:
//   - the reference-image window (region + halo) is staged in LDS (clamp addressing baked in),
//   - each thread hoists everything that depends only on its reference pixel out of the
//     hypothesis x view loop: the S bilateral weights (kept in LDS, [tap][thread] so a wave reads
//     consecutive banks), sum(w), sum(w r), sum(w r^2) and the reference variance.  The reference
//     recomputes these S exp() and 3 sums for every one of ~14 hypotheses x N views
//     (gipuma.cu:259-277); the values are identical, only the work is hoisted.
//   - pixels whose reference window has no texture (var_ref < 1e-5) can never change (every
//     hypothesis scores MAXCOST, gipuma.cu:289-291) and stop there.
// Source taps: the homography-warped position is bilinearly sampled in software (no texture unit on
// gfx950).  For 8-bit imagery each view is pre-packed into 2x2 texel quads (plane_kernels.hip build_quad_kernel), so a
// tap is ONE 4-byte gather instead of four.
#pragma once
#include <type_traits>

#include "tsar_device_math.h"

#define PM_BLOCK 256
#define PM_RW 32  // region width in pixels (all kernels)

#include "pm_tap_common.h"   // the per-tap pieces every tap loop below is made of

// DIFF (fast arithmetic only, oracle S7 (6)): the blend as (t00 + ax d1) + ay (d2 + ax d3) over the texel differences
template <bool QUAD, bool DIFF = false>
DEVFN float sample_bilinear(const DevView& vw, int w, int h, int qpitch, float u, float v, bool q8 = false) {
    // tex2D(tex, u + .5, v + .5), linear filter, clamp addressing (main.cpp:1215-1219).
    u = fminf(fmaxf(u, -1.0f), (float)w);
    v = fminf(fmaxf(v, -1.0f), (float)h);
    const float fu = floorf(u), fv = floorf(v);
    float ax = u - fu, ay = v - fv;
    if (q8) { ax = rintf(ax * 256.0f) * 0.00390625f; ay = rintf(ay * 256.0f) * 0.00390625f; }   // TSAR_FLAG_TEX_FILTER_8BIT (wave-uniform)
    const int iu = (int)fu, iv = (int)fv;
    float t00, t10, t01, t11;
    if (QUAD) {
        // byte offset kept in 32 bits (a view is < 4 GiB) so the gather is `global_load_dword v, v_off, s[base]`
        const uint32_t off = (uint32_t)(__mul24(iv + 1, qpitch) + iu + 1) * 4u;
        const uint32_t q = *(global_u32_ptr)((const char __attribute__((address_space(1)))*)vw.quad + off);
        t00 = (float)(q & 0xffu);
        t10 = (float)((q >> 8) & 0xffu);
        t01 = (float)((q >> 16) & 0xffu);
        t11 = (float)(q >> 24);
    } else {
        const int x0 = min(max(iu, 0), w - 1), x1 = min(max(iu + 1, 0), w - 1);
        const int y0 = min(max(iv, 0), h - 1), y1 = min(max(iv + 1, 0), h - 1);
        const global_f32_ptr r0 = (global_f32_ptr)vw.img + (size_t)y0 * w;
        const global_f32_ptr r1 = (global_f32_ptr)vw.img + (size_t)y1 * w;
        t00 = r0[x0]; t10 = r0[x1]; t01 = r1[x0]; t11 = r1[x1];
    }
    return blend_texels<DIFF>(t00, t10, t01, t11, ax, ay);
}

// Stage the reference window of this workgroup's region in LDS.  tile is (RW + 2hr) x (RH + 2vr).
// Reference-window texel type: 8-bit imagery (QUAD path) keeps the window as 16-bit entries holding the upper half
// of each texel's fp32 pattern (bf16; exact for the integers 0..255), which is what lets four 256-thread workgroups
// (weights 36 KiB + window 2.1 KiB each) share one CU's 160 KiB of LDS, and lets the fast tap loop load a texel
// straight into the upper half of a register (ds_read_u16_d16_hi) with no convert instruction.
template <bool QUAD> struct TileOf { typedef float type; };
template <> struct TileOf<true> { typedef unsigned short type; };     // upper half of the fp32 pattern: exact for 0..255
DEVFN float tile_value(float t) { return t; }
DEVFN float tile_value(unsigned short t) { return __uint_as_float((uint32_t)t << 16); }
DEVFN void tile_store(float* t, float v) { *t = v; }
DEVFN void tile_store(unsigned short* t, float v) { *t = (unsigned short)(__float_as_uint(v) >> 16); }
template <bool QUAD>
__host__ __device__ constexpr size_t tile_bytes(int tw, int th) {
    return ((size_t)tw * th * sizeof(typename TileOf<QUAD>::type) + 15) & ~(size_t)15;
}

// pad_rows: rows staged below the window (clamp addressing, so finite texels): pm_core_lut.h reads past a row's end
template <int RH, typename TileT, int BLK = PM_BLOCK, int RW = PM_RW>
DEVFN void stage_ref_tile(const DevScene* __restrict__ sc, TileT* tile, int x0, int y0, int hr, int vr, int pad_rows = 0) {
    const int tw = RW + 2 * hr, th = RH + 2 * vr + pad_rows;
    const global_f32_ptr img = (global_f32_ptr)sc->view[0].img;
    const int w = sc->w, h = sc->h;
    for (int k = threadIdx.x; k < tw * th; k += BLK) {
        const int ty = k / tw, tx = k - ty * tw;
        const int gx = min(max(x0 + tx - hr, 0), w - 1), gy = min(max(y0 + ty - vr, 0), h - 1);
        tile_store(&tile[k], img[(size_t)gy * w + gx]);
    }
}

// Bilateral weights + reference moments (gipuma.cu:247-277, the parts that depend on the reference
// image only).  own = index of this thread's pixel in the tile, wts = LDS weight column of this thread.
template <int HR, typename TileT, int BLK = PM_BLOCK>
DEVFN PixelRef hoist_reference(const TileT* tile, int tw, int own, float* wts, int hr_rt, int vr_rt) {
    const int hr = HR > 0 ? HR : hr_rt, vr = HR > 0 ? HR : vr_rt;
    const float cen = tile_value(tile[own]);
    float sum_ref = 0.f, sum_ref_ref = 0.f, wsum = 0.f;
    int tap = 0;
#pragma unroll
    for (int i = -hr; i <= hr; i += 2) {
#pragma unroll
        for (int j = -vr; j <= vr; j += 2) {
            const float r = tile_value(tile[own + j * tw + i]);
            const float sd = sqrtf((float)(i * i + j * j));
            const float cd = fabsf(r - cen);
            const float wt = tsar_expf(-sd / 50.0f - cd / 18.0f);   // sigma_spatial 5, sigma_color 3 (gipuma.cu:248-249,268)
            wts[tap * BLK] = wt;
            const float wr = wt * r;
            sum_ref += wr;
            sum_ref_ref = fma_(wr, r, sum_ref_ref);
            wsum += wt;
            ++tap;
        }
    }
    return pixel_ref_from_sums(sum_ref, sum_ref_ref, 1.0f / wsum);
}

// pmCost gipuma.cu:229-298 for one source view, given the hoisted reference terms: any window, both arithmetic modes, float or
// quad images, one tap at a time in the oracle's order.  (The production loops: pm_tap_r5.h for the scripts' box 11 on 8-bit
// imagery, pm_core_lut.h for every other window on 8-bit imagery; this one serves float imagery and the 8-bit-filter mode's init.)
// BLK: threads per workgroup = stride, in floats, between the weights of consecutive taps of one thread ([tap][thread])
template <int HR, bool STRICT, bool QUAD, int BLK = PM_BLOCK>
DEVFN float view_cost_generic(const DevScene* __restrict__ sc, const DevView& vw, const typename TileOf<QUAD>::type* tile, int tw, int own, const float* wts,
                              const PixelRef& pr, int x, int y, const float4& n4) {
    const int hr = HR > 0 ? HR : sc->hrad, vr = HR > 0 ? HR : sc->vrad;
    const int w = sc->w, h = sc->h, qp = sc->quad_pitch;
    float H[9];
    if (STRICT) plane_homography(sc->ref, vw, n4, H, sc->k_sparse != 0);
    else plane_homography_fast(sc->ref, vw, n4, H);
    float sum_src = 0.f, sum_src_src = 0.f, sum_ref_src = 0.f;
    int tap = 0;
#pragma unroll 1
    for (int i = -hr; i <= hr; i += 2) {
        float bx, by, bz;
        tap_line_base<STRICT>(H, (float)(x + i), bx, by, bz);
#pragma unroll
        for (int j = -vr; j <= vr; j += 2) {
            float X, Y, Z, u, v;
            tap_homogeneous<STRICT>(H, (float)(y + j), bx, by, bz, X, Y, Z);
            tap_divide<STRICT, true>(X, Y, Z, u, v);
            const float s = sample_bilinear<QUAD, !STRICT>(vw, w, h, qp, u, v, (sc->flags & TSAR_FLAG_TEX_FILTER_8BIT) != 0);
            const float r = tile_value(tile[own + j * tw + i]);
            const float wt = wts[tap * BLK];
            const TapSums t = tap_accumulate<STRICT>(TapSums{sum_src, sum_src_src, sum_ref_src}, wt, r, s);
            sum_src = t.src; sum_src_src = t.src_src; sum_ref_src = t.ref_src;
            ++tap;
        }
    }
    // (the tail of ncc_cost, pm_tap_common.h, with the compiler's sqrtf: float imagery has no bound on the variances)
    sum_src *= pr.inv_wsum;
    sum_src_src *= pr.inv_wsum;
    sum_ref_src *= pr.inv_wsum;
    const float var_src = sum_src_src - sum_src * sum_src;
    if (var_src < 1e-5f) return TSAR_MAXCOST;
    const float covar = sum_ref_src - pr.mean_ref * sum_src;
    const float vrs = sqrtf(pr.var_ref * var_src);
    return fmaxf(0.0f, fminf(TSAR_MAXCOST, 1.0f - covar / vrs));
}

#include "pm_tap_r5.h"     // view_cost_r5: the production loop for box 11 on 8-bit imagery (variants 114 / 122 / 250, + TSAR_V_BUF = buffer loads)
#include "pm_core_lut.h"   // view_cost_lut: any window, weights from a shared table (variant bit 10; chunk length in bits 11-13)

// The geometric-consistency term lambda e of view vi for the hypothesis whose depth at (x, y) is D (include/tsar.h states the
// sequence; tests/test_geom_cpu.py restates it in numpy float32).  Every operation is one IEEE fp32 operation (no contraction: the
// library is built with -ffp-contract=off and no fma_ is written here); the two quotient pairs are persp_divide_exact's correctly rounded
// ones and the root is sqrt_rsq_exact's, so the value is the same in both arithmetic modes.  The projection into the view uses
// DevView A = K_v R K_ref^-1 and b = K_v t (the point D K_ref^-1 (x, y, 1) moved and projected in one 3 x 4 product), the way back
// the host's geom_back matrix.  A view without a depth map adds 0 (scalar branch: the pointer is wave-uniform).
DEVFN float geom_term(const DevScene* __restrict__ sc, const DevView& vw, int vi, int x, int y, float D) {
    const float* dm = sc->geom_depth[vi];
    if (dm == nullptr) return 0.0f;
    const int w = sc->w, h = sc->h;
    const float xf = (float)x, yf = (float)y;
    const float xd = xf * D, yd = yf * D;
    const float a = ((vw.A[0] * xd + vw.A[1] * yd) + vw.A[2] * D) + vw.b[0];
    const float b = ((vw.A[3] * xd + vw.A[4] * yd) + vw.A[5] * D) + vw.b[1];
    const float s = ((vw.A[6] * xd + vw.A[7] * yd) + vw.A[8] * D) + vw.b[2];
    float u, v;
    persp_divide_exact<true>(a, b, s, u, v);
    const float cf = floorf(u + 0.5f), rf = floorf(v + 0.5f);
    // (NaN fails every comparison: a non-finite projection is "outside")
    const bool inside = s > 0.0f && cf >= 0.0f && cf <= (float)(w - 1) && rf >= 0.0f && rf <= (float)(h - 1);
    float Dv = 0.0f;
    if (inside) Dv = ((global_f32_ptr)dm)[(int)rf * w + (int)cf];
    const float* M = sc->geom_back[vi];
    const float cd = cf * Dv, rd = rf * Dv;
    const float p0 = ((M[0] * cd + M[1] * rd) + M[2] * Dv) + M[3];
    const float p1 = ((M[4] * cd + M[5] * rd) + M[6] * Dv) + M[7];
    const float p2 = ((M[8] * cd + M[9] * rd) + M[10] * Dv) + M[11];
    float xq, yq;
    persp_divide_exact<true>(p0, p1, p2, xq, yq);
    const float dx = xq - xf, dy = yq - yf;
    const float e2 = dx * dx + dy * dy;
    const float tau = sc->geom_clip;
    // e2 in [2^-100, tau^2): the correctly rounded root (sqrt_rsq_exact's range holds: tau <= 2^20); below: 0; else (also NaN): tau
    const float r = sqrt_rsq_exact(fminf(fmaxf(e2, 0x1p-100f), 0x1p100f));
    float e = e2 < 0x1p-100f ? 0.0f : r;
    e = (inside && Dv > 0.0f && p2 > 0.0f && e2 < sc->geom_clip_sq) ? fminf(e, tau) : tau;
    return sc->geom_weight * e;
}

// The plane-prior term t of the hypothesis n4 whose depth at (x, y) is D, added to its multi-view cost c (include/tsar.h states the
// sequence; tests/test_plane_prior_cpu.py restates it in numpy float32).  Every operation is one IEEE fp32 operation and the three
// quotients are the compiler's correctly rounded `/` (once per hypothesis, beside n_sel tap loops), so the value is the same in both
// arithmetic modes.  (x, y) is the SCORED pixel: the packed sweep scores other lanes' pixels.  No prior installed is one scalar
// branch (the pointer is wave-uniform); a pixel without a prior (held entry all zero) keeps c.
DEVFN float add_prior_term(const DevScene* __restrict__ sc, int x, int y, const float4& n4, float D, float c) {
    const float4* pp = sc->prior;
    if (pp == nullptr) return c;
    typedef float prior_entry __attribute__((ext_vector_type(4)));       // one 16-byte global load
    const prior_entry q = ((const __attribute__((address_space(1))) prior_entry*)pp)[y * sc->w + x];
    const float Dp = q.w;
    const float a = fabsf(D - Dp);
    const float rel = a / Dp;
    const float dclip = sc->prior_depth_clip, nclip = sc->prior_normal_clip;
    const float r_d = rel < dclip ? rel / dclip : 1.0f;                  // (NaN fails the comparison)
    const float s = 1.0f - ((n4.x * q.x + n4.y * q.y) + n4.z * q.z);
    const float s0 = s < 0.0f ? 0.0f : s;
    const float r_n = s < nclip ? s0 / nclip : 1.0f;
    const float t = (sc->prior_weight_depth * r_d) + (sc->prior_weight_normal * r_n);
    return Dp > 0.0f ? c + t : c;
}

// pmCostMultiview_cu gipuma.cu:455-518: best-N combination over the selected views.  The NB
// smallest costs are kept sorted in registers (sort_small :425-434 sorts all of them).
// V & TSAR_V_GEOM: each view's cost becomes c_v + lambda e_v (geom_term) after the validity test, which stays on c_v; the depth of the
// hypothesis at (x, y) is computed once, before the view loop; after the best-N division the plane-prior term is added
// (add_prior_term), which leaves best view and ratio alone.  The other bits of V name the tap loop.
// V & TSAR_V_PRUNE (the sweep's best-view-only kernels, pruned_cost in pm_sweep_impl.h): while `prune` (wave-uniform), a view may be
// left early when the partial-window bound proves its cost >= cost_now for every active lane; it then counts as invalid (MAXCOST) and
// `skipped` is raised: the result is exact for a lane only if it is not below cost_now — pruned_cost repeats the hypothesis otherwise.
template <int NB, int HR, bool STRICT, bool QUAD, int V = 0, int BLK = PM_BLOCK>
DEVFN float multiview_cost(const DevScene* __restrict__ sc, const typename TileOf<QUAD>::type* tile, int tw, int own, const float* wts, const PixelRef& pr,
                           int x, int y, const float4& n4, int& beview, float& ratio, bool prune = false, float cost_now = 0.0f, int* skipped = nullptr) {
    constexpr bool GEOM = (V & TSAR_V_GEOM) != 0;
    constexpr bool PRUNE = (V & TSAR_V_PRUNE) != 0;
    static_assert(!PRUNE || !GEOM, "the bound speaks of the photometric cost alone");
    constexpr bool PAIR = (V & TSAR_V_PAIR) != 0;
    static_assert(!PAIR || (!PRUNE && !GEOM), "the paired gathers exist for the plain fast box-11 kernels");
    constexpr bool RING = (V & TSAR_V_RING) != 0;
    constexpr int VT = V & ~(TSAR_V_GEOM | TSAR_V_REDRAW | TSAR_V_PRUNE | TSAR_V_PAIR | TSAR_V_RING);
    static_assert(!RING || (VT == (250 | TSAR_V_BUF | TSAR_V_MIX) && !GEOM && !PAIR && !STRICT && QUAD && HR == 5), "the ring exists for the fast difference-texture box-11 kernels");
    float best[NB];
#pragma unroll
    for (int k = 0; k < NB; k++) best[k] = __builtin_inff();
    const int num = sc->n_sel;
    int valid = 0, bv = -1;
    float cmin = __builtin_inff();
    float depth_h = 0.0f;
    if constexpr (GEOM) depth_h = plane_depth(sc->ref, n4, x, y);
    int vi_next = sc->sel[0];
    for (int i = 0; i < num; i++) {
        // the NEXT view's index is loaded now (scalar load, wave-uniform), a whole view of tap loops ahead of its use: otherwise
        // every view starts with two dependent scalar-memory round trips (index, then camera block) in front of its first instruction
        const int vi = vi_next;
        vi_next = sc->sel[i + 1 < num ? i + 1 : i];
        float c;
        // V names the tap loop: bit 10 = the general-window loop (chunk length in bits 11-13), a production variant of the box-11
        // loop (pm_tap_r5.h), 0 = the generic one-tap loop; anything else exists in the experiments build only
        if constexpr ((VT & TSAR_V_LUT) != 0) c = view_cost_lut<STRICT, (VT >> 11) & 7, (VT & TSAR_V_BUF) != 0 && !STRICT, (VT & TSAR_V_MIX) != 0 && !STRICT>(sc, sc->view[vi], tile, tw, own, wts, pr, x, y, n4);
        else if constexpr (QUAD && HR == 5 && r5_production_variant(VT) && PRUNE) {
            static_assert((VT & 250) == 250 && !STRICT, "pruning instantiations exist for the fast row-wise loop");
            ViewPrune vp;
            vp.on = prune; vp.skipped = false;
            vp.cost_now = cmin < cost_now ? TSAR_MAXCOST : cost_now;          // (a lane that will accept needs exact values)
            c = view_cost_r5<false, true, true, (VT & TSAR_V_BUF) != 0, (VT & TSAR_V_MIX) != 0, BLK, 0, true, false, RING>(sc, sc->view[vi], tile, tw, own, wts, pr, x, y, n4, &vp);
            if (vp.skipped) *skipped += 1;
        } else if constexpr (QUAD && HR == 5 && PAIR && VT == 250) {
            static_assert(!STRICT, "the paired gathers exist for the fast row-wise loop");
            c = view_cost_r5<false, true, true, false, false, BLK, 0, false, true>(sc, sc->view[vi], tile, tw, own, wts, pr, x, y, n4);
        } else if constexpr (QUAD && HR == 5 && r5_production_variant(VT))
            c = view_cost_r5<STRICT, (VT & 128) != 0 && !STRICT, (VT & 8) != 0, (VT & TSAR_V_BUF) != 0, (VT & TSAR_V_MIX) != 0, BLK, 0, false, false, RING>(sc, sc->view[vi], tile, tw, own, wts, pr, x, y, n4);
#ifdef TSAR_EXPERIMENTS
        else if constexpr (QUAD && HR == 5 && PAIR && VT == (250 | 4194304))
            c = view_cost_r5<false, true, true, false, false, BLK, 3, false, true>(sc, sc->view[vi], tile, tw, own, wts, pr, x, y, n4);
        else if constexpr (QUAD && HR == 5 && r5_diag_variant(VT))
            c = view_cost_r5<false, true, true, true, true, BLK, (VT & 4194304) ? 1 : 2>(sc, sc->view[vi], tile, tw, own, wts, pr, x, y, n4);
#endif
        else {
            static_assert(VT == 0, "unknown tap-loop variant");
            c = view_cost_generic<HR, STRICT, QUAD, BLK>(sc, sc->view[vi], tile, tw, own, wts, pr, x, y, n4);
        }
        // if (c < MAXCOST) valid++; else c = MAXCOST;  if (c <= cmin) { cmin = c; bv = vi; } (last view attaining the minimum,
        // gipuma.cu:506-510) — written on sign bits instead of lane masks (v_cndmask / v_addc issue at several times a v_fma's cost
        // here): c is a finite cost or MAXCOST, never NaN, so c < MAXCOST  <=>  c - MAXCOST < 0 and c > cmin  <=>  cmin - c < 0
        // (v_min / v_max by asm: fminf / fmaxf make the compiler canonicalise each operand first, a v_max_f32 x, x per call; the
        // operands here are never NaN)
        auto vmin = [](float a, float b) { float r; asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; };
        auto vmax = [](float a, float b) { float r; asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b)); return r; };
        c = vmin(c, TSAR_MAXCOST);
        valid -= (int32_t)__float_as_uint(c - TSAR_MAXCOST) >> 31;
        if constexpr (GEOM) c = c + geom_term(sc, sc->view[vi], vi, x, y, depth_h);     // (validity was decided on the photometric cost)
        {
            const uint32_t worse = (uint32_t)((int32_t)__float_as_uint(cmin - c) >> 31);      // all ones where c > cmin (cmin = +inf at first: inf - c > 0)
            asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(bv) : "v"(worse), "v"(bv), "s"(vi));       // (worse & bv) | (~worse & vi): the compiler turns the C form back into v_cmp + v_cndmask
            cmin = vmin(cmin, c);
        }
        float v = c;
#pragma unroll
        for (int k = 0; k < NB; k++) {
            const float lo = vmin(best[k], v), hi = vmax(best[k], v);
            best[k] = lo;
            v = hi;
        }
    }
    int nb = valid;
    if (sc->cost_comb == TSAR_COMB_BEST_N) nb = min(nb, sc->n_best);
    if (nb <= 0) { beview = -1; ratio = 0.f; return TSAR_MAXCOST; }
    float cost = 0.f;
#pragma unroll
    for (int k = 0; k < NB; k++)
        if (k < nb) cost += best[k];
    cost = cost / (float)nb;
    ratio = num >= 2 ? best[0] / best[1] : 0.f;
    beview = bv;
    if constexpr (GEOM) cost = add_prior_term(sc, x, y, n4, depth_h, cost);
    return cost;
}

// XCD-aware tile order (guide §5.5 T1): workgroups are dealt round-robin to the 8 XCDs, so remap the
// linear id such that each XCD walks one contiguous band of tiles and neighbouring tiles (which share
// reference halo and source footprints) hit the same 4 MiB L2.  Bijective for any n.
// Tile order inside that walk: strips of `sw` tiles across, row-major inside a strip, so that the ~128 workgroups
// an XCD has in flight cover a compact 2-D patch (sw x 8 tiles) of the reference image: their source footprints then
// overlap in both directions and fit the XCD's 4 MiB L2, instead of one 1-tile-high band as wide as the image.
// sw <= 0: plain row-major.
DEVFN void strip_tile(int t, int tiles_x, int tiles_y, int sw, int& tx, int& ty) {
    if (sw <= 0) { ty = t / tiles_x; tx = t - ty * tiles_x; return; }
    const int per_strip = sw * tiles_y;
    const int strip = t / per_strip, within = t - strip * per_strip;
    const int width = min(sw, tiles_x - strip * sw);      // the last strip may be narrower
    ty = within / width;
    tx = strip * sw + within - ty * width;
}

// Strip width: the tile list is cut into 8 contiguous chunks, one per XCD (xcd_tile); with strips of ceil(tiles_x / 8)
// tiles every XCD walks (almost exactly) one vertical band of the image, so the L2s hold disjoint parts of the source
// views.  Measured at 6048 x 4032 (189 tiles across): 24 -> 41.25 ms per sweep, 16 -> 41.9, 32 -> 42.0, 48 -> 42.4.
static inline int strip_width(int requested, int tiles_x) {
    if (requested >= 0) return requested;
    const int sw = (tiles_x + 7) / 8;
    return sw < 8 ? 8 : sw;
}

DEVFN int xcd_tile(int bid, int n) {
    const int chunk = n >> 3, rem = n & 7;
    const int xcd = bid & 7, slot = bid >> 3;
    return xcd * chunk + min(xcd, rem) + slot;
}
