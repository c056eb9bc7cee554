// pm_tap_common.h — what is the same for every tap of every tap loop (view_cost_generic in pm_core.h, view_cost_r5 in pm_tap_r5.h,
// view_cost_lut in pm_core_lut.h), written once: where a tap falls in the source view, how its four texels are addressed, gathered
// and blended, how it enters the three sums, and what the sums become.  The loops differ in how they walk the window and where their
// weights come from; everything here is called by them and carries no state or options of its own.  Included by pm_core.h.
#pragma once

// Image pointers come out of the DevScene table in memory, so the compiler only knows them as generic
// ("flat") pointers; flat loads count on both vmcnt and lgkmcnt and serialise against the LDS reads of
// the tap loop.  They are HBM pointers by construction: say so, and the gathers become global_load.
typedef const uint32_t __attribute__((address_space(1)))* global_u32_ptr;
typedef const float __attribute__((address_space(1)))* global_f32_ptr;

// ---- where a tap falls -------------------------------------------------------------------------------------------------------------
// getCorrespondingPoint_cu gipuma.cu:161-171 (matvecmul4noz, config.h:150-162): (m[0] x + m[1] y) + m[2].  Strict mode keeps the
// text's association, the constant added LAST (oracle S4: mul, fma, add); the fast arithmetic folds it into the line term (oracle
// S7 (7): two fused operations per coordinate).  A window is walked in lines: `a` is the line's coordinate (x of a column, or y of
// a row when ROW), `t` the tap's coordinate along the line.
template <bool STRICT, bool ROW = false>
DEVFN void tap_line_base(const float* H, float a, float& bx, float& by, float& bz) {
    bx = STRICT ? H[0] * a : fma_(H[ROW ? 1 : 0], a, H[2]);
    by = STRICT ? H[3] * a : fma_(H[ROW ? 4 : 3], a, H[5]);
    bz = STRICT ? H[6] * a : fma_(H[ROW ? 7 : 6], a, H[8]);
}
template <bool STRICT, bool ROW = false>
DEVFN void tap_homogeneous(const float* H, float t, float bx, float by, float bz, float& X, float& Y, float& Z) {
    X = fma_(H[ROW ? 0 : 1], t, bx); Y = fma_(H[ROW ? 3 : 4], t, by); Z = fma_(H[ROW ? 6 : 7], t, bz);
    if (STRICT) { X += H[2]; Y += H[5]; Z += H[8]; }
}
// the fast arithmetic's position of pixel (xi, yj), as the clamp-free decisions of both modes evaluate it
DEVFN void pixel_homogeneous(const float* H, float xi, float yj, float& X, float& Y, float& Z) {
    float bx, by, bz;
    tap_line_base<false>(H, xi, bx, by, bz);
    tap_homogeneous<false>(H, yj, bx, by, bz, X, Y, Z);
}

// STRICT: the oracle's quotients X / Z, Y / Z bit for bit (persp_divide_exact, tsar_device_math.h; GUARD = its per-tap operand
// guard); fast: v_rcp_f32 and two multiplies.
template <bool STRICT, bool GUARD>
DEVFN void tap_divide(float X, float Y, float Z, float& u, float& v) {
    if (STRICT) {
        persp_divide_exact<GUARD>(X, Y, Z, u, v);
    } else {
        const float rz = __builtin_amdgcn_rcpf(Z);
        u = X * rz;
        v = Y * rz;
    }
}

// From a tap's homogeneous position to its bilinear fractions and the element index of its quad entry, for the loops that address
// the quad texture from entry (1, 1) with an unsigned offset.  CLAMP = false: the caller has shown that the tap lies inside the
// image (pm_tap_r5.h: strict mode's corner test, the fast loops' centre-and-extent test) — strict mode then also drops the divide's operand guard.
// (pm_tap_r5.h PAIR reads 16 bytes at the entry and relies on iu <= w - 1, iv <= h - 1 below: a wider range here moves its bound.)
// Clamp range.  The oracle clamps to [-1, w] (tex2D at u + .5 with clamp addressing).  The offset is unsigned from entry (1, 1), so
// floor(u) must be >= 0: clamp to [0, w - 1] = [0, uhi] instead.  The sample is the same bit for bit: for u in [-1, 0) both texels
// of the pair are T(0) (edge replication), so the blend returns T(0) whatever the fraction — exactly what u = 0 returns (fraction
// 0); likewise beyond w - 1, and per axis.  Strict mode clamps with min/max as the oracle does, fast mode with v_med3_f32.
// u, v >= 0 after that (clamped, or inside the image): v_fract_f32 = u - floor(u) exactly (the difference is representable) and
// v_cvt_flr_i32_f32 = (int)floor(u) — the oracle's floor / subtract / convert.  The element index of quad entry (iv + 1, iu + 1)
// counted from entry (1, 1) is one 24-bit multiply-add with the pitch qp.
template <bool STRICT, bool CLAMP>
DEVFN void tap_position(float X, float Y, float Z, float uhi, float vhi, int qp, float& ax, float& ay, int& lin) {
    float u, v;
    tap_divide<STRICT, CLAMP>(X, Y, Z, u, v);
    if (CLAMP) {
        if (STRICT) {
            u = fminf(fmaxf(u, 0.0f), uhi);
            v = fminf(fmaxf(v, 0.0f), vhi);
        } else {
            u = __builtin_amdgcn_fmed3f(u, 0.0f, uhi);
            v = __builtin_amdgcn_fmed3f(v, 0.0f, vhi);
        }
    }
    int iu, iv;
    ax = __builtin_amdgcn_fractf(u);
    ay = __builtin_amdgcn_fractf(v);
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(iu) : "v"(u));
    asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(iv) : "v"(v));
    asm("v_mad_i32_i24 %0, %1, %2, %3" : "=v"(lin) : "v"(iv), "s"(qp), "v"(iu));
}

// ---- how its texels are addressed and gathered --------------------------------------------------------------------------------------
// A view's quad texture (four 8-bit texels per 4-byte entry, plane_kernels.hip build_quad_kernel) or, MIX, its half-float difference
// texture (8-byte entries, same pitch and border, build_dquad_kernel), from entry (0 + 1, 0 + 1) on: the border offset is folded
// into the base so that a tap's offset is unsigned.
DEVFN int quad_border_bytes(int qp) { return (qp + 1) << 2; }            // byte offset of quad entry (0 + 1, 0 + 1)
template <bool MIX>
DEVFN uint64_t quad_origin(const DevView& vw, int qorg) {
    if (MIX) return (uint64_t)(uintptr_t)vw.dquad + 2 * (uint64_t)(uint32_t)qorg;
    return (uint64_t)(uintptr_t)vw.quad + (uint32_t)qorg;
}
// That base opaque to the optimiser, so that it stays in two SGPRs across the view (the compiler otherwise re-loads it with s_load
// in every line and waits for it, and for the line's LDS loads, right before issuing the gathers).
DEVFN void pin_quad_base(uint64_t base, uint32_t& lo, uint32_t& hi) {
    lo = __builtin_amdgcn_readfirstlane((uint32_t)base);
    hi = __builtin_amdgcn_readfirstlane((uint32_t)(base >> 32));
    asm volatile("" : "+s"(lo), "+s"(hi));
}
// The structured-buffer view of the same entries, for gathers as `buffer_load ... idxen`: the texture addresser scales the element
// index by the stride (4, MIX: 8), so the per-tap shift goes away.  rows = h + 1: the image's rows and the border row below them.
typedef uint32_t u32x4s __attribute__((ext_vector_type(4)));
template <bool MIX>
DEVFN u32x4s quad_descriptor(uint64_t base, int rows, int qp) {
    u32x4s rsrc;
    rsrc.x = __builtin_amdgcn_readfirstlane((uint32_t)base);
    rsrc.y = __builtin_amdgcn_readfirstlane(((uint32_t)(base >> 32) & 0xffffu) | ((MIX ? 8u : 4u) << 16));     // base[47:32] | stride
    rsrc.z = __builtin_amdgcn_readfirstlane((uint32_t)(qp * rows - 1));                    // records from entry (1, 1) on
    rsrc.w = 0x00020000u;                                                                   // 32-bit data format (gfx9 family)
    asm volatile("" : "+s"(rsrc));
    return rsrc;
}

// The gather of element `lin` as a structured buffer load of 4 / 8 (MIX) bytes.  No compiler builtin reaches idxen: the loads are
// issued by asm and the compiler does not count them, so each loop writes out the vmcnt waits of their users.  (The third form, a
// global load from the pinned base, is plain C++ in each loop.)
template <bool MIX>
DEVFN std::conditional_t<MIX, uint64_t, uint32_t> buffer_gather(int lin, u32x4s rsrc) {
    std::conditional_t<MIX, uint64_t, uint32_t> q;
    if constexpr (MIX) asm volatile("buffer_load_dwordx2 %0, %1, %2, 0 idxen" : "=v"(q) : "v"(lin), "s"(rsrc));
    else asm volatile("buffer_load_dword %0, %1, %2, 0 idxen" : "=v"(q) : "v"(lin), "s"(rsrc));
    return q;
}
// A 16-byte gather from a 4-byte-aligned address (one global_load_dwordx4), and dword k (0..3) of its result per lane: two levels
// of v_perm_b32, whose selector 0x03020100 takes the second operand and 0x07060504 the first.  What the compiler emits for it
// (tools/isa.sh on pm_pair.hip): the three v_perm_b32, and each selector as v_and / v_cmp / v_cndmask between the two constants
// held in registers, not the mask arithmetic written here: 9 VALU, 11 per pair with the index difference and the range test.  Left
// so: the kernels that run it are bound by L1 look-ups and have the issue slots (profiles/pair_gather).  Any k gives some dword of
// the four.
typedef u32x4s u32x4s_a4 __attribute__((aligned(4)));
typedef const u32x4s_a4 __attribute__((address_space(1)))* global_u32x4_a4_ptr;
DEVFN uint32_t pick_dword(u32x4s a, uint32_t k) {
    const uint32_t b0 = (uint32_t)((int32_t)(k << 31) >> 31), b1 = (uint32_t)((int32_t)(k << 30) >> 31);      // all ones where the bit is set
    const uint32_t s0 = (b0 & 0x04040404u) | 0x03020100u, s1 = (b1 & 0x04040404u) | 0x03020100u;
    const uint32_t lo = __builtin_amdgcn_perm(a.y, a.x, s0), hi = __builtin_amdgcn_perm(a.w, a.z, s0);
    return __builtin_amdgcn_perm(hi, lo, s1);
}
// ---- how they are blended --------------------------------------------------------------------------------------------------------
// FAST = false: the reference's blend, two horizontal interpolations and one vertical (tex2D, linear filter).  FAST (the fast
// arithmetic, oracle S7 (6)): (t00 + ax d1) + ay (d2 + ax d3) over the texel differences, exact for integer texels.
template <bool FAST>
DEVFN float blend_texels(float t00, float t10, float t01, float t11, float ax, float ay) {
    if (FAST) {
        const float d1 = t10 - t00, d2 = t01 - t00, d3 = (t11 - t01) - d1;
        return fma_(ay, fma_(ax, d3, d2), fma_(ax, d1, t00));
    }
    const float top = fma_(ax, t10 - t00, t00);
    const float bot = fma_(ax, t11 - t01, t01);
    return fma_(ay, bot - top, top);
}
// a quad entry: one convert per texel, no shifts or masks
template <bool FAST>
DEVFN float blend_quad(uint32_t q, float ax, float ay) {
    float t00, t10, t01, t11;
    asm("v_cvt_f32_ubyte0 %0, %1" : "=v"(t00) : "v"(q));
    asm("v_cvt_f32_ubyte1 %0, %1" : "=v"(t10) : "v"(q));
    asm("v_cvt_f32_ubyte2 %0, %1" : "=v"(t01) : "v"(q));
    asm("v_cvt_f32_ubyte3 %0, %1" : "=v"(t11) : "v"(q));
    return blend_texels<FAST>(t00, t10, t01, t11, ax, ay);
}
// A difference-texture entry (halfs t00, d1 = t10 - t00, d2 = t01 - t00, d3 = t11 - t10 - t01 + t00), the fast blend with the halfs
// read in place: two mixed-precision FMAs on the gathered dwords and one plain FMA, one fp32 rounding each — the same values as
// blend_quad<true> (the halfs are exact integers), with no byte converts and no subtractions (-9 issue units of a tap's 34).
DEVFN float blend_dquad(uint64_t q2, float ax, float ay) {
    const uint32_t lo = (uint32_t)q2, hi = (uint32_t)(q2 >> 32);
    float ta, tb;
    asm("v_fma_mix_f32 %0, %1, %2, %2 op_sel:[0,1,0] op_sel_hi:[0,1,1]" : "=v"(ta) : "v"(ax), "v"(lo));          // ax * d1 + t00: the top row's interpolation
    asm("v_fma_mix_f32 %0, %1, %2, %2 op_sel:[0,1,0] op_sel_hi:[0,1,1]" : "=v"(tb) : "v"(ax), "v"(hi));          // ax * d3 + d2: bottom row minus top row, rounded once
    return fma_(ay, tb, ta);
}

// ---- how it enters the sums, and what they become ---------------------------------------------------------------------------------
// The three sums of a view's taps: sum(w s), sum(w s^2), sum(w r s); one tap (weight wt, reference texel r, source sample s) into
// them.  (By value: the sums stay registers of the caller's loop from the first pass of the optimiser on.)
struct TapSums { float src, src_src, ref_src; };
template <bool STRICT>
DEVFN TapSums tap_accumulate(TapSums a, float wt, float r, float s) {
    const float ws = wt * s;
    a.src += ws;
    a.src_src = fma_(ws, s, a.src_src);
    if (STRICT) a.ref_src = fma_(wt * r, s, a.ref_src);      // (w r) s, the oracle's order
    else a.ref_src = fma_(ws, r, a.ref_src);                 // (w s) r: one multiply fewer per tap
    return a;
}

// Per-pixel quantities that do not depend on the hypothesis.
struct PixelRef {
    float inv_wsum;   // 1 / sum(w)
    float mean_ref;   // sum(w r) / sum(w)
    float var_ref;    // E[r^2] - E[r]^2
    bool textured;    // var_ref >= kMinVar
};
// ... from the reference window's sums sum(w r), sum(w r^2) and 1 / sum(w)
DEVFN PixelRef pixel_ref_from_sums(float sum_ref, float sum_ref_ref, float inv_wsum) {
    PixelRef pr;
    pr.inv_wsum = inv_wsum;
    sum_ref *= pr.inv_wsum;
    sum_ref_ref *= pr.inv_wsum;
    pr.mean_ref = sum_ref;
    pr.var_ref = sum_ref_ref - sum_ref * sum_ref;
    pr.textured = !(pr.var_ref < 1e-5f);
    return pr;
}

// ---- the partial-window bound of the pruning kernels (variant bit TSAR_V_PRUNE; pm_tap_r5.h runs it, DESIGN.md section 4 argues it) ----
// What multiview_cost hands a view's tap loop, and what comes back: `on` and `skipped` are wave-uniform.
struct ViewPrune {
    float cost_now;   // the lane's cost, or >= 1 for a lane that must not be proven (it has seen a view below its cost: it will accept)
    bool on;          // this hypothesis is checked at all
    bool skipped;     // out: every lane was proven and the view was left (its cost is >= cost_now, value unknown)
};
// e bounds the rounding of each W-normalised second moment the cost tail forms (var_ref, var_src, covar; 36 taps of 8-bit data summed
// in fp32: <= 227 u 255^2 = 0.881, u = 2^-24); e_A the same for the W_A-scaled moments of the taps walked so far (<= 103 u 255^2 = 0.40).
#define PM_PRUNE_E 0.9f
#define PM_PRUNE_EA 0.45f
#define PM_PRUNE_SLACK 1.0e-4f     // every other rounding: the tail's root, quotient and 1 - x (< 2e-6), this test's own operations
// The test after the taps of A: aw, ar, arr = sum(w), sum(w r), sum(w r^2) over A, t = the view's running sums.  With a = W_A S_rr,A,
// b = W_A S_ss,A, c = W_A S_rs,A (centred sums times W_A), Q_A = (a - c^2 / b) / W_A grows with a and b and falls with |c|, so
// q <= Q_A is formed from a - E, b - E, |c| + E, E = e_A W_A^2.  Then, for the exact moments of the whole window,
// ncc^2 <= 1 - Q_A / (W var_ref) <= n2 = 1 - q / (W (var_ref_k + e)), var_src >= S_ss,A / W >= vs, var_ref >= vr = var_ref_k - e, and
// the tail's own value obeys ncc_k^2 <= (ncc^2 + 2 e / g + (e / g)^2) / ((1 - e / vr) (1 - e / vs)) with g = sqrt(vr vs).  Proven:
// that is <= (1 - cost_now)^2 - slack.  Six reciprocal-class operations per check, three checks per view of ~7000 issue units.
// Anything non-finite or out of range fails.
DEVFN bool prune_proven(const TapSums& t, float aw, float ar, float arr, const PixelRef& pr, float cost_now) {
    const float E = PM_PRUNE_EA * aw * aw;
    const float a_lo = fma_(aw, arr, -(ar * ar)) - E;
    const float b_lo = fma_(aw, t.src_src, -(t.src * t.src)) - E;
    const float c_hi = fabsf(fma_(aw, t.ref_src, -(ar * t.src))) + E;
    const float raw = __builtin_amdgcn_rcpf(aw);
    const float q = fma_(-(c_hi * c_hi), __builtin_amdgcn_rcpf(b_lo), a_lo) * raw;
    const float vs = (b_lo * raw) * pr.inv_wsum, vr = pr.var_ref - PM_PRUNE_E;
    const float n2 = fma_(-q, pr.inv_wsum * __builtin_amdgcn_rcpf(pr.var_ref + PM_PRUNE_E), 1.0f);
    const float eg = PM_PRUNE_E * __builtin_amdgcn_rsqf(vr * vs);
    const float tt = 1.0f - cost_now;
    const float lhs = fma_(eg, 2.0f + eg, n2);
    const float rhs = (fma_(tt, tt, -PM_PRUNE_SLACK) * (1.0f - PM_PRUNE_E * __builtin_amdgcn_rcpf(vr))) * (1.0f - PM_PRUNE_E * __builtin_amdgcn_rcpf(vs));
    return cost_now < 1.0f && vr >= 2.0f * PM_PRUNE_E && vs >= 2.0f * PM_PRUNE_E && lhs <= rhs;
}

// The cost of a view from its three sums, the tail of pmCost (gipuma.cu:229-298), on 8-bit imagery: MAXCOST below the variance
// threshold, else 1 - NCC clamped to [0, MAXCOST].  Both variances are >= 1e-5 here and at most 255^2, so their product lies
// inside sqrt_rsq_exact's range by construction and the correctly rounded root needs no guard (and none of the six v_cndmask of
// the compiler's sqrtf, which the one-tap loop of pm_core.h keeps for float imagery).
DEVFN float ncc_cost(const PixelRef& pr, TapSums t) {
    t.src *= pr.inv_wsum;
    t.src_src *= pr.inv_wsum;
    t.ref_src *= pr.inv_wsum;
    const float var_src = t.src_src - t.src * t.src;
    if (var_src < 1e-5f) return TSAR_MAXCOST;
    const float covar = t.ref_src - pr.mean_ref * t.src;
    const float vrs = sqrt_rsq_exact(pr.var_ref * var_src);
    return fmaxf(0.0f, fminf(TSAR_MAXCOST, 1.0f - covar / vrs));
}
