// pm_tap_r5.h — the production tap loop: pmCost (gipuma.cu:229-298) of one source view for the scripts' window (--blocksize=11:
// radius 5, taps at {-5,-3,-1,1,3,5}^2, scripts/courtyard.sh:10-15) on 8-bit imagery (quad textures), given the hoisted reference
// terms of pm_core.h.  Both arithmetic modes run this one function, built from the per-tap pieces of pm_tap_common.h; included by
// pm_core.h.
//
// Template switches (the kernels' variant number V keeps naming them in profiles: 114 = none, 122 = D16, 250 = D16 + ROW,
// + TSAR_V_BUF = BUF):
//   STRICT  the oracle's values bit for bit: correctly rounded quotients (persp_divide_exact), min/max clamp, (w r) s, and the
//           oracle's summation order (window columns).  Fast mode: v_rcp_f32 + 2 multiplies, v_med3_f32 clamp, (w s) r.
//   ROW     fast mode only: the window is walked row by row (six taps along x per trip).  A row's six taps of one lane fall into
//           one or two cache lines of the source texture, so where neighbouring lanes' footprints are unrelated (random planes:
//           init, the first sweep) the six gathers of a trip reuse the lines the first one brought into L1; -4 % converged,
//           -18..25 % on random planes.  Changes the summation order of the three tap sums, hence not in strict mode.
//   D16     the line's six reference texels are loaded with ds_read_u16_d16_hi straight into the upper half of a register
//           (= their fp32 value, no convert).  gfx950 runs with SRAM ECC, where a D16 load writes the whole register;
//           tsar_create probes this once (pm_sweep.hip) and the library falls back to D16 = false if it does not hold.
//   BUF     the gathers as structured buffer loads (buffer_load_dword ... idxen) through a stride-4 resource descriptor: the texture
//           addresser scales the element index, the per-tap shift goes away (-0.65 % on a converged launch, +4 ms on the first
//           sweep of a view, so the launcher uses it from the second sweep on in fast mode, the third in strict mode).  No compiler builtin reaches idxen: the loads are
//           issued by asm and their vmcnt waits are written out (buffer_gather, pm_tap_common.h; the waits below).
//   MIX     with BUF, fast mode: the gather reads 8 bytes from the view's half-float difference texture (t00, t10 - t00, t01 - t00,
//           t11 - t10 - t01 + t00; plane_kernels.hip build_dquad_kernel) and the fast arithmetic's blend (t00 + ax d1) + ay (d2 + ax d3)
//           is two v_fma_mix_f32 on the halfs in place and one v_fma_f32 (blend_dquad, pm_tap_common.h): no byte converts, no subtractions
//           (-9 issue units of a tap's 34).  Same values bit for bit as the byte-texture form of that blend, which the global-load
//           launches (init, the first two sweeps) keep.
//           (Strict mode can form the reference's blend from the same halfs bit-exactly — t10 - t00 is stored, t01 and t11 - t01 are
//           one exact v_fma_mix_f32 each, -4.5 issue units per tap — and was measured SLOWER, 48.1 -> 51.6 ms per launch: its
//           column-order walk touches six texture rows per lane and trip, and 8-byte entries double that footprint.  Not kept.)
// Always on (each measured, profiles/r01-r02): a line (six taps) per trip in three explicit phases — all six tap positions, all six
// gathers, then unpack / blend / accumulate — so that six gathers are in flight per wave whatever the scheduler decides; the view's
// quad-texture base (border offset folded in) pinned in SGPRs for the whole view; the line's six weights loaded at the top of the
// line with its reference texels; s_setprio 3 while a wave computes tap positions and issues gathers, 0 while it blends; a
// clamp-free loop for waves whose windows project inside the source image.
// BLK: threads per workgroup = stride, in floats, between the weights of consecutive taps of one thread ([tap][thread]).
#pragma once

// the partial-window checks (PRUNE below) run after lines PM_PRUNE_FIRST_LINE .. PM_PRUNE_LAST_LINE of the six
#define PM_PRUNE_FIRST_LINE 2
#define PM_PRUNE_LAST_LINE 4

// DIAG (experiments build only, WRONG RESULTS by construction; the ceilings of profiles/r04): 1 = the MIX body with every gather
// removed (the tap's halfs are synthesised from its element index: the VALU floor of the shipping body), 2 = every gather replaced
// by an 8-byte LDS read at a per-lane address (ds_read_b64: the instruction mix of source patches staged in LDS, before any staging).
// PRUNE (variant bit TSAR_V_PRUNE; fast mode, ROW + D16 only): while vp.on, the view is left after its second, third or fourth line
// when the partial-window bound (prune_proven, pm_tap_common.h) shows for EVERY active lane that this loop's own result would be
// >= the lane's cost_now; vp.skipped then tells the caller that the returned MAXCOST stands for "not below cost_now".  The three
// reference sums over the lines walked so far are formed from LDS at each check (no register lives across a line for them: the
// kernels have none to spare).  The decision is wave-uniform, like the clamp-free one.
// PAIR (variant bit TSAR_V_PAIR; the plain fast form only: ROW + D16, global loads on the byte texture, no pruning): a row's six taps
// are 2 px apart in the reference and land ~2 entries apart in the source texture, so the 16 bytes from tap j's entry on hold tap
// j + 1's entry for ~87 % of lanes on random planes (tools/pair_gather_census.py).  Taps 0, 2, 4 are gathered as 16 bytes
// (global_load_dwordx4, 4-byte aligned); a lane whose k = lin[j + 1] - lin[j] is in 0..3 takes dword k of them for tap j + 1, the
// others gather tap j + 1 as before, after the three wide loads.  The test is on the element indices alone and every tap's entry
// reaches blend_quad unchanged and in the same order: the same bits, with ~38 % fewer L1 look-ups where every lane is on its own
// line (init, the first sweep of a view).
// DIAG 3 (experiments build only, WRONG RESULTS): PAIR with the uncovered lanes' gathers left out: the ceiling of the paired loop.
// RING (variant bit TSAR_V_RING; the MIX form only, with or without PRUNE): the unrolled clamp-free walk as a ring of six taps.  The
// three-phase line issues six gathers and waits at once for the oldest; the ring issues line 0's six, then per tap t = 0..29 waits
// for tap t alone (vmcnt(5): gathers return in order), blends and accumulates it, computes the position of tap t + 6 and issues its
// gather into the slot tap t has just left; taps 30..35 drain with the counts 5..0.  Five or six gathers are in flight from the
// first tap of a view to its thirtieth.  The same calls with the same operands in the same order per tap, and the taps enter the three
// sums in the same order: the same bits.  A line's base is dead once its sixth position exists, so the next line's takes its
// registers; a line's nine LDS loads are issued at the line's first blend (their registers hold the previous line's until then).
// The ring drains at the end of a view: the next view's homography is not known earlier.  Every other loop is as it was.
template <bool STRICT, bool ROW, bool D16, bool BUF, bool MIX, int BLK, int DIAG = 0, bool PRUNE = false, bool PAIR = false, bool RING = false>
DEVFN float view_cost_r5(const DevScene* __restrict__ sc, const DevView& vw, const unsigned short* tile, int tw, int own, const float* wts,
                         const PixelRef& pr, int x, int y, const float4& n4, ViewPrune* vp = nullptr) {
    static_assert(!RING || (MIX && ROW && D16 && DIAG == 0 && !PAIR), "the ring is a form of the unrolled difference-texture walk");
    static_assert(!(STRICT && ROW), "the row-wise walk changes the summation order: fast mode only");
    static_assert(!PRUNE || (ROW && D16 && !STRICT && DIAG == 0), "the partial-window bound is written for the fast row-wise loop");
    static_assert(!MIX || (BUF && !STRICT), "the half-float difference texture serves the fast arithmetic's blend through buffer loads");
    static_assert(!PAIR || (ROW && D16 && !STRICT && !BUF && !MIX && !PRUNE), "the paired gathers are written for the plain fast row-wise loop on the byte texture");
    static_assert(DIAG != 3 || PAIR, "DIAG 3 is a form of the paired loop");
    const int w = sc->w, h = sc->h, qp = sc->quad_pitch;
    const int qorg = quad_border_bytes(qp);
    float H[9];
    if (STRICT) plane_homography(sc->ref, vw, n4, H, sc->k_sparse != 0);
    else plane_homography_fast(sc->ref, vw, n4, H);
    float sum_src = 0.f, sum_src_src = 0.f, sum_ref_src = 0.f;
    // Clamp-free loop: if every active lane's window lands inside the source image with Z > 0, no tap needs the clamp and the wave
    // runs a tap loop without it.  Wave-uniform decision, identical results.  Strict mode decides on the four corner taps
    // (the window then maps into the convex quadrilateral they span).  The texture is addressed from entry (1, 1) with an unsigned offset, so the
    // clamp-free loop must never see floor(u) = -1: both tests keep a pixel of margin (rounding moves a tap by ~1e-4 pixel).
    bool need_clamp;
    if (!STRICT) {
        // Fast mode: the same decision from the window's CENTRE and a bound on its extent — one reciprocal instead of four and ~20
        // instructions fewer per hypothesis and view.  With (Xc, Yc, Zc) the centre's homogeneous position, a tap is at
        // (Xc + dX, Yc + dY, Zc + dZ) with |dX| <= a = 5 (|H0| + |H1|), |dY| <= b = 5 (|H3| + |H4|), |dZ| <= c = 5 (|H6| + |H7|); for
        // Zmin = Zc - c > 0 every tap has Z >= Zmin and |u_tap - u_c| = |dX Zc - Xc dZ| / (Z_tap Zc) <= (a Zc + |Xc| c) / (Zmin Zc).
        // The window is inside when the centre keeps that distance (+ the pixel of margin the unsigned addressing needs, + half a
        // pixel for the rounding of this bound itself: its terms are evaluated to ~1e-6 relative on distances of a few pixels and
        // positions of a few thousand).  More conservative than the corner test by the slack of the bound: waves whose windows come
        // within ~2 extents of the border take the clamp loop, which returns the same bits.
        float Xc, Yc, Zc;
        pixel_homogeneous(H, (float)x, (float)y, Xc, Yc, Zc);
        const float a = fabsf(H[0]) + fabsf(H[1]), b = fabsf(H[3]) + fabsf(H[4]), c = fabsf(H[6]) + fabsf(H[7]);
        const float Zmin = fma_(-5.0f, c, Zc);
        const float r = __builtin_amdgcn_rcpf(Zmin * Zc);
        const float r5 = 5.0f * r, rc = Zmin * r;                 // 5 / (Zmin Zc), 1 / Zc
        const float du = fma_(a, Zc, fabsf(Xc) * c) * r5, dv = fma_(b, Zc, fabsf(Yc) * c) * r5;
        const float uc = Xc * rc, vc = Yc * rc;
        const bool inside = Zmin > 0.0f && fminf(uc - du, vc - dv) >= 1.5f && uc + du <= (float)(w - 1) - 1.5f && vc + dv <= (float)(h - 1) - 1.5f;
        need_clamp = !__all(inside);
    } else {
        bool inside = true;
        float zmin = __builtin_inff(), zmax = 0.0f;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            float X, Y, Z;
            pixel_homogeneous(H, (float)(x + ((c & 1) ? 5 : -5)), (float)(y + ((c & 2) ? 5 : -5)), X, Y, Z);
            const float rz = __builtin_amdgcn_rcpf(Z);
            const float u = X * rz, v = Y * rz;
            inside = inside && Z > 0.0f && u >= 1.0f && u <= (float)(w - 1) - 1.0f && v >= 1.0f && v <= (float)(h - 1) - 1.0f;
            zmin = fminf(zmin, Z); zmax = fmaxf(zmax, Z);
        }
        // The clamp-free loop of strict mode also drops the per-tap operand guard of persp_divide_exact, so "inside" must imply
        // that X, Y, Z of EVERY tap lie in [2^-20, 2^38].  With cm >= |x|, |y| of any tap: Z is affine in the tap position, so at
        // every tap it lies between the corner values up to the rounding of its three-term evaluation, dZ <= 3 * 2^-24 * sz with
        // sz = (|H6| + |H7|) cm + |H8|.  sz cm <= 2^19 zmin bounds dZ / Z by 3 * 2^-5 / cm <= 1.2 % (cm >= 8), so Z stays in
        // [2^-19, 2^18] for zmin >= 2^-18, zmax <= 2^17.  u = X / Z of a tap lies in the hull of the corners' true u (Z > 0: the
        // map is projective), which are >= 1 - 0.15: computed u >= 1, and a computed corner is off by u dZ / Z <= cm * 3 * 2^-24
        // * 2^19 / cm = 0.094 plus dX / Z <= 3 * 2^-24 * sx / zmin <= 0.047 for sx = (|H0| + |H1|) cm + |H2| <= 2^18 zmin.  Hence
        // X >= 0.8 zmin >= 2^-20 and |X| <= sx <= 2^35; the same for Y.
        const float cm = (float)(max(w, h) + 32);
        const float sz = fma_(fabsf(H[6]) + fabsf(H[7]), cm, fabsf(H[8]));
        const float sx = fma_(fabsf(H[0]) + fabsf(H[1]), cm, fabsf(H[2]));
        const float sy = fma_(fabsf(H[3]) + fabsf(H[4]), cm, fabsf(H[5]));
        inside = inside && zmin >= 3.814697265625e-06f && zmax <= 131072.0f && sz * cm <= 524288.0f * zmin && fmaxf(sx, sy) <= 262144.0f * zmin;
        need_clamp = !__all(inside);
    }
    // the view's quad texture: pinned base for the global loads, descriptor for the buffer-load forms (which address through it alone:
    // no second pointer load per view)
    uint32_t qb_lo = 0, qb_hi = 0;
    u32x4s rsrc = {0u, 0u, 0u, 0u};
    if (!BUF) pin_quad_base(quad_origin<false>(vw, qorg), qb_lo, qb_hi);
    else rsrc = quad_descriptor<MIX>(quad_origin<MIX>(vw, qorg), h + 1, qp);
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    // one line of the window: `i` is the column offset (the row offset when ROW) and the six taps run along the other axis
    // unr_tag: the caller's loop over the six lines is fully unrolled (`i` is a constant after inlining): the line's LDS loads then
    // take their line offset as an immediate from loop-invariant base addresses instead of two address additions per line
    auto line6 = [&](int i, auto clamp_tag, auto unr_tag) {
        constexpr bool CLAMP = decltype(clamp_tag)::value;
        constexpr bool UNR = decltype(unr_tag)::value;
        static_assert(!UNR || (ROW && D16), "the unrolled form is written for the row-wise walk with D16 window loads");
        const float xi = (float)((ROW ? y : x) + i);
        float bx, by, bz;
        tap_line_base<STRICT, ROW>(H, xi, bx, by, bz);
        const int line = (i + 5) >> 1;                // 0..5: which column (or row) this is
        float rcol[6];
        f32x2 wcol[3];
        {
            // the line's six weights, [tap][thread] layout, tap = 6 * column + row: taps are BLK floats apart = BLK / 64 units of
            // ds_read2st64's 256-byte stride; along a row consecutive taps are 6 taps apart
            constexpr int U = BLK / 64, S = ROW ? 6 : 1;
            const uint32_t wa = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)(wts + (UNR ? 0 : (ROW ? line : 6 * line) * BLK));
#pragma unroll
            for (int k = 0; k < 3; k++)
                asm("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(wcol[k]) : "v"(wa), "n"(2 * U * S * k + (UNR ? U * line : 0)), "n"(2 * U * S * k + U * S + (UNR ? U * line : 0)), "v"(bz));
        }
        if (D16) {
            // The loads are invisible to the compiler's waitcnt bookkeeping, which stays correct (LDS returns in order, its own
            // waits only get more conservative); the wait for these six is the asm before their first use below.  Neither asm is
            // volatile (a volatile one fences the gathers and serialises the taps); the unused bz operand keeps the loads inside
            // the line loop instead of being hoisted out of the view and hypothesis loops into 36 live registers.
            // (UNR: base = the window's first row; the window is PM_RW + 10 texels wide in every kernel that runs this loop)
            const uint32_t a0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned short*)(UNR ? tile + own - 5 * tw - 5 : ROW ? tile + own + i * tw - 5 : tile + own + i - 5 * tw);
#pragma unroll
            for (int jj = 0; jj < 6; jj++)
                asm("ds_read_u16_d16_hi %0, %1 offset:%2" : "=v"(rcol[jj]) : "v"(a0), "n"((ROW ? jj * 4 : jj * 2 * (PM_RW + 10) * 2) + (UNR ? line * 2 * (PM_RW + 10) * 2 : 0)), "v"(bz));
        }
        float ax[6], ay[6];
        uint32_t q[6];
        uint64_t q2[6];                              // MIX: the tap's four halfs
        int linv[6];                                 // PAIR: the taps' element indices
        u32x4s wide[3];                              // PAIR: the 16 bytes from taps 0, 2, 4 on
        __builtin_amdgcn_s_setprio(3);               // a wave computing tap positions / issuing gathers goes ahead of waves that are blending
#pragma unroll
        for (int jj = 0; jj < 6; jj++) {                        // phase 1: tap positions -> element index; phase 2: gathers
            const float yj = (float)((ROW ? x : y) + 2 * jj - 5);
            float X, Y, Z;
            tap_homogeneous<STRICT, ROW>(H, yj, bx, by, bz, X, Y, Z);
            const float uhi = (float)(w - 1), vhi = (float)(h - 1);
            int lin;
            tap_position<STRICT, CLAMP>(X, Y, Z, uhi, vhi, qp, ax[jj], ay[jj], lin);
            if (MIX && DIAG == 1) {
                q2[jj] = ((uint64_t)(uint32_t)~lin << 32) | (uint32_t)lin;      // (two different dwords: identical ones would let the compiler merge the blend's two mixed FMAs)
            } else if (MIX && DIAG == 2) {
                uint32_t la;                                    // inside the workgroup's first 32 KiB of LDS, lanes 16 bytes apart like a staged patch
                asm("v_bfe_u32 %0, %1, 0, 12" : "=v"(la) : "v"(lin));
                asm volatile("ds_read_b64 %0, %1" : "=v"(q2[jj]) : "v"(la << 3));
            } else if (MIX) {
                q2[jj] = buffer_gather<true>(lin, rsrc);
            } else if (BUF) {
                q[jj] = buffer_gather<false>(lin, rsrc);
            } else if constexpr (PAIR) {
                // Reading past the last entry: the base is entry (1, 1) of a texture of (h + 2) rows of qp = w + 2 entries
                // (tsar_api.hip: dev_alloc of (w + 2) (h + 2) dwords), and lin <= (h - 1) qp + (w - 1) (tap_position: iu <= w - 1,
                // iv <= h - 1), i.e. entry h qp + w of the allocation at most.  The 16 bytes end with entry h qp + w + 3 =
                // (h + 1) qp + 1, inside the border row below the image: no padding is needed.  (The bound on lin is tap_position's
                // clamp range [0, w - 1] x [0, h - 1], pm_tap_common.h "Clamp range", and the clamp-free loop's inside test above.)
                linv[jj] = lin;
                if ((jj & 1) == 0) wide[jj >> 1] = *(global_u32x4_a4_ptr)((const char __attribute__((address_space(1)))*)(uintptr_t)(((uint64_t)qb_hi << 32) | qb_lo) + ((uint32_t)lin << 2));
            } else {                                            // base already holds the border offset: the byte offset is a plain shift
                const uint32_t off2 = (uint32_t)lin << 2;
                q[jj] = *(global_u32_ptr)((const char __attribute__((address_space(1)))*)(uintptr_t)(((uint64_t)qb_hi << 32) | qb_lo) + off2);
            }
        }
        if constexpr (PAIR && DIAG != 3) {
            // the lanes whose odd tap is not among the anchor's four entries: today's gather, behind the three wide ones
#pragma unroll
            for (int jj = 1; jj < 6; jj += 2)
                if ((uint32_t)(linv[jj] - linv[jj - 1]) > 3u)
                    q[jj] = *(global_u32_ptr)((const char __attribute__((address_space(1)))*)(uintptr_t)(((uint64_t)qb_hi << 32) | qb_lo) + ((uint32_t)linv[jj] << 2));
        }
        __builtin_amdgcn_sched_barrier(0);           // nothing of phase 3 may move above the last gather
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int jj = 0; jj < 6; jj++) {                        // phase 3: unpack, blend, accumulate
            if (MIX && DIAG == 1) {
            } else if (MIX && DIAG == 2) {                      // LDS returns in order: tap jj has 5 - jj reads behind it
                if (jj == 0) asm("s_waitcnt lgkmcnt(5)" : "+v"(q2[0]), "+v"(rcol[0]), "+v"(rcol[1]), "+v"(rcol[2]), "+v"(rcol[3]), "+v"(rcol[4]), "+v"(rcol[5]),
                                 "+v"(wcol[0]), "+v"(wcol[1]), "+v"(wcol[2]) : "v"(q2[5]));
                else asm("s_waitcnt lgkmcnt(%2)" : "+v"(q2[jj]), "+v"(sum_src_src) : "n"(5 - jj), "v"(q2[5]));
            } else if (MIX) {
                if (jj == 0) asm("s_waitcnt vmcnt(5)" : "+v"(q2[0]) : "v"(q2[5]));
                if (jj == 1) asm("s_waitcnt vmcnt(4)" : "+v"(q2[1]), "+v"(sum_src_src) : "v"(q2[5]));
                if (jj == 2) asm("s_waitcnt vmcnt(3)" : "+v"(q2[2]), "+v"(sum_src_src) : "v"(q2[5]));
                if (jj == 3) asm("s_waitcnt vmcnt(2)" : "+v"(q2[3]), "+v"(sum_src_src) : "v"(q2[5]));
                if (jj == 4) asm("s_waitcnt vmcnt(1)" : "+v"(q2[4]), "+v"(sum_src_src) : "v"(q2[5]));
                if (jj == 5) asm("s_waitcnt vmcnt(0)" : "+v"(q2[5]), "+v"(sum_src_src));
            } else if (BUF) {
                // the asm-issued gathers return in order: tap jj has 5 - jj behind it.  Not volatile (a volatile wait is
                // scheduled with the loads, ahead of every blend); the q[5] input keeps each wait behind the issue of the last load, the
                // accumulator behind the previous tap's blend
                if (jj == 0) asm("s_waitcnt vmcnt(5)" : "+v"(q[0]) : "v"(q[5]));
                if (jj == 1) asm("s_waitcnt vmcnt(4)" : "+v"(q[1]), "+v"(sum_src_src) : "v"(q[5]));
                if (jj == 2) asm("s_waitcnt vmcnt(3)" : "+v"(q[2]), "+v"(sum_src_src) : "v"(q[5]));
                if (jj == 3) asm("s_waitcnt vmcnt(2)" : "+v"(q[3]), "+v"(sum_src_src) : "v"(q[5]));
                if (jj == 4) asm("s_waitcnt vmcnt(1)" : "+v"(q[4]), "+v"(sum_src_src) : "v"(q[5]));
                if (jj == 5) asm("s_waitcnt vmcnt(0)" : "+v"(q[5]), "+v"(sum_src_src));
            }
            if constexpr (PAIR) {
                // selected as each pair returns: the anchor's four dwords die with its odd tap
                if ((jj & 1) == 0) q[jj] = wide[jj >> 1].x;
                else {
                    const uint32_t k = (uint32_t)(linv[jj] - linv[jj - 1]);
                    if (DIAG == 3 || k <= 3u) q[jj] = pick_dword(wide[jj >> 1], k);
                }
            }
            float s;
            if (MIX) s = blend_dquad(q2[jj], ax[jj], ay[jj]);
            else s = blend_quad<!STRICT>(q[jj], ax[jj], ay[jj]);
            // one wait per line, at its first tap: every LDS load of the line (six texels when they are D16 loads, three weight
            // pairs) was issued before the gathers, in order, and has long returned when the first gather does
            if (jj == 0 && DIAG != 2) {
                if (D16)
                    asm("s_waitcnt lgkmcnt(0)" : "+v"(rcol[0]), "+v"(rcol[1]), "+v"(rcol[2]), "+v"(rcol[3]), "+v"(rcol[4]), "+v"(rcol[5]),
                        "+v"(wcol[0]), "+v"(wcol[1]), "+v"(wcol[2]), "+v"(s));
                else
                    asm("s_waitcnt lgkmcnt(0)" : "+v"(wcol[0]), "+v"(wcol[1]), "+v"(wcol[2]), "+v"(s));
            }
            const float r = D16 ? rcol[jj] : tile_value(ROW ? tile[own + i * tw + (2 * jj - 5)] : tile[own + (2 * jj - 5) * tw + i]);
            const float wt = wcol[jj >> 1][jj & 1];
            const TapSums t = tap_accumulate<STRICT>(TapSums{sum_src, sum_src_src, sum_ref_src}, wt, r, s);
            sum_src = t.src; sum_src_src = t.src_src; sum_ref_src = t.ref_src;
        }
    };
    // after line `line` (0-based): true = every active lane is proven, leave the view
    auto pruned = [&](int line) {
        if constexpr (PRUNE) {
            if (vp->on && line >= PM_PRUNE_FIRST_LINE - 1 && line < PM_PRUNE_LAST_LINE) {
                float pa_w = 0.f, pa_r = 0.f, pa_rr = 0.f;
#pragma unroll 1
                for (int l = 0; l <= line; l++) {
#pragma unroll
                    for (int jj = 0; jj < 6; jj++) {
                        const float wt = wts[(6 * jj + l) * BLK], r = tile_value(tile[own + (2 * l - 5) * tw + (2 * jj - 5)]);
                        const float wr = wt * r;
                        pa_w += wt;
                        pa_r += wr;
                        pa_rr = fma_(wr, r, pa_rr);
                    }
                }
                if (__all(prune_proven(TapSums{sum_src, sum_src_src, sum_ref_src}, pa_w, pa_r, pa_rr, pr, vp->cost_now))) { vp->skipped = true; return true; }
            }
        }
        return false;
    };
    if (need_clamp) {
#pragma unroll 1
        for (int i = -5; i <= 5; i += 2) { line6(i, std::true_type(), std::false_type()); if (pruned((i + 5) >> 1)) return TSAR_MAXCOST; }
    } else if (MIX && !(PRUNE && vp->on)) {      // (a checked hypothesis walks the rolled loop below: the checks sit between its trips)
        // the converged launches' hot path: the six lines unrolled (-6 VALU and the loop's scalar bookkeeping per line; +0.65 %
        // Mpix/s, profiles/r04/ab_unrolled_lines)
        if constexpr (RING) {
            constexpr int U = BLK / 64;
            const float uhi = (float)(w - 1), vhi = (float)(h - 1);
            const uint32_t wa = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) float*)wts;
            const uint32_t a0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned short*)(tile + own - 5 * tw - 5);
            float bx, by, bz, ax[6], ay[6], rcol[6];
            f32x2 wcol[3];
            uint64_t q2[6];
            __builtin_amdgcn_s_setprio(2);               // constant: the ring has no phases (none: +1 ms per view, 1 / 2 / 3 alike: profiles/ring)
            tap_line_base<false, true>(H, (float)(y - 5), bx, by, bz);
#pragma unroll
            for (int jj = 0; jj < 6; jj++) {                    // prologue: line 0's positions and gathers
                float X, Y, Z;
                int lin;
                tap_homogeneous<false, true>(H, (float)(x + 2 * jj - 5), bx, by, bz, X, Y, Z);
                tap_position<false, false>(X, Y, Z, uhi, vhi, qp, ax[jj], ay[jj], lin);
                q2[jj] = buffer_gather<true>(lin, rsrc);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int t = 0; t < 36; t++) {
                const int line = t / 6, jj = t % 6;
                if (jj == 0) {
                    // the line's weights and reference texels (line6's loads, unrolled form); the unused operand keeps them behind the
                    // previous line's last tap, whose registers they take, and inside the view loop
                    const float dep = line == 0 ? bz : sum_ref_src;
#pragma unroll
                    for (int k = 0; k < 3; k++)
                        asm("ds_read2st64_b32 %0, %1 offset0:%2 offset1:%3" : "=v"(wcol[k]) : "v"(wa), "n"(2 * U * 6 * k + U * line), "n"(2 * U * 6 * k + U * 6 + U * line), "v"(dep));
#pragma unroll
                    for (int k = 0; k < 6; k++)
                        asm("ds_read_u16_d16_hi %0, %1 offset:%2" : "=v"(rcol[k]) : "v"(a0), "n"(k * 4 + line * 2 * (PM_RW + 10) * 2), "v"(dep));
                }
                // tap t is the oldest gather in flight: five younger ones behind it until tap 30, then 35 - t.  The input is the
                // youngest gather issued (each wait stays behind it), the accumulator keeps the wait behind the previous tap
                if (t == 0) asm("s_waitcnt vmcnt(5)" : "+v"(q2[0]) : "v"(q2[5]));
                else if (t < 35) asm("s_waitcnt vmcnt(%2)" : "+v"(q2[jj]), "+v"(sum_src_src) : "n"(t < 30 ? 5 : 35 - t), "v"(q2[t < 30 ? (jj + 5) % 6 : 5]));
                else asm("s_waitcnt vmcnt(0)" : "+v"(q2[5]), "+v"(sum_src_src));
                float s = blend_dquad(q2[jj], ax[jj], ay[jj]);
                if (jj == 0)
                    asm("s_waitcnt lgkmcnt(0)" : "+v"(rcol[0]), "+v"(rcol[1]), "+v"(rcol[2]), "+v"(rcol[3]), "+v"(rcol[4]), "+v"(rcol[5]),
                        "+v"(wcol[0]), "+v"(wcol[1]), "+v"(wcol[2]), "+v"(s));
                const TapSums ts = tap_accumulate<false>(TapSums{sum_src, sum_src_src, sum_ref_src}, wcol[jj >> 1][jj & 1], rcol[jj], s);
                sum_src = ts.src; sum_src_src = ts.src_src; sum_ref_src = ts.ref_src;
                if (t < 30) {                                   // tap t + 6 into the slot tap t has left
                    if (jj == 0) tap_line_base<false, true>(H, (float)(y + 2 * (line + 1) - 5), bx, by, bz);
                    float X, Y, Z;
                    int lin;
                    tap_homogeneous<false, true>(H, (float)(x + 2 * jj - 5), bx, by, bz, X, Y, Z);
                    tap_position<false, false>(X, Y, Z, uhi, vhi, qp, ax[jj], ay[jj], lin);
                    q2[jj] = buffer_gather<true>(lin, rsrc);
                }
                __builtin_amdgcn_sched_barrier(0);              // one tap at a time: the gathers stay one per tap
            }
            __builtin_amdgcn_s_setprio(0);
        } else {
#pragma unroll
            for (int i = -5; i <= 5; i += 2) line6(i, std::false_type(), std::bool_constant<MIX>());
        }
    } else {
#pragma unroll 1
        for (int i = -5; i <= 5; i += 2) { line6(i, std::false_type(), std::false_type()); if (pruned((i + 5) >> 1)) return TSAR_MAXCOST; }
    }
    return ncc_cost(pr, TapSums{sum_src, sum_src_src, sum_ref_src});
}

// The variant numbers the production kernels are instantiated with (and which profiles name): bits 1, 4, 5, 6 always set.
// + TSAR_V_MIX (with 250 | TSAR_V_BUF): MIX
// + 4194304 / + 8388608 (experiments build): DIAG 1 / 2 of the MIX body
__host__ __device__ constexpr bool r5_diag_variant(int V) { return V == (250 | TSAR_V_BUF | TSAR_V_MIX | 4194304) || V == (250 | TSAR_V_BUF | TSAR_V_MIX | 8388608); }
// + TSAR_V_PRUNE (with 250 and its BUF / MIX forms): PRUNE; masked off before this test, like TSAR_V_GEOM
// + TSAR_V_PAIR (with 250 alone): PAIR; masked off likewise (+ 4194304, experiments build: DIAG 3)
__host__ __device__ constexpr bool r5_production_variant(int V) { return V == 114 || V == 122 || V == 250 || V == (114 | TSAR_V_BUF) || V == (122 | TSAR_V_BUF) || V == (250 | TSAR_V_BUF) || V == (250 | TSAR_V_BUF | TSAR_V_MIX); }
