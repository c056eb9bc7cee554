// pm_core_lut.h — the matching cost for ANY window (box 1..63, square or not) on 8-bit imagery: the production tap loop
// (view_cost_r5, pm_tap_r5.h) is written for the scripts' box 11; every other box — the reference binary's own
// default is 19 (algorithmparameters.h:25) — used to fall to a one-tap-at-a-time loop whose S hoisted weights per thread
// (100 KiB of LDS per workgroup at box 19) left one wave per SIMD.  Included by pm_core.h.
//
// What differs from the box-11 loop:
//   * weights.  exp(-sqrt(i^2 + j^2) / 50 - |r - centre| / 18) (gipuma.cu:268) takes its second argument from the integers
//     0..255 on 8-bit imagery and its first from the few distinct tap distances of the window (14 at box 19), so the
//     workgroup keeps ONE table [distance class][0..255] in LDS — evaluated with the same expression, so the values are the
//     oracle's bit for bit — and a tap looks its weight up with |r - centre| as the index.  LDS per workgroup: 15 KiB at box 19
//     instead of 100, occupancy is bounded by registers again (four waves per SIMD).  Cost: three VALU instructions and one
//     LDS gather per tap.
//   * shape.  A line of the window (a row in fast mode, a column — the oracle's summation order — in strict mode) is walked
//     in chunks of CH = 4, 5 or 6 taps, each chunk in the three phases of the box-11 loop (positions, gathers, blend), CH
//     chosen by the host so that the line length rounds up with the fewest padding slots.  A padding slot repeats the line's
//     last tap with a weight from the table's all-zero row: it adds +0 to the three sums, so the result does not depend on CH.
#pragma once

// The table: (classes + 1) rows of 256 floats at the start of the workgroup's LDS.
template <int BLK>
DEVFN void build_weight_lut(const DevScene* __restrict__ sc, float* lut) {
    const int nc = sc->lut_classes;
    for (int k = threadIdx.x; k < (nc + 1) * 256; k += BLK) {
        const int cls = k >> 8;
        float wt = 0.0f;
        if (cls < nc) {
            const float sd = sqrtf((float)sc->lut_d2[cls]);
            const float cd = (float)(k & 255);
            wt = tsar_expf(-sd / 50.0f - cd / 18.0f);      // the expression of hoist_reference (pm_core.h), gipuma.cu:268
        }
        lut[k] = wt;
    }
}

DEVFN float lut_weight(const float* lut, uint32_t row_bytes, float r, float cen) {
    const int idx = (int)fabsf(r - cen);                    // integer-valued: texels are 0..255
    return *(const float*)((const char*)lut + row_bytes + (uint32_t)idx * 4u);
}

// hoist_reference (pm_core.h) with the weights read from the table; the oracle's tap order (columns).
DEVFN PixelRef hoist_reference_lut(const DevScene* __restrict__ sc, const unsigned short* tile, int tw, int own, const float* lut) {
    const int hr = sc->hrad, vr = sc->vrad;
    const bool rowm = sc->lut_row_major != 0;
    const int pt = sc->lut_pad_taps;
    const float cen = tile_value(tile[own]);
    float sum_ref = 0.f, sum_ref_ref = 0.f, wsum = 0.f;
    for (int ii = 0; ii <= hr; ii++) {
        const int i = 2 * ii - hr;
        for (int jj = 0; jj <= vr; jj++) {
            const int j = 2 * jj - vr;
            const float r = tile_value(tile[own + j * tw + i]);
            const float wt = lut_weight(lut, rowm ? sc->tap_row[jj * pt + ii] : sc->tap_row[ii * pt + jj], r, cen);
            const float wr = wt * r;
            sum_ref += wr;
            sum_ref_ref = fma_(wr, r, sum_ref_ref);
            wsum += wt;
        }
    }
    return pixel_ref_from_sums(sum_ref, sum_ref_ref, 1.0f / wsum);
}

// pmCost (gipuma.cu:229-298) for one source view, any window, 8-bit quad textures.
// Fast mode (rows): the window of the workgroup is staged with one extra row (LUT_TILE_PAD_ROWS), so that the padding slots of a
// row's last chunk may read the texels that follow the row (finite values, zero weight) with immediate offsets.
#define LUT_TILE_PAD_ROWS 1
// The chunk's D16 window loads (issued by asm, invisible to the compiler's counters) have returned.  `after`: the byte offset of
// the chunk's last gather — an input, so that the wait cannot be scheduled above the tap-position arithmetic.
template <int CH>
DEVFN void lut_wait_lds(float (&r)[CH], uint32_t after) {
    if constexpr (CH == 4) asm("s_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]) : "v"(after));
    else if constexpr (CH == 5) asm("s_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]) : "v"(after));
    else asm("s_waitcnt lgkmcnt(0)" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]) : "v"(after));
}
template <bool STRICT, int CH, bool BUF = false, bool MIX = false>
DEVFN float view_cost_lut(const DevScene* __restrict__ sc, const DevView& vw, const unsigned short* tile, int tw, int own, const float* lut,
                          const PixelRef& pr, int x, int y, const float4& n4) {
    constexpr bool ROW = !STRICT;                           // fast mode walks window rows (pm_tap_r5.h ROW)
    const int hr = sc->hrad, vr = sc->vrad;
    const int rt = ROW ? hr : vr, rl = ROW ? vr : hr;       // radius along / across the lines
    const int w = sc->w, h = sc->h, qp = sc->quad_pitch;
    float H[9];
    if (STRICT) plane_homography(sc->ref, vw, n4, H, sc->k_sparse != 0);
    else plane_homography_fast(sc->ref, vw, n4, H);
    // clamp-free loop when the four corner taps of every active lane land inside the source image with Z > 0 and a pixel of
    // margin (pm_tap_r5.h): wave-uniform, identical results.  In fast mode the padding slots of a row's last chunk
    // are sampled where they fall, beyond the window's right edge: the corners include them.
    const int xr = ROW ? 2 * (sc->lut_pad_taps - 1) - hr : hr;
    bool inside = true;
    float zmin = __builtin_inff(), zmax = 0.0f;
    if (!STRICT) {
        // fast mode: the decision from the window's centre and a bound on its extent (derived in pm_tap_r5.h): one reciprocal instead of four.
        // |dx| <= max(hr, xr) (the padding slots reach further right than the window), |dy| <= vr
        const float ex = (float)max(hr, xr), ey = (float)vr;
        float Xc, Yc, Zc;
        pixel_homogeneous(H, (float)x, (float)y, Xc, Yc, Zc);
        const float a = fma_(ex, fabsf(H[0]), ey * fabsf(H[1])), b = fma_(ex, fabsf(H[3]), ey * fabsf(H[4])), c = fma_(ex, fabsf(H[6]), ey * fabsf(H[7]));
        const float Zmin = Zc - c;
        const float r = __builtin_amdgcn_rcpf(Zmin * Zc);
        const float rc = Zmin * r;                                  // 1 / Zc
        const float du = fma_(a, Zc, fabsf(Xc) * c) * r, dv = fma_(b, Zc, fabsf(Yc) * c) * r;
        const float uc = Xc * rc, vc = Yc * rc;
        inside = Zmin > 0.0f && fminf(uc - du, vc - dv) >= 1.5f && uc + du <= (float)(w - 1) - 1.5f && vc + dv <= (float)(h - 1) - 1.5f;
    } else
#pragma unroll
    for (int c = 0; c < 4; c++) {
        float X, Y, Z;
        pixel_homogeneous(H, (float)(x + ((c & 1) ? xr : -hr)), (float)(y + ((c & 2) ? vr : -vr)), X, Y, Z);
        const float rz = __builtin_amdgcn_rcpf(Z);
        const float u = X * rz, v = Y * rz;
        inside = inside && Z > 0.0f && u >= 1.0f && u <= (float)(w - 2) && v >= 1.0f && v <= (float)(h - 2);
        if (STRICT) { zmin = fminf(zmin, Z); zmax = fmaxf(zmax, Z); }
    }
    if (STRICT) {       // the clamp-free strict loop runs persp_divide_exact without its per-tap guard: the bounds are proved in pm_tap_r5.h
        const float cm = (float)(max(w, h) + 32);
        const float sz = fma_(fabsf(H[6]) + fabsf(H[7]), cm, fabsf(H[8]));
        const float sx = fma_(fabsf(H[0]) + fabsf(H[1]), cm, fabsf(H[2]));
        const float sy = fma_(fabsf(H[3]) + fabsf(H[4]), cm, fabsf(H[5]));
        inside = inside && zmin >= 3.814697265625e-06f && zmax <= 131072.0f && sz * cm <= 524288.0f * zmin && fmaxf(sx, sy) <= 262144.0f * zmin;
    }
    const bool need_clamp = !__all(inside);
    // the view's quad texture (pm_tap_common.h): the base pinned for the whole view; BUF (fast mode, from the second sweep of a run on)
    // / MIX the descriptor of the structured buffer loads
    static_assert(!MIX || (BUF && !STRICT), "the half-float difference texture serves the fast arithmetic's blend through buffer loads");
    uint32_t qb_lo, qb_hi;
    pin_quad_base(quad_origin<false>(vw, quad_border_bytes(qp)), qb_lo, qb_hi);
    u32x4s rsrc = {0u, 0u, 0u, 0u};
    if constexpr (MIX) rsrc = quad_descriptor<true>(quad_origin<true>(vw, quad_border_bytes(qp)), h + 1, qp);
    else if constexpr (BUF) rsrc = quad_descriptor<false>(((uint64_t)qb_hi << 32) | qb_lo, h + 1, qp);
    const float cen = tile_value(tile[own]);
    const float fa = (float)(ROW ? x : y), fl = (float)(ROW ? y : x);
    const float uhi = (float)(w - 1), vhi = (float)(h - 1);
    const bool q8 = (sc->flags & TSAR_FLAG_TEX_FILTER_8BIT) != 0;   // bilinear weights with 8 fractional bits (wave-uniform)
    float sum_src = 0.f, sum_src_src = 0.f, sum_ref_src = 0.f;
    // rows: the table rows of this chunk's taps (scalars, loaded while the previous chunk ran)
    auto chunk = [&](const unsigned short* trow, const uint32_t (&rows)[CH], int c0, float bx, float by, float bz, auto clamp_tag) {
        constexpr bool CLAMP = decltype(clamp_tag)::value;
        float r[CH], ax[CH], ay[CH], wv[CH];
        uint32_t q[CH], off_last = 0;
        uint64_t q2[CH];                                    // MIX: the tap's four halfs
        float yj0 = 0.f;
        if constexpr (ROW) {
            // the chunk's reference texels, each loaded into bits 31:16 of a register = its fp32 value (pm_tap_r5.h D16);
            // the wait for them is lut_wait_lds below, after the gathers are on their way
            const uint32_t a0 = (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) unsigned short*)(trow + 2 * c0);
#pragma unroll
            for (int jj = 0; jj < CH; jj++) asm("ds_read_u16_d16_hi %0, %1 offset:%2" : "=v"(r[jj]) : "v"(a0), "n"(jj * 4), "v"(bz));
            yj0 = fa + (float)(2 * c0 - rt);
        } else {
#pragma unroll
            for (int jj = 0; jj < CH; jj++) r[jj] = tile_value(trow[min(c0 + jj, rt) * 2 * tw]);
        }
        __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int jj = 0; jj < CH; jj++) {                   // phase 1: tap positions -> byte offsets; phase 2: gathers
            const float yj = ROW ? yj0 + (float)(2 * jj) : fa + (float)(2 * min(c0 + jj, rt) - rt);
            float X, Y, Z;
            tap_homogeneous<STRICT, ROW>(H, yj, bx, by, bz, X, Y, Z);
            int lin;
            tap_position<STRICT, CLAMP>(X, Y, Z, uhi, vhi, qp, ax[jj], ay[jj], lin);
            if constexpr (BUF) {
                off_last = (uint32_t)lin;
                if constexpr (MIX) q2[jj] = buffer_gather<true>(lin, rsrc);
                else q[jj] = buffer_gather<false>(lin, rsrc);
            } else {
                off_last = (uint32_t)lin << 2;
                q[jj] = *(global_u32_ptr)((const char __attribute__((address_space(1)))*)(uintptr_t)(((uint64_t)qb_hi << 32) | qb_lo) + off_last);
            }
        }
        if constexpr (ROW) lut_wait_lds<CH>(r, off_last);
#pragma unroll
        for (int jj = 0; jj < CH; jj++) wv[jj] = lut_weight(lut, rows[jj], r[jj], cen);
        if (q8) {                                           // one scalar branch per chunk; the oracle's rounding (sample_bilinear, pm_core.h)
#pragma unroll
            for (int jj = 0; jj < CH; jj++) {
                ax[jj] = rintf(ax[jj] * 256.0f) * 0.00390625f;
                ay[jj] = rintf(ay[jj] * 256.0f) * 0.00390625f;
            }
        }
        __builtin_amdgcn_sched_barrier(0);                  // nothing of phase 3 may move above the last gather
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int jj = 0; jj < CH; jj++) {                   // phase 3: unpack, blend, accumulate
            float s;
            if constexpr (MIX) {
                asm("s_waitcnt vmcnt(%3)" : "+v"(q2[jj]), "+v"(sum_src_src) : "v"(q2[CH - 1]), "n"(CH - 1 - jj));
                s = blend_dquad(q2[jj], ax[jj], ay[jj]);
            } else {
                if constexpr (BUF)      // the asm-issued gathers return in order: tap jj has CH - 1 - jj behind it; why the waits take these operands: pm_tap_r5.h, at its BUF waits
                    asm("s_waitcnt vmcnt(%3)" : "+v"(q[jj]), "+v"(sum_src_src) : "v"(q[CH - 1]), "n"(CH - 1 - jj));
                s = blend_quad<!STRICT>(q[jj], ax[jj], ay[jj]);
            }
            const TapSums t = tap_accumulate<STRICT>(TapSums{sum_src, sum_src_src, sum_ref_src}, wv[jj], r[jj], s);
            sum_src = t.src; sum_src_src = t.src_src; sum_ref_src = t.ref_src;
        }
    };
    auto lines = [&](auto clamp_tag) {
        const uint32_t* rp = sc->tap_row;                   // walked linearly: chunks are consecutive in the table
        uint32_t rows[CH];
#pragma unroll
        for (int jj = 0; jj < CH; jj++) rows[jj] = rp[jj];
#pragma unroll 1
        for (int l = 0; l <= rl; l++) {
            const int ol = 2 * l - rl;
            const float xi = fl + (float)ol;
            float bx, by, bz;
            tap_line_base<STRICT, ROW>(H, xi, bx, by, bz);
            const unsigned short* trow = tile + own + (ROW ? ol * tw - rt : ol - rt * tw);
#pragma unroll 1
            for (int c0 = 0; c0 <= rt; c0 += CH) {
                rp += CH;
                uint32_t nxt[CH];                           // (the table has slack after its last chunk)
#pragma unroll
                for (int jj = 0; jj < CH; jj++) nxt[jj] = rp[jj];
                chunk(trow, rows, c0, bx, by, bz, clamp_tag);
#pragma unroll
                for (int jj = 0; jj < CH; jj++) rows[jj] = nxt[jj];
            }
        }
    };
    if (need_clamp) lines(std::true_type());
    else lines(std::false_type());
    return ncc_cost(pr, TapSums{sum_src, sum_src_src, sum_ref_src});
}
