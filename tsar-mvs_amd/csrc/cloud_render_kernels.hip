// cloud_render_kernels.hip — a point cloud rendered into one calibrated view with a square occluder (include/tsar.h tsar_cloud_render) or a
// normal-oriented one (tsar_cloud_render_oriented), and a depth map scored against a ground-truth map (tsar_depth_compare).
// tests/cloud_render_ref.py and tests/cloud_splat_ref.py restate them in numpy float32.
//
// The render is a scatter like geom_reproject_kernels.hip's, one lane per POINT, with a footprint that varies per point and two z-buffers.
// One driver (run_cloud_render) and one count, support and resolve kernel serve both entries; only the scatter differs:
//   count    the landings' clipped footprint sizes summed: one wave-level reduction, one 64-bit add per wave.  The host reads the sum and
//            refuses the call above max_splats before anything is written;
//   scatter  centre buffer: a 64-bit unsigned minimum of bits(p_2) << 32 | i into a plane preset to all ones (positive finite floats
//            order like their bits: the front-most depth, then the smallest index);  occluder buffer: a 32-bit unsigned minimum over the
//            footprint's pixels.  A minimum only falls, so a plain load that already shows a value <= the lane's lets the lane skip the
//            atomic; a stale larger value only costs a redundant atomic (TSAR_RENDER_SKIP=0 issues them all: A/B runs).
//            square:    bits(p_2) over the whole clipped square;
//            oriented:  the depth of the point's tangent plane along each pixel's ray, and only where that ray meets the plane within
//                       `radius` of the point (the tangent disc).  Per point once: a = X - C, num = n . a, g = M^T n.  Per row once: the terms
//                       in v.  Per pixel: one division z = num / den, the ray's point z * d - a, its squared length against r2.  The centre
//                       pixel takes p_2 itself, so Zo <= Zc holds as in the square; a point without a usable normal covers the whole square
//                       with p_2.  n_covered: the covering (point, pixel) pairs, counted per lane before the skip, one wave reduction, one
//                       64-bit add per wave;
//   support  the landing recomputed, Zc read with a plain load (the kernel boundary orders it after the scatter's atomics), and an integer
//            add of 1 at the centre where the landing lies within depth_diff * Zc of Zc;
//   resolve  per pixel: visible, count against min_points, the caller's outputs (oriented: the occluder plane as well).
// Every atomic is relaxed, agent scope, issued without a return value and only by lanes that land.  Minima and integer sums do not depend
// on the order of arrival.  No LDS in the render, no floating-point atomic, no scratch; the same code in both arithmetic modes (`/` is the
// correctly rounded quotient, no contraction: -ffp-contract=off and no fma_ in the chain; z * d_k - a_k is a product and a difference).
#include <float.h>
#include <math.h>

#include "tsar_device_math.h"

#define CR_BLOCK 256
#define CR_EMPTY32 0xFFFFFFFFu             // an occluder entry nothing covers (no float that lands has these bits: they are a NaN's)
#define CR_EMPTY64 0xFFFFFFFFFFFFFFFFull   // a centre entry nothing landed on

struct CrView {
    float P[12];          // K [R | t], float64 products rounded once
    float fr;             // fl(K[0] * radius); 0 with radius 0
    float max_px;         // (float)max_px
    int w, h;
};
struct CsView {
    float M[9];           // (K R)^-1, row-major: the ray of pixel (u, v) is M (u, v, 1)
    float C[3];           // the camera centre -R^T t
    float r2;             // fl(radius * radius)
};

struct CrLanding {
    bool lands;
    int xi, yi, s;        // valid when lands
    float p2;
};

template <bool FOOT>
DEVFN CrLanding cr_land(const float* __restrict__ pts, long long i, int stride, const CrView& v) {
    const float* p = pts + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    const bool candidate = fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX;   // (NaN fails)
    const float p0 = ((v.P[0] * x + v.P[1] * y) + v.P[2] * z) + v.P[3];
    const float p1 = ((v.P[4] * x + v.P[5] * y) + v.P[6] * z) + v.P[7];
    const float p2 = ((v.P[8] * x + v.P[9] * y) + v.P[10] * z) + v.P[11];
    const float xq = p0 / p2, yq = p1 / p2;
    const float xi = floorf(xq + 0.5f), yi = floorf(yq + 0.5f);
    CrLanding l;
    // (NaN fails every comparison: a non-finite projection does not land, so xi and yi stay inside the planes)
    l.lands = candidate && p2 > 0.0f && p2 < __builtin_inff() && xi >= 0.0f && xi <= (float)(v.w - 1) && yi >= 0.0f && yi <= (float)(v.h - 1);
    l.xi = l.lands ? (int)xi : 0;
    l.yi = l.lands ? (int)yi : 0;
    l.p2 = p2;
    // (p_2 > 0 and fr >= 0, both finite: the quotient is in [0, inf], never NaN, and the minimum is in [0, max_px])
    l.s = FOOT && l.lands ? (int)fminf(floorf(v.fr / p2 + 0.5f), v.max_px) : 0;
    return l;
}

// the footprint clipped to the image: [x0, x1] x [y0, y1]
DEVFN void cr_clip(const CrLanding& l, const CrView& v, int& x0, int& x1, int& y0, int& y1) {
    x0 = l.xi - l.s < 0 ? 0 : l.xi - l.s;
    x1 = l.xi + l.s > v.w - 1 ? v.w - 1 : l.xi + l.s;
    y0 = l.yi - l.s < 0 ? 0 : l.yi - l.s;
    y1 = l.yi + l.s > v.h - 1 ? v.h - 1 : l.yi + l.s;
}

static inline unsigned cr_blocks(long long n) { return (unsigned)((n + CR_BLOCK - 1) / CR_BLOCK); }

// n_splats: the pixels the scatter examines (the oriented entry always has a footprint: FOOT)
template <bool FOOT>
__global__ __launch_bounds__(CR_BLOCK) void cloud_render_count_kernel(const float* __restrict__ pts, long long n, int stride, CrView v,
                                                                      unsigned long long* __restrict__ n_splats) {
    unsigned long long cnt = 0;
    for (long long i = (long long)blockIdx.x * CR_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * CR_BLOCK) {
        const CrLanding l = cr_land<FOOT>(pts, i, stride, v);
        if (!l.lands) continue;
        int x0, x1, y0, y1;
        cr_clip(l, v, x0, x1, y0, y1);
        cnt += (unsigned long long)((x1 - x0 + 1) * (y1 - y0 + 1));          // at most 33 * 33
    }
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
    if ((threadIdx.x & 63) == 0 && cnt) __hip_atomic_fetch_add(n_splats, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// zc [h][w] uint64 preset to CR_EMPTY64; zo [h][w] uint32 preset to CR_EMPTY32 (FOOT only)
template <bool FOOT, bool SKIP>
__global__ __launch_bounds__(CR_BLOCK) void cloud_render_scatter_kernel(const float* __restrict__ pts, long long n, int stride, CrView v, unsigned long long* zc,
                                                                        uint32_t* zo) {
    const long long i = (long long)blockIdx.x * CR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const CrLanding l = cr_land<FOOT>(pts, i, stride, v);
    if (!l.lands) return;
    const uint32_t bits = __float_as_uint(l.p2);
    const size_t at = (size_t)l.yi * v.w + l.xi;
    __hip_atomic_fetch_min(zc + at, ((unsigned long long)bits << 32) | (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (FOOT) {
        int x0, x1, y0, y1;
        cr_clip(l, v, x0, x1, y0, y1);
        for (int yy = y0; yy <= y1; yy++) {
            uint32_t* row = zo + (size_t)yy * v.w;
            for (int xx = x0; xx <= x1; xx++) {
                if (SKIP && row[xx] <= bits) continue;                           // already covered at this depth or nearer
                __hip_atomic_fetch_min(row + xx, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}

// zc [h][w] uint64 preset to CR_EMPTY64; zo [h][w] uint32 preset to CR_EMPTY32; nrm: the normal of point i at nrm + i * nstride
template <bool SKIP>
__global__ __launch_bounds__(CR_BLOCK) void cloud_splat_scatter_kernel(const float* __restrict__ pts, const float* __restrict__ nrm, long long n, int stride, int nstride,
                                                                       CrView v, CsView c, unsigned long long* zc, uint32_t* zo,
                                                                       unsigned long long* __restrict__ n_covered) {
    const long long i = (long long)blockIdx.x * CR_BLOCK + threadIdx.x;
    uint32_t covered = 0;                                                        // at most 33 * 33 per lane
    if (i < n) {
        const CrLanding l = cr_land<true>(pts, i, stride, v);
        if (l.lands) {
            const uint32_t cbits = __float_as_uint(l.p2);
            __hip_atomic_fetch_min(zc + (size_t)l.yi * v.w + l.xi, ((unsigned long long)cbits << 32) | (uint32_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const float* p = pts + (size_t)i * stride;
            const float* q = nrm + (size_t)i * nstride;
            const float n0 = q[0], n1 = q[1], n2 = q[2];
            const bool oriented = fabsf(n0) <= FLT_MAX && fabsf(n1) <= FLT_MAX && fabsf(n2) <= FLT_MAX && (n0 != 0.0f || n1 != 0.0f || n2 != 0.0f);
            const float a0 = p[0] - c.C[0], a1 = p[1] - c.C[1], a2 = p[2] - c.C[2];
            const float num = (n0 * a0 + n1 * a1) + n2 * a2;
            const float g0 = (c.M[0] * n0 + c.M[3] * n1) + c.M[6] * n2;
            const float g1 = (c.M[1] * n0 + c.M[4] * n1) + c.M[7] * n2;
            const float g2 = (c.M[2] * n0 + c.M[5] * n1) + c.M[8] * n2;
            int x0, x1, y0, y1;
            cr_clip(l, v, x0, x1, y0, y1);
            for (int yy = y0; yy <= y1; yy++) {
                uint32_t* row = zo + (size_t)yy * v.w;
                const float fv = (float)yy;
                const float rden = g1 * fv + g2;
                const float r0 = c.M[1] * fv + c.M[2], r1 = c.M[4] * fv + c.M[5], r2 = c.M[7] * fv + c.M[8];
                for (int xx = x0; xx <= x1; xx++) {
                    uint32_t bits = cbits;
                    if (oriented && !(xx == l.xi && yy == l.yi)) {
                        const float fu = (float)xx;
                        const float den = g0 * fu + rden;
                        const float z = num / den;
                        const float e0 = z * (c.M[0] * fu + r0) - a0;
                        const float e1 = z * (c.M[3] * fu + r1) - a1;
                        const float e2 = z * (c.M[6] * fu + r2) - a2;
                        const float qq = (e0 * e0 + e1 * e1) + e2 * e2;
                        if (!(z > 0.0f && z < __builtin_inff() && qq <= c.r2)) continue;     // (NaN fails: the ray misses the disc)
                        bits = __float_as_uint(z);
                    }
                    covered++;
                    if (SKIP && row[xx] <= bits) continue;                       // already covered at this depth or nearer
                    __hip_atomic_fetch_min(row + xx, bits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
        }
    }
    for (int s = 32; s > 0; s >>= 1) covered += __shfl_xor(covered, s, 64);     // (every lane of the wave arrives here; 64 * 1089 < 2^32)
    if ((threadIdx.x & 63) == 0 && covered) __hip_atomic_fetch_add(n_covered, (unsigned long long)covered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(CR_BLOCK) void cloud_render_support_kernel(const float* __restrict__ pts, long long n, int stride, CrView v, float depth_diff,
                                                                        const unsigned long long* __restrict__ zc, uint32_t* __restrict__ support) {
    const long long i = (long long)blockIdx.x * CR_BLOCK + threadIdx.x;
    if (i >= n) return;
    const CrLanding l = cr_land<false>(pts, i, stride, v);
    if (!l.lands) return;
    const size_t at = (size_t)l.yi * v.w + l.xi;
    const float Zc = __uint_as_float((uint32_t)(zc[at] >> 32));                  // (this landing took part in the minimum: Zc is a float, <= p2)
    const float dd = depth_diff * Zc;
    if (__builtin_fabsf(l.p2 - Zc) <= dd) __hip_atomic_fetch_add(support + at, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ORIENTED: zo is there and occluder_out may be; else occluder_out is not read, and zo null: no footprint, Zo = Zc.
// support null: no support pass was needed (min_points 1 and no count_out: the winner supports itself)
template <bool ORIENTED>
__global__ __launch_bounds__(CR_BLOCK) void cloud_render_resolve_kernel(long long np, float occlusion_diff, int min_points, const unsigned long long* __restrict__ zc,
                                                                        const uint32_t* __restrict__ zo, const uint32_t* __restrict__ support,
                                                                        float* __restrict__ depth_out, uint8_t* __restrict__ count_out, int32_t* __restrict__ index_out,
                                                                        float* __restrict__ occluder_out) {
    const long long p = (long long)blockIdx.x * CR_BLOCK + threadIdx.x;
    if (p >= np) return;
    const unsigned long long code = zc[p];
    const bool landed = code != CR_EMPTY64;
    const float Zc = __uint_as_float((uint32_t)(code >> 32));
    const float Zo = ORIENTED || zo ? __uint_as_float(zo[p]) : Zc;               // (landed: the centre's own p_2 covers it, Zo is a float <= Zc)
    const bool visible = landed && Zc - Zo <= occlusion_diff * Zo;
    const uint32_t count = !landed ? 0u : (support ? support[p] : 1u);
    const bool kept = visible && count >= (uint32_t)min_points;
    if (count_out) count_out[p] = (uint8_t)(count > 255u ? 255u : count);
    if (depth_out) depth_out[p] = kept ? Zc : 0.0f;
    if (index_out) index_out[p] = kept ? (int32_t)(uint32_t)code : -1;
    if (ORIENTED && occluder_out) occluder_out[p] = __float_as_uint(Zo) != CR_EMPTY32 ? Zo : 0.0f;
}

// Both renders.  sh null: the square occluder (normals and occluder_out are null too, n_covered_out is not written); else the oriented
// one, which always has a footprint and an occluder buffer.  cloud, normals and the four outputs are device pointers (the frame's views;
// outputs may be null); the arguments have been checked (tsar_api.hip).  The frame names the entry; the timers are named after it as
// include/tsar.h promises.
int run_cloud_render(CallFrame& f, const float* cloud, const float* normals, long long n, int stride, int normal_stride, const CrViewHost& vh, const CsViewHost* sh,
                     float occlusion_diff, float depth_diff, int min_points, long long max_splats, float* depth_out, uint8_t* count_out, int32_t* index_out,
                     float* occluder_out, int64_t* n_splats_out, int64_t* n_covered_out) {
    tsar_ctx* ctx = f.ctx;
    hipStream_t st = ctx->stream;
    const bool oriented = sh != nullptr;
    const bool foot = oriented || vh.foot;
    CrView v;
    for (int e = 0; e < 12; e++) v.P[e] = vh.P[e];
    v.fr = vh.fr; v.max_px = (float)vh.max_px; v.w = vh.w; v.h = vh.h;
    CsView c = {};
    if (oriented) {
        for (int e = 0; e < 9; e++) c.M[e] = sh->M[e];
        for (int e = 0; e < 3; e++) c.C[e] = sh->C[e];
        c.r2 = sh->r2;
    }
    const long long np = (long long)vh.w * vh.h;
    const size_t n_sums = oriented ? 2 : 1;                                      // n_splats; oriented: n_covered
    unsigned long long* d_sums = f.tmp<unsigned long long>(n_sums);
    if (!f.ok()) return f.finish();
    f.zero(d_sums, n_sums * sizeof(unsigned long long));
    if (n > 0 && f.ok()) {
        ScopedKernelTimer tm(ctx, oriented ? "cloud_splat_count" : "cloud_render_count");
        const unsigned blocks = cr_blocks(n) < 4096u ? cr_blocks(n) : 4096u;
        if (foot) hipLaunchKernelGGL(cloud_render_count_kernel<true>, dim3(blocks), dim3(CR_BLOCK), 0, st, cloud, n, stride, v, d_sums);
        else hipLaunchKernelGGL(cloud_render_count_kernel<false>, dim3(blocks), dim3(CR_BLOCK), 0, st, cloud, n, stride, v, d_sums);
    }
    f.launched();
    unsigned long long splats = 0;
    f.copy(&splats, d_sums, sizeof splats, hipMemcpyDeviceToHost);
    if (!f.sync()) return f.finish();
    if (n_splats_out) *n_splats_out = (int64_t)splats;
    if (splats > (unsigned long long)max_splats) {
        char msg[256];
        snprintf(msg, sizeof msg,
                 oriented ? "tsar_cloud_render_oriented: the call would examine %llu footprint pixels, more than max_splats = %lld: lower radius or max_px, or raise max_splats"
                          : "tsar_cloud_render: the call would issue %llu footprint atomics, more than max_splats = %lld: lower radius or max_px, or raise max_splats",
                 splats, max_splats);
        return f.fail(TSAR_ERR_INVALID, msg);
    }
    const bool want_support = count_out != nullptr || min_points > 1;
    unsigned long long* zc = f.tmp<unsigned long long>((size_t)np);
    uint32_t* zo = foot ? f.tmp<uint32_t>((size_t)np) : nullptr;
    uint32_t* support = want_support ? f.tmp<uint32_t>((size_t)np) : nullptr;
    if (!f.ok()) return f.finish();
    f.hip(hipMemsetAsync(zc, 0xFF, (size_t)np * 8, st), "hipMemsetAsync");
    if (zo && f.ok()) f.hip(hipMemsetAsync(zo, 0xFF, (size_t)np * 4, st), "hipMemsetAsync");
    if (support) f.zero(support, (size_t)np * 4);
    if (n > 0 && f.ok()) {
        ScopedKernelTimer tm(ctx, oriented ? "cloud_splat_scatter" : "cloud_render_scatter");
        const dim3 grid(cr_blocks(n)), block(CR_BLOCK);
        if (oriented) {
            if (ctx->render_skip) hipLaunchKernelGGL(cloud_splat_scatter_kernel<true>, grid, block, 0, st, cloud, normals, n, stride, normal_stride, v, c, zc, zo, d_sums + 1);
            else hipLaunchKernelGGL(cloud_splat_scatter_kernel<false>, grid, block, 0, st, cloud, normals, n, stride, normal_stride, v, c, zc, zo, d_sums + 1);
        } else if (!foot) hipLaunchKernelGGL((cloud_render_scatter_kernel<false, false>), grid, block, 0, st, cloud, n, stride, v, zc, zo);
        else if (ctx->render_skip) hipLaunchKernelGGL((cloud_render_scatter_kernel<true, true>), grid, block, 0, st, cloud, n, stride, v, zc, zo);
        else hipLaunchKernelGGL((cloud_render_scatter_kernel<true, false>), grid, block, 0, st, cloud, n, stride, v, zc, zo);
    }
    f.launched();
    if (n > 0 && support && f.ok()) {
        ScopedKernelTimer tm(ctx, oriented ? "cloud_splat_support" : "cloud_render_support");
        hipLaunchKernelGGL(cloud_render_support_kernel, dim3(cr_blocks(n)), dim3(CR_BLOCK), 0, st, cloud, n, stride, v, depth_diff, zc, support);
    }
    f.launched();
    if (f.ok()) {
        ScopedKernelTimer tm(ctx, oriented ? "cloud_splat_resolve" : "cloud_render_resolve");
        const dim3 grid(cr_blocks(np)), block(CR_BLOCK);
        if (oriented) hipLaunchKernelGGL(cloud_render_resolve_kernel<true>, grid, block, 0, st, np, occlusion_diff, min_points, zc, zo, support, depth_out, count_out, index_out, occluder_out);
        else hipLaunchKernelGGL(cloud_render_resolve_kernel<false>, grid, block, 0, st, np, occlusion_diff, min_points, zc, zo, support, depth_out, count_out, index_out, nullptr);
    }
    f.launched();
    if (oriented) {
        unsigned long long covered = 0;
        f.copy(&covered, d_sums + 1, sizeof covered, hipMemcpyDeviceToHost);
        if (!f.sync()) return f.finish();
        if (n_covered_out) *n_covered_out = (int64_t)covered;
    }
    return f.finish();
}

// ---- tsar_depth_compare ----------------------------------------------------------------------------------------------------------------
// counters: 0 n_gt, 1 n_both, 2 n_front, 3 n_behind, 4 + k within[k].  Per lane in registers (the loops over the tolerances are unrolled
// over the fixed maximum, so nothing is indexed at run time), then block_add_counters (LDS: the partials of the block's waves).
#define DC_COUNTERS (4 + TSAR_DEPTH_COMPARE_MAX_TOL)
struct DcTol { float t[TSAR_DEPTH_COMPARE_MAX_TOL]; int n; };

__global__ __launch_bounds__(CR_BLOCK) void depth_compare_kernel(const float* __restrict__ depth, const float* __restrict__ gt, const uint8_t* __restrict__ mask, long long n,
                                                                 DcTol tol, unsigned long long* __restrict__ counters, float* __restrict__ error_out) {
    uint32_t c[DC_COUNTERS];
#pragma unroll
    for (int k = 0; k < DC_COUNTERS; k++) c[k] = 0;
    for (long long i = (long long)blockIdx.x * CR_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * CR_BLOCK) {
        const float D = depth[i], G = gt[i];
        const bool is_gt = G > 0.0f && G < __builtin_inff() && (!mask || mask[i] != 0);
        const bool both = is_gt && D > 0.0f && D < __builtin_inff();
        const float diff = D - G;
        const float t0 = tol.t[0] * G;
        c[0] += is_gt;
        c[1] += both;
        c[2] += both && diff < -t0;
        c[3] += both && diff > t0;
#pragma unroll
        for (int k = 0; k < TSAR_DEPTH_COMPARE_MAX_TOL; k++) c[4 + k] += k < tol.n && both && __builtin_fabsf(diff) <= tol.t[k] * G;
        if (error_out) error_out[i] = both ? diff / G : __builtin_nanf("");
    }
    block_add_counters<DC_COUNTERS, CR_BLOCK>(c, counters);
}

// depth, gt, mask and error_out are device pointers; counters_out: host [DC_COUNTERS]
int run_depth_compare(CallFrame& f, const float* depth, const float* gt, const uint8_t* mask, long long n, int n_tol, const float* tol, float* error_out,
                      unsigned long long* counters_out) {
    tsar_ctx* ctx = f.ctx;
    DcTol t;
    for (int k = 0; k < TSAR_DEPTH_COMPARE_MAX_TOL; k++) t.t[k] = k < n_tol ? tol[k] : 0.0f;
    t.n = n_tol;
    unsigned long long* d = f.tmp<unsigned long long>(DC_COUNTERS);
    if (!f.ok()) return f.finish();
    f.zero(d, DC_COUNTERS * sizeof(unsigned long long));
    if (n > 0 && f.ok()) {
        ScopedKernelTimer tm(ctx, "depth_compare");
        // (a lane's own counts stay below 2^32: at most 2^31 / 256 pixels per lane)
        const unsigned blocks = cr_blocks(n) < 4096u ? cr_blocks(n) : 4096u;
        hipLaunchKernelGGL(depth_compare_kernel, dim3(blocks), dim3(CR_BLOCK), 0, ctx->stream, depth, gt, mask, n, t, d, error_out);
    }
    f.launched();
    f.copy(counters_out, d, DC_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    return f.finish();
}
