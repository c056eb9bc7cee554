// cloud_render_kernels.hip — a point cloud rendered into one calibrated view (include/tsar.h tsar_cloud_render), and a depth map scored
// against a ground-truth map (tsar_depth_compare).  tests/cloud_render_ref.py restates both in numpy float32.
//
// The render is a scatter like geom_reproject_kernels.hip's, one lane per POINT, with a footprint that varies per point and two z-buffers:
//   count    the landings' clipped footprint sizes summed: one wave-level reduction, one 64-bit add per wave.  The host reads the sum and
//            refuses the call above max_splats before anything is written;
//   scatter  centre buffer: a 64-bit unsigned minimum of bits(p_2) << 32 | i into a plane preset to all ones (positive finite floats
//            order like their bits: the front-most depth, then the smallest index);  occluder buffer: a 32-bit unsigned minimum of
//            bits(p_2) over the footprint's pixels.  A minimum only falls, so a plain load that already shows a value <= the lane's lets
//            the lane skip the atomic; a stale larger value only costs a redundant atomic (TSAR_RENDER_SKIP=0 issues them all: A/B runs);
//   support  the landing recomputed, Zc read with a plain load (the kernel boundary orders it after the scatter's atomics), and an integer
//            add of 1 at the centre where the landing lies within depth_diff * Zc of Zc;
//   resolve  per pixel: visible, count against min_points, the caller's outputs.
// Every atomic is relaxed, agent scope, issued without a return value and only by lanes that land.  Minima and integer sums do not depend
// on the order of arrival.  No LDS in the render, no floating-point atomic, no scratch; the same code in both arithmetic modes (`/` is the
// correctly rounded quotient, no contraction: -ffp-contract=off and no fma_ in the chain).
#include "cloud_render_dev.h"   // CrView, cr_land, cr_clip: the landing and the clipped footprint, shared with cloud_splat_kernels.hip

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

// zo null: no footprint, Zo = Zc.  support null: no support pass was needed (min_points 1 and no count_out: the winner supports itself)
__global__ __launch_bounds__(CR_BLOCK) void cloud_render_resolve_kernel(long long np, float occlusion_diff, int min_points, const unsigned long long* __restrict__ zc,
                                                                        const uint32_t* __restrict__ zo, const uint32_t* __restrict__ support,
                                                                        float* __restrict__ depth_out, uint8_t* __restrict__ count_out, int32_t* __restrict__ index_out) {
    const long long p = (long long)blockIdx.x * CR_BLOCK + threadIdx.x;
    if (p >= np) return;
    const unsigned long long code = zc[p];
    const bool landed = code != CR_EMPTY64;
    const float Zc = __uint_as_float((uint32_t)(code >> 32));
    const float Zo = zo ? __uint_as_float(zo[p]) : Zc;                           // (landed: the centre's own footprint covers it, Zo is a float)
    const bool visible = landed && Zc - Zo <= occlusion_diff * Zo;
    const uint32_t count = !landed ? 0u : (support ? support[p] : 1u);
    const bool kept = visible && count >= (uint32_t)min_points;
    if (count_out) count_out[p] = (uint8_t)(count > 255u ? 255u : count);
    if (depth_out) depth_out[p] = kept ? Zc : 0.0f;
    if (index_out) index_out[p] = kept ? (int32_t)(uint32_t)code : -1;
}

// cloud and the three outputs are device pointers (the frame's views; outputs may be null); the arguments have been checked (tsar_api.hip)
int run_cloud_render(CallFrame& f, const float* cloud, long long n, int stride, const CrViewHost& vh, float occlusion_diff, float depth_diff, int min_points,
                     long long max_splats, float* depth_out, uint8_t* count_out, int32_t* index_out, int64_t* n_splats_out) {
    tsar_ctx* ctx = f.ctx;
    hipStream_t st = ctx->stream;
    CrView v;
    for (int e = 0; e < 12; e++) v.P[e] = vh.P[e];
    v.fr = vh.fr; v.max_px = (float)vh.max_px; v.w = vh.w; v.h = vh.h;
    const bool foot = vh.foot;
    const long long np = (long long)vh.w * vh.h;
    unsigned long long* d_splats = f.tmp<unsigned long long>(1);
    if (!f.ok()) return f.finish();
    f.zero(d_splats, sizeof(unsigned long long));
    if (n > 0 && f.ok()) {
        ScopedKernelTimer tm(ctx, "cloud_render_count");
        const unsigned blocks = cr_blocks(n) < 4096u ? cr_blocks(n) : 4096u;
        if (foot) hipLaunchKernelGGL(cloud_render_count_kernel<true>, dim3(blocks), dim3(CR_BLOCK), 0, st, cloud, n, stride, v, d_splats);
        else hipLaunchKernelGGL(cloud_render_count_kernel<false>, dim3(blocks), dim3(CR_BLOCK), 0, st, cloud, n, stride, v, d_splats);
    }
    f.launched();
    unsigned long long splats = 0;
    f.copy(&splats, d_splats, sizeof splats, hipMemcpyDeviceToHost);
    if (!f.sync()) return f.finish();
    if (n_splats_out) *n_splats_out = (int64_t)splats;
    if (splats > (unsigned long long)max_splats) {
        char msg[256];
        snprintf(msg, sizeof msg, "tsar_cloud_render: the call would issue %llu footprint atomics, more than max_splats = %lld: lower radius or max_px, or raise max_splats",
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
        ScopedKernelTimer tm(ctx, "cloud_render_scatter");
        const dim3 grid(cr_blocks(n)), block(CR_BLOCK);
        if (!foot) hipLaunchKernelGGL((cloud_render_scatter_kernel<false, false>), grid, block, 0, st, cloud, n, stride, v, zc, zo);
        else if (ctx->render_skip) hipLaunchKernelGGL((cloud_render_scatter_kernel<true, true>), grid, block, 0, st, cloud, n, stride, v, zc, zo);
        else hipLaunchKernelGGL((cloud_render_scatter_kernel<true, false>), grid, block, 0, st, cloud, n, stride, v, zc, zo);
    }
    f.launched();
    if (n > 0 && support && f.ok()) {
        ScopedKernelTimer tm(ctx, "cloud_render_support");
        hipLaunchKernelGGL(cloud_render_support_kernel, dim3(cr_blocks(n)), dim3(CR_BLOCK), 0, st, cloud, n, stride, v, depth_diff, zc, support);
    }
    f.launched();
    if (f.ok()) {
        ScopedKernelTimer tm(ctx, "cloud_render_resolve");
        hipLaunchKernelGGL(cloud_render_resolve_kernel, dim3(cr_blocks(np)), dim3(CR_BLOCK), 0, st, np, occlusion_diff, min_points, zc, zo, support, depth_out, count_out,
                           index_out);
    }
    f.launched();
    return f.finish();
}

// ---- tsar_depth_compare ----------------------------------------------------------------------------------------------------------------
// counters: 0 n_gt, 1 n_both, 2 n_front, 3 n_behind, 4 + k within[k].  Per lane in registers (the loops over the tolerances are unrolled
// over the fixed maximum, so nothing is indexed at run time), one block-level reduction, then one atomic per block and counter.
#define DC_COUNTERS (4 + TSAR_DEPTH_COMPARE_MAX_TOL)
struct DcTol { float t[TSAR_DEPTH_COMPARE_MAX_TOL]; int n; };

__global__ __launch_bounds__(CR_BLOCK) void depth_compare_kernel(const float* __restrict__ depth, const float* __restrict__ gt, const uint8_t* __restrict__ mask, long long n,
                                                                 DcTol tol, unsigned long long* __restrict__ counters, float* __restrict__ error_out) {
    __shared__ uint32_t part[CR_BLOCK / 64][DC_COUNTERS];
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
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < DC_COUNTERS; k++) {
        uint32_t s = c[k];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) part[wave][k] = s;
    }
    __syncthreads();
    if (threadIdx.x < DC_COUNTERS) {
        unsigned long long s = 0;
        for (int wv = 0; wv < CR_BLOCK / 64; wv++) s += part[wv][threadIdx.x];
        if (s) __hip_atomic_fetch_add(counters + threadIdx.x, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
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
