// cloud_splat_kernels.hip — tsar_cloud_render with a normal-oriented occluder (include/tsar.h tsar_cloud_render_oriented).
// tests/cloud_splat_ref.py restates it in numpy float32.
//
// Everything is cloud_render_kernels.hip's (the landing, the clipped square, the two z-buffers, support, resolve: cloud_render_dev.h holds
// what the two units share) except the value a point writes into the occluder buffer: instead of p_2 over the whole square, the depth of
// the point's tangent plane along each pixel's ray, and only where that ray meets the plane within `radius` of the point (the tangent disc).
//   count    the clipped squares' sizes summed (n_splats, the pixels the scatter examines), as the square render counts them;
//   scatter  one lane per POINT.  Per point once: a = X - C, num = n . a, g = M^T n.  Per row once: the terms in v.  Per pixel: one
//            division z = num / den, the ray's point z * d - a, its squared length against r2.  The centre pixel takes p_2 itself, so
//            Zo <= Zc holds as before; a point without a usable normal covers the whole square with p_2, the square render's rule.
//            n_covered: the covering (point, pixel) pairs, counted per lane before the skip, one wave reduction, one 64-bit add per wave;
//   support  the square render's pass, restated here (a kernel is registered with the unit that defines it);
//   resolve  the square render's, plus the occluder plane for the caller.
// Atomics as there: relaxed, agent scope, no return value, integer minima and sums.  No LDS, no floating-point atomic, no scratch; `/` is
// the correctly rounded quotient and nothing contracts (-ffp-contract=off: z * d_k - a_k is a product and a difference).
#include "cloud_render_dev.h"

struct CsView {
    float M[9];           // (K R)^-1, row-major: the ray of pixel (u, v) is M (u, v, 1)
    float C[3];           // the camera centre -R^T t
    float r2;             // fl(radius * radius)
};

__global__ __launch_bounds__(CR_BLOCK) void cloud_splat_count_kernel(const float* __restrict__ pts, long long n, int stride, CrView v,
                                                                     unsigned long long* __restrict__ n_splats) {
    unsigned long long cnt = 0;
    for (long long i = (long long)blockIdx.x * CR_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * CR_BLOCK) {
        const CrLanding l = cr_land<true>(pts, i, stride, v);
        if (!l.lands) continue;
        int x0, x1, y0, y1;
        cr_clip(l, v, x0, x1, y0, y1);
        cnt += (unsigned long long)((x1 - x0 + 1) * (y1 - y0 + 1));          // at most 33 * 33
    }
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s, 64);
    if ((threadIdx.x & 63) == 0 && cnt) __hip_atomic_fetch_add(n_splats, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

__global__ __launch_bounds__(CR_BLOCK) void cloud_splat_support_kernel(const float* __restrict__ pts, long long n, int stride, CrView v, float depth_diff,
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

// support null: no support pass was needed (min_points 1 and no count_out: the winner supports itself)
__global__ __launch_bounds__(CR_BLOCK) void cloud_splat_resolve_kernel(long long np, float occlusion_diff, int min_points, const unsigned long long* __restrict__ zc,
                                                                       const uint32_t* __restrict__ zo, const uint32_t* __restrict__ support,
                                                                       float* __restrict__ depth_out, uint8_t* __restrict__ count_out, int32_t* __restrict__ index_out,
                                                                       float* __restrict__ occluder_out) {
    const long long p = (long long)blockIdx.x * CR_BLOCK + threadIdx.x;
    if (p >= np) return;
    const unsigned long long code = zc[p];
    const uint32_t obits = zo[p];
    const bool landed = code != CR_EMPTY64;
    const float Zc = __uint_as_float((uint32_t)(code >> 32));
    const float Zo = __uint_as_float(obits);                                     // (landed: the centre's own p_2 covers it, Zo is a float <= Zc)
    const bool visible = landed && Zc - Zo <= occlusion_diff * Zo;
    const uint32_t count = !landed ? 0u : (support ? support[p] : 1u);
    const bool kept = visible && count >= (uint32_t)min_points;
    if (count_out) count_out[p] = (uint8_t)(count > 255u ? 255u : count);
    if (depth_out) depth_out[p] = kept ? Zc : 0.0f;
    if (index_out) index_out[p] = kept ? (int32_t)(uint32_t)code : -1;
    if (occluder_out) occluder_out[p] = obits != CR_EMPTY32 ? Zo : 0.0f;
}

// cloud, normals and the four outputs are device pointers (the frame's views; outputs may be null); the arguments have been checked (tsar_api.hip)
int run_cloud_splat(CallFrame& f, const float* cloud, const float* normals, long long n, int stride, int normal_stride, const CrViewHost& vh, const CsViewHost& sh,
                    float occlusion_diff, float depth_diff, int min_points, long long max_splats, float* depth_out, uint8_t* count_out, int32_t* index_out,
                    float* occluder_out, int64_t* n_splats_out, int64_t* n_covered_out) {
    tsar_ctx* ctx = f.ctx;
    hipStream_t st = ctx->stream;
    CrView v;
    for (int e = 0; e < 12; e++) v.P[e] = vh.P[e];
    v.fr = vh.fr; v.max_px = (float)vh.max_px; v.w = vh.w; v.h = vh.h;
    CsView c;
    for (int e = 0; e < 9; e++) c.M[e] = sh.M[e];
    for (int e = 0; e < 3; e++) c.C[e] = sh.C[e];
    c.r2 = sh.r2;
    const long long np = (long long)vh.w * vh.h;
    unsigned long long* d_sums = f.tmp<unsigned long long>(2);                  // n_splats, n_covered
    if (!f.ok()) return f.finish();
    f.zero(d_sums, 2 * sizeof(unsigned long long));
    if (n > 0 && f.ok()) {
        ScopedKernelTimer tm(ctx, "cloud_splat_count");
        const unsigned blocks = cr_blocks(n) < 4096u ? cr_blocks(n) : 4096u;
        hipLaunchKernelGGL(cloud_splat_count_kernel, dim3(blocks), dim3(CR_BLOCK), 0, st, cloud, n, stride, v, d_sums);
    }
    f.launched();
    unsigned long long splats = 0;
    f.copy(&splats, d_sums, sizeof splats, hipMemcpyDeviceToHost);
    if (!f.sync()) return f.finish();
    if (n_splats_out) *n_splats_out = (int64_t)splats;
    if (splats > (unsigned long long)max_splats) {
        char msg[256];
        snprintf(msg, sizeof msg, "tsar_cloud_render_oriented: the call would examine %llu footprint pixels, more than max_splats = %lld: lower radius or max_px, or raise max_splats",
                 splats, max_splats);
        return f.fail(TSAR_ERR_INVALID, msg);
    }
    const bool want_support = count_out != nullptr || min_points > 1;
    unsigned long long* zc = f.tmp<unsigned long long>((size_t)np);
    uint32_t* zo = f.tmp<uint32_t>((size_t)np);
    uint32_t* support = want_support ? f.tmp<uint32_t>((size_t)np) : nullptr;
    if (!f.ok()) return f.finish();
    f.hip(hipMemsetAsync(zc, 0xFF, (size_t)np * 8, st), "hipMemsetAsync");
    if (f.ok()) f.hip(hipMemsetAsync(zo, 0xFF, (size_t)np * 4, st), "hipMemsetAsync");
    if (support) f.zero(support, (size_t)np * 4);
    if (n > 0 && f.ok()) {
        ScopedKernelTimer tm(ctx, "cloud_splat_scatter");
        const dim3 grid(cr_blocks(n)), block(CR_BLOCK);
        if (ctx->render_skip) hipLaunchKernelGGL(cloud_splat_scatter_kernel<true>, grid, block, 0, st, cloud, normals, n, stride, normal_stride, v, c, zc, zo, d_sums + 1);
        else hipLaunchKernelGGL(cloud_splat_scatter_kernel<false>, grid, block, 0, st, cloud, normals, n, stride, normal_stride, v, c, zc, zo, d_sums + 1);
    }
    f.launched();
    if (n > 0 && support && f.ok()) {
        ScopedKernelTimer tm(ctx, "cloud_splat_support");
        hipLaunchKernelGGL(cloud_splat_support_kernel, dim3(cr_blocks(n)), dim3(CR_BLOCK), 0, st, cloud, n, stride, v, depth_diff, zc, support);
    }
    f.launched();
    if (f.ok()) {
        ScopedKernelTimer tm(ctx, "cloud_splat_resolve");
        hipLaunchKernelGGL(cloud_splat_resolve_kernel, dim3(cr_blocks(np)), dim3(CR_BLOCK), 0, st, np, occlusion_diff, min_points, zc, zo, support, depth_out, count_out,
                           index_out, occluder_out);
    }
    f.launched();
    unsigned long long covered = 0;
    f.copy(&covered, d_sums + 1, sizeof covered, hipMemcpyDeviceToHost);
    if (!f.sync()) return f.finish();
    if (n_covered_out) *n_covered_out = (int64_t)covered;
    return f.finish();
}
