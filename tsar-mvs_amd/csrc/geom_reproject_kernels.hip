// geom_reproject_kernels.hip — the source views' depth maps rendered into the reference camera (tsar_geom_reproject), and the two small
// kernels of tsar_pm_merge_depths, which offers such a map to the matcher (include/tsar.h states both; tests/test_geom_reproject_cpu.py
// restates the render in numpy float32).
//
// The render is a scatter, the only one here: one lane per SOURCE pixel, the lanes of a wave along x (the map read is one line), the
// view on blockIdx.z, so that the map pointer and the 3 x 4 matrix B of a view are scalar loads from the scene block.  A source pixel
// with a depth lands on the reference pixel nearest to its reprojection; the landings of a wave fall on neighbouring reference pixels.
//   pass 1  z-buffer: a 32-bit unsigned minimum of p_2's bit pattern into a plane preset to all ones (positive finite floats order
//           like their bits, and a minimum does not depend on the order of arrival: the result is the same bits in every run);
//   pass 2  support:  the landing recomputed, Z read with a plain load (the kernel boundary orders it after pass 1's atomics), and a
//           64-bit OR of 1 << v where the landing lies within depth_diff * Z of Z (an OR does not depend on the order either);
//   pass 3  resolve:  per reference pixel, the number of set bits against min_views; the caller's outputs.
// Both atomics are issued without a return value and only by lanes that land.  No LDS, no scratch; the same code in both arithmetic
// modes (persp_divide_exact's correctly rounded quotients, no contraction: -ffp-contract=off and no fma_ in the chain).
#include "tsar_device_math.h"

typedef const float __attribute__((address_space(1)))* gr_f32_ptr;

#define GR_BLOCK 256      // 64 x 4 pixels
#define GR_EMPTY 0xFFFFFFFFu   // a z-buffer entry nothing landed on (no float that lands has these bits: they are a NaN's)

struct ReprojLanding {
    bool lands;
    int at;               // yi * w + xi, valid when lands
    float p2;             // the source point's depth in the reference camera
};

// steps 1-6 of include/tsar.h for pixel (c, r) of view v's map dm; M = B of view v
DEVFN ReprojLanding reproject_pixel(const float* dm, const float* M, int c, int r, int w, int h) {
    const float Dv = ((gr_f32_ptr)dm)[(size_t)r * w + c];
    const bool candidate = Dv > 0.0f && Dv < __builtin_inff();   // (NaN fails both)
    const float cf = (float)c, rf = (float)r;
    const float cd = cf * Dv, rd = rf * Dv;
    const float p0 = ((M[0] * cd + M[1] * rd) + M[2] * Dv) + M[3];
    const float p1 = ((M[4] * cd + M[5] * rd) + M[6] * Dv) + M[7];
    const float p2 = ((M[8] * cd + M[9] * rd) + M[10] * Dv) + M[11];
    float xq, yq;
    persp_divide_exact<true>(p0, p1, p2, xq, yq);
    const float xi = floorf(xq + 0.5f), yi = floorf(yq + 0.5f);
    ReprojLanding l;
    // (NaN fails every comparison: a non-finite projection does not land, so `at` stays inside the planes)
    l.lands = candidate && p2 > 0.0f && p2 < __builtin_inff() && xi >= 0.0f && xi <= (float)(w - 1) && yi >= 0.0f && yi <= (float)(h - 1);
    l.at = l.lands ? (int)yi * w + (int)xi : 0;
    l.p2 = p2;
    return l;
}

// SUPPORT = false: pass 1 (zbuf is written); true: pass 2 (zbuf is read, mask is written)
template <bool SUPPORT>
__global__ __launch_bounds__(GR_BLOCK) void geom_reproject_scatter_kernel(const DevScene* __restrict__ sc, float depth_diff, uint32_t* zbuf,
                                                                          unsigned long long* __restrict__ mask) {
    const int w = sc->w, h = sc->h;
    const int v = (int)blockIdx.z + 1;
    const float* dm = sc->geom_depth[v];
    if (dm == nullptr) return;                             // (uniform over the workgroup)
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), r = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (c >= w || r >= h) return;                          // partial last tiles in x and in y
    const ReprojLanding l = reproject_pixel(dm, sc->geom_back[v], c, r, w, h);
    if (!l.lands) return;
    if (!SUPPORT) {
        __hip_atomic_fetch_min(zbuf + l.at, __float_as_uint(l.p2), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else {
        const float Z = __uint_as_float(zbuf[l.at]);       // (this landing took part in the minimum: Z is a float, <= p2)
        const float dd = depth_diff * Z;
        if (__builtin_fabsf(l.p2 - Z) <= dd) __hip_atomic_fetch_or(mask + l.at, 1ull << v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(GR_BLOCK) void geom_reproject_resolve_kernel(const DevScene* __restrict__ sc, int min_views, const uint32_t* __restrict__ zbuf,
                                                                          const unsigned long long* __restrict__ mask, float* __restrict__ depth_out,
                                                                          uint8_t* __restrict__ count_out) {
    const int w = sc->w, h = sc->h;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const uint32_t zb = zbuf[p];
    const bool landed = zb != GR_EMPTY;
    const int count = landed ? __popcll(mask[p]) : 0;      // (at most TSAR_MAX_VIEWS - 1 = 63)
    if (count_out) count_out[p] = (uint8_t)count;
    if (depth_out) depth_out[p] = landed && count >= min_views ? __uint_as_float(zb) : 0.0f;
}

// zbuf [h][w] uint32 and mask [h][w] uint64: the call's temporaries; depth_out / count_out (device) may be null
int launch_geom_reproject(tsar_ctx* ctx, const tsar_geom_reproject_params* p, uint32_t* zbuf, unsigned long long* mask, float* depth_out, uint8_t* count_out) {
    const size_t np = (size_t)ctx->w * ctx->h;
    const dim3 tiles((ctx->w + 63) / 64, (ctx->h + 3) / 4);
    const dim3 scatter(tiles.x, tiles.y, ctx->n_views - 1);
    {
        ScopedKernelTimer tm(ctx, "geom_reproject");
        TSAR_HIP_TRY(ctx, hipMemsetAsync(zbuf, 0xFF, np * sizeof(uint32_t), ctx->stream));
        TSAR_HIP_TRY(ctx, hipMemsetAsync(mask, 0, np * sizeof(unsigned long long), ctx->stream));
        if (ctx->n_views > 1) hipLaunchKernelGGL(geom_reproject_scatter_kernel<false>, scatter, dim3(GR_BLOCK), 0, ctx->stream, ctx->dscene, p->depth_diff, zbuf, mask);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    {
        ScopedKernelTimer tm(ctx, "geom_reproject");
        if (ctx->n_views > 1) hipLaunchKernelGGL(geom_reproject_scatter_kernel<true>, scatter, dim3(GR_BLOCK), 0, ctx->stream, ctx->dscene, p->depth_diff, zbuf, mask);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    {
        ScopedKernelTimer tm(ctx, "geom_reproject");
        hipLaunchKernelGGL(geom_reproject_resolve_kernel, tiles, dim3(GR_BLOCK), 0, ctx->stream, ctx->dscene, p->min_views, zbuf, mask, depth_out, count_out);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    return TSAR_OK;
}

// ---- tsar_pm_merge_depths: the candidate planes, and the choice between the state and the scored candidates ------------------------
// Q = (P's normal, the offset of the plane with that normal through the pixel at depth D) where D is usable, else P
__global__ __launch_bounds__(GR_BLOCK) void merge_candidate_kernel(const DevScene* __restrict__ sc, const float* __restrict__ depth, const float4* __restrict__ own,
                                                                   float4* __restrict__ cand) {
    const int w = sc->w, h = sc->h;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;
    const size_t p = (size_t)y * w + x;
    const DevRef& rf = sc->ref;
    float4 q = own[p];
    const float D = depth[p];
    if (D >= rf.depthMin && D <= rf.depthMax) {            // (finite; NaN fails both)
        const float n[3] = {q.x, q.y, q.z};
        q.w = plane_offset(rf, n, x, y, D);
    }
    cand[p] = q;
}

// where the candidate scored strictly lower, the pixel takes its plane, cost, best view and ratio; one count per wave
__global__ __launch_bounds__(GR_BLOCK) void merge_select_kernel(const DevScene* __restrict__ sc, const float4* __restrict__ cand, const float* __restrict__ cand_c,
                                                                const int32_t* __restrict__ cand_bv, const float* __restrict__ cand_rt, float4* __restrict__ n4,
                                                                float* __restrict__ c, int32_t* __restrict__ bv, float* __restrict__ rt,
                                                                unsigned long long* __restrict__ n_taken) {
    const int w = sc->w, h = sc->h;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const bool in_image = x < w && y < h;
    const size_t p = in_image ? (size_t)y * w + x : 0;
    const bool take = in_image && cand_c[p] < c[p];        // (strictly: the own plane wins ties; NaN never wins)
    if (take) {
        n4[p] = cand[p];
        c[p] = cand_c[p];
        bv[p] = cand_bv[p];
        rt[p] = cand_rt[p];
    }
    const unsigned long long votes = __ballot(take);
    if ((threadIdx.x & 63) == 0 && votes) atomicAdd(n_taken, (unsigned long long)__popcll(votes));
}

int launch_merge_candidates(tsar_ctx* ctx, const float* depth, float4* cand) {
    const dim3 tiles((ctx->w + 63) / 64, (ctx->h + 3) / 4);
    {
        ScopedKernelTimer tm(ctx, "pm_merge_depths");
        hipLaunchKernelGGL(merge_candidate_kernel, tiles, dim3(GR_BLOCK), 0, ctx->stream, ctx->dscene, depth, ctx->buf[0].n4, cand);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    return TSAR_OK;
}
int launch_merge_select(tsar_ctx* ctx, const float4* cand, const float* cand_c, const int32_t* cand_bv, const float* cand_rt, unsigned long long* n_taken) {
    const dim3 tiles((ctx->w + 63) / 64, (ctx->h + 3) / 4);
    {
        ScopedKernelTimer tm(ctx, "pm_merge_depths");
        hipLaunchKernelGGL(merge_select_kernel, tiles, dim3(GR_BLOCK), 0, ctx->stream, ctx->dscene, cand, cand_c, cand_bv, cand_rt, ctx->buf[0].n4, ctx->buf[0].c,
                           ctx->beview, ctx->ratio, n_taken);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    return TSAR_OK;
}
