// geom_check_kernels.hip — the geometric-consistency check of a depth map against the source views' maps (tsar_geom_check;
// include/tsar.h states the arithmetic, tests/test_geom_check_cpu.py restates it in numpy float32).  Per pixel: in how many source
// views the depth reprojects back within reproj_error pixels and depth_diff relative depth; the pixel is kept when that count reaches
// min_consistent.  It is the chain of the geometric-consistency term (pm_core.h geom_term) up to e2, without the square root, plus the
// depth test on p_2, the source point's depth in the reference camera.
//
// One lane per pixel, the lanes of a wave along x: the map read and the three stores of a wave are one line each, and the source
// gathers of neighbouring pixels land on neighbouring texels.  The view loop is wave-uniform: the map pointer and the two 3 x 4
// matrices of a view come from the scene block through scalar loads.  No LDS, no scratch; the same code in both arithmetic modes
// (persp_divide_exact's correctly rounded quotients, no contraction: -ffp-contract=off and no fma_ here).
#include "tsar_device_math.h"

// the maps are HBM pointers by construction (pm_tap_common.h says why that is worth saying): the loads become global_load
typedef const float __attribute__((address_space(1)))* gc_f32_ptr;

#define GC_BLOCK 256      // 64 x 4 pixels

struct GeomCheckArgs {
    float reproj_sq;      // reproj_error * reproj_error
    float depth_diff;
    int min_consistent;
    int n_views;
    int depth_stride;     // floats between two pixels of `depth`: 1 for a map, 4 for the w component of the result plane (out4)
};

__global__ __launch_bounds__(GC_BLOCK) void geom_check_kernel(const DevScene* __restrict__ sc, const float* depth, GeomCheckArgs a,
                                                              uint8_t* __restrict__ count_out, float* depth_out, float* __restrict__ scale) {
    // (depth and depth_out carry no restrict: a caller may filter a map in place, each lane reads its pixel before it writes it)
    const int w = sc->w, h = sc->h;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;                          // partial last tiles in x and in y
    const size_t p = (size_t)y * w + x;
    const float D = ((gc_f32_ptr)depth)[p * (size_t)a.depth_stride];
    const bool candidate = D > 0.0f && D < __builtin_inff();   // (NaN fails both)
    const float xf = (float)x, yf = (float)y;
    const float xd = xf * D, yd = yf * D;
    const float dd = a.depth_diff * D;
    int count = 0;
    for (int vi = 1; vi < a.n_views; vi++) {
        const float* dm = sc->geom_depth[vi];
        if (dm == nullptr) continue;                       // (wave-uniform)
        const DevView& vw = sc->view[vi];
        const float fa = ((vw.A[0] * xd + vw.A[1] * yd) + vw.A[2] * D) + vw.b[0];
        const float fb = ((vw.A[3] * xd + vw.A[4] * yd) + vw.A[5] * D) + vw.b[1];
        const float fs = ((vw.A[6] * xd + vw.A[7] * yd) + vw.A[8] * D) + vw.b[2];
        float u, v;
        persp_divide_exact<true>(fa, fb, fs, u, v);
        const float cf = floorf(u + 0.5f), rf = floorf(v + 0.5f);
        // (NaN fails every comparison: a non-finite projection is "outside", so the gather below stays inside the map)
        const bool inside = fs > 0.0f && cf >= 0.0f && cf <= (float)(w - 1) && rf >= 0.0f && rf <= (float)(h - 1);
        float Dv = 0.0f;
        if (inside) Dv = ((gc_f32_ptr)dm)[(int)rf * w + (int)cf];
        const float* M = sc->geom_back[vi];
        const float cd = cf * Dv, rd = rf * Dv;
        const float p0 = ((M[0] * cd + M[1] * rd) + M[2] * Dv) + M[3];
        const float p1 = ((M[4] * cd + M[5] * rd) + M[6] * Dv) + M[7];
        const float p2 = ((M[8] * cd + M[9] * rd) + M[10] * Dv) + M[11];
        float xq, yq;
        persp_divide_exact<true>(p0, p1, p2, xq, yq);
        const float dx = xq - xf, dy = yq - yf;
        const float e2 = dx * dx + dy * dy;
        const bool ok = inside && Dv > 0.0f && p2 > 0.0f && e2 < a.reproj_sq && __builtin_fabsf(p2 - D) < dd;
        count += ok ? 1 : 0;
    }
    if (!candidate) count = 0;
    const bool keep = count >= a.min_consistent;
    scale[p] = keep ? 1.0f : 0.0f;
    if (count_out) count_out[p] = (uint8_t)count;          // (at most TSAR_MAX_VIEWS - 1 = 63)
    if (depth_out) depth_out[p] = keep ? D : 0.0f;
}

// depth: [h][w] floats depth_stride apart, on the device; count_out / depth_out may be null; scale = ctx->scale is always written
int launch_geom_check(tsar_ctx* ctx, const float* depth, int depth_stride, const tsar_geom_check_params* p, uint8_t* count_out, float* depth_out) {
    GeomCheckArgs a;
    a.reproj_sq = p->reproj_error * p->reproj_error;
    a.depth_diff = p->depth_diff;
    a.min_consistent = p->min_consistent;
    a.n_views = ctx->n_views;
    a.depth_stride = depth_stride;
    const dim3 grid((ctx->w + 63) / 64, (ctx->h + 3) / 4);
    {
        ScopedKernelTimer tm(ctx, "geom_check");
        hipLaunchKernelGGL(geom_check_kernel, grid, dim3(GC_BLOCK), 0, ctx->stream, ctx->dscene, depth, a, count_out, depth_out, ctx->scale);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    return TSAR_OK;
}
