// tsar_pyramid.hip — one level of the image pyramid (tsar_pyramid_views): OpenCV's pyrDown, which the reference uses to
// shrink its images (main.cpp:377-379, 621-622).  One thread per output pixel; the 5 x 5 window is read straight from the
// fine view (a level has a quarter of the pixels of its source: a few tens of microseconds at 24 MP, not a hot path).
//
//   kernel   [1 4 6 4 1]^T [1 4 6 4 1] / 256, centred on source pixel (2x, 2y)
//   border   BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba)
//   size     ((w + 1) / 2, (h + 1) / 2)
//   8-bit    integer sum s of the 25 weighted texels, out = (s + 128) >> 8 (pyrDown on CV_8U); written as bytes
//   float    per source row r_j = (((t0 + 4 t1) + 6 t2) + 4 t3) + t4, then (((r0 + 4 r1) + 6 r2) + 4 r3) + r4, times 1/256 (exact):
//            float32, every product and sum rounded in that order, no fused multiply-add
#include "tsar_dev.h"

#define PYR_BLOCK 256

__device__ __forceinline__ int reflect101(int i, int n) {
    i = i < 0 ? -i : i;
    return i >= n ? 2 * n - 2 - i : i;
}

template <bool U8>
__global__ __launch_bounds__(PYR_BLOCK) void pyr_down_kernel(const float* __restrict__ src, int w, int h, void* __restrict__ dst, int cw, int ch) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cw || y >= ch) return;
    int xs[5];
#pragma unroll
    for (int i = 0; i < 5; i++) xs[i] = reflect101(2 * x - 2 + i, w);
    if (U8) {
        const int k[5] = {1, 4, 6, 4, 1};
        int s = 0;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const float* row = src + (size_t)reflect101(2 * y - 2 + j, h) * w;
            int r = 0;
#pragma unroll
            for (int i = 0; i < 5; i++) r += k[i] * (int)row[xs[i]];      // the views hold the 8-bit decode: integral 0..255
            s += k[j] * r;
        }
        ((uint8_t*)dst)[(size_t)y * cw + x] = (uint8_t)((s + 128) >> 8);
    } else {
        float rs[5];
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const float* row = src + (size_t)reflect101(2 * y - 2 + j, h) * w;
            float r = row[xs[0]];
            r = __fadd_rn(r, __fmul_rn(4.0f, row[xs[1]]));
            r = __fadd_rn(r, __fmul_rn(6.0f, row[xs[2]]));
            r = __fadd_rn(r, __fmul_rn(4.0f, row[xs[3]]));
            rs[j] = __fadd_rn(r, row[xs[4]]);
        }
        float s = rs[0];
        s = __fadd_rn(s, __fmul_rn(4.0f, rs[1]));
        s = __fadd_rn(s, __fmul_rn(6.0f, rs[2]));
        s = __fadd_rn(s, __fmul_rn(4.0f, rs[3]));
        s = __fadd_rn(s, rs[4]);
        ((float*)dst)[(size_t)y * cw + x] = __fmul_rn(s, 0.00390625f);
    }
}

// src: a fine view [h][w] (float32); dst: [(h + 1) / 2][(w + 1) / 2] bytes (u8) or float32, on ctx's device, written on ctx's stream
int launch_pyr_down(tsar_ctx* ctx, const float* src, int w, int h, void* dst, bool u8) {
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    const dim3 grid((cw + 63) / 64, (ch + 3) / 4);
    {
        ScopedKernelTimer tm(ctx, "pyr_down");
        if (u8) hipLaunchKernelGGL(pyr_down_kernel<true>, grid, dim3(PYR_BLOCK), 0, ctx->stream, src, w, h, dst, cw, ch);
        else hipLaunchKernelGGL(pyr_down_kernel<false>, grid, dim3(PYR_BLOCK), 0, ctx->stream, src, w, h, dst, cw, ch);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    return TSAR_OK;
}

// ---- the geometric-consistency pass coarse to fine (tsar_geom_pyramid / tsar_pyramid_planes) -------------------------------------
// Coarse pixel (x, y) lies on fine pixel (2x, 2y) (the coarse K is the fine one with fx, fy, cx, cy halved).  Both kernels only move
// values, one thread per coarse pixel: memory-bound passes over a quarter of the fine map.

// A source view's depth map one level down: Df[2y][2x] if > 0, else the first value > 0 among Df[2y][2x+1], Df[2y+1][2x],
// Df[2y+1][2x+1] that lies inside the image, else 0 (no estimate).  (NaN is not > 0: it is skipped like a hole.)
__global__ __launch_bounds__(PYR_BLOCK) void geom_pyramid_kernel(const float* __restrict__ src, int w, int h, float* __restrict__ dst, int cw, int ch) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cw || y >= ch) return;
    const int fx = 2 * x, fy = 2 * y;        // inside: cw = (w + 1) / 2, ch = (h + 1) / 2
    const bool right = fx + 1 < w, below = fy + 1 < h;
    const float* row0 = src + (size_t)fy * w;
    float d = row0[fx];
    if (!(d > 0.0f)) {
        const float d1 = right ? row0[fx + 1] : 0.0f;
        const float d2 = below ? row0[w + fx] : 0.0f;
        const float d3 = right && below ? row0[w + fx + 1] : 0.0f;
        d = d1 > 0.0f ? d1 : d2 > 0.0f ? d2 : d3 > 0.0f ? d3 : 0.0f;
    }
    dst[(size_t)y * cw + x] = d;
}

// Plane decimation: the coarse plane at (x, y) is the fine plane at (2x, 2y), bit for bit (planes (n, d) are metric, getD_cu).
__global__ __launch_bounds__(PYR_BLOCK) void pm_pyramid_planes_kernel(const float4* __restrict__ src, int w, float4* __restrict__ dst, int cw, int ch) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= cw || y >= ch) return;
    dst[(size_t)y * cw + x] = src[(size_t)(2 * y) * w + 2 * x];
}

// src: a fine depth map [h][w]; dst: [(h + 1) / 2][(w + 1) / 2]; both on ctx's device, written on ctx's stream
int launch_geom_pyramid(tsar_ctx* ctx, const float* src, int w, int h, float* dst) {
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    const dim3 grid((cw + 63) / 64, (ch + 3) / 4);
    {
        ScopedKernelTimer tm(ctx, "geom_pyramid");
        hipLaunchKernelGGL(geom_pyramid_kernel, grid, dim3(PYR_BLOCK), 0, ctx->stream, src, w, h, dst, cw, ch);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    return TSAR_OK;
}
// src: fine planes [h][w]; dst: [(h + 1) / 2][(w + 1) / 2]
int launch_pyramid_planes(tsar_ctx* ctx, const float4* src, int w, int h, float4* dst) {
    const int cw = (w + 1) / 2, ch = (h + 1) / 2;
    const dim3 grid((cw + 63) / 64, (ch + 3) / 4);
    {
        ScopedKernelTimer tm(ctx, "pm_pyramid_planes");
        hipLaunchKernelGGL(pm_pyramid_planes_kernel, grid, dim3(PYR_BLOCK), 0, ctx->stream, src, w, dst, cw, ch);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    return TSAR_OK;
}
