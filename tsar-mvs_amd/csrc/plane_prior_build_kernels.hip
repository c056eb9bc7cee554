// plane_prior_build_kernels.hip — the plane prior built from a filtered depth map (tsar_build_plane_prior; include/tsar.h states the
// arithmetic, tests/test_plane_prior_build_cpu.py restates it in numpy).  A hierarchical lattice triangulation: level l cuts the image
// into cells of edge cell << l, every cell keeps its best candidate pixel as its support point, four neighbouring support points make
// a quad of two triangles, and a pixel takes the first triangle that contains it, finest level first.  Everything up to the choice of
// the triangle is integer arithmetic on minima, so no order of arrival can show; the plane of the chosen triangle is one small
// float64 solve per pixel (-ffp-contract=off: one IEEE operation per operator), rounded once to float32.
//
// A support point is one 64-bit key, (score bits << 32) | (y << 16) | x: non-negative floats order like their bit patterns, and (y, x)
// orders like the raster index, so the key's minimum is the minimum of (score, raster index).  PPB_EMPTY (all ones) is a cell without
// a candidate; no candidate has that key, because a candidate's score is finite.
//   ppb_support0_kernel   one lane per level-0 cell walks its cell x cell pixels, neighbouring lanes read neighbouring row segments
//   ppb_coarsen_kernel    one lane per coarser cell: the minimum of its (up to) four children
//   ppb_lookup_kernel     one lane per pixel, the lanes of a wave along x: per level the 3 x 3 cells around the pixel's own, the four
//                         quads they form, integer edge tests; then the solve, once
// The grids of all levels lie behind one another in one temporary of the call (a few MB at 6048 x 4032: L2-resident).  Every index
// into a grid or a map is derived from grid integers and clamped before use.  No LDS, no scratch, no atomics.
#include "tsar_device_math.h"

typedef const float __attribute__((address_space(1)))* ppb_f32_ptr;
typedef const unsigned long long __attribute__((address_space(1)))* ppb_u64_ptr;

#define PPB_BLOCK 256      // 64 x 4 pixels (look-up); 256 cells (supports)
#define PPB_EMPTY 0xFFFFFFFFFFFFFFFFull

struct PpbLevels {
    int n;                                        // levels in use, 1 .. TSAR_PLANE_PRIOR_MAX_LEVELS
    int cell;                                     // level-0 cell edge
    int gw[TSAR_PLANE_PRIOR_MAX_LEVELS];          // cells per row and per column of level l
    int gh[TSAR_PLANE_PRIOR_MAX_LEVELS];
    int off[TSAR_PLANE_PRIOR_MAX_LEVELS];         // first key of level l in the grid buffer
};

__global__ __launch_bounds__(PPB_BLOCK) void ppb_support0_kernel(const float* __restrict__ depth, const float* __restrict__ score, int w, int h,
                                                                 int cell, int gw, int gh, unsigned long long* __restrict__ grid) {
    const int c = blockIdx.x * PPB_BLOCK + threadIdx.x;
    if (c >= gw * gh) return;
    const int j = c / gw, i = c - j * gw;
    const int x0 = i * cell, y0 = j * cell;
    const int x1 = min(x0 + cell, w), y1 = min(y0 + cell, h);   // partial cells in the last column and row
    const float inf = __builtin_inff();
    unsigned long long best = PPB_EMPTY;
    for (int y = y0; y < y1; y++) {
        for (int x = x0; x < x1; x++) {
            const size_t p = (size_t)y * w + x;
            const float D = ((ppb_f32_ptr)depth)[p];
            bool cand = D > 0.0f && D < inf;                     // (NaN and -0.0 fail)
            unsigned int sb = 0;
            if (score) {
                const float s = ((ppb_f32_ptr)score)[p];
                cand = cand && s >= 0.0f && s < inf;             // (NaN fails; -0.0 passes and counts as 0: its sign bit is dropped)
                sb = __float_as_uint(s) & 0x7FFFFFFFu;
            }
            const unsigned long long key = ((unsigned long long)sb << 32) | ((unsigned int)y << 16) | (unsigned int)x;
            if (cand && key < best) best = key;
        }
    }
    grid[c] = best;
}

__global__ __launch_bounds__(PPB_BLOCK) void ppb_coarsen_kernel(const unsigned long long* __restrict__ fine, int fw, int fh, int gw, int gh,
                                                                unsigned long long* __restrict__ coarse) {
    const int c = blockIdx.x * PPB_BLOCK + threadIdx.x;
    if (c >= gw * gh) return;
    const int j = c / gw, i = c - j * gw;
    unsigned long long best = PPB_EMPTY;
#pragma unroll
    for (int dj = 0; dj < 2; dj++)
#pragma unroll
        for (int di = 0; di < 2; di++) {
            const int fi = 2 * i + di, fj = 2 * j + dj;
            if (fi < fw && fj < fh) {
                const unsigned long long k = ((ppb_u64_ptr)fine)[(size_t)fj * fw + fi];
                if (k < best) best = k;
            }
        }
    coarse[c] = best;
}

// orient(A, B, C) = (Bx - Ax)(Cy - Ay) - (By - Ay)(Cx - Ax): each product is below w * h in magnitude, the difference needs 64 bits
DEVFN long long ppb_orient(int ax, int ay, int bx, int by, int cx, int cy) {
    return (long long)(bx - ax) * (long long)(cy - ay) - (long long)(by - ay) * (long long)(cx - ax);
}
// the pixel is inside (A, B, C) when the triangle has an area and the three edge functions are each zero or of the area's sign
DEVFN bool ppb_inside(int ax, int ay, int bx, int by, int cx, int cy, int x, int y) {
    const long long area2 = ppb_orient(ax, ay, bx, by, cx, cy);
    if (area2 == 0) return false;
    const long long e0 = ppb_orient(ax, ay, bx, by, x, y), e1 = ppb_orient(bx, by, cx, cy, x, y), e2 = ppb_orient(cx, cy, ax, ay, x, y);
    return area2 > 0 ? (e0 >= 0 && e1 >= 0 && e2 >= 0) : (e0 <= 0 && e1 <= 0 && e2 <= 0);
}

__global__ __launch_bounds__(PPB_BLOCK) void ppb_lookup_kernel(const DevScene* __restrict__ sc, const float* __restrict__ depth,
                                                               const unsigned long long* __restrict__ grid, PpbLevels lv,
                                                               float* __restrict__ depth_out, float* __restrict__ normal_out,
                                                               uint8_t* __restrict__ level_out) {
    const int w = sc->w, h = sc->h;
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= w || y >= h) return;                          // partial last tiles in x and in y
    const size_t p = (size_t)y * w + x;
    const int i0 = x / lv.cell, j0 = y / lv.cell;          // the pixel's cell at level l is (i0 >> l, j0 >> l)
    int level = 255;
    int ax = 0, ay = 0, bx = 0, by = 0, cx = 0, cy = 0;
    for (int l = 0; l < lv.n && level == 255; l++) {
        const int gw = lv.gw[l], gh = lv.gh[l];
        ppb_u64_ptr g = (ppb_u64_ptr)grid + lv.off[l];
        const int i = min(i0 >> l, gw - 1), j = min(j0 >> l, gh - 1);   // (inside the grid by construction; the clamp costs nothing)
        // the 3 x 3 cells around (i, j); a cell outside the grid reads as empty, so a quad that needs it does not exist
        unsigned long long k[3][3];
#pragma unroll
        for (int dj = 0; dj < 3; dj++)
#pragma unroll
            for (int di = 0; di < 3; di++) {
                const int ci = i + di - 1, cj = j + dj - 1;
                const bool in = ci >= 0 && ci < gw && cj >= 0 && cj < gh;
                const int cci = min(max(ci, 0), gw - 1), ccj = min(max(cj, 0), gh - 1);
                const unsigned long long v = g[(size_t)ccj * gw + cci];
                k[dj][di] = in ? v : PPB_EMPTY;
            }
        // quads with origin (i-1, j-1), (i, j-1), (i-1, j), (i, j), in that order
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int qi = q & 1, qj = q >> 1;
            const unsigned long long k00 = k[qj][qi], k10 = k[qj][qi + 1], k01 = k[qj + 1][qi], k11 = k[qj + 1][qi + 1];
            if (level != 255 || k00 == PPB_EMPTY || k10 == PPB_EMPTY || k01 == PPB_EMPTY || k11 == PPB_EMPTY) continue;
            const int x00 = (int)(k00 & 0xFFFF), y00 = (int)((k00 >> 16) & 0xFFFF), x10 = (int)(k10 & 0xFFFF), y10 = (int)((k10 >> 16) & 0xFFFF);
            const int x01 = (int)(k01 & 0xFFFF), y01 = (int)((k01 >> 16) & 0xFFFF), x11 = (int)(k11 & 0xFFFF), y11 = (int)((k11 >> 16) & 0xFFFF);
            const long long o1 = ppb_orient(x00, y00, x11, y11, x10, y10), o2 = ppb_orient(x00, y00, x11, y11, x01, y01);
            const bool main_diag = (o1 > 0 && o2 < 0) || (o1 < 0 && o2 > 0);
            // first triangle: (P00, P10, P11) or (P00, P10, P01); second: (P00, P11, P01) or (P10, P11, P01)
            const int t1cx = main_diag ? x11 : x01, t1cy = main_diag ? y11 : y01;
            const int t2ax = main_diag ? x00 : x10, t2ay = main_diag ? y00 : y10;
            if (ppb_inside(x00, y00, x10, y10, t1cx, t1cy, x, y)) {
                level = l; ax = x00; ay = y00; bx = x10; by = y10; cx = t1cx; cy = t1cy;
            } else if (ppb_inside(t2ax, t2ay, x11, y11, x01, y01, x, y)) {
                level = l; ax = t2ax; ay = t2ay; bx = x11; by = y11; cx = x01; cy = y01;
            }
        }
    }
    float Dp = 0.0f, n0 = 0.0f, n1 = 0.0f, n2 = 0.0f;
    if (level != 255) {
        // (support points are candidates' pixels: inside the image by construction; the clamp keeps a gather inside the map regardless)
        ax = min(max(ax, 0), w - 1); bx = min(max(bx, 0), w - 1); cx = min(max(cx, 0), w - 1);
        ay = min(max(ay, 0), h - 1); by = min(max(by, 0), h - 1); cy = min(max(cy, 0), h - 1);
        const double wA = 1.0 / (double)((ppb_f32_ptr)depth)[(size_t)ay * w + ax];
        const double wB = 1.0 / (double)((ppb_f32_ptr)depth)[(size_t)by * w + bx];
        const double wC = 1.0 / (double)((ppb_f32_ptr)depth)[(size_t)cy * w + cx];
        const double area2 = (double)ppb_orient(ax, ay, bx, by, cx, cy);
        const double dB = wB - wA, dC = wC - wA;
        const double gx = (dB * (double)(cy - ay) - dC * (double)(by - ay)) / area2;
        const double gy = (dC * (double)(bx - ax) - dB * (double)(cx - ax)) / area2;
        const double wp = (wA + gx * (double)(x - ax)) + gy * (double)(y - ay);
        if (wp > 0.0) {                                    // (NaN fails; what a wild depth range can do to the sum: no prior then)
            const double c0 = (wA - gx * (double)ax) - gy * (double)ay;
            const float* K = sc->ref.K;
            const double m0 = ((double)K[0] * gx + (double)K[3] * gy) + (double)K[6] * c0;
            const double m1 = ((double)K[1] * gx + (double)K[4] * gy) + (double)K[7] * c0;
            const double m2 = ((double)K[2] * gx + (double)K[5] * gy) + (double)K[8] * c0;
            const double len = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
            const double q0 = -m0 / len, q1 = -m1 / len, q2 = -m2 / len;
            const float* R = sc->ref.Rorig;                // world = R^T camera, as compute_disp_kernel carries a normal out
            n0 = (float)(((double)R[0] * q0 + (double)R[3] * q1) + (double)R[6] * q2);
            n1 = (float)(((double)R[1] * q0 + (double)R[4] * q1) + (double)R[7] * q2);
            n2 = (float)(((double)R[2] * q0 + (double)R[5] * q1) + (double)R[8] * q2);
            Dp = (float)(1.0 / wp);
        } else {
            level = 255;
        }
    }
    if (depth_out) depth_out[p] = Dp;
    if (normal_out) { normal_out[3 * p] = n0; normal_out[3 * p + 1] = n1; normal_out[3 * p + 2] = n2; }
    if (level_out) level_out[p] = (uint8_t)level;
}

// the levels of a w x h image: level l exists while both grid dimensions are >= 2 and l < max_levels (0 = all that fit); returns the
// number of keys of all levels
static size_t ppb_levels(int w, int h, int cell, int max_levels, PpbLevels* lv) {
    lv->n = 0;
    lv->cell = cell;
    size_t total = 0;
    for (int l = 0; l < TSAR_PLANE_PRIOR_MAX_LEVELS && (max_levels == 0 || l < max_levels); l++) {
        const long long s = (long long)cell << l;
        const int gw = (int)((w + s - 1) / s), gh = (int)((h + s - 1) / s);
        if (gw < 2 || gh < 2) break;
        lv->gw[l] = gw; lv->gh[l] = gh; lv->off[l] = (int)total;
        total += (size_t)gw * gh;
        lv->n = l + 1;
    }
    for (int l = lv->n; l < TSAR_PLANE_PRIOR_MAX_LEVELS; l++) { lv->gw[l] = lv->gh[l] = 2; lv->off[l] = 0; }   // never read
    return total;
}

size_t plane_prior_build_grid_keys(int w, int h, int cell, int max_levels) {
    PpbLevels lv;
    return ppb_levels(w, h, cell, max_levels, &lv);
}

// depth, score (may be null) and the outputs (each may be null) are [h][w] on the device; grid: plane_prior_build_grid_keys() keys
int launch_plane_prior_build(tsar_ctx* ctx, const float* depth, const float* score, int cell, int max_levels, unsigned long long* grid,
                             float* depth_out, float* normal_out, uint8_t* level_out) {
    PpbLevels lv;
    ppb_levels(ctx->w, ctx->h, cell, max_levels, &lv);
    if (lv.n < 1) { ctx->err = "tsar_build_plane_prior: the image is too small for one level"; return TSAR_ERR_INVALID; }
    {
        ScopedKernelTimer tm(ctx, "plane_prior_build_supports");
        const int cells = lv.gw[0] * lv.gh[0];
        hipLaunchKernelGGL(ppb_support0_kernel, dim3((cells + PPB_BLOCK - 1) / PPB_BLOCK), dim3(PPB_BLOCK), 0, ctx->stream, depth, score, ctx->w,
                           ctx->h, cell, lv.gw[0], lv.gh[0], grid + lv.off[0]);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    if (lv.n > 1) {
        ScopedKernelTimer tm(ctx, "plane_prior_build_levels");
        for (int l = 1; l < lv.n; l++) {
            const int cells = lv.gw[l] * lv.gh[l];
            hipLaunchKernelGGL(ppb_coarsen_kernel, dim3((cells + PPB_BLOCK - 1) / PPB_BLOCK), dim3(PPB_BLOCK), 0, ctx->stream, grid + lv.off[l - 1],
                               lv.gw[l - 1], lv.gh[l - 1], lv.gw[l], lv.gh[l], grid + lv.off[l]);
        }
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    {
        ScopedKernelTimer tm(ctx, "plane_prior_build");
        const dim3 tiles((ctx->w + 63) / 64, (ctx->h + 3) / 4);
        hipLaunchKernelGGL(ppb_lookup_kernel, tiles, dim3(PPB_BLOCK), 0, ctx->stream, ctx->dscene, depth, grid, lv, depth_out, normal_out, level_out);
    }
    TSAR_HIP_TRY(ctx, hipGetLastError());
    return TSAR_OK;
}
