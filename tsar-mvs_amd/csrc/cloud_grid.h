// cloud_grid.h — what the operators on point clouds share (cloud_distance_kernels.hip, cloud_voxel_kernels.hip,
// cloud_neighbor_kernels.hip): the candidate rule, the order-preserving float codes, the float64 cell function of include/tsar.h, the
// bounds pass over a cloud, the radix sort of (key, index) pairs and, for the two searches, the grid of edge R (1 + 2^-10), its 16-byte
// records and the walk over a query's nine key ranges.  Kernels here are `static`: each translation unit that includes this file carries
// its own copy.
#pragma once
#include <float.h>
#include <math.h>
#include <rocprim/device/device_radix_sort.hpp>

#include "tsar_dev.h"

#define CD_BLOCK 256

__device__ __forceinline__ bool cd_candidate(float x, float y, float z) { return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX; }   // NaN fails
// unsigned codes in the order of the floats they stand for (-0.0 below +0.0: the same double either way)
__device__ __forceinline__ uint32_t cd_code(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
static inline float cd_decode(uint32_t c) { const uint32_t u = (c & 0x80000000u) ? (c & 0x7fffffffu) : ~c; float f; memcpy(&f, &u, 4); return f; }
// the cell coordinate of include/tsar.h, as a double: floor(((double)p - (double)o) / e), the quotient correctly rounded
__device__ __forceinline__ double cd_cell(float p, double o, double e) { return floor(((double)p - o) / e); }
static inline double cd_cell_host(float p, double o, double e) { return floor(((double)p - o) / e); }

__device__ __forceinline__ uint32_t cd_wave_min(uint32_t v) { for (int s = 32; s > 0; s >>= 1) { const uint32_t o = __shfl_xor(v, s, 64); v = o < v ? o : v; } return v; }
__device__ __forceinline__ uint32_t cd_wave_max(uint32_t v) { for (int s = 32; s > 0; s >>= 1) { const uint32_t o = __shfl_xor(v, s, 64); v = o > v ? o : v; } return v; }
__device__ __forceinline__ unsigned long long cd_wave_sum(unsigned long long v) { for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64); return v; }

// bounds[0..2] = codes of the per-axis minima, bounds[3..5] = of the maxima, *count = the candidates
static __global__ __launch_bounds__(CD_BLOCK) void cd_bounds_kernel(const float* __restrict__ pts, long long n, int stride, uint32_t* __restrict__ bounds,
                                                                    unsigned long long* __restrict__ count) {
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    unsigned long long cnt = 0;
    for (long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * CD_BLOCK) {
        const float* p = pts + (size_t)i * stride;
        const float x = p[0], y = p[1], z = p[2];
        if (!cd_candidate(x, y, z)) continue;
        const uint32_t c[3] = {cd_code(x), cd_code(y), cd_code(z)};
        for (int a = 0; a < 3; a++) { lo[a] = c[a] < lo[a] ? c[a] : lo[a]; hi[a] = c[a] > hi[a] ? c[a] : hi[a]; }
        cnt++;
    }
    for (int a = 0; a < 3; a++) { lo[a] = cd_wave_min(lo[a]); hi[a] = cd_wave_max(hi[a]); }
    cnt = cd_wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) {
        for (int a = 0; a < 3; a++) { atomicMin(&bounds[a], lo[a]); atomicMax(&bounds[3 + a], hi[a]); }
        atomicAdd(count, cnt);
    }
}

static inline unsigned cd_blocks(long long n) { return (unsigned)((n + CD_BLOCK - 1) / CD_BLOCK); }
static inline unsigned cd_bounds_blocks(long long n) { return cd_blocks(n) < 2048u ? cd_blocks(n) : 2048u; }

#define CD_T_NONE (1ull << 60)            // key of a target that is no candidate: above every cell key (3 x 20 bits)
#define CD_Q_NONE (1ull << 63)            // key of a query that is no candidate: above every query key (3 x 21 bits)
#define CD_MAX_EXTENT (1 << 20)           // cells per axis: refused from here on

struct CdGrid {
    double ox, oy, oz;                    // per-axis minimum of the candidate targets
    double e;                             // cell edge (double)R * (1 + 2^-10)
    int ex, ey, ez;                       // cells per axis: the targets' cells are 0 .. ex - 1
};
struct __align__(16) CdRec { float x, y, z; uint32_t j; };

__device__ __forceinline__ int cd_clampi(double c, int lo, int hi) { return c < (double)lo ? lo : (c > (double)hi ? hi : (int)c); }

// [b, e) = the sorted keys in [klo, khi]: a binary search for the start, then a gallop for the end (a range is short next to n)
__device__ __forceinline__ void cd_range(const unsigned long long* __restrict__ keys, uint32_t n, unsigned long long klo, unsigned long long khi, uint32_t& b, uint32_t& e) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { const uint32_t mid = lo + ((hi - lo) >> 1); if (keys[mid] < klo) lo = mid + 1; else hi = mid; }
    b = lo;
    uint32_t l = lo, h = lo, step = 1;
    while (h < n && keys[h] <= khi) { l = h + 1; h = (n - h > step) ? h + step : n; step <<= 1; }
    while (l < h) { const uint32_t mid = l + ((h - l) >> 1); if (keys[mid] <= khi) l = mid + 1; else h = mid; }
    e = l;
}

// the query's r-th range, r = 3 (dz + 1) + (dy + 1): false when that row of cells lies outside the grid
__device__ __forceinline__ bool cd_query_range(unsigned long long qkey, int r, const CdGrid& g, const unsigned long long* __restrict__ tkeys, uint32_t n_cand,
                                               uint32_t& b, uint32_t& e) {
    const int cx = (int)(qkey & 0x1fffffu) - 2, cy = (int)((qkey >> 21) & 0x1fffffu) - 2, cz = (int)((qkey >> 42) & 0x1fffffu) - 2;
    const int ty = cy + (r % 3) - 1, tz = cz + (r / 3) - 1;
    const int xlo = cx - 1 < 0 ? 0 : cx - 1, xhi = cx + 1 > g.ex - 1 ? g.ex - 1 : cx + 1;
    if (ty < 0 || ty >= g.ey || tz < 0 || tz >= g.ez || xlo > xhi) return false;
    const unsigned long long row = ((unsigned long long)tz << 40) | ((unsigned long long)ty << 20);
    cd_range(tkeys, n_cand, row | (unsigned)xlo, row | (unsigned)xhi, b, e);
    return true;
}

// keys_in / vals_in sorted into keys_out / vals_out (bits [0, end_bit)); the sort's scratch is a piece of the frame
template <typename F>
static bool cd_sort(F& f, const char* name, unsigned long long* keys_in, unsigned long long* keys_out, uint32_t* vals_in, uint32_t* vals_out, long long n, int end_bit) {
    size_t bytes = 0;
    if (!f.ok() || !f.hip(rocprim::radix_sort_pairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, end_bit, f.ctx->stream), "rocprim::radix_sort_pairs sizing")) return false;
    void* tmp = f.template tmp<char>(bytes);
    if (!f.ok()) return false;
    ScopedKernelTimer tm(f.ctx, name);
    return f.hip(rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, end_bit, f.ctx->stream), "rocprim::radix_sort_pairs");
}
