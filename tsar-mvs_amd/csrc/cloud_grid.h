// cloud_grid.h — what the operators on point clouds share (cloud_distance_kernels.hip, cloud_voxel_kernels.hip,
// cloud_neighbor_kernels.hip, cloud_normal_kernels.hip).  Inlined into their kernels from here: the candidate rule, the order-preserving
// float codes, the float64 cell function of include/tsar.h, the wave reductions and, for the three searches, the grid of edge
// R (1 + 2^-10), its 16-byte records, the walk over a query's nine key ranges and the query key of a sorted record.  Compiled once, in
// cloud_grid.hip, and declared here: the bounds pass over a cloud (cd_measure), the grid over those bounds (cd_grid), the radix sort of
// (key, index) pairs (cd_sort), the sorted index of a cloud's cells with its records (cd_index) and, for the two searches of a cloud among
// its own points, everything up to the max_pairs refusal (cd_self_search).
#pragma once
#include <float.h>
#include <math.h>

#include <functional>

#include "tsar_dev.h"

#define CD_BLOCK 256

__device__ __forceinline__ bool cd_candidate(float x, float y, float z) { return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX; }   // NaN fails
// unsigned codes in the order of the floats they stand for (-0.0 below +0.0: the same double either way)
__device__ __forceinline__ uint32_t cd_code(float f) { const uint32_t u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
// the cell coordinate of include/tsar.h, as a double: floor(((double)p - (double)o) / e), the quotient correctly rounded
__device__ __forceinline__ double cd_cell(float p, double o, double e) { return floor(((double)p - o) / e); }

__device__ __forceinline__ uint32_t cd_wave_min(uint32_t v) { for (int s = 32; s > 0; s >>= 1) { const uint32_t o = __shfl_xor(v, s, 64); v = o < v ? o : v; } return v; }
__device__ __forceinline__ uint32_t cd_wave_max(uint32_t v) { for (int s = 32; s > 0; s >>= 1) { const uint32_t o = __shfl_xor(v, s, 64); v = o > v ? o : v; } return v; }
__device__ __forceinline__ unsigned long long cd_wave_sum(unsigned long long v) { for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64); return v; }

static inline unsigned cd_blocks(long long n) { return (unsigned)((n + CD_BLOCK - 1) / CD_BLOCK); }

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

// a sorted record's cell key (3 x 20 bits) as the query key cd_query_range reads (3 x 21 bits, each coordinate + 2)
__device__ __forceinline__ unsigned long long cd_self_query_key(unsigned long long key) {
    return (((key >> 40) + 2ull) << 42) | ((((key >> 20) & 0xfffffull) + 2ull) << 21) | ((key & 0xfffffull) + 2ull);
}

// ---- cloud_grid.hip's host steps: every one works on the call's frame and leaves a failure in it (false: the caller returns f.finish()) ----

// The counters of one call, a piece of the frame: what the bounds pass fills, and two slots that are the operator's own (the searches
// count their candidate queries and their pairs there), so that one upload zeroes them all.
struct CdCounters {
    uint32_t bounds[6];                   // codes of the per-axis minima [0..2] and maxima [3..5] of the candidates
    uint32_t pad[2];
    unsigned long long n_cand;
    unsigned long long own[2];
};
struct CdBounds { float lo[3], hi[3]; long long n_cand; };   // lo / hi mean nothing when n_cand is 0

// *dc initialised, the bounds pass over the cloud (timer cloud_bounds), the result read back: the stream is idle on return
bool cd_measure(CallFrame& f, const float* pts, long long n, int stride, CdCounters* dc, CdBounds& b);
// the grid of edge `edge` whose origin is b.lo; the frame fails with `refusal` when an axis has `limit` cells or more
bool cd_grid(CallFrame& f, const CdBounds& b, double edge, int limit, const char* refusal, CdGrid& g);
// keys_in / vals_in sorted into keys_out / vals_out (bits [0, end_bit)); the sort's scratch is a piece of the frame
bool cd_sort(CallFrame& f, const char* name, unsigned long long* keys_in, unsigned long long* keys_out, uint32_t* vals_in, uint32_t* vals_out, long long n, int end_bit);
// The cloud's 60-bit z-major cell keys (timer cloud_keys), sorted with the indices (cloud_sort; stable: equal keys keep index order;
// the non-candidates last) and the candidates copied into key order as records (cloud_gather).  also_keys, if any, launches the
// caller's own key kernel in the cloud_keys group.
struct CdIndex { unsigned long long* keys; uint32_t* vals; CdRec* rec; };   // n sorted keys, n sorted indices, n_cand records
bool cd_index(CallFrame& f, const float* pts, long long n, int stride, long long n_cand, const CdGrid& g, CdIndex& ix, const std::function<void()>& also_keys = nullptr);
// What a search of a cloud among its own points begins with (tsar_cloud_neighbors, tsar_cloud_normals; the frame names the entry in the
// two refusals): the call's counters, cd_measure, cd_grid with cells of `edge` (refused from CD_MAX_EXTENT cells on an axis), cd_index,
// the pair count (timer cloud_pairs: per sorted record the sizes of its nine key ranges, into own[0]) read back and given to *pairs_out,
// and the max_pairs refusal.  Without a candidate there is no grid and no index, and no pair.  own[1] is the caller's; the stream is idle
// on return.
struct CdSelf { CdCounters* dc; long long n_cand; CdGrid g; CdIndex ix; };
bool cd_self_search(CallFrame& f, const float* pts, long long n, int stride, double edge, long long max_pairs, int64_t* pairs_out, CdSelf& s);
