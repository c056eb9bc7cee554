// cloud_neighbor_kernels.hip — neighbourhood statistics of one point cloud (include/tsar.h tsar_cloud_neighbors): per point the number of
// other points within a radius R and the k smallest squared distances among them.  The result is the brute-force definition written
// there (a count and an order statistic of float32 d2 over every other candidate); the uniform grid only decides which pairs are looked
// at, and every pair with d2 <= fl(R * R) lies in the 27 cells around the point's (include/tsar.h says why), so no bit of the result
// depends on it, nor on the order in which a point's neighbours arrive.
//
// Per call:  bounds of the candidates -> 60-bit z-major cell keys, radix-sorted with the indices
//            -> the candidates copied into key order as 16-byte records (x, y, z, index)
//            -> the pair count: per sorted record the sizes of its 9 key ranges (the record itself is in one of them), and the
//               max_pairs refusal                               [so far: cd_self_search of cloud_grid.hip, shared with cloud_normal_kernels.hip]
//            -> the search kernel: lane t takes sorted record t as its query, so that a wave's lanes walk the same cells and one sort
//               serves queries and targets; a count, and a sorted list of the KCAP smallest d2 kept in registers.
// The list is indexed by compile-time constants only (a template over KCAP, every loop over it unrolled): insertion is a chain of
// integer min / max on the bit patterns (d2 >= +0 and never NaN, so the bits order like the values), run only when some lane of the wave
// holds a value below its list's last entry.  No atomics on the per-point outputs, no LDS, no scratch.
#include "cloud_grid.h"

#define CN_INF_BITS 0x7f800000u

// One lane per candidate, in key order.  KCAP = 0: the count only.  k <= KCAP values of the list are written.
template <int KCAP>
__global__ __launch_bounds__(CD_BLOCK) void cn_search_kernel(const unsigned long long* __restrict__ keys, const CdRec* __restrict__ rec, uint32_t n_cand, CdGrid g, float r2,
                                                             int k, int32_t* __restrict__ count_out, float* __restrict__ knn_out) {
    const uint32_t t = blockIdx.x * CD_BLOCK + threadIdx.x;
    if (t >= n_cand) return;
    const CdRec q = rec[t];
    const unsigned long long qkey = cd_self_query_key(keys[t]);
    uint32_t a[KCAP > 0 ? KCAP : 1];
#pragma unroll
    for (int s = 0; s < KCAP; s++) a[s] = CN_INF_BITS;
    int32_t cnt = 0;
    for (int r = 0; r < 9; r++) {
        uint32_t b, e;
        if (!cd_query_range(qkey, r, g, keys, n_cand, b, e)) continue;
#pragma unroll 4
        for (uint32_t u = b; u < e; u++) {       // (unrolled like cd_query_kernel: four record loads in flight per lane)
            const CdRec c = rec[u];
            const float dx = q.x - c.x, dy = q.y - c.y, dz = q.z - c.z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;                  // no fused operation: the library is built with -ffp-contract=off
            const bool in = d2 <= r2 && c.j != q.j;                          // the point itself is excluded by index, not by distance
            cnt += in ? 1 : 0;
            if constexpr (KCAP > 0) {
                uint32_t x = in ? __float_as_uint(d2) : CN_INF_BITS;
                if (__ballot(x < a[KCAP - 1])) {                             // wave-uniform among the lanes still in the loop
#pragma unroll
                    for (int s = 0; s < KCAP; s++) {
                        const uint32_t lo = a[s] < x ? a[s] : x;
                        x = a[s] < x ? x : a[s];
                        a[s] = lo;
                    }
                }
            }
        }
    }
    if (count_out) count_out[q.j] = cnt;
    if constexpr (KCAP > 0) {
        float* o = knn_out + (size_t)q.j * k;
#pragma unroll
        for (int s = 0; s < KCAP; s++)
            if (s < k) o[s] = __uint_as_float(a[s]);
    }
}

// the records that are no candidates: count -1, every distance +inf (the search kernel writes the candidates' rows)
__global__ __launch_bounds__(CD_BLOCK) void cn_fill_kernel(const float* __restrict__ pts, long long n, int stride, int k, int32_t* __restrict__ count_out,
                                                           float* __restrict__ knn_out) {
    const long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float* p = pts + (size_t)i * stride;
    if (cd_candidate(p[0], p[1], p[2])) return;
    if (count_out) count_out[i] = -1;
    if (knn_out)
        for (int s = 0; s < k; s++) knn_out[(size_t)i * k + s] = INFINITY;
}

template <int KCAP>
static void cn_launch_search(hipStream_t st, const unsigned long long* keys, const CdRec* rec, uint32_t n_cand, const CdGrid& g, float r2, int k, int32_t* count_out,
                             float* knn_out) {
    hipLaunchKernelGGL(cn_search_kernel<KCAP>, dim3(cd_blocks(n_cand)), dim3(CD_BLOCK), 0, st, keys, rec, n_cand, g, r2, k, count_out, knn_out);
}

// cloud and the two per-point outputs are device pointers (the frame's views of the caller's buffers); n_valid_out and pairs_out are the
// caller's host memory.  The arguments have been checked (tsar_api.hip): 0 <= n < 2^31, 0 <= k <= TSAR_CLOUD_KNN_MAX, knn_out only with k > 0.
int run_cloud_neighbors(CallFrame& f, const float* cloud, long long n, int stride, float r2, double edge, int k, long long max_pairs, int32_t* count_out, float* knn_out,
                        int64_t* n_valid_out, int64_t* pairs_out) {
    tsar_ctx* ctx = f.ctx;
    hipStream_t st = ctx->stream;
    CdSelf s;
    if (!cd_self_search(f, cloud, n, stride, edge, max_pairs, pairs_out, s)) return f.finish();
    const long long n_cand = s.n_cand;
    const CdGrid& g = s.g;
    const CdIndex& ix = s.ix;
    if (f.ok() && n > 0 && n_cand < n && (count_out || knn_out)) {
        ScopedKernelTimer tm(ctx, "cloud_neighbors");
        hipLaunchKernelGGL(cn_fill_kernel, dim3(cd_blocks(n)), dim3(CD_BLOCK), 0, st, cloud, n, stride, k, count_out, knn_out);
    }
    f.launched();
    if (f.ok() && n_cand > 0 && (count_out || knn_out)) {
        ScopedKernelTimer tm(ctx, "cloud_neighbors");
        const int kk = knn_out ? k : 0;          // the smallest list that holds k
        if (kk == 0) cn_launch_search<0>(st, ix.keys, ix.rec, (uint32_t)n_cand, g, r2, 0, count_out, nullptr);
        else if (kk <= 4) cn_launch_search<4>(st, ix.keys, ix.rec, (uint32_t)n_cand, g, r2, k, count_out, knn_out);
        else if (kk <= 8) cn_launch_search<8>(st, ix.keys, ix.rec, (uint32_t)n_cand, g, r2, k, count_out, knn_out);
        else if (kk <= 16) cn_launch_search<16>(st, ix.keys, ix.rec, (uint32_t)n_cand, g, r2, k, count_out, knn_out);
        else cn_launch_search<32>(st, ix.keys, ix.rec, (uint32_t)n_cand, g, r2, k, count_out, knn_out);
    }
    f.launched();
    if (n_valid_out) *n_valid_out = (int64_t)n_cand;
    return f.finish();
}
