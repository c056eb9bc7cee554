// cloud_distance_kernels.hip — truncated nearest-neighbour distances between two point clouds (include/tsar.h tsar_cloud_distance).
// The result is the brute-force definition written there (a minimum of float32 d2 over every candidate target); the uniform grid below
// only decides which pairs are looked at, and every pair with d2 <= fl(R * R) lies in the 27 cells around the query's
// (include/tsar.h says why), so no bit of the result depends on it.
//
// Per call:  bounds of the candidate targets (integer atomics on order-preserving float codes: a minimum, exact in any order)
//            -> 60-bit z-major cell keys of the targets, radix-sorted with their indices (stable: equal keys keep index order)
//            -> the targets copied into key order as 16-byte records (x, y, z, index)        [these three: cloud_grid.hip]
//            -> 63-bit cell keys of the queries, radix-sorted, so that a wave's lanes walk the same cells
//            -> the pair count: per query the sizes of its 9 key ranges (cells x-1 .. x+1 of one (y, z) are one contiguous range)
//            -> the query kernel: one lane per query in key order, a running minimum of the 64-bit (d2 bits, index) code.
// No floating-point atomics and no order of arrival anywhere: the outputs are the same bits in every run.
// (The candidate rule, the float codes, the cell function, the grid and the walk over a query's key ranges are inlined from cloud_grid.h;
// the bounds pass, the sort and the targets' index are cloud_grid.hip's, shared with cloud_voxel_kernels.hip and cloud_neighbor_kernels.hip.)
#include "cloud_grid.h"

// a query's cell may lie outside the targets' grid: kept exactly from -2 (no cell of the grid is its neighbour) to extent + 1, plus 2
__global__ __launch_bounds__(CD_BLOCK) void cd_query_keys_kernel(const float* __restrict__ pts, long long n, int stride, CdGrid g,
                                                                 unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals,
                                                                 unsigned long long* __restrict__ n_valid) {
    const long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x;
    bool cand = false;
    if (i < n) {
        const float* p = pts + (size_t)i * stride;
        const float x = p[0], y = p[1], z = p[2];
        unsigned long long key = CD_Q_NONE;
        cand = cd_candidate(x, y, z);
        if (cand) {
            const unsigned long long cx = (unsigned)(cd_clampi(cd_cell(x, g.ox, g.e), -2, g.ex + 1) + 2), cy = (unsigned)(cd_clampi(cd_cell(y, g.oy, g.e), -2, g.ey + 1) + 2),
                                     cz = (unsigned)(cd_clampi(cd_cell(z, g.oz, g.e), -2, g.ez + 1) + 2);
            key = (cz << 42) | (cy << 21) | cx;
        }
        keys[i] = key;
        vals[i] = (uint32_t)i;
    }
    const unsigned long long m = __ballot(cand);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(n_valid, (unsigned long long)__popcll(m));
}

// *pairs += the number of targets in the 27 cells around every candidate query: what the query kernel would evaluate
__global__ __launch_bounds__(CD_BLOCK) void cd_pairs_kernel(const unsigned long long* __restrict__ qkeys, long long n_query, CdGrid g,
                                                            const unsigned long long* __restrict__ tkeys, uint32_t n_cand, unsigned long long* __restrict__ pairs) {
    const long long k = (long long)blockIdx.x * CD_BLOCK + threadIdx.x;
    unsigned long long cnt = 0;
    if (k < n_query) {
        const unsigned long long qkey = qkeys[k];
        if (qkey != CD_Q_NONE)
            for (int r = 0; r < 9; r++) {
                uint32_t b, e;
                if (cd_query_range(qkey, r, g, tkeys, n_cand, b, e)) cnt += e - b;
            }
    }
    cnt = cd_wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(pairs, cnt);
}

// one lane per query, in key order: the minimum over its 27 cells of the 64-bit code (d2 bits, index) — d2 >= +0, so the codes order
// like the distances and, among equal distances, like the indices
__global__ __launch_bounds__(CD_BLOCK) void cd_query_kernel(const float* __restrict__ query, int stride, const unsigned long long* __restrict__ qkeys,
                                                            const uint32_t* __restrict__ qvals, long long n_query, CdGrid g,
                                                            const unsigned long long* __restrict__ tkeys, const CdRec* __restrict__ rec, uint32_t n_cand, float r2,
                                                            int n_tol, const float* __restrict__ tol2, float* __restrict__ dist2_out, int32_t* __restrict__ index_out,
                                                            unsigned long long* __restrict__ within) {
    const long long k = (long long)blockIdx.x * CD_BLOCK + threadIdx.x;
    float d2min = INFINITY;
    if (k < n_query) {
        const unsigned long long qkey = qkeys[k];
        const uint32_t i = qvals[k];
        unsigned long long best = ~0ull;
        if (qkey != CD_Q_NONE) {
            const float* p = query + (size_t)i * stride;
            const float qx = p[0], qy = p[1], qz = p[2];
            for (int r = 0; r < 9; r++) {
                uint32_t b, e;
                if (!cd_query_range(qkey, r, g, tkeys, n_cand, b, e)) continue;
#pragma unroll 4
                for (uint32_t t = b; t < e; t++) {   // (unrolled: four record loads in flight per lane; the launch waits on this load, profiles/cloud_distance)
                    const CdRec c = rec[t];
                    const float dx = qx - c.x, dy = qy - c.y, dz = qz - c.z;
                    const float d2 = (dx * dx + dy * dy) + dz * dz;          // no fused operation: the library is built with -ffp-contract=off
                    const unsigned long long code = ((unsigned long long)__float_as_uint(d2) << 32) | c.j;
                    best = code < best ? code : best;
                }
            }
        }
        const float d2 = __uint_as_float((uint32_t)(best >> 32));             // (the initial code reads as a NaN: fails the comparison)
        const bool hit = d2 <= r2;
        d2min = hit ? d2 : INFINITY;
        if (dist2_out) dist2_out[i] = d2min;
        if (index_out) index_out[i] = hit ? (int32_t)(uint32_t)best : -1;
    }
    for (int t = 0; t < n_tol; t++) {
        const unsigned long long m = __ballot(d2min <= tol2[t]);
        if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(&within[t], (unsigned long long)__popcll(m));
    }
}

// no candidate target: every query gets +inf and -1; the candidate queries are still counted
__global__ __launch_bounds__(CD_BLOCK) void cd_fill_kernel(const float* __restrict__ query, long long n_query, int stride, float* __restrict__ dist2_out,
                                                           int32_t* __restrict__ index_out, unsigned long long* __restrict__ n_valid) {
    const long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x;
    bool cand = false;
    if (i < n_query) {
        const float* p = query + (size_t)i * stride;
        cand = cd_candidate(p[0], p[1], p[2]);
        if (dist2_out) dist2_out[i] = INFINITY;
        if (index_out) index_out[i] = -1;
    }
    const unsigned long long m = __ballot(cand);
    if (m && (threadIdx.x & 63) == (unsigned)(__ffsll((long long)m) - 1)) atomicAdd(n_valid, (unsigned long long)__popcll(m));
}

// query / target and the two per-query outputs are device pointers (the frame's views of the caller's buffers); tol2, within_out,
// n_valid_out and pairs_out are the caller's host arrays.  The arguments have been checked (tsar_api.hip); 0 <= n < 2^31 on both sides.
int run_cloud_distance(CallFrame& f, const float* query, long long n_query, int query_stride, const float* target, long long n_target, int target_stride, float r2,
                       double edge, long long max_pairs, int n_tol, const float* tol2, float* dist2_out, int32_t* index_out, int64_t* within_out,
                       int64_t* n_valid_out, int64_t* pairs_out) {
    tsar_ctx* ctx = f.ctx;
    hipStream_t st = ctx->stream;
    // counters (cloud_grid.h): own[0] the candidate queries, own[1] the pairs; within[n_tol] follows them
    char* d_head = f.tmp<char>(sizeof(CdCounters) + 8 * (size_t)(n_tol > 0 ? n_tol : 1));
    float* d_tol2 = f.tmp<float>(n_tol > 0 ? n_tol : 1);
    if (!f.ok()) return f.finish();
    CdCounters* dc = (CdCounters*)d_head;
    unsigned long long *d_n_valid = &dc->own[0], *d_pairs = &dc->own[1], *d_within = (unsigned long long*)(d_head + sizeof(CdCounters));
    unsigned long long own[2] = {0, 0};              // the host's copy of dc->own
    f.zero(d_within, 8 * (size_t)(n_tol > 0 ? n_tol : 1));
    if (n_tol > 0) f.copy(d_tol2, tol2, 4 * (size_t)n_tol, hipMemcpyHostToDevice);
    CdBounds bounds;
    if (!cd_measure(f, target, n_target, target_stride, dc, bounds)) return f.finish();
    const long long n_cand = bounds.n_cand;
    std::vector<unsigned long long> h_within(n_tol > 0 ? n_tol : 1, 0ull);
    if (n_cand == 0 || n_query == 0) {               // nothing to search: +inf and -1 throughout
        if (n_query > 0) {
            ScopedKernelTimer tm(ctx, "cloud_distance");
            hipLaunchKernelGGL(cd_fill_kernel, dim3(cd_blocks(n_query)), dim3(CD_BLOCK), 0, st, query, n_query, query_stride, dist2_out, index_out, d_n_valid);
        }
        f.launched();
        f.copy(own, dc->own, sizeof own, hipMemcpyDeviceToHost);
        if (!f.sync()) return f.finish();
        if (pairs_out) *pairs_out = 0;
        if (n_valid_out) *n_valid_out = (int64_t)own[0];
        for (int t = 0; t < n_tol && within_out; t++) within_out[t] = 0;
        return f.finish();
    }
    CdGrid g;
    if (!cd_grid(f, bounds, edge, CD_MAX_EXTENT,
                 "tsar_cloud_distance: the targets span 2^20 cells or more of edge max_dist on an axis: max_dist is too small for this cloud's extent", g))
        return f.finish();

    unsigned long long *qk0 = f.tmp<unsigned long long>((size_t)n_query), *qk1 = f.tmp<unsigned long long>((size_t)n_query);
    uint32_t *qv0 = f.tmp<uint32_t>((size_t)n_query), *qv1 = f.tmp<uint32_t>((size_t)n_query);
    CdIndex tx;                                       // the targets', with the query keys launched in its cloud_keys group
    if (!cd_index(f, target, n_target, target_stride, n_cand, g, tx, [&] {
            hipLaunchKernelGGL(cd_query_keys_kernel, dim3(cd_blocks(n_query)), dim3(CD_BLOCK), 0, st, query, n_query, query_stride, g, qk0, qv0, d_n_valid);
        }))
        return f.finish();
    if (!cd_sort(f, "cloud_sort", qk0, qk1, qv0, qv1, n_query, 64)) return f.finish();
    {
        ScopedKernelTimer tm(ctx, "cloud_pairs");
        hipLaunchKernelGGL(cd_pairs_kernel, dim3(cd_blocks(n_query)), dim3(CD_BLOCK), 0, st, qk1, n_query, g, tx.keys, (uint32_t)n_cand, d_pairs);
    }
    f.launched();
    f.copy(own, dc->own, sizeof own, hipMemcpyDeviceToHost);
    if (!f.sync()) return f.finish();
    if (pairs_out) *pairs_out = (int64_t)own[1];
    if (own[1] > (unsigned long long)max_pairs) {
        char msg[256];
        snprintf(msg, sizeof msg, "tsar_cloud_distance: the call would evaluate %llu pairs, more than max_pairs = %lld: lower max_dist or raise max_pairs",
                 own[1], max_pairs);
        return f.fail(TSAR_ERR_INVALID, msg);
    }
    {
        ScopedKernelTimer tm(ctx, "cloud_distance");
        hipLaunchKernelGGL(cd_query_kernel, dim3(cd_blocks(n_query)), dim3(CD_BLOCK), 0, st, query, query_stride, qk1, qv1, n_query, g, tx.keys, tx.rec, (uint32_t)n_cand, r2,
                           n_tol, d_tol2, dist2_out, index_out, d_within);
    }
    f.launched();
    if (n_tol > 0) f.copy(h_within.data(), d_within, 8 * (size_t)n_tol, hipMemcpyDeviceToHost);
    if (!f.sync()) return f.finish();
    if (n_valid_out) *n_valid_out = (int64_t)own[0];
    for (int t = 0; t < n_tol && within_out; t++) within_out[t] = (int64_t)h_within[t];
    return f.finish();
}
