// cloud_normal_kernels.hip — per point of one cloud the indices of its k nearest neighbours within a radius, the PCA normal and surface
// variation of that neighbourhood (include/tsar.h tsar_cloud_normals), and the agreement of two sets of normals as integer counts
// (tsar_cloud_normal_compare).  Every output is the brute-force definition written there: the neighbour list is an order statistic of
// the 64-bit codes bits(d2) << 32 | j, the moments are float64 sums in list order, the eigenvectors a fixed number of Jacobi sweeps, so
// no bit depends on the grid or on the order in which a point's neighbours arrive.  tests/cloud_normals_ref.py restates both in numpy.
//
// Per call:  cd_self_search of cloud_grid.hip (bounds, keys, sort, records in key order, the pair count, the refusals), as cloud_neighbor_kernels.hip
//            -> nr_normals_kernel: lane t takes sorted record t as its query; the KCAP smallest codes kept sorted in registers (a
//               template over KCAP, every loop over the list unrolled, insertion only when some lane of the wave holds a code below its
//               list's last entry); then the moments, by re-loading the listed points from the cloud; then six Jacobi sweeps.
// No LDS, no scratch; one atomic per wave for the count of normals.  The library is built with -ffp-contract=off: no product and sum
// below is fused, and float64 `/` and `sqrt` are correctly rounded on the device (plane_prior_build_kernels.hip relies on the same).
#include "cloud_grid.h"
#include "tsar_device_math.h"             // block_add_counters

#define NR_NONE 0xffffffffffffffffull     // above every code: d2 <= R2 is finite, so bits(d2) < 0x7f800000

struct NrArgs {
    const float* pts;                     // the cloud, `stride` floats per record
    int stride, k, min_neighbors, orient;
    float r2;
    float vx, vy, vz;                     // the viewpoint (orient 1)
    int32_t* knn_index;                   // [n][k]
    int32_t* n_used;                      // [n]
    float* normal;                        // [n][3]
    float* curvature;                     // [n]
    double* cov;                          // [n][6]
    unsigned long long* n_normals;
};

// One Jacobi rotation in the (p, q) plane of the symmetric a, r the third index; skipped iff a_pq == 0 (include/tsar.h)
__device__ __forceinline__ void nr_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& v0p, double& v0q, double& v1p, double& v1q, double& v2p,
                                          double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    app = app - h;
    aqq = aqq + h;
    apq = 0.0;
    double x = arp, y = arq;
    arp = c * x - s * y;
    arq = s * x + c * y;
    x = v0p, y = v0q;
    v0p = c * x - s * y;
    v0q = s * x + c * y;
    x = v1p, y = v1q;
    v1p = c * x - s * y;
    v1q = s * x + c * y;
    x = v2p, y = v2q;
    v2p = c * x - s * y;
    v2q = s * x + c * y;
}

// column 0, 1 (s1) or 2 (s2) of a row of V: two selects on registers
__device__ __forceinline__ double nr_pick(bool s1, bool s2, double x0, double x1, double x2) {
    const double x = s1 ? x1 : x0;
    return s2 ? x2 : x;
}

// One lane per candidate, in key order.  The first k <= KCAP entries of the list are the point's neighbours.
template <int KCAP>
__global__ __launch_bounds__(CD_BLOCK) void nr_normals_kernel(const unsigned long long* __restrict__ keys, const CdRec* __restrict__ rec, uint32_t n_cand, CdGrid g, NrArgs A) {
    const uint32_t t = blockIdx.x * CD_BLOCK + threadIdx.x;
    bool has = false;
    if (t < n_cand) {
        const CdRec q = rec[t];
        const unsigned long long qkey = cd_self_query_key(keys[t]);
        unsigned long long a[KCAP];
#pragma unroll
        for (int s = 0; s < KCAP; s++) a[s] = NR_NONE;
        for (int r = 0; r < 9; r++) {
            uint32_t b, e;
            if (!cd_query_range(qkey, r, g, keys, n_cand, b, e)) continue;
#pragma unroll 4
            for (uint32_t u = b; u < e; u++) {       // (unrolled like cn_search_kernel: four record loads in flight per lane)
                const CdRec c = rec[u];
                const float dx = q.x - c.x, dy = q.y - c.y, dz = q.z - c.z;
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                const bool in = d2 <= A.r2 && c.j != q.j;                      // the point itself is excluded by index, not by distance
                unsigned long long x = in ? ((unsigned long long)__float_as_uint(d2) << 32) | c.j : NR_NONE;
                if (__ballot(x < a[KCAP - 1])) {                               // wave-uniform among the lanes still in the loop
#pragma unroll
                    for (int s = 0; s < KCAP; s++) {
                        const bool lt = a[s] < x;
                        const unsigned long long lo = lt ? a[s] : x;
                        x = lt ? x : a[s];
                        a[s] = lo;
                    }
                }
            }
        }
        // the list cut at k: its length, its indices, and the float64 moments relative to the point, in list order
        const double px = (double)q.x, py = (double)q.y, pz = (double)q.z;
        int32_t m = 0;
        double sx = 0.0, sy = 0.0, sz = 0.0, qxx = 0.0, qxy = 0.0, qxz = 0.0, qyy = 0.0, qyz = 0.0, qzz = 0.0;
        int32_t* ko = A.knn_index ? A.knn_index + (size_t)q.j * A.k : nullptr;
#pragma unroll
        for (int s = 0; s < KCAP; s++) {
            const bool used = s < A.k && a[s] != NR_NONE;
            const uint32_t j = (uint32_t)a[s];
            if (ko && s < A.k) ko[s] = used ? (int32_t)j : -1;
            if (used) {
                const float* pj = A.pts + (size_t)j * A.stride;
                const double ux = (double)pj[0] - px, uy = (double)pj[1] - py, uz = (double)pj[2] - pz;
                sx += ux;
                sy += uy;
                sz += uz;
                qxx += ux * ux;
                qxy += ux * uy;
                qxz += ux * uz;
                qyy += uy * uy;
                qyz += uy * uz;
                qzz += uz * uz;
                m++;
            }
        }
        if (A.n_used) A.n_used[q.j] = m;
        has = m >= A.min_neighbors;
        float nx = 0.0f, ny = 0.0f, nz = 0.0f, curv = -1.0f;
        double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
        if (has) {
            const double M = (double)(m + 1);                                  // the point itself is part of its neighbourhood, u = 0
            const double mx = sx / M, my = sy / M, mz = sz / M;
            c00 = qxx / M - mx * mx;
            c01 = qxy / M - mx * my;
            c02 = qxz / M - mx * mz;
            c11 = qyy / M - my * my;
            c12 = qyz / M - my * mz;
            c22 = qzz / M - mz * mz;
            double a00 = c00, a01 = c01, a02 = c02, a11 = c11, a12 = c12, a22 = c22;
            double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
            for (int sweep = 0; sweep < 6; sweep++) {
                nr_rotate(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);      // (p, q, r) = (0, 1, 2)
                nr_rotate(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);      // (0, 2, 1)
                nr_rotate(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);      // (1, 2, 0)
            }
            const bool s1 = a11 < a00;                                         // the smallest diagonal entry, the lowest index on ties
            const double l1 = s1 ? a11 : a00;
            const bool s2 = a22 < l1;
            const double l0 = s2 ? a22 : l1;
            double ex = nr_pick(s1, s2, v00, v01, v02), ey = nr_pick(s1, s2, v10, v11, v12), ez = nr_pick(s1, s2, v20, v21, v22);
            double big = ex;                                                   // the component of largest magnitude, the lowest index on ties
            if (fabs(ey) > fabs(big)) big = ey;
            if (fabs(ez) > fabs(big)) big = ez;
            if (big < 0.0) { ex = -ex; ey = -ey; ez = -ez; }
            if (A.orient != 0) {
                double wx, wy, wz;
                if (A.orient == 1) {
                    wx = (double)A.vx - px;
                    wy = (double)A.vy - py;
                    wz = (double)A.vz - pz;
                } else {
                    const float* pi = A.pts + (size_t)q.j * A.stride;
                    wx = (double)pi[3];
                    wy = (double)pi[4];
                    wz = (double)pi[5];
                }
                const double d = (ex * wx + ey * wy) + ez * wz;
                if (d < 0.0) { ex = -ex; ey = -ey; ez = -ez; }                 // (a NaN d leaves the canonical sign)
            }
            nx = (float)ex;
            ny = (float)ey;
            nz = (float)ez;
            const double sum = (a00 + a11) + a22;
            curv = sum > 0.0 ? (float)((l0 > 0.0 ? l0 : 0.0) / sum) : 0.0f;
        }
        if (A.normal) {
            float* o = A.normal + (size_t)q.j * 3;
            o[0] = nx;
            o[1] = ny;
            o[2] = nz;
        }
        if (A.curvature) A.curvature[q.j] = curv;
        if (A.cov) {
            double* o = A.cov + (size_t)q.j * 6;
            o[0] = c00;
            o[1] = c01;
            o[2] = c02;
            o[3] = c11;
            o[4] = c12;
            o[5] = c22;
        }
    }
    const unsigned long long cnt = cd_wave_sum(has ? 1ull : 0ull);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(A.n_normals, cnt);
}

// the records that are no candidates: no neighbours, no normal (the normals kernel writes the candidates' rows)
__global__ __launch_bounds__(CD_BLOCK) void nr_fill_kernel(long long n, NrArgs A) {
    const long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float* p = A.pts + (size_t)i * A.stride;
    if (cd_candidate(p[0], p[1], p[2])) return;
    if (A.knn_index)
        for (int s = 0; s < A.k; s++) A.knn_index[(size_t)i * A.k + s] = -1;
    if (A.n_used) A.n_used[i] = -1;
    if (A.normal)
        for (int s = 0; s < 3; s++) A.normal[(size_t)i * 3 + s] = 0.0f;
    if (A.curvature) A.curvature[i] = -1.0f;
    if (A.cov)
        for (int s = 0; s < 6; s++) A.cov[(size_t)i * 6 + s] = 0.0;
}

template <int KCAP>
static void nr_launch_normals(hipStream_t st, const unsigned long long* keys, const CdRec* rec, uint32_t n_cand, const CdGrid& g, const NrArgs& A) {
    hipLaunchKernelGGL(nr_normals_kernel<KCAP>, dim3(cd_blocks(n_cand)), dim3(CD_BLOCK), 0, st, keys, rec, n_cand, g, A);
}

// cloud and the five per-point outputs are device pointers (the frame's views of the caller's buffers); the three counts are the caller's
// host memory.  The arguments have been checked (tsar_api.hip): 0 <= n < 2^31, 3 <= k <= TSAR_CLOUD_KNN_MAX, 2 <= min_neighbors <= k.
int run_cloud_normals(CallFrame& f, const float* cloud, long long n, int stride, float r2, double edge, const tsar_cloud_normals_params& p, int32_t* knn_index_out,
                      int32_t* n_used_out, float* normal_out, float* curvature_out, double* cov_out, int64_t* n_valid_out, int64_t* n_normals_out, int64_t* pairs_out) {
    tsar_ctx* ctx = f.ctx;
    hipStream_t st = ctx->stream;
    CdSelf s;                                        // (cloud_grid.h) own[1] of its counters: the points with a normal
    if (!cd_self_search(f, cloud, n, stride, edge, p.max_pairs, pairs_out, s)) return f.finish();
    const long long n_cand = s.n_cand;
    const CdGrid& g = s.g;
    const CdIndex& ix = s.ix;
    CdCounters* dc = s.dc;
    unsigned long long n_normals = 0;
    NrArgs A = {cloud, stride, p.k, p.min_neighbors, p.orient, r2, p.viewpoint[0], p.viewpoint[1], p.viewpoint[2], knn_index_out, n_used_out, normal_out, curvature_out,
                cov_out, &dc->own[1]};
    const bool any_out = knn_index_out || n_used_out || normal_out || curvature_out || cov_out;
    if (f.ok() && n > 0 && n_cand < n && any_out) {
        ScopedKernelTimer tm(ctx, "cloud_normals");
        hipLaunchKernelGGL(nr_fill_kernel, dim3(cd_blocks(n)), dim3(CD_BLOCK), 0, st, n, A);
    }
    f.launched();
    if (f.ok() && n_cand > 0 && (any_out || n_normals_out)) {
        ScopedKernelTimer tm(ctx, "cloud_normals");
        if (p.k <= 8) nr_launch_normals<8>(st, ix.keys, ix.rec, (uint32_t)n_cand, g, A);             // the smallest list that holds k
        else if (p.k <= 16) nr_launch_normals<16>(st, ix.keys, ix.rec, (uint32_t)n_cand, g, A);
        else nr_launch_normals<32>(st, ix.keys, ix.rec, (uint32_t)n_cand, g, A);
        f.launched();
        f.copy(&n_normals, &dc->own[1], sizeof n_normals, hipMemcpyDeviceToHost);
    }
    const int rc = f.finish();                       // (synchronises: n_normals is complete)
    if (rc != TSAR_OK) return rc;
    if (n_valid_out) *n_valid_out = (int64_t)n_cand;
    if (n_normals_out) *n_normals_out = (int64_t)n_normals;
    return rc;
}

// ---- tsar_cloud_normal_compare --------------------------------------------------------------------------------------------------------------
// counters: 0 n_compared, 1 + k within[k].  Per lane in registers (the loop over the thresholds is unrolled over the fixed maximum, so
// nothing is indexed at run time), then block_add_counters (LDS: the partials of the block's waves), as depth_compare_kernel.
#define NC_COUNTERS (1 + TSAR_NORMAL_COMPARE_MAX_TOL)
struct NcTol { double c[TSAR_NORMAL_COMPARE_MAX_TOL]; int n; };

__global__ __launch_bounds__(CD_BLOCK) void nr_compare_kernel(const float* __restrict__ na, int stride_a, long long n, const float* __restrict__ nb, int stride_b, long long n_b,
                                                              const int32_t* __restrict__ index, const float* __restrict__ dist2, float md2, NcTol tol, int is_signed,
                                                              float* __restrict__ cos_out, unsigned long long* __restrict__ counters) {
    uint32_t cnt[NC_COUNTERS];
#pragma unroll
    for (int k = 0; k < NC_COUNTERS; k++) cnt[k] = 0;
    for (long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * CD_BLOCK) {
        const int32_t j = index[i];
        bool cmp = j >= 0 && (long long)j < n_b && (!dist2 || dist2[i] <= md2);        // (a NaN dist2 fails)
        double c = 0.0;
        if (cmp) {
            const float* pa = na + (size_t)i * stride_a;
            const float* pb = nb + (size_t)j * stride_b;
            const float ax = pa[0], ay = pa[1], az = pa[2], bx = pb[0], by = pb[1], bz = pb[2];
            const double dax = ax, day = ay, daz = az, dbx = bx, dby = by, dbz = bz;
            const double aa = (dax * dax + day * day) + daz * daz, bb = (dbx * dbx + dby * dby) + dbz * dbz;
            cmp = cd_candidate(ax, ay, az) && cd_candidate(bx, by, bz) && aa > 0.0 && bb > 0.0;
            c = ((dax * dbx + day * dby) + daz * dbz) / sqrt(aa * bb);
            if (!is_signed) c = fabs(c);
        }
        cnt[0] += cmp;
#pragma unroll
        for (int k = 0; k < TSAR_NORMAL_COMPARE_MAX_TOL; k++) cnt[1 + k] += k < tol.n && cmp && c >= tol.c[k];
        if (cos_out) cos_out[i] = cmp ? (float)c : __builtin_nanf("");
    }
    block_add_counters<NC_COUNTERS, CD_BLOCK>(cnt, counters);
}

// the arrays are device pointers; min_cos (n_tol thresholds) and counters_out ([NC_COUNTERS]) are host memory.  dist2 == NULL: md2 is not read
int run_cloud_normal_compare(CallFrame& f, const float* normal_a, int stride_a, long long n, const float* normal_b, int stride_b, long long n_b, const int32_t* index,
                             const float* dist2, float md2, int n_tol, const double* min_cos, int is_signed, float* cos_out, unsigned long long* counters_out) {
    tsar_ctx* ctx = f.ctx;
    NcTol t;
    for (int k = 0; k < TSAR_NORMAL_COMPARE_MAX_TOL; k++) t.c[k] = k < n_tol ? min_cos[k] : 2.0;
    t.n = n_tol;
    unsigned long long* d = f.tmp<unsigned long long>(NC_COUNTERS);
    if (!f.ok()) return f.finish();
    f.zero(d, NC_COUNTERS * sizeof(unsigned long long));
    if (n > 0 && f.ok()) {
        ScopedKernelTimer tm(ctx, "cloud_normal_compare");
        // (a lane's own counts stay below 2^32: at most 2^31 / 256 rows per lane)
        const unsigned blocks = cd_blocks(n) < 4096u ? cd_blocks(n) : 4096u;
        hipLaunchKernelGGL(nr_compare_kernel, dim3(blocks), dim3(CD_BLOCK), 0, ctx->stream, normal_a, stride_a, n, normal_b, stride_b, n_b, index, dist2, md2, t, is_signed,
                           cos_out, d);
    }
    f.launched();
    f.copy(counters_out, d, NC_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    return f.finish();
}
