// Host stand-in of libtsar_hip.so for tests/test_outlier_cli_cpu.py: the entries of tsar_stub_voxels.cpp plus the neighbourhood statistics of
// include/tsar.h (tsar_cloud_neighbors) by brute force on the host in float32 (this file is built with -ffp-contract=off).  `pairs` is what
// brute force looks at: candidates times candidates.
#include "tsar_stub_voxels.cpp"

#include <algorithm>

extern "C" {

void tsar_default_cloud_neighbors_params(tsar_cloud_neighbors_params* p) {
    p->radius = 0.0f;
    p->k = 0;
    p->max_pairs = (int64_t)1 << 40;
}

int tsar_cloud_neighbors_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_neighbors_params* p, int32_t* count_out, float* knn_dist2_out,
                             int64_t* n_valid_out, int64_t* pairs_out, int mem) {
    if (mem != TSAR_MEM_HOST || stride < 3) { ctx->err = "stub: host memory and strides >= 3 only"; return TSAR_ERR_INVALID; }
    const volatile float r2v = p->radius * p->radius;
    const float r2 = r2v;
    if (!(r2 > 0.0f) || !isfinite(r2)) { ctx->err = "tsar_cloud_neighbors: radius must be finite and > 0"; return TSAR_ERR_INVALID; }
    if (p->k < 0 || p->k > TSAR_CLOUD_KNN_MAX || (p->k == 0 && knn_dist2_out)) { ctx->err = "tsar_cloud_neighbors: k must be in 0..32, and > 0 with knn_dist2_out"; return TSAR_ERR_INVALID; }
    int64_t nc = 0;
    for (int64_t i = 0; i < n; i++) nc += candidate(cloud + i * stride);
    if (pairs_out) *pairs_out = nc * nc;
    if (nc * nc > p->max_pairs) { ctx->err = "tsar_cloud_neighbors: more than max_pairs pairs"; return TSAR_ERR_INVALID; }
    if (n_valid_out) *n_valid_out = nc;
    std::vector<float> near;
    for (int64_t i = 0; i < n; i++) {
        const float* q = cloud + i * stride;
        near.clear();
        if (candidate(q))
            for (int64_t j = 0; j < n; j++) {
                const float* t = cloud + j * stride;
                if (j == i || !candidate(t)) continue;
                const float dx = q[0] - t[0], dy = q[1] - t[1], dz = q[2] - t[2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 <= r2) near.push_back(d2);
            }
        if (count_out) count_out[i] = candidate(q) ? (int32_t)near.size() : -1;
        if (knn_dist2_out) {
            std::sort(near.begin(), near.end());
            for (int s = 0; s < p->k; s++) knn_dist2_out[i * p->k + s] = (size_t)s < near.size() ? near[(size_t)s] : INFINITY;
        }
    }
    return TSAR_OK;
}

int tsar_cloud_neighbors(int device, const float* cloud, int64_t n, int stride, const tsar_cloud_neighbors_params* p, int32_t* count_out, float* knn_dist2_out,
                         int64_t* n_valid_out, int64_t* pairs_out, int mem) {
    tsar_ctx* ctx = nullptr;
    if (tsar_create(device, &ctx) != TSAR_OK) return TSAR_ERR_HIP;
    const int rc = tsar_cloud_neighbors_ctx(ctx, cloud, n, stride, p, count_out, knn_dist2_out, n_valid_out, pairs_out, mem);
    tsar_destroy(ctx);
    return rc;
}

}   // extern "C"
