// Host stand-in of libtsar_hip.so for tests/test_normals_cli_cpu.py: the entries of tsar_stub_neighbors.cpp plus tsar_cloud_normals and
// tsar_cloud_normal_compare of include/tsar.h by brute force on the host, operation for operation (this file is built with
// -ffp-contract=off): a third statement of the header, beside the kernel and tests/cloud_normals_ref.py.  `pairs` is what brute force looks
// at: candidates times candidates.  The normals entry also exports its per-point outputs, so that the test can hold them to the restatement.
#include "tsar_stub_neighbors.cpp"

#include <utility>

static void stub_rotate(double a[3][3], double V[3][3], int p, int q, int r) {
    const double apq = a[p][q];
    if (apq == 0.0) return;
    const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    const double h = t * apq;
    a[p][p] = a[p][p] - h;
    a[q][q] = a[q][q] + h;
    a[p][q] = a[q][p] = 0.0;
    const double x = a[r][p], y = a[r][q];
    a[r][p] = a[p][r] = c * x - s * y;
    a[r][q] = a[q][r] = s * x + c * y;
    for (int k = 0; k < 3; k++) {
        const double vx = V[k][p], vy = V[k][q];
        V[k][p] = c * vx - s * vy;
        V[k][q] = s * vx + c * vy;
    }
}

extern "C" {

void tsar_default_cloud_normals_params(tsar_cloud_normals_params* p) {
    p->radius = 0.0f;
    p->k = 16;
    p->min_neighbors = 5;
    p->orient = 0;
    p->viewpoint[0] = p->viewpoint[1] = p->viewpoint[2] = 0.0f;
    p->max_pairs = (int64_t)1 << 40;
}

int tsar_cloud_normals_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_normals_params* p, int32_t* knn_index_out, int32_t* n_used_out,
                           float* normal_out, float* curvature_out, double* cov_out, int64_t* n_valid_out, int64_t* n_normals_out, int64_t* pairs_out, int mem) {
    if (mem != TSAR_MEM_HOST || stride < 3) { ctx->err = "stub: host memory and strides >= 3 only"; return TSAR_ERR_INVALID; }
    const volatile float r2v = p->radius * p->radius;
    const float r2 = r2v;
    if (!(r2 > 0.0f) || !isfinite(r2)) { ctx->err = "tsar_cloud_normals: radius must be finite and > 0"; return TSAR_ERR_INVALID; }
    if (p->k < 3 || p->k > TSAR_CLOUD_KNN_MAX) { ctx->err = "tsar_cloud_normals: k must be in 3..32"; return TSAR_ERR_INVALID; }
    if (p->min_neighbors < 2 || p->min_neighbors > p->k) { ctx->err = "tsar_cloud_normals: min_neighbors must be in 2..k"; return TSAR_ERR_INVALID; }
    if (p->orient < 0 || p->orient > 2 || (p->orient == 2 && stride < 6)) { ctx->err = "tsar_cloud_normals: orient"; return TSAR_ERR_INVALID; }
    int64_t nc = 0, normals = 0;
    for (int64_t i = 0; i < n; i++) nc += candidate(cloud + i * stride);
    if (pairs_out) *pairs_out = nc * nc;
    if (nc * nc > p->max_pairs) { ctx->err = "tsar_cloud_normals: more than max_pairs pairs"; return TSAR_ERR_INVALID; }
    if (n_valid_out) *n_valid_out = nc;
    std::vector<std::pair<uint64_t, int64_t>> near;
    for (int64_t i = 0; i < n; i++) {
        const float* q = cloud + i * stride;
        near.clear();
        if (candidate(q))
            for (int64_t j = 0; j < n; j++) {
                const float* t = cloud + j * stride;
                if (j == i || !candidate(t)) continue;
                const float dx = q[0] - t[0], dy = q[1] - t[1], dz = q[2] - t[2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                uint32_t bits;
                memcpy(&bits, &d2, 4);
                if (d2 <= r2) near.push_back({((uint64_t)bits << 32) | (uint64_t)j, j});
            }
        std::sort(near.begin(), near.end());
        const int m = (int)std::min<size_t>(near.size(), (size_t)p->k);
        for (int s = 0; s < p->k && knn_index_out; s++) knn_index_out[i * p->k + s] = s < m ? (int32_t)near[(size_t)s].second : -1;
        if (n_used_out) n_used_out[i] = candidate(q) ? m : -1;
        float nrm[3] = {0.0f, 0.0f, 0.0f}, curv = -1.0f;
        double C[6] = {0, 0, 0, 0, 0, 0};
        if (candidate(q) && m >= p->min_neighbors) {
            double S[3] = {0, 0, 0}, Q[6] = {0, 0, 0, 0, 0, 0};
            for (int s = 0; s < m; s++) {
                const float* t = cloud + near[(size_t)s].second * stride;
                const double u[3] = {(double)t[0] - (double)q[0], (double)t[1] - (double)q[1], (double)t[2] - (double)q[2]};
                for (int a = 0; a < 3; a++) S[a] += u[a];
                Q[0] += u[0] * u[0]; Q[1] += u[0] * u[1]; Q[2] += u[0] * u[2]; Q[3] += u[1] * u[1]; Q[4] += u[1] * u[2]; Q[5] += u[2] * u[2];
            }
            const double M = (double)(m + 1);
            const double mu[3] = {S[0] / M, S[1] / M, S[2] / M};
            C[0] = Q[0] / M - mu[0] * mu[0]; C[1] = Q[1] / M - mu[0] * mu[1]; C[2] = Q[2] / M - mu[0] * mu[2];
            C[3] = Q[3] / M - mu[1] * mu[1]; C[4] = Q[4] / M - mu[1] * mu[2]; C[5] = Q[5] / M - mu[2] * mu[2];
            double a[3][3] = {{C[0], C[1], C[2]}, {C[1], C[3], C[4]}, {C[2], C[4], C[5]}}, V[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
            for (int sweep = 0; sweep < 6; sweep++) {
                stub_rotate(a, V, 0, 1, 2);
                stub_rotate(a, V, 0, 2, 1);
                stub_rotate(a, V, 1, 2, 0);
            }
            int c0 = 0;
            for (int c = 1; c < 3; c++)
                if (a[c][c] < a[c0][c0]) c0 = c;
            double v[3] = {V[0][c0], V[1][c0], V[2][c0]};
            double big = v[0];
            for (int c = 1; c < 3; c++)
                if (fabs(v[c]) > fabs(big)) big = v[c];
            if (big < 0.0) for (int c = 0; c < 3; c++) v[c] = -v[c];
            if (p->orient) {
                double w[3];
                for (int c = 0; c < 3; c++) w[c] = p->orient == 1 ? (double)p->viewpoint[c] - (double)q[c] : (double)q[3 + c];
                const double d = (v[0] * w[0] + v[1] * w[1]) + v[2] * w[2];
                if (d < 0.0) for (int c = 0; c < 3; c++) v[c] = -v[c];
            }
            for (int c = 0; c < 3; c++) nrm[c] = (float)v[c];
            const double sum = (a[0][0] + a[1][1]) + a[2][2], l0 = a[c0][c0];
            curv = sum > 0.0 ? (float)((l0 > 0.0 ? l0 : 0.0) / sum) : 0.0f;
            normals++;
        }
        for (int c = 0; c < 3 && normal_out; c++) normal_out[i * 3 + c] = nrm[c];
        if (curvature_out) curvature_out[i] = curv;
        for (int c = 0; c < 6 && cov_out; c++) cov_out[i * 6 + c] = C[c];
    }
    if (n_normals_out) *n_normals_out = normals;
    return TSAR_OK;
}

int tsar_cloud_normals(int device, const float* cloud, int64_t n, int stride, const tsar_cloud_normals_params* p, int32_t* knn_index_out, int32_t* n_used_out,
                       float* normal_out, float* curvature_out, double* cov_out, int64_t* n_valid_out, int64_t* n_normals_out, int64_t* pairs_out, int mem) {
    tsar_ctx* ctx = nullptr;
    if (tsar_create(device, &ctx) != TSAR_OK) return TSAR_ERR_HIP;
    const int rc = tsar_cloud_normals_ctx(ctx, cloud, n, stride, p, knn_index_out, n_used_out, normal_out, curvature_out, cov_out, n_valid_out, n_normals_out, pairs_out, mem);
    tsar_destroy(ctx);
    return rc;
}

int tsar_cloud_normal_compare_ctx(tsar_ctx* ctx, const float* normal_a, int stride_a, int64_t n, const float* normal_b, int stride_b, int64_t n_b, const int32_t* index,
                                  const float* dist2, float max_dist, int n_tol, const double* min_cos, int is_signed, float* cos_out, int64_t* within_out,
                                  int64_t* n_compared_out, int mem) {
    if (mem != TSAR_MEM_HOST || stride_a < 3 || stride_b < 3) { ctx->err = "stub: host memory and strides >= 3 only"; return TSAR_ERR_INVALID; }
    if (n_tol < 0 || n_tol > TSAR_NORMAL_COMPARE_MAX_TOL) { ctx->err = "tsar_cloud_normal_compare: n_tol must be in 0..16"; return TSAR_ERR_INVALID; }
    const volatile float md2v = max_dist * max_dist;
    const float md2 = md2v;
    int64_t compared = 0;
    for (int k = 0; k < n_tol && within_out; k++) within_out[k] = 0;
    for (int64_t i = 0; i < n; i++) {
        bool cmp = index[i] >= 0 && index[i] < n_b && (!dist2 || dist2[i] <= md2);
        double c = 0.0;
        if (cmp) {
            const float* a = normal_a + i * stride_a;
            const float* b = normal_b + (int64_t)index[i] * stride_b;
            const double ax = a[0], ay = a[1], az = a[2], bx = b[0], by = b[1], bz = b[2];
            const double aa = (ax * ax + ay * ay) + az * az, bb = (bx * bx + by * by) + bz * bz;
            cmp = candidate(a) && candidate(b) && aa > 0.0 && bb > 0.0;
            c = ((ax * bx + ay * by) + az * bz) / sqrt(aa * bb);
            if (!is_signed) c = fabs(c);
        }
        compared += cmp;
        for (int k = 0; k < n_tol && within_out; k++) within_out[k] += cmp && c >= min_cos[k];
        if (cos_out) cos_out[i] = cmp ? (float)c : NAN;
    }
    if (n_compared_out) *n_compared_out = compared;
    return TSAR_OK;
}

int tsar_cloud_normal_compare(int device, const float* normal_a, int stride_a, int64_t n, const float* normal_b, int stride_b, int64_t n_b, const int32_t* index,
                              const float* dist2, float max_dist, int n_tol, const double* min_cos, int is_signed, float* cos_out, int64_t* within_out,
                              int64_t* n_compared_out, int mem) {
    tsar_ctx* ctx = nullptr;
    if (tsar_create(device, &ctx) != TSAR_OK) return TSAR_ERR_HIP;
    const int rc = tsar_cloud_normal_compare_ctx(ctx, normal_a, stride_a, n, normal_b, stride_b, n_b, index, dist2, max_dist, n_tol, min_cos, is_signed, cos_out, within_out,
                                                 n_compared_out, mem);
    tsar_destroy(ctx);
    return rc;
}

}   // extern "C"
