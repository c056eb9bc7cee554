// Host stand-in of libtsar_hip.so for tests/test_cloud_splat_cpu.py: tsar_stub_render.cpp's entries, and tsar_cloud_render_oriented_ctx of
// include/tsar.h by brute force on the host in float32 (this file is built with -ffp-contract=off).  "Device" memory is host memory here.
// tsar_cloud_normals_ctx estimates nothing: it shows what the tool handed over.  Point i gets the "normal" (k, min_neighbors, radius), and
// every third point (i % 3 == 0) none, 0 0 0, so that the square fall-back takes part.
#include "tsar_stub_render.cpp"

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
    (void)cloud; (void)mem;
    if (!p || stride != 3 || !(p->radius > 0.0f) || !normal_out || knn_index_out || n_used_out || curvature_out || cov_out) { ctx->err = "stub: bad arguments"; return TSAR_ERR_INVALID; }
    int64_t normals = 0;
    for (int64_t i = 0; i < n; i++) {
        const bool has = i % 3 != 0;
        normal_out[i * 3 + 0] = has ? (float)p->k : 0.0f;
        normal_out[i * 3 + 1] = has ? (float)p->min_neighbors : 0.0f;
        normal_out[i * 3 + 2] = has ? p->radius : 0.0f;
        normals += has;
    }
    if (n_valid_out) *n_valid_out = n;
    if (n_normals_out) *n_normals_out = normals;
    if (pairs_out) *pairs_out = 0;
    return TSAR_OK;
}

int tsar_cloud_render_oriented_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const float* normals, int normal_stride, const tsar_camera* cam, int w, int h,
                                   const tsar_cloud_render_params* p, float* depth_out, uint8_t* count_out, int32_t* index_out, float* occluder_out, int64_t* n_splats_out,
                                   int64_t* n_covered_out, int mem) {
    (void)mem;
    if (!p || !cam || stride < 3 || w < 1 || h < 1 || (!depth_out && !count_out && !index_out && !occluder_out) || (!normals && stride < 6) || (normals && normal_stride < 3)) {
        ctx->err = "stub: bad arguments";
        return TSAR_ERR_INVALID;
    }
    const volatile float frv = cam->K[0] * p->radius;
    const float fr = frv;
    if (!(p->radius >= 0.0f && p->radius <= FLT_MAX) || !(fr >= 0.0f && fr <= FLT_MAX)) { ctx->err = "tsar_cloud_render_oriented: radius must be finite and >= 0"; return TSAR_ERR_INVALID; }
    float P[12], M[9], C[3];
    for (int k = 0; k < 3; k++) {
        const double k0 = cam->K[k * 3], k1 = cam->K[k * 3 + 1], k2 = cam->K[k * 3 + 2];
        for (int j = 0; j < 3; j++) P[k * 4 + j] = (float)((k0 * (double)cam->R[j] + k1 * (double)cam->R[3 + j]) + k2 * (double)cam->R[6 + j]);
        P[k * 4 + 3] = (float)((k0 * (double)cam->t[0] + k1 * (double)cam->t[1]) + k2 * (double)cam->t[2]);
    }
    double A[3][3], c[3][3];
    for (int k = 0; k < 3; k++)
        for (int j = 0; j < 3; j++) A[k][j] = (double)P[k * 4 + j];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) c[i][j] = A[(i + 1) % 3][(j + 1) % 3] * A[(i + 2) % 3][(j + 2) % 3] - A[(i + 1) % 3][(j + 2) % 3] * A[(i + 2) % 3][(j + 1) % 3];
    const double det = (A[0][0] * c[0][0] + A[0][1] * c[0][1]) + A[0][2] * c[0][2];
    bool finite = det != 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { M[j * 3 + i] = (float)(c[i][j] / det); finite = finite && isfinite(M[j * 3 + i]); }
    for (int j = 0; j < 3; j++) {
        C[j] = (float)-(((double)cam->R[j] * (double)cam->t[0] + (double)cam->R[3 + j] * (double)cam->t[1]) + (double)cam->R[6 + j] * (double)cam->t[2]);
        finite = finite && isfinite(C[j]);
    }
    if (!finite) { ctx->err = "tsar_cloud_render_oriented: K R is singular"; return TSAR_ERR_INVALID; }
    const volatile float r2v = p->radius * p->radius;
    const float r2 = r2v;
    const size_t np = (size_t)w * h;
    std::vector<float> Zc(np, INFINITY), Zo(np, INFINITY);
    std::vector<int64_t> winner(np, -1), support(np, 0);
    int64_t splats = 0, covered = 0;
    for (int pass = 0; pass < 3; pass++) {                // 0: the splat count; 1: both minima; 2: the support counts
        for (int64_t i = 0; i < n; i++) {
            const float* X = cloud + i * stride;
            const Landing l = land(X, P, fr, true, p->max_px, w, h);
            if (!l.lands) continue;
            const size_t at = (size_t)l.yi * w + l.xi;
            if (pass == 2) {
                const float dd = p->depth_diff * Zc[at];
                if (fabsf(l.p2 - Zc[at]) <= dd) support[at]++;
                continue;
            }
            if (pass == 1 && (winner[at] < 0 || l.p2 < Zc[at])) { Zc[at] = l.p2; winner[at] = i; }   // (ascending i: the first of equals stays)
            const float* nn = normals ? normals + i * normal_stride : X + 3;
            const bool oriented = isfinite(nn[0]) && isfinite(nn[1]) && isfinite(nn[2]) && (nn[0] != 0.0f || nn[1] != 0.0f || nn[2] != 0.0f);
            const float a[3] = {X[0] - C[0], X[1] - C[1], X[2] - C[2]};
            const float num = (nn[0] * a[0] + nn[1] * a[1]) + nn[2] * a[2];
            float g[3];
            for (int j = 0; j < 3; j++) g[j] = (M[j] * nn[0] + M[3 + j] * nn[1]) + M[6 + j] * nn[2];
            for (int yy = l.yi - l.s; yy <= l.yi + l.s; yy++)
                for (int xx = l.xi - l.s; xx <= l.xi + l.s; xx++) {
                    if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
                    if (pass == 0) { splats++; continue; }
                    float value = l.p2;
                    if (oriented && !(xx == l.xi && yy == l.yi)) {
                        const float u = (float)xx, v = (float)yy;
                        const float den = g[0] * u + (g[1] * v + g[2]);
                        const float z = num / den;
                        float q = 0.0f, e[3];
                        for (int k = 0; k < 3; k++) {
                            const float d = M[k * 3] * u + (M[k * 3 + 1] * v + M[k * 3 + 2]);
                            e[k] = z * d - a[k];
                        }
                        q = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2];
                        if (!(z > 0.0f && z < INFINITY && q <= r2)) continue;
                        value = z;
                    }
                    covered++;
                    if (value < Zo[(size_t)yy * w + xx]) Zo[(size_t)yy * w + xx] = value;
                }
        }
        if (pass == 0) {
            if (n_splats_out) *n_splats_out = splats;
            if (splats > p->max_splats) { ctx->err = "tsar_cloud_render_oriented: more than max_splats splats"; return TSAR_ERR_INVALID; }
        }
    }
    if (n_covered_out) *n_covered_out = covered;
    for (size_t q = 0; q < np; q++) {
        const bool landed = winner[q] >= 0;
        const bool visible = landed && Zc[q] - Zo[q] <= p->occlusion_diff * Zo[q];
        const bool kept = visible && support[q] >= p->min_points;
        if (count_out) count_out[q] = (uint8_t)(support[q] > 255 ? 255 : support[q]);
        if (depth_out) depth_out[q] = kept ? Zc[q] : 0.0f;
        if (index_out) index_out[q] = kept ? (int32_t)winner[q] : -1;
        if (occluder_out) occluder_out[q] = Zo[q] < INFINITY ? Zo[q] : 0.0f;
    }
    return TSAR_OK;
}

}   // extern "C"
