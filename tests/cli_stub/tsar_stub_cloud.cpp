// Host stand-in of libtsar_hip.so for tests/test_evaluate_cli_cpu.py: the entries host/tsar_evaluate.cpp calls, with the cloud distances of
// include/tsar.h by brute force on the host in float32 (this file is built with -ffp-contract=off).  `pairs` is what brute force evaluates:
// candidate queries times candidate targets.
#include <math.h>
#include <string.h>

#include <string>

#include "../../include/tsar.h"

struct tsar_ctx { std::string err; };

static bool candidate(const float* p) { return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]); }

extern "C" {

int tsar_create(int device, tsar_ctx** out) {
    if (device != 0) return TSAR_ERR_HIP;
    *out = new tsar_ctx;
    return TSAR_OK;
}
int tsar_destroy(tsar_ctx* ctx) { delete ctx; return TSAR_OK; }
const char* tsar_last_error(const tsar_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void tsar_default_cloud_distance_params(tsar_cloud_distance_params* p) {
    p->max_dist = 0.0f;
    p->max_pairs = (int64_t)1 << 40;
}

int tsar_cloud_distance_ctx(tsar_ctx* ctx, const float* query, int64_t n_query, int query_stride, const float* target, int64_t n_target, int target_stride,
                            const tsar_cloud_distance_params* p, int n_tol, const float* tol, float* dist2_out, int32_t* index_out, int64_t* within_out,
                            int64_t* n_valid_query_out, int64_t* pairs_out, int mem) {
    if (mem != TSAR_MEM_HOST || query_stride < 3 || target_stride < 3) { ctx->err = "stub: host memory and strides >= 3 only"; return TSAR_ERR_INVALID; }
    const volatile float r2v = p->max_dist * p->max_dist;
    const float r2 = r2v;
    if (!(r2 > 0.0f) || !isfinite(r2)) { ctx->err = "tsar_cloud_distance: max_dist must be finite and > 0"; return TSAR_ERR_INVALID; }
    int64_t nq = 0, nt = 0;
    for (int64_t i = 0; i < n_query; i++) nq += candidate(query + i * query_stride);
    for (int64_t j = 0; j < n_target; j++) nt += candidate(target + j * target_stride);
    if (pairs_out) *pairs_out = nq * nt;
    if (nq * nt > p->max_pairs) { ctx->err = "tsar_cloud_distance: more than max_pairs pairs"; return TSAR_ERR_INVALID; }
    if (n_valid_query_out) *n_valid_query_out = nq;
    for (int k = 0; k < n_tol && within_out; k++) within_out[k] = 0;
    for (int64_t i = 0; i < n_query; i++) {
        const float* q = query + i * query_stride;
        float best = INFINITY;
        int32_t best_j = -1;
        if (candidate(q))
            for (int64_t j = 0; j < n_target; j++) {
                const float* t = target + j * target_stride;
                if (!candidate(t)) continue;
                const float dx = q[0] - t[0], dy = q[1] - t[1], dz = q[2] - t[2];
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                if (d2 <= r2 && d2 < best) { best = d2; best_j = (int32_t)j; }
            }
        if (dist2_out) dist2_out[i] = best;
        if (index_out) index_out[i] = best_j;
        for (int k = 0; k < n_tol && within_out; k++) {
            const volatile float t2 = tol[k] * tol[k];
            if (best <= t2) within_out[k]++;
        }
    }
    return TSAR_OK;
}

int tsar_cloud_distance(int device, const float* query, int64_t n_query, int query_stride, const float* target, int64_t n_target, int target_stride,
                        const tsar_cloud_distance_params* p, int n_tol, const float* tol, float* dist2_out, int32_t* index_out, int64_t* within_out,
                        int64_t* n_valid_query_out, int64_t* pairs_out, int mem) {
    tsar_ctx* ctx = nullptr;
    if (tsar_create(device, &ctx) != TSAR_OK) return TSAR_ERR_HIP;
    const int rc = tsar_cloud_distance_ctx(ctx, query, n_query, query_stride, target, n_target, target_stride, p, n_tol, tol, dist2_out, index_out, within_out,
                                           n_valid_query_out, pairs_out, mem);
    tsar_destroy(ctx);
    return rc;
}

}   // extern "C"
