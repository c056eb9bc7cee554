// Host stand-in of libtsar_hip.so for tests/test_cloud_render_cpu.py: the entries host/tsar_evaluate_maps.cpp calls, with the render and the
// comparison of include/tsar.h by brute force on the host in float32 (this file is built with -ffp-contract=off).  "Device" memory is host
// memory here.
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/tsar.h"

struct tsar_ctx { std::string err; };

extern "C" {

int tsar_create(int device, tsar_ctx** out) {
    if (device != 0) return TSAR_ERR_HIP;
    *out = new tsar_ctx;
    return TSAR_OK;
}
int tsar_destroy(tsar_ctx* ctx) { delete ctx; return TSAR_OK; }
const char* tsar_last_error(const tsar_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }

void* tsar_device_alloc(int, size_t bytes) { return bytes ? malloc(bytes) : nullptr; }
void tsar_device_free(int, void* p) { free(p); }
int tsar_device_write(int, void* dst, const void* host_src, size_t bytes) { memcpy(dst, host_src, bytes); return TSAR_OK; }
int tsar_device_read(int, void* host_dst, const void* src, size_t bytes) { memcpy(host_dst, src, bytes); return TSAR_OK; }

void tsar_default_cloud_render_params(tsar_cloud_render_params* p) {
    p->radius = 0.0f;
    p->max_px = 8;
    p->occlusion_diff = 0.02f;
    p->depth_diff = 0.01f;
    p->min_points = 1;
    p->max_splats = (int64_t)1 << 34;
}

struct Landing { bool lands; int xi, yi, s; float p2; };

static Landing land(const float* q, const float* P, float fr, bool foot, int max_px, int w, int h) {
    const float x = q[0], y = q[1], z = q[2];
    const float p0 = ((P[0] * x + P[1] * y) + P[2] * z) + P[3];
    const float p1 = ((P[4] * x + P[5] * y) + P[6] * z) + P[7];
    const float p2 = ((P[8] * x + P[9] * y) + P[10] * z) + P[11];
    const float xq = p0 / p2, yq = p1 / p2;
    const float xi = floorf(xq + 0.5f), yi = floorf(yq + 0.5f);
    Landing l;
    l.lands = isfinite(x) && isfinite(y) && isfinite(z) && p2 > 0.0f && p2 < INFINITY && xi >= 0.0f && xi <= (float)(w - 1) && yi >= 0.0f && yi <= (float)(h - 1);
    l.xi = l.lands ? (int)xi : 0;
    l.yi = l.lands ? (int)yi : 0;
    l.p2 = p2;
    l.s = 0;
    if (l.lands && foot) {
        const float sf = floorf(fr / p2 + 0.5f);
        l.s = sf < (float)max_px ? (int)sf : max_px;
    }
    return l;
}

int tsar_cloud_render_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_camera* cam, int w, int h, const tsar_cloud_render_params* p, float* depth_out,
                          uint8_t* count_out, int32_t* index_out, int64_t* n_splats_out, int mem) {
    (void)mem;                                            // host and "device" memory are the same here
    if (!p || !cam || stride < 3 || w < 1 || h < 1 || (!depth_out && !count_out && !index_out)) { ctx->err = "stub: bad arguments"; return TSAR_ERR_INVALID; }
    const volatile float frv = cam->K[0] * p->radius;
    const float fr = frv;
    if (!(p->radius >= 0.0f && p->radius <= FLT_MAX) || !(fr >= 0.0f && fr <= FLT_MAX)) { ctx->err = "tsar_cloud_render: radius must be finite and >= 0"; return TSAR_ERR_INVALID; }
    float P[12];
    for (int k = 0; k < 3; k++) {
        const double k0 = cam->K[k * 3], k1 = cam->K[k * 3 + 1], k2 = cam->K[k * 3 + 2];
        for (int j = 0; j < 3; j++) P[k * 4 + j] = (float)((k0 * (double)cam->R[j] + k1 * (double)cam->R[3 + j]) + k2 * (double)cam->R[6 + j]);
        P[k * 4 + 3] = (float)((k0 * (double)cam->t[0] + k1 * (double)cam->t[1]) + k2 * (double)cam->t[2]);
    }
    const bool foot = p->radius > 0.0f;
    const size_t np = (size_t)w * h;
    std::vector<float> Zc(np, INFINITY), Zo(np, INFINITY);
    std::vector<int64_t> winner(np, -1), support(np, 0);
    int64_t splats = 0;
    for (int pass = 0; pass < 3; pass++) {                // 0: the splat count; 1: both minima; 2: the support counts
        for (int64_t i = 0; i < n; i++) {
            const Landing l = land(cloud + i * stride, P, fr, foot, p->max_px, w, h);
            if (!l.lands) continue;
            const size_t at = (size_t)l.yi * w + l.xi;
            if (pass == 2) {
                const float dd = p->depth_diff * Zc[at];
                if (fabsf(l.p2 - Zc[at]) <= dd) support[at]++;
                continue;
            }
            if (pass == 1 && (winner[at] < 0 || l.p2 < Zc[at])) { Zc[at] = l.p2; winner[at] = i; }   // (ascending i: the first of equals stays)
            for (int yy = l.yi - l.s; yy <= l.yi + l.s; yy++)
                for (int xx = l.xi - l.s; xx <= l.xi + l.s; xx++) {
                    if (xx < 0 || xx >= w || yy < 0 || yy >= h) continue;
                    if (pass == 0) splats++;
                    else if (l.p2 < Zo[(size_t)yy * w + xx]) Zo[(size_t)yy * w + xx] = l.p2;
                }
        }
        if (pass == 0) {
            if (n_splats_out) *n_splats_out = splats;
            if (splats > p->max_splats) { ctx->err = "tsar_cloud_render: more than max_splats splats"; return TSAR_ERR_INVALID; }
        }
    }
    for (size_t q = 0; q < np; q++) {
        const bool landed = winner[q] >= 0;
        const bool visible = landed && Zc[q] - Zo[q] <= p->occlusion_diff * Zo[q];
        const bool kept = visible && support[q] >= p->min_points;
        if (count_out) count_out[q] = (uint8_t)(support[q] > 255 ? 255 : support[q]);
        if (depth_out) depth_out[q] = kept ? Zc[q] : 0.0f;
        if (index_out) index_out[q] = kept ? (int32_t)winner[q] : -1;
    }
    return TSAR_OK;
}

int tsar_depth_compare_ctx(tsar_ctx* ctx, const float* depth, const float* gt, const uint8_t* mask, int64_t n, int n_tol, const float* tol, int64_t* n_gt_out,
                           int64_t* n_both_out, int64_t* within_out, int64_t* n_front_out, int64_t* n_behind_out, float* error_out, int mem) {
    (void)mem;
    if (n_tol < 1 || n_tol > TSAR_DEPTH_COMPARE_MAX_TOL || !tol) { ctx->err = "tsar_depth_compare: n_tol must be in 1..16, and tol not NULL"; return TSAR_ERR_INVALID; }
    int64_t n_gt = 0, n_both = 0, n_front = 0, n_behind = 0;
    std::vector<int64_t> within((size_t)n_tol, 0);
    for (int64_t i = 0; i < n; i++) {
        const float D = depth[i], G = gt[i];
        const bool is_gt = G > 0.0f && G < INFINITY && (!mask || mask[i] != 0);
        const bool both = is_gt && D > 0.0f && D < INFINITY;
        n_gt += is_gt;
        n_both += both;
        if (error_out) error_out[i] = both ? (D - G) / G : NAN;
        if (!both) continue;
        const float diff = D - G;
        const float t0 = tol[0] * G;
        n_front += diff < -t0;
        n_behind += diff > t0;
        for (int k = 0; k < n_tol; k++) {
            const float tk = tol[k] * G;
            within[(size_t)k] += fabsf(diff) <= tk;
        }
    }
    if (n_gt_out) *n_gt_out = n_gt;
    if (n_both_out) *n_both_out = n_both;
    if (n_front_out) *n_front_out = n_front;
    if (n_behind_out) *n_behind_out = n_behind;
    for (int k = 0; k < n_tol && within_out; k++) within_out[k] = within[(size_t)k];
    return TSAR_OK;
}

}   // extern "C"
