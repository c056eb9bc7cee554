// Host stand-in of libtsar_hip.so for tests/test_voxel_cli_cpu.py: the cloud-distance entries of tsar_stub_cloud.cpp plus the voxel grid of
// include/tsar.h (tsar_cloud_voxels) by brute force on the host: a map from the voxel key to its points (this file is built with
// -ffp-contract=off).
#include "tsar_stub_cloud.cpp"

#include <map>
#include <vector>

extern "C" {

void tsar_default_cloud_voxels_params(tsar_cloud_voxels_params* p) { p->voxel = 0.0f; }

int tsar_cloud_voxels_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_voxels_params* p, const float* dist2, int n_tol, const float* tol,
                          int32_t* rank_out, int64_t cap, int32_t* rep_out, int32_t* count_out, int32_t* within_out, int64_t* n_voxels_out, int64_t* n_valid_out, int mem) {
    if (mem != TSAR_MEM_HOST || stride < 3 || cap < 0) { ctx->err = "stub: host memory, strides >= 3 and cap >= 0 only"; return TSAR_ERR_INVALID; }
    if (!(p->voxel > 0.0f) || !isfinite(p->voxel)) { ctx->err = "tsar_cloud_voxels: voxel must be finite and > 0"; return TSAR_ERR_INVALID; }
    if ((n_tol > 0 && (!tol || (!dist2 && n > 0))) || (n_tol == 0 && within_out)) { ctx->err = "tsar_cloud_voxels: tolerances and dist2 go together"; return TSAR_ERR_INVALID; }
    const double V = (double)p->voxel;
    float o[3] = {INFINITY, INFINITY, INFINITY};
    int64_t n_valid = 0;
    for (int64_t i = 0; i < n; i++) {
        const float* q = cloud + i * stride;
        if (!candidate(q)) continue;
        n_valid++;
        for (int a = 0; a < 3; a++) o[a] = q[a] < o[a] ? q[a] : o[a];
    }
    std::map<uint64_t, std::vector<int64_t>> voxels;          // ascending key order; the points of a voxel in index order
    for (int64_t i = 0; i < n; i++) {
        const float* q = cloud + i * stride;
        if (!candidate(q)) continue;
        uint64_t c[3];
        for (int a = 0; a < 3; a++) {
            const double cell = floor(((double)q[a] - (double)o[a]) / V);
            if (!(cell < 2097152.0)) { ctx->err = "tsar_cloud_voxels: 2^21 cells or more on an axis"; return TSAR_ERR_INVALID; }
            c[a] = (uint64_t)cell;
        }
        voxels[(c[2] << 42) | (c[1] << 21) | c[0]].push_back(i);
    }
    for (int64_t i = 0; i < n && rank_out; i++) rank_out[i] = -1;
    int64_t v = 0;
    for (const auto& kv : voxels) {
        const uint64_t c[3] = {kv.first & 0x1fffffu, (kv.first >> 21) & 0x1fffffu, kv.first >> 42};
        uint64_t best = ~(uint64_t)0;
        std::vector<int32_t> within((size_t)(n_tol > 0 ? n_tol : 1), 0);
        for (const int64_t i : kv.second) {
            const float* q = cloud + i * stride;
            double d[3];
            for (int a = 0; a < 3; a++) {
                const double prod = ((double)c[a] + 0.5) * V;
                const double centre = (double)o[a] + prod;
                d[a] = (double)q[a] - centre;
            }
            const double d2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
            const float d2f = (float)d2;
            uint32_t bits;
            memcpy(&bits, &d2f, 4);
            const uint64_t code = ((uint64_t)bits << 32) | (uint64_t)i;
            best = code < best ? code : best;
            for (int k = 0; k < n_tol; k++) {
                const volatile float t2 = tol[k] * tol[k];
                if (dist2[i] <= t2) within[(size_t)k]++;
            }
            if (rank_out) rank_out[i] = (int32_t)v;
        }
        if (v < cap) {
            if (rep_out) rep_out[v] = (int32_t)(uint32_t)best;
            if (count_out) count_out[v] = (int32_t)kv.second.size();
            for (int k = 0; k < n_tol && within_out; k++) within_out[v * n_tol + k] = within[(size_t)k];
        }
        v++;
    }
    if (n_voxels_out) *n_voxels_out = v;
    if (n_valid_out) *n_valid_out = n_valid;
    return TSAR_OK;
}

int tsar_cloud_voxels(int device, const float* cloud, int64_t n, int stride, const tsar_cloud_voxels_params* p, const float* dist2, int n_tol, const float* tol,
                      int32_t* rank_out, int64_t cap, int32_t* rep_out, int32_t* count_out, int32_t* within_out, int64_t* n_voxels_out, int64_t* n_valid_out, int mem) {
    tsar_ctx* ctx = nullptr;
    if (tsar_create(device, &ctx) != TSAR_OK) return TSAR_ERR_HIP;
    const int rc = tsar_cloud_voxels_ctx(ctx, cloud, n, stride, p, dist2, n_tol, tol, rank_out, cap, rep_out, count_out, within_out, n_voxels_out, n_valid_out, mem);
    tsar_destroy(ctx);
    return rc;
}

}   // extern "C"
