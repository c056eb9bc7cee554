// A recording stand-in for the C ABI (include/tsar.h), for tests/test_cli_phases_cpu.py: every tsar_* entry that host/tsar_gipuma.cpp
// calls, without HIP and without a device.  Each call appends one line to the file named by TSAR_STUB_TRACE: the function, the
// context's ordinal in order of tsar_create, every integer argument, every float argument as %.9g, null / set for each pointer and
// the fields of a params struct.  Outputs are fixed functions of the pixel index, so the files the tool writes are complete and
// comparable.  TSAR_STUB_FAIL=<function>:<n> makes the n-th call of that function return TSAR_ERR_HIP, once.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <map>
#include <mutex>
#include <string>

#include "../../include/tsar.h"

struct tsar_ctx { int ord, device, w, h; };

namespace {
std::mutex g_mu;
int g_created = 0;
std::map<std::string, int> g_calls;

// one trace line "<fn> <args>"; the status the call returns (TSAR_ERR_HIP on the call TSAR_STUB_FAIL names, and the line says so)
int trace(const char* fn, const char* fmt, ...) {
    std::lock_guard<std::mutex> lk(g_mu);
    int rc = TSAR_OK;
    const int nth = ++g_calls[fn];
    if (const char* f = getenv("TSAR_STUB_FAIL")) {
        const char* colon = strrchr(f, ':');
        if (colon && std::string(f, colon) == fn && atoi(colon + 1) == nth) rc = TSAR_ERR_HIP;
    }
    const char* path = getenv("TSAR_STUB_TRACE");
    if (path && *path)
        if (FILE* fp = fopen(path, "a")) {
            fputs(fn, fp);
            if (*fmt) fputc(' ', fp);
            va_list ap;
            va_start(ap, fmt);
            vfprintf(fp, fmt, ap);
            va_end(ap);
            fputs(rc == TSAR_OK ? "\n" : " -> TSAR_ERR_HIP\n", fp);
            fclose(fp);
        }
    return rc;
}
const char* ps(const void* p) { return p ? "set" : "null"; }
int ord(const tsar_ctx* c) { return c ? c->ord : -1; }
size_t npix(const tsar_ctx* c) { return (size_t)c->w * c->h; }
bool kept(size_t p) { return p % 3 != 0; }      // the pixels the check keeps
}   // namespace

extern "C" {

int tsar_create(int device, tsar_ctx** out) {
    int o;
    { std::lock_guard<std::mutex> lk(g_mu); o = g_created++; }
    const int rc = trace("tsar_create", "device=%d ctx=%d", device, o);
    if (rc != TSAR_OK) return rc;
    *out = new tsar_ctx{o, device, 0, 0};
    return TSAR_OK;
}
int tsar_destroy(tsar_ctx* ctx) {
    if (!ctx) return TSAR_OK;                    // (the tool destroys a worker's context whether it has one or not)
    const int rc = trace("tsar_destroy", "ctx=%d", ord(ctx));
    delete ctx;
    return rc;
}
const char* tsar_last_error(const tsar_ctx* ctx) {
    trace("tsar_last_error", "ctx=%d", ord(ctx));
    return "stub: injected failure";
}
int tsar_synchronize(tsar_ctx* ctx) { return trace("tsar_synchronize", "ctx=%d", ord(ctx)); }

void tsar_default_params(tsar_params* p) {
    trace("tsar_default_params", "");
    memset(p, 0, sizeof *p);
    p->box_hsize = p->box_vsize = 19; p->n_best = 2; p->cost_comb = TSAR_COMB_BEST_N;
    p->depth_min = 2.0f; p->depth_max = 20.0f; p->cam_scale = 1.0f;
}
void tsar_default_fusion_params(tsar_fusion_params* p) {
    trace("tsar_default_fusion_params", "");
    p->num_consistent = 1; p->reproj_error = 2.0f; p->depth_diff = 0.01f; p->angle_deg = 15.0f; p->used_list = 1;
}
void tsar_default_geom_check_params(tsar_geom_check_params* p) {
    trace("tsar_default_geom_check_params", "");
    p->reproj_error = 2.0f; p->depth_diff = 0.01f; p->min_consistent = 2;
}
void tsar_default_geom_reproject_params(tsar_geom_reproject_params* p) {
    trace("tsar_default_geom_reproject_params", "");
    p->depth_diff = 0.01f; p->min_views = 1;
}
void tsar_default_plane_prior_params(tsar_plane_prior_params* p) {
    trace("tsar_default_plane_prior_params", "");
    p->weight_depth = 0.1f; p->weight_normal = 0.05f; p->depth_clip = 0.02f; p->normal_clip = (float)(1.0 - 0.86602540378443864676);
}

int tsar_set_params(tsar_ctx* ctx, const tsar_params* p) {
    return trace("tsar_set_params", "ctx=%d box=%dx%d n_best=%d cost_comb=%d depth_min=%.9g depth_max=%.9g cam_scale=%.9g flags=%u seed=%llu", ord(ctx),
                 p->box_hsize, p->box_vsize, p->n_best, p->cost_comb, (double)p->depth_min, (double)p->depth_max, (double)p->cam_scale, p->flags,
                 (unsigned long long)p->seed);
}
int tsar_set_views_u8(tsar_ctx* ctx, int n_views, int w, int h, const uint8_t* const* gray, int mem, const tsar_camera* cams) {
    ctx->w = w; ctx->h = h;
    return trace("tsar_set_views_u8", "ctx=%d n_views=%d w=%d h=%d gray=%s mem=%d cams=%s", ord(ctx), n_views, w, h, ps(gray), mem, ps(cams));
}
int tsar_set_view_subset(tsar_ctx* ctx, int n, const int32_t* view_idx) {
    std::string idx;
    for (int i = 0; i < n; i++) idx += (i ? "," : "") + std::to_string(view_idx[i]);
    return trace("tsar_set_view_subset", "ctx=%d n=%d view_idx=%s", ord(ctx), n, idx.c_str());
}

int tsar_pm_init(tsar_ctx* ctx) { return trace("tsar_pm_init", "ctx=%d", ord(ctx)); }
int tsar_pm_iterate(tsar_ctx* ctx, int iters) { return trace("tsar_pm_iterate", "ctx=%d iters=%d", ord(ctx), iters); }
int tsar_pm_rescore(tsar_ctx* ctx) { return trace("tsar_pm_rescore", "ctx=%d", ord(ctx)); }
int tsar_load_planes(tsar_ctx* ctx, const float* depth, const float* normal_world, int mem) {
    return trace("tsar_load_planes", "ctx=%d depth=%s normal_world=%s mem=%d", ord(ctx), ps(depth), ps(normal_world), mem);
}
int tsar_compute_disp(tsar_ctx* ctx) { return trace("tsar_compute_disp", "ctx=%d", ord(ctx)); }
int tsar_compute_disp_final_upsampled(tsar_ctx* ctx, const float* text, int mem) {
    return trace("tsar_compute_disp_final_upsampled", "ctx=%d text=%s mem=%d", ord(ctx), ps(text), mem);
}

int tsar_pyramid_views(tsar_ctx* coarse, const tsar_ctx* fine) {
    coarse->w = (fine->w + 1) / 2; coarse->h = (fine->h + 1) / 2;
    return trace("tsar_pyramid_views", "coarse=%d fine=%d", ord(coarse), ord(fine));
}
int tsar_upsample_planes(tsar_ctx* fine, const tsar_ctx* coarse) { return trace("tsar_upsample_planes", "fine=%d coarse=%d", ord(fine), ord(coarse)); }
int tsar_geom_pyramid(tsar_ctx* coarse, const tsar_ctx* fine) { return trace("tsar_geom_pyramid", "coarse=%d fine=%d", ord(coarse), ord(fine)); }
int tsar_pyramid_planes(tsar_ctx* coarse, const tsar_ctx* fine) { return trace("tsar_pyramid_planes", "coarse=%d fine=%d", ord(coarse), ord(fine)); }
int tsar_upsample_merge(tsar_ctx* fine, const tsar_ctx* coarse) { return trace("tsar_upsample_merge", "fine=%d coarse=%d", ord(fine), ord(coarse)); }

int tsar_set_geom_depths(tsar_ctx* ctx, int n_views, const float* const* depth, int mem, float weight, float clip) {
    std::string maps;
    for (int i = 0; i < n_views; i++) maps += std::string(i ? "," : "") + ps(depth[i]);
    return trace("tsar_set_geom_depths", "ctx=%d n_views=%d depth=%s mem=%d weight=%.9g clip=%.9g", ord(ctx), n_views, maps.c_str(), mem, (double)weight, (double)clip);
}
int tsar_clear_geom(tsar_ctx* ctx) { return trace("tsar_clear_geom", "ctx=%d", ord(ctx)); }
int tsar_geom_check(tsar_ctx* ctx, const float* depth, const tsar_geom_check_params* p, uint8_t* count_out, float* depth_out, int mem) {
    const int rc = trace("tsar_geom_check", "ctx=%d depth=%s reproj_error=%.9g depth_diff=%.9g min_consistent=%d count_out=%s depth_out=%s mem=%d", ord(ctx),
                         ps(depth), (double)p->reproj_error, (double)p->depth_diff, p->min_consistent, ps(count_out), ps(depth_out), mem);
    if (rc != TSAR_OK) return rc;
    for (size_t k = 0; k < npix(ctx); k++) {
        if (count_out) count_out[k] = kept(k) ? (uint8_t)p->min_consistent : 0;
        if (depth_out) depth_out[k] = kept(k) && depth ? depth[k] : 0.0f;
    }
    return TSAR_OK;
}
int tsar_geom_reproject(tsar_ctx* ctx, const tsar_geom_reproject_params* p, float* depth_out, uint8_t* count_out, int mem) {
    const int rc = trace("tsar_geom_reproject", "ctx=%d depth_diff=%.9g min_views=%d depth_out=%s count_out=%s mem=%d", ord(ctx), (double)p->depth_diff,
                         p->min_views, ps(depth_out), ps(count_out), mem);
    if (rc != TSAR_OK) return rc;
    for (size_t k = 0; k < npix(ctx); k++) {
        if (depth_out) depth_out[k] = kept(k) ? 1.0f : 0.0f;
        if (count_out) count_out[k] = kept(k) ? 1 : 0;
    }
    return TSAR_OK;
}
int tsar_pm_merge_depths(tsar_ctx* ctx, const float* depth, int mem, int64_t* n_taken_out) {
    if (n_taken_out) *n_taken_out = 0;
    return trace("tsar_pm_merge_depths", "ctx=%d depth=%s mem=%d n_taken_out=%s", ord(ctx), ps(depth), mem, ps(n_taken_out));
}
int tsar_set_plane_prior(tsar_ctx* ctx, const float* depth, const float* normal_world, int mem, const tsar_plane_prior_params* p) {
    return trace("tsar_set_plane_prior", "ctx=%d depth=%s normal_world=%s mem=%d weight_depth=%.9g weight_normal=%.9g depth_clip=%.9g normal_clip=%.9g", ord(ctx),
                 ps(depth), ps(normal_world), mem, (double)p->weight_depth, (double)p->weight_normal, (double)p->depth_clip, (double)p->normal_clip);
}
int tsar_clear_plane_prior(tsar_ctx* ctx) { return trace("tsar_clear_plane_prior", "ctx=%d", ord(ctx)); }

// depth in (0, inf) and one of three exact unit normals, by pixel index
int tsar_get_result(tsar_ctx* ctx, float* depth, float* normal_world, float* cost, float* confid, int mem) {
    const int rc = trace("tsar_get_result", "ctx=%d depth=%s normal_world=%s cost=%s confid=%s mem=%d", ord(ctx), ps(depth), ps(normal_world), ps(cost), ps(confid), mem);
    if (rc != TSAR_OK) return rc;
    static const float N[3][3] = {{0.f, 0.f, -1.f}, {0.6f, 0.f, -0.8f}, {0.f, 0.6f, -0.8f}};
    for (size_t k = 0; k < npix(ctx); k++) {
        if (depth) depth[k] = 1.0f + (float)(k % 97) * 0.03125f;
        if (normal_world) memcpy(normal_world + 3 * k, N[k % 3], sizeof N[0]);
        if (cost) cost[k] = 0.5f;
        if (confid) confid[k] = 1.0f;
    }
    return TSAR_OK;
}

int tsar_set_reliable_mask(tsar_ctx* ctx, const float* scale, int mem) { return trace("tsar_set_reliable_mask", "ctx=%d scale=%s mem=%d", ord(ctx), ps(scale), mem); }
int tsar_get_reliable_mask(tsar_ctx* ctx, float* scale, int mem) {
    const int rc = trace("tsar_get_reliable_mask", "ctx=%d scale=%s mem=%d", ord(ctx), ps(scale), mem);
    if (rc != TSAR_OK) return rc;
    for (size_t k = 0; k < npix(ctx); k++) scale[k] = kept(k) ? 1.0f : 0.0f;
    return TSAR_OK;
}
int tsar_getview(tsar_ctx* ctx) { return trace("tsar_getview", "ctx=%d", ord(ctx)); }
int tsar_detect_weak_texture(tsar_ctx* ctx, int32_t* labels_out, int mem, int* n_regions_out, float* text_out, float* size_out, int cap) {
    const int rc = trace("tsar_detect_weak_texture", "ctx=%d labels_out=%s mem=%d n_regions_out=%s text_out=%s size_out=%s cap=%d", ord(ctx), ps(labels_out), mem,
                         ps(n_regions_out), ps(text_out), ps(size_out), cap);
    if (rc != TSAR_OK) return rc;
    if (labels_out) memset(labels_out, 0, npix(ctx) * sizeof(int32_t));      // one region, textureless
    if (n_regions_out) *n_regions_out = 1;
    if (text_out && cap > 0) text_out[0] = -1.0f;
    if (size_out && cap > 0) size_out[0] = (float)npix(ctx);
    return TSAR_OK;
}
int tsar_ransac_regions(tsar_ctx* ctx, float* region_planes_out, float* inlier_ratio_out) {
    const int rc = trace("tsar_ransac_regions", "ctx=%d region_planes_out=%s inlier_ratio_out=%s", ord(ctx), ps(region_planes_out), ps(inlier_ratio_out));
    if (rc != TSAR_OK) return rc;
    if (region_planes_out) { const float pl[4] = {0.f, 0.f, -1.f, 1.f}; memcpy(region_planes_out, pl, sizeof pl); }
    if (inlier_ratio_out) inlier_ratio_out[0] = 1.0f;
    return TSAR_OK;
}
int tsar_fake_depth(tsar_ctx* ctx, float* fakedepth_out, int mem) { return trace("tsar_fake_depth", "ctx=%d fakedepth_out=%s mem=%d", ord(ctx), ps(fakedepth_out), mem); }
int tsar_fill_textureless(tsar_ctx* ctx) { return trace("tsar_fill_textureless", "ctx=%d", ord(ctx)); }

int tsar_fuse(int device, int n_views, int w, int h, const tsar_camera* cams, const float* const* depth, const float* const* normal_world, const float* const* gray,
              int mem, const int32_t* src_off, const int32_t* src_idx, const tsar_fusion_params* params, float* points_out, int64_t cap, int64_t* n_points_out) {
    std::string csr;
    for (int v = 0; v < n_views; v++) {
        csr += v ? "|" : "";
        for (int32_t k = src_off[v]; k < src_off[v + 1]; k++) csr += (k > src_off[v] ? "," : "") + std::to_string(src_idx[k]);
    }
    const int rc = trace("tsar_fuse", "device=%d n_views=%d w=%d h=%d cams=%s depth=%s normal_world=%s gray=%s mem=%d sources=%s num_consistent=%d reproj_error=%.9g "
                         "depth_diff=%.9g angle_deg=%.9g used_list=%d points_out=%s cap=%lld n_points_out=%s", device, n_views, w, h, ps(cams), ps(depth),
                         ps(normal_world), ps(gray), mem, csr.c_str(), params->num_consistent, (double)params->reproj_error, (double)params->depth_diff,
                         (double)params->angle_deg, params->used_list, ps(points_out), (long long)cap, ps(n_points_out));
    if (rc != TSAR_OK) return rc;
    static const float pts[18] = {0.f, 0.f, 1.f, 0.f, 0.f, -1.f, 128.f, 2.f, 0.f, 1.f, 2.f, 3.f, 0.6f, 0.f, -0.8f, 64.f, 3.f, 1.f};
    if (points_out && cap >= 2) memcpy(points_out, pts, sizeof pts);
    *n_points_out = 2;
    return TSAR_OK;
}

void* tsar_host_alloc(size_t bytes) { trace("tsar_host_alloc", "bytes=%zu", bytes); return malloc(bytes); }
void tsar_host_free(void* p) { trace("tsar_host_free", "p=%s", ps(p)); free(p); }
void* tsar_device_alloc(int device, size_t bytes) { trace("tsar_device_alloc", "device=%d bytes=%zu", device, bytes); return malloc(bytes); }
void tsar_device_free(int device, void* p) { trace("tsar_device_free", "device=%d p=%s", device, ps(p)); free(p); }
int tsar_device_write(int device, void* dst, const void* host_src, size_t bytes) {
    const int rc = trace("tsar_device_write", "device=%d dst=%s host_src=%s bytes=%zu", device, ps(dst), ps(host_src), bytes);
    if (rc == TSAR_OK) memcpy(dst, host_src, bytes);
    return rc;
}
int tsar_peer_copy(int dst_device, void* dst, int src_device, const void* src, size_t bytes) {
    const int rc = trace("tsar_peer_copy", "dst_device=%d dst=%s src_device=%d src=%s bytes=%zu", dst_device, ps(dst), src_device, ps(src), bytes);
    if (rc == TSAR_OK) memcpy(dst, src, bytes);
    return rc;
}

int tsar_enable_kernel_timing(tsar_ctx* ctx, int enable) { return trace("tsar_enable_kernel_timing", "ctx=%d enable=%d", ord(ctx), enable); }
int tsar_reset_kernel_timing(tsar_ctx* ctx) { return trace("tsar_reset_kernel_timing", "ctx=%d", ord(ctx)); }
int tsar_get_kernel_timing(tsar_ctx* ctx, tsar_kernel_timing* out, int cap, int* n_out) {
    if (n_out) *n_out = 0;
    return trace("tsar_get_kernel_timing", "ctx=%d out=%s cap=%d n_out=%s", ord(ctx), ps(out), cap, ps(n_out));
}

}   // extern "C"
