// fusion_kernels.hip — geometric-consistency depth-map fusion on the GPU.
// The reference ships the fuser only as a binary (Fusion.exe, driven by x/1.sh:20-30 with
// --num_consistent= --reproj_error= --depth_diff= --angle= --used_list=); this is the published ACMH/ACMM
// fusion that binary derives from, fed directly from device-resident depth / normal maps (e.g. the buffers
// the RCCL gather of bench.py / driver.py delivers), so the pipeline closes on the GPU.
//
// One launch per reference view (views are processed in order because "used" marks made by one view gate
// the next): each thread owns a pixel, back-projects it, visits its source views, and keeps the pixel when
// enough sources agree.  Marks go to a second array that becomes visible when the next view starts, and the
// accepted points are compacted in raster order (rocPRIM select), so the output is deterministic.
#include <math.h>
#include <rocprim/device/device_select.hpp>

#include "tsar_dev.h"

#define FU_BLOCK 256
#define FU_MAX_SRC 64

struct FuCam { float K[9], R[9], t[3]; };
struct FuRec { float v[9]; };   // xyz, unit normal, gray, n_consistent, view

__device__ __forceinline__ float fdot3(const float* a, const float* b) { return __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0])); }
__device__ __forceinline__ void unproject(const FuCam& c, float x, float y, float depth, float* X) {
    const float pc[3] = {depth * (x - c.K[2]) / c.K[0], depth * (y - c.K[5]) / c.K[4], depth};
    const float d[3] = {pc[0] - c.t[0], pc[1] - c.t[1], pc[2] - c.t[2]};
    X[0] = __builtin_fmaf(c.R[6], d[2], __builtin_fmaf(c.R[3], d[1], c.R[0] * d[0]));
    X[1] = __builtin_fmaf(c.R[7], d[2], __builtin_fmaf(c.R[4], d[1], c.R[1] * d[0]));
    X[2] = __builtin_fmaf(c.R[8], d[2], __builtin_fmaf(c.R[5], d[1], c.R[2] * d[0]));
}
__device__ __forceinline__ void project(const FuCam& c, const float* X, float& px, float& py, float& depth) {
    const float pc[3] = {fdot3(c.R, X) + c.t[0], fdot3(c.R + 3, X) + c.t[1], fdot3(c.R + 6, X) + c.t[2]};
    depth = pc[2];
    px = c.K[0] * pc[0] / pc[2] + c.K[2];
    py = c.K[4] * pc[1] / pc[2] + c.K[5];
}

__global__ __launch_bounds__(FU_BLOCK) void fuse_view_kernel(int view, int w, int h, const FuCam* __restrict__ cams, const float* const* __restrict__ depth,
                                                             const float* const* __restrict__ normal, const float* const* __restrict__ gray,
                                                             const int32_t* __restrict__ src, int ns, const uint8_t* __restrict__ mask,
                                                             uint8_t* __restrict__ pending, int num_consistent, float reproj_error, float depth_diff,
                                                             float cos_angle, int use_marks, FuRec* __restrict__ rec, uint8_t* __restrict__ keep) {
    const int p = blockIdx.x * FU_BLOCK + threadIdx.x;
    const size_t np = (size_t)w * h;
    if (p >= (int)np) return;
    keep[p] = 0;
    if (use_marks && mask[(size_t)view * np + p]) return;
    const float ref_depth = depth[view][p];
    if (!(ref_depth > 0.0f)) return;
    const int r = p / w, c = p - r * w;
    const FuCam ci = cams[view];
    const float* rn = normal[view] + 3 * (size_t)p;
    const float rnv[3] = {rn[0], rn[1], rn[2]};
    float X[3];
    unproject(ci, (float)c, (float)r, ref_depth, X);
    float acc[3] = {X[0], X[1], X[2]}, nacc[3] = {rnv[0], rnv[1], rnv[2]}, gacc = gray[view][p];
    int ncons = 0;
    unsigned long long used_bits = 0ull;
    int used_q[FU_MAX_SRC];
    for (int k = 0; k < ns && k < FU_MAX_SRC; k++) {
        const int j = src[k];
        const FuCam cj = cams[j];
        float sx, sy, sd;
        project(cj, X, sx, sy, sd);
        if (!(sd > 0.0f)) continue;
        const int sr = (int)floorf(sy + 0.5f), scn = (int)floorf(sx + 0.5f);
        if (sr < 0 || sr >= h || scn < 0 || scn >= w) continue;
        const size_t q = (size_t)sr * w + scn;
        if (use_marks && mask[(size_t)j * np + q]) continue;
        const float src_depth = depth[j][q];
        if (!(src_depth > 0.0f)) continue;
        float Y[3], bx, by, bd;
        unproject(cj, (float)scn, (float)sr, src_depth, Y);
        project(ci, Y, bx, by, bd);
        const float ex = (float)c - bx, ey = (float)r - by;
        const float err = sqrtf(__builtin_fmaf(ex, ex, ey * ey));
        const float rel = fabsf(bd - ref_depth) / ref_depth;
        const float* sn = normal[j] + 3 * q;
        const float snv[3] = {sn[0], sn[1], sn[2]};
        const float cosang = fdot3(rnv, snv);
        if (err < reproj_error && rel < depth_diff && cosang >= cos_angle) {
            acc[0] += Y[0]; acc[1] += Y[1]; acc[2] += Y[2];
            nacc[0] += snv[0]; nacc[1] += snv[1]; nacc[2] += snv[2];
            gacc += gray[j][q];
            used_bits |= 1ull << k;
            used_q[k] = (int)q;
            ncons++;
        }
    }
    if (ncons < num_consistent) return;
    const float inv = 1.0f / (float)(ncons + 1);
    FuRec o;
    o.v[0] = acc[0] * inv; o.v[1] = acc[1] * inv; o.v[2] = acc[2] * inv;
    const float nn[3] = {nacc[0] * inv, nacc[1] * inv, nacc[2] * inv};
    const float nl = 1.0f / sqrtf(fdot3(nn, nn));
    o.v[3] = nn[0] * nl; o.v[4] = nn[1] * nl; o.v[5] = nn[2] * nl;
    o.v[6] = gacc * inv; o.v[7] = (float)ncons; o.v[8] = (float)view;
    rec[p] = o;
    keep[p] = 1;
    if (use_marks)
        for (int k = 0; k < ns && k < FU_MAX_SRC; k++)
            if (used_bits >> k & 1ull) pending[(size_t)src[k] * np + (size_t)used_q[k]] = 1;
}

// On a context: its stream, and every temporary (uploaded maps, marks, records, rocPRIM scratch) out of its scratch arena — a host
// that fuses scene after scene (or the tests, call after call) allocates nothing from the second call on (tsar_dev.h CallFrame).
extern "C" int tsar_fuse_ctx(tsar_ctx* ctx, int n_views, int w, int h, const tsar_camera* cams, const float* const* depth, const float* const* normal_world,
                             const float* const* gray, int mem, const int32_t* src_off, const int32_t* src_idx, const tsar_fusion_params* prm,
                             float* points_out, int64_t cap, int64_t* n_points_out) {
    CHECK_CTX(ctx);
    if (n_views < 2 || w < 1 || h < 1 || !cams || !depth || !normal_world || !gray || !src_off || !src_idx || !prm || !n_points_out)
        return fail(ctx, TSAR_ERR_INVALID, "tsar_fuse: null argument, fewer than two views or an empty image");
    if (mem != TSAR_MEM_DEVICE && mem != TSAR_MEM_HOST) return fail(ctx, TSAR_ERR_INVALID, "tsar_fuse: mem must be TSAR_MEM_HOST or TSAR_MEM_DEVICE");
    const size_t np = (size_t)w * h;
    hipStream_t st = ctx->stream;
    CallFrame f(ctx, "tsar_fuse");
    const char* bad_view = "tsar_fuse: a view's maps are NULL or a source index is out of range";
    // inputs
    std::vector<const float*> hd(n_views), hn(n_views), hg(n_views);
    for (int v = 0; v < n_views; v++) {
        if (!depth[v] || !normal_world[v] || !gray[v]) return f.fail(TSAR_ERR_INVALID, bad_view);
        hd[v] = f.in(depth[v], np, mem);
        hn[v] = f.in(normal_world[v], 3 * np, mem);
        hg[v] = f.in(gray[v], np, mem);
    }
    std::vector<FuCam> hc(n_views);
    for (int v = 0; v < n_views; v++) { memcpy(hc[v].K, cams[v].K, 36); memcpy(hc[v].R, cams[v].R, 36); memcpy(hc[v].t, cams[v].t, 12); }
    FuCam* d_cams = f.tmp<FuCam>(n_views);
    const float **d_depth = f.tmp<const float*>(n_views), **d_normal = f.tmp<const float*>(n_views), **d_gray = f.tmp<const float*>(n_views);
    const int n_src_total = src_off[n_views];
    int32_t* d_src = f.tmp<int32_t>(n_src_total > 0 ? n_src_total : 1);
    uint8_t *mask = f.tmp<uint8_t>((size_t)n_views * np), *pending = f.tmp<uint8_t>((size_t)n_views * np), *keep = f.tmp<uint8_t>(np);
    FuRec *rec = f.tmp<FuRec>(np), *compact = f.tmp<FuRec>(np);
    unsigned int* d_count = f.tmp<unsigned int>(1);
    f.copy(d_cams, hc.data(), sizeof(FuCam) * n_views, hipMemcpyHostToDevice);
    f.copy((void*)d_depth, hd.data(), 8 * n_views, hipMemcpyHostToDevice);
    f.copy((void*)d_normal, hn.data(), 8 * n_views, hipMemcpyHostToDevice);
    f.copy((void*)d_gray, hg.data(), 8 * n_views, hipMemcpyHostToDevice);
    f.copy(d_src, src_idx, (size_t)(n_src_total > 0 ? n_src_total : 0) * 4, hipMemcpyHostToDevice);
    f.zero(mask, (size_t)n_views * np);
    f.zero(pending, (size_t)n_views * np);
    size_t tmp_bytes = 0;
    if (!f.ok() || !f.hip(rocprim::select(nullptr, tmp_bytes, rec, keep, compact, d_count, np, st), "rocprim::select sizing")) return f.finish();
    void* tmp = f.tmp<char>(tmp_bytes);
    if (!f.ok()) return f.finish();
    const float cos_angle = (float)cos((double)prm->angle_deg * 3.14159265358979323846 / 180.0);
    int64_t n_out = 0;
    for (int v = 0; v < n_views; v++) {
        const int ns = src_off[v + 1] - src_off[v];
        for (int k = 0; k < ns; k++)
            if (src_idx[src_off[v] + k] < 0 || src_idx[src_off[v] + k] >= n_views) return f.fail(TSAR_ERR_INVALID, bad_view);
        hipLaunchKernelGGL(fuse_view_kernel, dim3((unsigned)((np + FU_BLOCK - 1) / FU_BLOCK)), dim3(FU_BLOCK), 0, st, v, w, h, d_cams, d_depth, d_normal, d_gray,
                           d_src + src_off[v], ns, mask, pending, prm->num_consistent, prm->reproj_error, prm->depth_diff, cos_angle, prm->used_list ? 1 : 0, rec, keep);
        f.hip(rocprim::select(tmp, tmp_bytes, rec, keep, compact, d_count, np, st), "rocprim::select");
        unsigned int cnt = 0;
        f.copy(&cnt, d_count, 4, hipMemcpyDeviceToHost);
        if (!f.sync()) return f.finish();
        if (points_out && n_out < cap) {
            const int64_t take = (int64_t)cnt < cap - n_out ? (int64_t)cnt : cap - n_out;
            f.copy(points_out + 9 * n_out, compact, (size_t)take * sizeof(FuRec), kind_from_dev(mem));
        }
        n_out += cnt;
        if (prm->used_list) {   // marks of this view become visible to the next one; only its source views can have changed
            for (int k = 0; k < ns; k++) {
                const size_t o = (size_t)src_idx[src_off[v] + k] * np;
                f.copy(mask + o, pending + o, np, hipMemcpyDeviceToDevice);
            }
        }
    }
    *n_points_out = n_out;
    return f.finish();
}

// Context-free form (the fuser binary's one call per scene): a context of its own for the duration of the call.
extern "C" int tsar_fuse(int device, int n_views, int w, int h, const tsar_camera* cams, const float* const* depth, const float* const* normal_world,
                         const float* const* gray, int mem, const int32_t* src_off, const int32_t* src_idx, const tsar_fusion_params* prm,
                         float* points_out, int64_t cap, int64_t* n_points_out) {
    tsar_ctx* ctx = nullptr;
    const int rc0 = tsar_create(device, &ctx);
    if (rc0 != TSAR_OK) return rc0;
    const int rc = tsar_fuse_ctx(ctx, n_views, w, h, cams, depth, normal_world, gray, mem, src_off, src_idx, prm, points_out, cap, n_points_out);
    tsar_destroy(ctx);
    return rc;
}

extern "C" void tsar_default_fusion_params(tsar_fusion_params* p) {   // x/1.sh:20-25
    if (!p) return;
    p->num_consistent = 1;
    p->reproj_error = 2.0f;
    p->depth_diff = 0.01f;
    p->angle_deg = 15.0f;
    p->used_list = 1;
}
