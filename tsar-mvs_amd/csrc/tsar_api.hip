// tsar_api.hip — the C ABI of include/tsar.h: context, device memory, camera algebra, call order.
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>

#include "tsar_dev.h"

// ---- kernel timing -------------------------------------------------------------------------------
ScopedKernelTimer::ScopedKernelTimer(tsar_ctx* c, const char* name) : ctx(c) {      // name == nullptr: no record
    if (!ctx->timing || !name) return;
    for (size_t k = 0; k < ctx->timers.size(); k++)
        if (ctx->timers[k].name == name) ti = (int)k;
    if (ti < 0) {
        ctx->timers.emplace_back();
        ctx->timers.back().name = name;
        ti = (int)ctx->timers.size() - 1;
    }
    if (hipEventCreate(&e0) != hipSuccess) { ti = -1; return; }
    if (hipEventCreate(&e1) != hipSuccess) { hipEventDestroy(e0); ti = -1; return; }
    hipEventRecord(e0, ctx->stream);
}
ScopedKernelTimer::~ScopedKernelTimer() {
    if (ti < 0) return;
    hipEventRecord(e1, ctx->stream);
    ctx->timers[ti].pending.emplace_back(e0, e1);
}
static void drain_timers(tsar_ctx* ctx) {
    for (auto& k : ctx->timers) {
        for (auto& pr : k.pending) {
            float ms = 0.f;
            if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                k.total_ms += ms;
                k.launches++;
            }
            hipEventDestroy(pr.first);
            hipEventDestroy(pr.second);
        }
        k.pending.clear();
    }
}

// ---- helpers -------------------------------------------------------------------------------------
// (fail, CHECK_CTX, NEED_*, TRY, dev_alloc, DevTmp, the copy kinds, install_regions and CallFrame — what a call that stages buffers
// or needs temporaries is written with — : tsar_dev.h, shared with the operators' own files)
template <typename T>
static void dev_free(T*& p) {
    if (p) hipFree(p);
    p = nullptr;
}
static void inv3(const double* m, double* o) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    const double s = 1.0 / det;
    o[0] = c00 * s; o[1] = (m[2] * m[7] - m[1] * m[8]) * s; o[2] = (m[1] * m[5] - m[2] * m[4]) * s;
    o[3] = c01 * s; o[4] = (m[0] * m[8] - m[2] * m[6]) * s; o[5] = (m[2] * m[3] - m[0] * m[5]) * s;
    o[6] = c02 * s; o[7] = (m[1] * m[6] - m[0] * m[7]) * s; o[8] = (m[0] * m[4] - m[1] * m[3]) * s;
}
static void mul3(const double* a, const double* b, double* o) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) o[3 * r + c] = a[3 * r] * b[c] + a[3 * r + 1] * b[3 + c] + a[3 * r + 2] * b[6 + c];
}
static void scale_k(const float* K, double s, double* o) {  // scaleK cameraGeometryUtils.h:143-154
    for (int i = 0; i < 9; i++) o[i] = K[i];
    o[0] /= s; o[4] /= s; o[2] /= s; o[5] /= s;
}

// Camera re-origin algebra of getCameraParameters (cameraGeometryUtils.h:270-356), without the
// decomposeProjectionMatrix round trip: K, R, t come straight from the cam files.
static void derive_cameras(tsar_ctx* ctx, const tsar_camera* cams) {
    DevScene& sc = ctx->hscene;
    const double s = ctx->params.cam_scale > 0 ? ctx->params.cam_scale : 1.0;
    double K0[9], R0t[9], t0[3];
    scale_k(cams[0].K, s, K0);
    for (int r = 0; r < 3; r++) {
        t0[r] = cams[0].t[r];
        for (int c = 0; c < 3; c++) R0t[3 * r + c] = cams[0].R[3 * c + r];
    }
    for (int v = 0; v < ctx->n_views; v++) {
        double Kv[9], Rv[9], Rrel[9], trel[3];
        scale_k(cams[v].K, s, Kv);
        for (int i = 0; i < 9; i++) Rv[i] = cams[v].R[i];
        mul3(Rv, R0t, Rrel);                                     // [R|t] [R0|t0]^-1
        for (int r = 0; r < 3; r++) trel[r] = cams[v].t[r] - (Rrel[3 * r] * t0[0] + Rrel[3 * r + 1] * t0[1] + Rrel[3 * r + 2] * t0[2]);
        if (v == 0) {                                            // the reference camera is exactly K[I|0]
            for (int i = 0; i < 9; i++) Rrel[i] = (i % 4 == 0) ? 1.0 : 0.0;
            trel[0] = trel[1] = trel[2] = 0.0;
        }
        DevView& dv = sc.view[v];
        for (int i = 0; i < 9; i++) { dv.K[i] = (float)Kv[i]; dv.R[i] = (float)Rrel[i]; }
        for (int r = 0; r < 3; r++) dv.t[r] = (float)trel[r];
        dv.t_abs_lo = std::min(std::min(fabsf(dv.t[0]), fabsf(dv.t[1])), fabsf(dv.t[2]));
        dv.t_abs_hi = std::max(std::max(fabsf(dv.t[0]), fabsf(dv.t[1])), fabsf(dv.t[2]));
        {                                                        // fast-mode split of the plane homography: A = K R K0^-1, b = K t
            double K0inv[9], KR[9], A[9];
            inv3(K0, K0inv);
            mul3(Kv, Rrel, KR);
            mul3(KR, K0inv, A);
            for (int i = 0; i < 9; i++) dv.A[i] = (float)A[i];
            for (int r = 0; r < 3; r++) dv.b[r] = (float)(Kv[3 * r] * trel[0] + Kv[3 * r + 1] * trel[1] + Kv[3 * r + 2] * trel[2]);
        }
        {                                                        // geometric consistency, the way back: [K0 R^T Kv^-1 | -K0 R^T t]
            double Kvinv[9], RT[9], K0RT[9], B[9];
            inv3(Kv, Kvinv);
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) RT[3 * r + c] = Rrel[3 * c + r];
            mul3(K0, RT, K0RT);
            mul3(K0RT, Kvinv, B);
            float* G = sc.geom_back[v];
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) G[4 * r + c] = (float)B[3 * r + c];
                G[4 * r + 3] = (float)(-(K0RT[3 * r] * trel[0] + K0RT[3 * r + 1] * trel[1] + K0RT[3 * r + 2] * trel[2]));
            }
        }
        if (v == 0) {
            DevRef& rf = sc.ref;
            double Kinv[9], M[9], Minv[9];
            inv3(Kv, Kinv);
            mul3(K0, Rrel, M);                                   // P = K_ref [R|t] (cameraGeometryUtils.h:302)
            inv3(M, Minv);
            for (int i = 0; i < 9; i++) {
                rf.K[i] = (float)Kv[i]; rf.Kinv[i] = (float)Kinv[i]; rf.Minv[i] = (float)Minv[i];
                rf.Rorig[i] = cams[0].R[i];
            }
            for (int r = 0; r < 3; r++)
                for (int c = 0; c < 3; c++) rf.RorigInv[3 * r + c] = cams[0].R[3 * c + r];
            for (int r = 0; r < 3; r++) {
                rf.P34[r] = (float)(K0[3 * r] * trel[0] + K0[3 * r + 1] * trel[1] + K0[3 * r + 2] * trel[2]);
                rf.C[r] = (float)(-(Rrel[r] * trel[0] + Rrel[3 + r] * trel[1] + Rrel[6 + r] * trel[2]));
            }
            rf.fx = (float)K0[0];
            rf.f = (float)K0[0];
            rf.alpha = (float)K0[0] / (float)K0[4];
            rf.baseline = 1.0f;                                  // cameraGeometryUtils.h:309
            rf.depthMin = ctx->params.depth_min;
            rf.depthMax = ctx->params.depth_max;
        }
    }
    // zero / one pattern of the intrinsics (cam files without skew, the only kind MVSNet-format scenes carry)
    auto sparse3 = [](const float* K) { return K[1] == 0.f && K[3] == 0.f && K[6] == 0.f && K[7] == 0.f && K[8] == 1.f; };
    sc.k_sparse = sparse3(sc.ref.Kinv) ? 1 : 0;
    for (int v = 0; v < ctx->n_views; v++) sc.k_sparse &= sparse3(sc.view[v].K) ? 1 : 0;
    // main.cpp:1393-1398
    sc.min_disp = sc.ref.f * sc.ref.baseline / ctx->params.depth_max;
    sc.max_disp = sc.ref.f * sc.ref.baseline / ctx->params.depth_min;
    int steps = 0;
    for (float dz = sc.max_disp / 2.0f; dz >= 0.01f; dz = dz / 10.0f) steps++;   // gipuma.cu:643-644
    sc.refine_steps = steps;
}

// gipuma_init_cu2 takes its window radius as box / 2 (gipuma.cu:693-694) where every other kernel takes (box - 1) / 2
// (:858-859, :1065-1066, :1175-1176): an even --blocksize initialises on a window one tap ring larger than the one it sweeps with.
// Reproduced by default; TSAR_FLAG_FIX_INIT_RADIUS initialises on the sweeps' window.
static bool init_window_differs(const tsar_ctx* ctx) {
    const tsar_params& p = ctx->params;
    return !(p.flags & TSAR_FLAG_FIX_INIT_RADIUS) && (p.box_hsize / 2 != (p.box_hsize - 1) / 2 || p.box_vsize / 2 != (p.box_vsize - 1) / 2);
}
static void fill_scene_params(tsar_ctx* ctx, bool for_init = false) {
    DevScene& sc = ctx->hscene;
    const tsar_params& p = ctx->params;
    const bool init_radius = for_init && !(p.flags & TSAR_FLAG_FIX_INIT_RADIUS);
    sc.hrad = init_radius ? p.box_hsize / 2 : (p.box_hsize - 1) / 2;   // gipuma.cu:693-694 : gipuma.cu:858-859
    sc.vrad = init_radius ? p.box_vsize / 2 : (p.box_vsize - 1) / 2;
    sc.n_best = p.n_best;
    sc.cost_comb = p.cost_comb;
    sc.flags = p.flags;
    sc.seed_lo = (uint32_t)p.seed;
    sc.seed_hi = (uint32_t)(p.seed >> 32);
    // weight table of the general-window tap loop (tsar_dev.h DevScene::tap_row): distance classes of the window's taps, and
    // per (line, tap of the line) the row of its class.  Fast mode walks window rows, strict mode the oracle's columns.
    sc.lut_row_major = (p.flags & TSAR_FLAG_STRICT_DIV) ? 0 : 1;
    std::vector<int> d2;
    for (int i = -sc.hrad; i <= sc.hrad; i += 2)
        for (int j = -sc.vrad; j <= sc.vrad; j += 2) d2.push_back(i * i + j * j);
    std::sort(d2.begin(), d2.end());
    d2.erase(std::unique(d2.begin(), d2.end()), d2.end());
    sc.lut_classes = (int)d2.size() <= TSAR_LUT_MAX_CLASSES ? (int)d2.size() : 0;
    for (int k = 0; k < sc.lut_classes; k++) sc.lut_d2[k] = d2[k];
    const int rl = sc.lut_row_major ? sc.vrad : sc.hrad, rt = sc.lut_row_major ? sc.hrad : sc.vrad;   // radius across / along the lines
    sc.lut_chunk = lut_chunk_taps(rt + 1);
    sc.lut_pad_taps = (rt + sc.lut_chunk) / sc.lut_chunk * sc.lut_chunk;
    for (uint32_t& r : sc.tap_row) r = (uint32_t)sc.lut_classes * 1024u;      // the zero row: slots beyond the end of a line
    for (int l = 0; l <= rl && sc.lut_classes; l++)
        for (int t = 0; t <= rt; t++) {
            const int a = 2 * l - rl, b = 2 * t - rt;
            sc.tap_row[l * sc.lut_pad_taps + t] = 1024u * (uint32_t)(std::lower_bound(d2.begin(), d2.end(), a * a + b * b) - d2.begin());
        }
}
static int upload_scene(tsar_ctx* ctx) {
    if (!ctx->dscene) TRY(dev_alloc(ctx, &ctx->dscene, 1));
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(ctx->dscene, &ctx->hscene, sizeof(DevScene), hipMemcpyHostToDevice, ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // hscene may be edited again by the caller's next call
    return TSAR_OK;
}

// ---- lifecycle -----------------------------------------------------------------------------------
extern "C" const char* tsar_version(void) {
#ifdef TSAR_EXPERIMENTS
    return "tsar-mvs_amd 0.2.0 (gfx950) +experiments";
#else
    return "tsar-mvs_amd 0.2.0 (gfx950)";
#endif
}

// Every environment knob of the library, read once per context.  All are diagnostics / A-B switches: the defaults
// are the measured best and nothing in the product path depends on one being set.
static void read_knobs(tsar_ctx* ctx) {
    auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e && e[0] ? atoi(e) : dflt; };
    auto on = [](const char* name, bool dflt) { const char* e = getenv(name); return e && e[0] ? e[0] != '0' : dflt; };
    ctx->variant = num("TSAR_VARIANT", ctx->variant);
    ctx->buffer_gather = on("TSAR_BUFFER_GATHER", true);
    ctx->mix_gather = on("TSAR_MIX_GATHER", true);
    ctx->strip_w = num("TSAR_STRIP", -1);
    ctx->buffer_from = num("TSAR_BUFFER_FROM", 1);
    ctx->force_block = num("TSAR_BLOCK", 0);
    ctx->memo_mode = num("TSAR_MEMO", 1);
    ctx->compact_from = num("TSAR_COMPACT_FROM", 6);
    ctx->prune = num("TSAR_PRUNE", 1);
    ctx->prune_steps = std::min(std::max(num("TSAR_PRUNE_STEPS", 2), 0), 8);      // (the census keeps eight steps' counters)
    ctx->prune_from = num("TSAR_PRUNE_FROM", 1);
    ctx->pair = num("TSAR_PAIR", 3);
    ctx->ring = num("TSAR_RING", ctx->ring);
    ctx->lut_mode = num("TSAR_LUT", 1);
    ctx->ransac_wgs = num("TSAR_RANSAC_WGS", 8);
    ctx->ransac_chain = num("TSAR_RANSAC_CHAIN", 8);
    ctx->ransac_lookahead = num("TSAR_RANSAC_LOOKAHEAD", 0);
    ctx->ransac_poll_limit = num("TSAR_RANSAC_POLL_LIMIT", 1 << 15);
    ctx->ransac_cooperative = on("TSAR_RANSAC_COOPERATIVE", true);
    ctx->ransac_force_fallback = on("TSAR_RANSAC_FORCE_FALLBACK", false);
    ctx->render_skip = on("TSAR_RENDER_SKIP", true);
    ctx->trace_host = getenv("TSAR_TRACE_HOST") != nullptr;
#ifdef TSAR_EXPERIMENTS
    ctx->lds_pad = (size_t)num("TSAR_LDS_PAD", 0);
#endif
}

extern "C" int tsar_create(int device, tsar_ctx** out) {
    if (!out) return TSAR_ERR_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TSAR_ERR_HIP;
    if (device < 0 || device >= n) return TSAR_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return TSAR_ERR_HIP;
    tsar_ctx* ctx = new (std::nothrow) tsar_ctx();
    if (!ctx) return TSAR_ERR_NOMEM;
    ctx->device = device;
    if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) { delete ctx; return TSAR_ERR_HIP; }
    tsar_default_params(&ctx->params);
    ctx->variant = probe_d16_hi_zeroes(ctx) ? 250 : 114;
    read_knobs(ctx);
    *out = ctx;
    return TSAR_OK;
}

static void free_views(tsar_ctx* ctx) {
    for (auto& p : ctx->img) dev_free(p);
    for (auto& p : ctx->quad) dev_free(p);
    for (auto& p : ctx->dquad) dev_free(p);
    ctx->img.clear();
    ctx->quad.clear();
    ctx->dquad.clear();
}
static void free_geom(tsar_ctx* ctx) {
    for (auto& p : ctx->geom_maps) dev_free(p);
    ctx->geom_maps.clear();
    for (auto& p : ctx->hscene.geom_depth) p = nullptr;
    ctx->hscene.geom_on = 0;
}
static void free_prior(tsar_ctx* ctx) {
    dev_free(ctx->prior);
    ctx->hscene.prior = nullptr;
}
static void free_planes(tsar_ctx* ctx) {
    for (int b = 0; b < 2; b++) { dev_free(ctx->buf[b].c); dev_free(ctx->buf[b].n4); }
    dev_free(ctx->ratio); dev_free(ctx->depth); dev_free(ctx->scale); dev_free(ctx->lrdiff); dev_free(ctx->confid);
    dev_free(ctx->fakedepth); dev_free(ctx->beview); dev_free(ctx->canny); dev_free(ctx->out4);
    dev_free(ctx->memo_cand); dev_free(ctx->memo_seq); dev_free(ctx->changed_seq);
    if (ctx->prune_counts) { (void)hipFree(ctx->prune_counts); ctx->prune_counts = nullptr; }
    dev_free(ctx->resize4);
    ctx->have_resize = false;
}

extern "C" int tsar_destroy(tsar_ctx* ctx) {
    if (!ctx) return TSAR_OK;
    (void)enter_ctx(ctx);                  // (a device that cannot be selected still gets its host side released)
    if (ctx->stream) hipStreamSynchronize(ctx->stream);
    drain_timers(ctx);
    free_views(ctx);
    free_planes(ctx);
    free_geom(ctx);
    free_prior(ctx);
    dev_free(ctx->dscene); dev_free(ctx->region_text); dev_free(ctx->region_size); dev_free(ctx->region_n4);
    if (ctx->scratch.base) hipFree(ctx->scratch.base);
    if (ctx->stream) hipStreamDestroy(ctx->stream);
    delete ctx;
    return TSAR_OK;
}
extern "C" const char* tsar_last_error(const tsar_ctx* ctx) { return ctx ? ctx->err.c_str() : "null context"; }
extern "C" int tsar_get_stream(tsar_ctx* ctx, void** stream_out) {
    if (!ctx || !stream_out) return TSAR_ERR_INVALID;
    *stream_out = (void*)ctx->stream;
    return TSAR_OK;
}
extern "C" int tsar_synchronize(tsar_ctx* ctx) {
    CHECK_CTX(ctx);
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}

// ---- inputs --------------------------------------------------------------------------------------
extern "C" void tsar_default_params(tsar_params* p) {   // algorithmparameters.h:21-52
    if (!p) return;
    memset(p, 0, sizeof(*p));
    p->box_hsize = 19;
    p->box_vsize = 19;
    p->n_best = 2;
    p->cost_comb = TSAR_COMB_BEST_N;
    p->depth_min = 2.0f;     // camera.h:37-44
    p->depth_max = 20.0f;
    p->cam_scale = 1.0f;
    p->flags = 0;
    p->seed = 0;
}

extern "C" int tsar_set_params(tsar_ctx* ctx, const tsar_params* p) {
    CHECK_CTX(ctx);
    if (!p) return fail(ctx, TSAR_ERR_INVALID, "params is NULL");
    if (p->box_hsize < 1 || p->box_vsize < 1 || p->box_hsize > 63 || p->box_vsize > 63) return fail(ctx, TSAR_ERR_INVALID, "box size must be in 1..63");
    if (p->n_best < 1 || p->n_best > TSAR_MAX_SELECTED) return fail(ctx, TSAR_ERR_INVALID, "n_best must be in 1..32 (the reference's costVector holds 32 views, gipuma.cu:467)");
    if (p->cost_comb < TSAR_COMB_ALL || p->cost_comb > TSAR_COMB_GOOD) return fail(ctx, TSAR_ERR_INVALID, "cost_comb must be one of TSAR_COMB_ALL / BEST_N / ANGLE / GOOD");
    if (!(p->depth_min > 0.f) || !(p->depth_max > p->depth_min)) return fail(ctx, TSAR_ERR_INVALID, "need 0 < depth_min < depth_max");
    if (!(p->cam_scale > 0.f)) return fail(ctx, TSAR_ERR_INVALID, "cam_scale must be > 0");
    ctx->params = *p;
    ctx->have_params = true;
    fill_scene_params(ctx);
    if (ctx->have_views) ctx->views_reset();   // depth range / scale feed the derived camera block: the views must be set again
    return TSAR_OK;
}

// Strict mode's quotients are bit-exact because persp_divide_exact / div_pair_rcp_exact (tsar_device_math.h) return the correctly
// rounded quotient — a property of THIS GPU's v_rcp_f32, enumerated over all 2^46 mantissa pairs on the device it was measured on
// (profiles/r03/div_exact_all_mantissa_pairs.json).  Like the D16 probe, it is re-checked where it is relied on: once per context,
// before the first strict-mode views are accepted, 2^22 random operand triples in each of the tap loop's two operand
// distributions through the SHIPPED unguarded code path against the compiler's IEEE division (~1 ms).  A device whose reciprocal
// differs fails loudly here instead of drifting from the oracle silently.
static int probe_exact_divide(tsar_ctx* ctx) {
    if (ctx->exact_div_probe != 0) return ctx->exact_div_probe;
    uint64_t bad = 0, total = 0;
    for (int mode = 0; mode < 2; mode++) {
        if (tsar_selftest_divide_random(ctx, 22, 0x5EEDD1F1DE5ull + (uint64_t)mode, mode, /*guarded=*/0, &bad, nullptr) != TSAR_OK) return 0;   // not probed: the caller reports ctx->err
        total += bad;
    }
    ctx->exact_div_probe = total == 0 ? 1 : -1;
    return ctx->exact_div_probe;
}
// The same for the square root of the cost's tail (sqrt_rsq_exact, tsar_device_math.h), which BOTH arithmetic modes run on 8-bit
// imagery: all 2^24 mantissa / exponent-parity cases against sqrtf on the device, once per context (~0.2 ms).
// Second pass (round 5): the enumeration covers two binades; that the result carries to other exponents rests on v_rsq_f32 scaling
// exactly with the exponent, so 2^24 random mantissas spread over the 67 binades the tail's operands can reach (var_ref * var_src in
// [1e-10, 4.3e9]) are checked per context as well.  Run only for contexts whose views are 8-bit imagery: the float-imagery loop and
// the refinement operators keep sqrtf.
static int probe_exact_sqrt(tsar_ctx* ctx) {
    if (ctx->exact_sqrt_probe != 0) return ctx->exact_sqrt_probe;
    uint64_t bad = 0, bad_range = 0;
    if (tsar_selftest_sqrt(ctx, 0, 0, &bad) != TSAR_OK) return 0;
    if (tsar_selftest_sqrt(ctx, 3, 0x5EED5A17ull, &bad_range) != TSAR_OK) return 0;
    ctx->exact_sqrt_probe = (bad | bad_range) == 0 ? 1 : -1;
    return ctx->exact_sqrt_probe;
}

// ---- tsar_set_views (elem = 4: float32 images) and tsar_set_views_u8 (elem = 1: the 8-bit decode itself, widened on the device), in
// four steps: the arguments, the images and textures, the window, the state planes ----
static int check_views_args(tsar_ctx* ctx, int n_views, int w, int h, const void* const* gray, const tsar_camera* cams) {
    if (!ctx->have_params) return fail(ctx, TSAR_ERR_STATE, "tsar_set_params must be called before tsar_set_views");
    if (ctx->params.flags & TSAR_FLAG_STRICT_DIV) {
        const int pr = probe_exact_divide(ctx);
        if (pr == 0) return TSAR_ERR_HIP;
        if (pr < 0) return fail(ctx, TSAR_ERR_HIP, "TSAR_FLAG_STRICT_DIV: this device's v_rcp_f32 does not give correctly rounded quotients through the short division "
                                                   "sequence (tsar_selftest_divide_random found mismatches against IEEE division); strict mode is refused rather than run inexactly");
    }
    if (n_views < 1 || n_views > TSAR_MAX_VIEWS) return fail(ctx, TSAR_ERR_INVALID, "n_views must be in 1..TSAR_MAX_VIEWS");
    if (w < 8 || h < 8 || (int64_t)w * h > (int64_t)1 << 28) return fail(ctx, TSAR_ERR_INVALID, "image size out of range");
    if (w + 2 >= (1 << 23) || h + 2 >= (1 << 23)) return fail(ctx, TSAR_ERR_INVALID, "image side too long for the 24-bit quad addressing (w + 2, h + 2 < 2^23)");
    if (!gray || !cams) return fail(ctx, TSAR_ERR_INVALID, "gray/cams is NULL");
    for (int v = 0; v < n_views; v++)
        if (!gray[v]) return fail(ctx, TSAR_ERR_INVALID, "gray[v] is NULL");
    return TSAR_OK;
}

// images, quad textures (and whether the imagery is 8-bit: use_quad), difference textures, derived cameras
static int upload_views(tsar_ctx* ctx, int n_views, int w, int h, const void* const* gray, int elem, int mem, const tsar_camera* cams) {
    free_geom(ctx);                        // depth maps of the previous views' sources: not this scene's
    free_prior(ctx);                       // nor is the prior
    // The image and quad-texture buffers of the previous views are kept when the size is the same (a worker matching view after
    // view of a scene): 2 x n_views hipMalloc + hipFree of ~100 MB each cost 55 ms per call at ETH3D size, more than the copies.
    // Buffers beyond n_views stay in the pool; a change of size releases everything.
    const size_t np = (size_t)w * h;
    if (w != ctx->w || h != ctx->h) { free_views(ctx); free_planes(ctx); }
    ctx->w = w; ctx->h = h; ctx->n_views = n_views;
    DevScene& sc = ctx->hscene;
    sc.w = w; sc.h = h; sc.quad_pitch = w + 2;
    if ((int)ctx->img.size() < n_views) ctx->img.resize(n_views, nullptr);
    if ((int)ctx->quad.size() < n_views) ctx->quad.resize(n_views, nullptr);
    if ((int)ctx->dquad.size() < n_views) ctx->dquad.resize(n_views, nullptr);
    DevTmp<int> dflag;
    TRY(dflag.alloc(ctx, 1));
    TSAR_HIP_TRY(ctx, hipMemsetAsync(dflag.p, 0, sizeof(int), ctx->stream));
    for (int v = 0; v < n_views; v++) {
        if (!ctx->img[v]) TRY(dev_alloc(ctx, &ctx->img[v], np));
        if (!ctx->quad[v]) TRY(dev_alloc(ctx, &ctx->quad[v], (size_t)(w + 2) * (h + 2)));
        if (elem == 4) {
            TSAR_HIP_TRY(ctx, hipMemcpyAsync(ctx->img[v], gray[v], np * sizeof(float), kind_to_dev(mem), ctx->stream));
        } else if (mem == TSAR_MEM_DEVICE) {
            TRY(launch_expand_u8(ctx, (const uint8_t*)gray[v], ctx->img[v], np));
        } else {
            // host bytes: staged in the view's own quad-texture buffer ((w + 2)(h + 2) dwords, written only by build_quad below, which
            // reads img[v]) — no extra allocation, and the copies of the views follow each other on the stream without a sync
            uint8_t* stage = (uint8_t*)ctx->quad[v];
            TSAR_HIP_TRY(ctx, hipMemcpyAsync(stage, gray[v], np, hipMemcpyHostToDevice, ctx->stream));
            TRY(launch_expand_u8(ctx, stage, ctx->img[v], np));
        }
        TRY(launch_build_quad(ctx, ctx->img[v], ctx->quad[v], w, h, dflag.p));
    }
    int hflag = 0;
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(&hflag, dflag.p, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    sc.use_quad = hflag ? 0 : 1;
    if (sc.use_quad) {   // the 8-bit tap loops are the only users of sqrt_rsq_exact: probed for the contexts that will run them
        const int ps = probe_exact_sqrt(ctx);
        if (ps == 0) return TSAR_ERR_HIP;
        if (ps < 0) return fail(ctx, TSAR_ERR_HIP, "this device's v_rsq_f32 does not give correctly rounded square roots through the one-correction sequence of the cost's tail "
                                                   "(tsar_selftest_sqrt found mismatches against sqrtf): refused rather than run with costs that differ from the oracle's");
    }
    for (int v = 0; v < n_views; v++) { sc.view[v].img = ctx->img[v]; sc.view[v].quad = ctx->quad[v]; sc.view[v].dquad = nullptr; }
    if (!sc.use_quad)
        for (auto& q : ctx->quad) dev_free(q);              // (float imagery: the textures are not used; re-allocated if a later call needs them)
    // Fast mode's converged sweeps (buffer gathers, from the third sweep of a run on; the box-11 loop and the general-window loop) read
    // the source views from a second texture with half-float differences (pm_tap_r5.h MIX): 8 bytes per texel quad, source views only.
    const bool want_dquad = sc.use_quad && !(ctx->params.flags & TSAR_FLAG_STRICT_DIV) && ctx->buffer_gather && ctx->mix_gather && ctx->variant == 250;
    for (int v = 1; v < n_views; v++) {
        if (!want_dquad) { dev_free(ctx->dquad[v]); continue; }
        if (!ctx->dquad[v]) TRY(dev_alloc(ctx, &ctx->dquad[v], (size_t)(w + 2) * (h + 2)));
        TRY(launch_build_dquad(ctx, ctx->quad[v], ctx->dquad[v], w, h));
        sc.view[v].dquad = ctx->dquad[v];
    }
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    derive_cameras(ctx, cams);
    ctx->cams.assign(cams, cams + n_views);
    ctx->views_u8 = elem == 1;
    return TSAR_OK;
}

// Can the matching kernels run this window?  Null, or the reason why not.  8-bit imagery shares one weight table per workgroup
// (pm_core_lut.h): any box whose taps have <= TSAR_LUT_MAX_CLASSES distinct distances (every square box; rectangular ones unless
// their radii have mixed parity, e.g. 63 x 61 -> 202).  Everything else keeps the hoisted bilateral weights per thread in LDS,
// (hrad+1)(vrad+1) taps x 256 threads x 4 B beside the reference window, which bounds the box at 23.  Checked for the sweeps' window
// and, for even boxes, gipuma_init_cu2's own (init_window_differs); a context with the reference view alone never matches
// (refinement operators only) and takes any box.  Leaves the scene block describing the sweeps' window.
static const char* window_problem(tsar_ctx* ctx) {
    DevScene& sc = ctx->hscene;
    auto problem_of = [&](bool for_init) -> const char* {
        fill_scene_params(ctx, for_init);
        if (lut_path_applies(ctx)) return nullptr;
        const size_t lds = (size_t)(sc.hrad + 1) * (sc.vrad + 1) * 1024 + (size_t)(32 + 2 * sc.hrad) * (16 + 2 * sc.vrad) * 4 + 16;
        if (lds <= 160 * 1024) return nullptr;
        if (!sc.use_quad) return "box too large for images that are not 8-bit: the per-thread weight table does not fit the 160 KiB of LDS per CU (largest square box: 23)";
        if (sc.lut_classes == 0) return "this rectangular box has more than 144 distinct tap distances (radii of mixed parity): the shared weight table cannot hold them and the per-thread table does not fit LDS; use radii of equal parity, or a box of at most 23";
        return "box too large for fast mode on this device: the D16 LDS-load probe failed, so the general-window loop is not available; use TSAR_FLAG_STRICT_DIV, or a box of at most 23";
    };
    const char* problem = ctx->n_views > 1 ? problem_of(false) : nullptr;
    if (!problem && ctx->n_views > 1 && init_window_differs(ctx)) problem = problem_of(true);
    fill_scene_params(ctx);
    return problem;
}

// state planes (LineState::resize linestate.h:71-110): kept from the previous views of the same size, cleared
static int alloc_state_planes(tsar_ctx* ctx) {
    const size_t np = (size_t)ctx->w * ctx->h;
    for (int b = 0; b < 2; b++) {
        if (!ctx->buf[b].c) TRY(dev_alloc(ctx, &ctx->buf[b].c, np));
        if (!ctx->buf[b].n4) TRY(dev_alloc(ctx, &ctx->buf[b].n4, np));
    }
    float** fplanes[] = {&ctx->ratio, &ctx->depth, &ctx->scale, &ctx->lrdiff, &ctx->confid, &ctx->fakedepth};
    for (float** fp : fplanes) {
        if (!*fp) TRY(dev_alloc(ctx, fp, np));
        TSAR_HIP_TRY(ctx, hipMemsetAsync(*fp, 0, np * sizeof(float), ctx->stream));
    }
    if (!ctx->beview) TRY(dev_alloc(ctx, &ctx->beview, np));
    if (!ctx->canny) TRY(dev_alloc(ctx, &ctx->canny, np));
    if (!ctx->out4) TRY(dev_alloc(ctx, &ctx->out4, np));
    TSAR_HIP_TRY(ctx, hipMemsetAsync(ctx->beview, 0, np * sizeof(int32_t), ctx->stream));
    TSAR_HIP_TRY(ctx, hipMemsetAsync(ctx->canny, 0, np * sizeof(int32_t), ctx->stream));
    return TSAR_OK;
}

static int set_views_impl(tsar_ctx* ctx, int n_views, int w, int h, const void* const* gray, int elem, int mem, const tsar_camera* cams) {
    CHECK_CTX(ctx);
    TRY(check_views_args(ctx, n_views, w, h, gray, cams));
    ctx->views_reset();
    TRY(upload_views(ctx, n_views, w, h, gray, elem, mem, cams));
    if (const char* problem = window_problem(ctx)) return fail(ctx, TSAR_ERR_INVALID, problem);
    DevScene& sc = ctx->hscene;
    sc.n_sel = std::min(n_views - 1, TSAR_MAX_SELECTED);   // default subset: the first 32 source views at most (tsar_set_view_subset picks others)
    for (int i = 0; i < sc.n_sel; i++) sc.sel[i] = i + 1;
    TRY(alloc_state_planes(ctx));
    TRY(upload_scene(ctx));
    ctx->have_views = true;
    return TSAR_OK;
}

extern "C" int tsar_set_views(tsar_ctx* ctx, int n_views, int w, int h, const float* const* gray, int mem, const tsar_camera* cams) {
    return set_views_impl(ctx, n_views, w, h, (const void* const*)gray, 4, mem, cams);
}
extern "C" int tsar_set_views_u8(tsar_ctx* ctx, int n_views, int w, int h, const uint8_t* const* gray, int mem, const tsar_camera* cams) {
    return set_views_impl(ctx, n_views, w, h, (const void* const*)gray, 1, mem, cams);
}

extern "C" int tsar_set_view_subset(tsar_ctx* ctx, int n, const int32_t* view_idx) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (n < 1 || n > TSAR_MAX_SELECTED || !view_idx) return fail(ctx, TSAR_ERR_INVALID, "subset size must be in 1..32 (the reference's viewSelectionSubset / costVector hold 32, gipuma.cu:467)");
    for (int i = 0; i < n; i++)
        if (view_idx[i] < 1 || view_idx[i] >= ctx->n_views) return fail(ctx, TSAR_ERR_INVALID, "view index must be in 1..n_views-1");
    ctx->hscene.n_sel = n;
    for (int i = 0; i < n; i++) ctx->hscene.sel[i] = view_idx[i];
    ctx->costs_voided();                   // scored under the previous subset
    return upload_scene(ctx);
}

// ---- PatchMatch ----------------------------------------------------------------------------------
extern "C" int tsar_pm_init(tsar_ctx* ctx) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    NEED_SOURCES(ctx);
    const bool own_window = init_window_differs(ctx);
    int rc = TSAR_OK;
    if (own_window) {                      // an even box: the scene block describes the init window for this one launch
        fill_scene_params(ctx, true);
        rc = upload_scene(ctx);
    }
    if (rc == TSAR_OK) rc = launch_pm_init(ctx);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == TSAR_OK) rc = fail(ctx, TSAR_ERR_HIP, "hipStreamSynchronize failed");
    if (own_window) {
        // back to the sweep window on EVERY path (also when the first upload failed: the host block was already rewritten); if the
        // device block cannot be restored, host and device disagree about the window and the views must be set again
        fill_scene_params(ctx, false);
        const int rc2 = upload_scene(ctx);
        if (rc2 != TSAR_OK) ctx->have_views = false;
        if (rc == TSAR_OK) rc = rc2;
    }
    TRY(rc);
    // c[p] is the score of n4[p] on the SWEEP window only if init ran on that window: otherwise a neighbour's identical plane may
    // well score lower than the stored cost, and the sweeps must not skip it
    ctx->state_scored(!own_window);
    return TSAR_OK;
}

static int pm_sweeps(tsar_ctx* ctx, int n_sweeps, int first_colour, int do_prop, int do_refine) {
    // cur[k]: which ping-pong buffer holds the current values of colour k.  Both start in buf[0].
    int cur[2] = {0, 0};
    // the propagation memo lives within this call: whatever happened to the state before (init, another subset, loaded planes) is
    // out of its reach
    ctx->memo_valid_from = ctx->launch_seq + 1;
    ctx->call_launch = 0;
    if (ctx->memo_mode && n_sweeps > 2 && !ctx->memo_cand) {
        // all three buffers or none: a failure part of the way leaves memo_cand null, and the next call tries again
        const size_t np = (size_t)ctx->w * ctx->h;
        DevTmp<int32_t> cand;
        DevTmp<uint32_t> seq, changed;
        TRY(cand.alloc(ctx, np * 8));
        TRY(seq.alloc(ctx, np));
        TRY(changed.alloc(ctx, np));
        TSAR_HIP_TRY(ctx, hipMemsetAsync(seq.p, 0, np * sizeof(uint32_t), ctx->stream));
        TSAR_HIP_TRY(ctx, hipMemsetAsync(changed.p, 0, np * sizeof(uint32_t), ctx->stream));
        ctx->memo_cand = cand.release();
        ctx->memo_seq = seq.release();
        ctx->changed_seq = changed.release();
    }
    for (int s = 0; s < n_sweeps; s++) {
        ctx->launch_seq++;
        const int colour = (first_colour + s) & 1;
        const PlaneBuf& same_in = ctx->buf[cur[colour]];
        const PlaneBuf& other = ctx->buf[cur[colour ^ 1]];
        const PlaneBuf& same_out = ctx->buf[cur[colour] ^ 1];
        TRY(launch_pm_sweep(ctx, colour, same_in, other, same_out, 1u + (uint32_t)ctx->sweeps_done, do_prop, do_refine));
        cur[colour] ^= 1;
        ctx->sweeps_done++;
        ctx->call_launch++;
    }
    // make buf[0] canonical again
    if (cur[0] == 1 && cur[1] == 1) {
        std::swap(ctx->buf[0], ctx->buf[1]);
    } else if (cur[0] != cur[1]) {
        // odd number of sweeps: one colour lives in buf[1]; merge it back (diagnostic path only)
        const size_t np = (size_t)ctx->w * ctx->h;
        const int moved = cur[0] == 1 ? 0 : 1;
        std::vector<float> c0(np), c1(np);
        std::vector<float4> n0(np), n1(np);
        TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        TSAR_HIP_TRY(ctx, hipMemcpy(c0.data(), ctx->buf[0].c, np * 4, hipMemcpyDeviceToHost));
        TSAR_HIP_TRY(ctx, hipMemcpy(c1.data(), ctx->buf[1].c, np * 4, hipMemcpyDeviceToHost));
        TSAR_HIP_TRY(ctx, hipMemcpy(n0.data(), ctx->buf[0].n4, np * 16, hipMemcpyDeviceToHost));
        TSAR_HIP_TRY(ctx, hipMemcpy(n1.data(), ctx->buf[1].n4, np * 16, hipMemcpyDeviceToHost));
        for (int y = 0; y < ctx->h; y++)
            for (int x = 0; x < ctx->w; x++)
                if (((x + y) & 1) == moved) { c0[(size_t)y * ctx->w + x] = c1[(size_t)y * ctx->w + x]; n0[(size_t)y * ctx->w + x] = n1[(size_t)y * ctx->w + x]; }
        TSAR_HIP_TRY(ctx, hipMemcpy(ctx->buf[0].c, c0.data(), np * 4, hipMemcpyHostToDevice));
        TSAR_HIP_TRY(ctx, hipMemcpy(ctx->buf[0].n4, n0.data(), np * 16, hipMemcpyHostToDevice));
    }
    return TSAR_OK;
}

extern "C" int tsar_pm_iterate(tsar_ctx* ctx, int iters) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    NEED_SOURCES(ctx);
    NEED_STATE(ctx);
    if (iters < 0) return fail(ctx, TSAR_ERR_INVALID, "iters must be >= 0");
    TRY(pm_sweeps(ctx, 2 * iters, 0, 1, 1));   // black then red, gipuma.cu:1744-1754
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->result_voided();
    return TSAR_OK;
}

// The iteration loop with the kernels' `final` argument true (gipuma.cu:1096-1138 take `bool final`; nothing in the
// snapshot passes true): pixels with text == -1 are not touched, ratio / beview are not written.
extern "C" int tsar_pm_iterate_final(tsar_ctx* ctx, int iters, const float* text, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    NEED_SOURCES(ctx);
    NEED_STATE(ctx);
    if (iters < 0) return fail(ctx, TSAR_ERR_INVALID, "iters must be >= 0");
    if (!text) return fail(ctx, TSAR_ERR_INVALID, "text is NULL");
    CallFrame f(ctx, __func__, nullptr, /*grow_arena=*/false);
    ctx->final_text = f.in(text, (size_t)ctx->w * ctx->h, mem);
    if (!f.ok()) { ctx->final_text = nullptr; return f.finish(); }   // nothing was swept
    f.take(pm_sweeps(ctx, 2 * iters, 0, 1, 1));
    ctx->final_text = nullptr;
    const int rc = f.finish();
    ctx->result_voided();
    return rc;
}

// Diagnostics entry (not in the reference): one half-iteration with propagation and/or refinement.
extern "C" int tsar_pm_sweep(tsar_ctx* ctx, int colour, int do_prop, int do_refine) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    NEED_SOURCES(ctx);
    NEED_STATE(ctx);
    TRY(pm_sweeps(ctx, 1, colour & 1, do_prop, do_refine));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->result_voided();
    return TSAR_OK;
}
extern "C" int tsar_set_sweep_counter(tsar_ctx* ctx, int n) {
    if (!ctx) return TSAR_ERR_INVALID;
    ctx->sweeps_done = n;
    return TSAR_OK;
}

extern "C" int tsar_pm_cost_planes(tsar_ctx* ctx, const float* planes, int mem, float* cost_out, int32_t* beview_out, float* ratio_out) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    NEED_SOURCES(ctx);
    if (!planes || !cost_out) return fail(ctx, TSAR_ERR_INVALID, "planes/cost_out is NULL");
    const size_t np = (size_t)ctx->w * ctx->h;
    CallFrame f(ctx, __func__, nullptr, /*grow_arena=*/false);   // a diagnostic does not grow what the context keeps
    const float4* dpl = (const float4*)f.in(planes, 4 * np, mem);
    float* dc = f.out(cost_out, np, mem);
    int32_t* dbv = f.out(beview_out, np, mem);
    float* drt = f.out(ratio_out, np, mem);
    if (f.ok()) f.take(launch_pm_cost_planes(ctx, dpl, dc, dbv, drt));
    return f.finish();
}

extern "C" int tsar_set_plane(tsar_ctx* ctx, const float* planes, const float* cost, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (!planes || !cost) return fail(ctx, TSAR_ERR_INVALID, "planes/cost is NULL");
    const size_t np = (size_t)ctx->w * ctx->h;
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[0].n4, planes, np * 16, kind_to_dev(mem), ctx->stream));
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(ctx->buf[0].c, cost, np * 4, kind_to_dev(mem), ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->state_given();
    return TSAR_OK;
}
extern "C" int tsar_get_plane(tsar_ctx* ctx, float* planes, float* cost, int32_t* beview, float* ratio, int mem) {
    CHECK_CTX(ctx);
    NEED_STATE(ctx);
    const size_t np = (size_t)ctx->w * ctx->h;
    if (planes) TSAR_HIP_TRY(ctx, hipMemcpyAsync(planes, ctx->buf[0].n4, np * 16, kind_from_dev(mem), ctx->stream));
    if (cost) TSAR_HIP_TRY(ctx, hipMemcpyAsync(cost, ctx->buf[0].c, np * 4, kind_from_dev(mem), ctx->stream));
    if (beview) TSAR_HIP_TRY(ctx, hipMemcpyAsync(beview, ctx->beview, np * 4, kind_from_dev(mem), ctx->stream));
    if (ratio) TSAR_HIP_TRY(ctx, hipMemcpyAsync(ratio, ctx->ratio, np * 4, kind_from_dev(mem), ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}

// ---- plane <-> depth -----------------------------------------------------------------------------

extern "C" int tsar_load_planes(tsar_ctx* ctx, const float* depth, const float* normal_world, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (!depth || !normal_world) return fail(ctx, TSAR_ERR_INVALID, "depth/normal_world is NULL");
    const size_t np = (size_t)ctx->w * ctx->h;
    CallFrame f(ctx, __func__);
    const float *d = f.in(depth, np, mem), *n = f.in(normal_world, 3 * np, mem);
    if (f.ok()) f.take(launch_get_disp(ctx, d, n));
    TRY(f.finish());
    ctx->state_given();
    return TSAR_OK;
}
extern "C" int tsar_compute_disp(tsar_ctx* ctx) {
    CHECK_CTX(ctx);
    NEED_STATE(ctx);
    TRY(launch_compute_disp(ctx));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->result_computed();
    return TSAR_OK;
}
extern "C" int tsar_compute_disp_final(tsar_ctx* ctx, const float* resize_planes, const float* text, int mem) {
    CHECK_CTX(ctx);
    NEED_STATE(ctx);
    if (!resize_planes || !text) return fail(ctx, TSAR_ERR_INVALID, "resize_planes/text is NULL");
    const size_t np = (size_t)ctx->w * ctx->h;
    CallFrame f(ctx, __func__, nullptr, /*grow_arena=*/false);
    const float *r = f.in(resize_planes, 4 * np, mem), *t = f.in(text, np, mem);
    if (!f.ok()) return f.finish();        // nothing was launched: the state stands
    ctx->costs_voided();
    f.take(launch_compute_disp_final(ctx, (const float4*)r, t));
    TRY(f.finish());
    ctx->result_computed();
    return TSAR_OK;
}
// ---- coarse-to-fine ------------------------------------------------------------------------------
// Orders `waiter`'s stream after the work issued so far on `producer`'s (the two contexts' streams are not ordered otherwise).
static int stream_after(tsar_ctx* waiter, tsar_ctx* producer) {
    hipEvent_t ev = nullptr;
    TSAR_HIP_TRY(waiter, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, producer->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(waiter->stream, ev, 0);
    hipEventDestroy(ev);
    if (e != hipSuccess) { waiter->err = std::string("stream ordering: ") + hipGetErrorString(e); return TSAR_ERR_HIP; }
    return TSAR_OK;
}

// The two-context calls.  `other` is a second context at all: not null, not the context itself
static bool is_other_ctx(const tsar_ctx* ctx, const tsar_ctx* other) { return other && other != ctx; }
// `coarse` holds views one pyramid level below `fine`'s, ((w + 1) / 2, (h + 1) / 2), on the same device
static bool is_level_below(const tsar_ctx* coarse, const tsar_ctx* fine) {
    return coarse->device == fine->device && coarse->have_views && coarse->w == (fine->w + 1) / 2 && coarse->h == (fine->h + 1) / 2;
}

extern "C" int tsar_pyramid_views(tsar_ctx* coarse, const tsar_ctx* fine_in) {
    CHECK_CTX(coarse);
    tsar_ctx* fine = const_cast<tsar_ctx*>(fine_in);   // its views are only read; its stream is recorded on
    if (!is_other_ctx(coarse, fine)) return fail(coarse, TSAR_ERR_INVALID, "tsar_pyramid_views: fine must be another context");
    if (fine->device != coarse->device) return fail(coarse, TSAR_ERR_INVALID, "tsar_pyramid_views: the two contexts are on different devices");
    if (!fine->have_views) return fail(coarse, TSAR_ERR_INVALID, "tsar_pyramid_views: the fine context has no views");
    if (fine->hscene.geom_on || coarse->hscene.geom_on)
        return fail(coarse, TSAR_ERR_STATE, "tsar_pyramid_views: coarse-to-fine with a geometric-consistency term is not supported (tsar_clear_geom first)");
    if (fine->hscene.prior || coarse->hscene.prior)
        return fail(coarse, TSAR_ERR_STATE, "tsar_pyramid_views: coarse-to-fine with a plane prior is not supported (tsar_clear_plane_prior first)");
    const tsar_params& fp = fine->params;
    const int cw = (fine->w + 1) / 2, ch = (fine->h + 1) / 2;
    if (cw < fp.box_hsize || ch < fp.box_vsize || cw < 8 || ch < 8)
        return fail(coarse, TSAR_ERR_INVALID, "tsar_pyramid_views: the coarse level would be smaller than the matching window (or than 8 x 8)");
    const int n = fine->n_views;
    TRY(tsar_set_params(coarse, &fp));
    std::vector<tsar_camera> cams(fine->cams);
    for (tsar_camera& c : cams) { c.K[0] *= 0.5f; c.K[2] *= 0.5f; c.K[4] *= 0.5f; c.K[5] *= 0.5f; }   // exact: a power of two
    const bool u8 = fine->views_u8;
    {
        CallFrame f(coarse, __func__);     // the levels are staged in the coarse context's arena until its views are installed
        f.take(stream_after(coarse, fine));
        std::vector<const void*> lv(n, nullptr);
        for (int v = 0; v < n && f.ok(); v++) {
            void* dst = f.tmp<char>((size_t)cw * ch * (u8 ? 1 : sizeof(float)));
            if (f.ok()) f.take(launch_pyr_down(coarse, fine->img[v], fine->w, fine->h, dst, u8));
            lv[v] = dst;
        }
        if (f.ok()) f.take(set_views_impl(coarse, n, cw, ch, lv.data(), u8 ? 1 : 4, TSAR_MEM_DEVICE, cams.data()));
        TRY(f.finish());
    }
    if (fine->hscene.n_sel >= 1) TRY(tsar_set_view_subset(coarse, fine->hscene.n_sel, fine->hscene.sel));
    return TSAR_OK;
}

extern "C" int tsar_upsample_planes(tsar_ctx* fine, const tsar_ctx* coarse_in) {
    CHECK_CTX(fine);
    tsar_ctx* coarse = const_cast<tsar_ctx*>(coarse_in);
    if (!is_other_ctx(fine, coarse)) return fail(fine, TSAR_ERR_INVALID, "tsar_upsample_planes: coarse must be another context");
    NEED_VIEWS(fine);
    NEED_SOURCES(fine);
    if (fine->hscene.geom_on || coarse->hscene.geom_on)
        return fail(fine, TSAR_ERR_STATE, "tsar_upsample_planes: coarse-to-fine with a geometric-consistency term is not supported (tsar_clear_geom first)");
    if (fine->hscene.prior || coarse->hscene.prior)
        return fail(fine, TSAR_ERR_STATE, "tsar_upsample_planes: coarse-to-fine with a plane prior is not supported (tsar_clear_plane_prior first)");
    if (!is_level_below(coarse, fine))
        return fail(fine, TSAR_ERR_INVALID, "tsar_upsample_planes: the coarse context must hold views of ((w + 1) / 2, (h + 1) / 2) of the fine one on the same device (tsar_pyramid_views)");
    if (!coarse->have_state) return fail(fine, TSAR_ERR_INVALID, "tsar_upsample_planes: the coarse context has no plane state");
    if (!fine->resize4) TRY(dev_alloc(fine, &fine->resize4, (size_t)fine->w * fine->h));
    fine->have_resize = false;
    TRY(stream_after(fine, coarse));
    TRY(launch_pm_upsample(fine, coarse->buf[0].n4, coarse->w, coarse->h));
    TSAR_HIP_TRY(fine, hipStreamSynchronize(fine->stream));
    fine->state_scored(true);
    fine->have_resize = true;
    return TSAR_OK;
}

extern "C" int tsar_compute_disp_final_upsampled(tsar_ctx* ctx, const float* text, int mem) {
    CHECK_CTX(ctx);
    NEED_STATE(ctx);
    if (!text) return fail(ctx, TSAR_ERR_INVALID, "text is NULL");
    if (!ctx->have_resize) return fail(ctx, TSAR_ERR_INVALID, "tsar_compute_disp_final_upsampled: no upsampled planes kept (call tsar_upsample_planes first)");
    CallFrame f(ctx, __func__, nullptr, /*grow_arena=*/false);
    const float* t = f.in(text, (size_t)ctx->w * ctx->h, mem);
    if (!f.ok()) return f.finish();        // nothing was launched: the state stands
    ctx->costs_voided();
    f.take(launch_compute_disp_final(ctx, ctx->resize4, t));
    TRY(f.finish());
    ctx->result_computed();
    return TSAR_OK;
}

extern "C" int tsar_get_view_image(tsar_ctx* ctx, int view, float* out, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (!out || view < 0 || view >= ctx->n_views) return fail(ctx, TSAR_ERR_INVALID, "tsar_get_view_image: view out of range or out is NULL");
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(out, ctx->img[view], (size_t)ctx->w * ctx->h * sizeof(float), kind_from_dev(mem), ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}

// ---- geometric consistency -----------------------------------------------------------------------
// Installs a geometric-consistency term: one map per source view that has one, owned by the context.  fill(v, &map) allocates
// (dev_alloc) and fills view v's [h][w] map on the context's stream, or leaves it null: no term for that view.  On failure the
// device block must not keep pointers to freed maps, so it is uploaded without any term.
template <typename Fill>
static int install_geom_term(tsar_ctx* ctx, float weight, float clip, Fill fill) {
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // no kernel may still read the maps about to be freed
    free_geom(ctx);
    ctx->geom_maps.assign(ctx->n_views, nullptr);
    DevScene& sc = ctx->hscene;
    for (int v = 1; v < ctx->n_views; v++) {
        const int rc = fill(v, &ctx->geom_maps[v]);
        if (rc != TSAR_OK) {
            hipStreamSynchronize(ctx->stream);
            free_geom(ctx);
            upload_scene(ctx);
            return rc;
        }
        sc.geom_depth[v] = ctx->geom_maps[v];
    }
    sc.geom_weight = weight;
    sc.geom_clip = clip;
    sc.geom_clip_sq = clip * clip;
    sc.geom_on = 1;
    ctx->costs_voided();                   // scored without this term, or with other maps
    return upload_scene(ctx);              // (synchronises the stream: the maps are complete on return)
}

extern "C" int tsar_set_geom_depths(tsar_ctx* ctx, int n_views, const float* const* depth, int mem, float weight, float clip) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (ctx->n_views < 2 || ctx->hscene.n_sel < 1) return fail(ctx, TSAR_ERR_STATE, "tsar_set_geom_depths: the context has no source views");
    if (n_views != ctx->n_views) return fail(ctx, TSAR_ERR_INVALID, "tsar_set_geom_depths: n_views must be the context's number of views (one map per view, [h][w] each)");
    if (!depth) return fail(ctx, TSAR_ERR_INVALID, "tsar_set_geom_depths: depth is NULL");
    if (!(weight >= 0.0f) || !(weight < 1e30f)) return fail(ctx, TSAR_ERR_INVALID, "tsar_set_geom_depths: weight must be finite and >= 0");
    if (!(clip > 0.0f) || !(clip <= 1048576.0f)) return fail(ctx, TSAR_ERR_INVALID, "tsar_set_geom_depths: clip must be in (0, 2^20] pixels");
    if (mem != TSAR_MEM_HOST && mem != TSAR_MEM_DEVICE) return fail(ctx, TSAR_ERR_INVALID, "tsar_set_geom_depths: mem must be TSAR_MEM_HOST or TSAR_MEM_DEVICE");
    const size_t np = (size_t)ctx->w * ctx->h;
    return install_geom_term(ctx, weight, clip, [&](int v, float** map) -> int {
        if (!depth[v]) return TSAR_OK;
        if (dev_alloc(ctx, map, np) != TSAR_OK) return TSAR_ERR_NOMEM;
        if (hipMemcpyAsync(*map, depth[v], np * sizeof(float), kind_to_dev(mem), ctx->stream) != hipSuccess)
            return fail(ctx, TSAR_ERR_HIP, "tsar_set_geom_depths: copy of a depth map failed");
        return TSAR_OK;
    });
}

extern "C" int tsar_clear_geom(tsar_ctx* ctx) {
    CHECK_CTX(ctx);
    if (!ctx->hscene.geom_on && ctx->geom_maps.empty()) return TSAR_OK;
    if (ctx->stream) TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    free_geom(ctx);
    ctx->costs_voided();                   // scored with the term
    return ctx->dscene ? upload_scene(ctx) : TSAR_OK;
}

// ---- plane prior ---------------------------------------------------------------------------------
extern "C" void tsar_default_plane_prior_params(tsar_plane_prior_params* p) {
    if (!p) return;
    p->weight_depth = 0.1f;
    p->weight_normal = 0.05f;
    p->depth_clip = 0.02f;
    p->normal_clip = (float)(1.0 - 0.86602540378443864676);   // 1 - cos(30 deg), rounded once from float64
}

extern "C" int tsar_set_plane_prior(tsar_ctx* ctx, const float* depth, const float* normal_world, int mem, const tsar_plane_prior_params* p) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (ctx->n_views < 2 || ctx->hscene.n_sel < 1) return fail(ctx, TSAR_ERR_STATE, "tsar_set_plane_prior: the context has no source views");
    if (!depth || !normal_world || !p) return fail(ctx, TSAR_ERR_INVALID, "tsar_set_plane_prior: depth, normal_world or params is NULL");
    if (mem != TSAR_MEM_HOST && mem != TSAR_MEM_DEVICE) return fail(ctx, TSAR_ERR_INVALID, "tsar_set_plane_prior: mem must be TSAR_MEM_HOST or TSAR_MEM_DEVICE");
    const float inf = __builtin_inff();
    if (!(p->weight_depth >= 0.0f) || !(p->weight_depth < inf) || !(p->weight_normal >= 0.0f) || !(p->weight_normal < inf))
        return fail(ctx, TSAR_ERR_INVALID, "tsar_set_plane_prior: the weights must be finite and >= 0");
    if (!(p->depth_clip > 0.0f) || !(p->depth_clip < inf)) return fail(ctx, TSAR_ERR_INVALID, "tsar_set_plane_prior: depth_clip must be finite and > 0");
    if (!(p->normal_clip > 0.0f) || !(p->normal_clip <= 2.0f)) return fail(ctx, TSAR_ERR_INVALID, "tsar_set_plane_prior: normal_clip must be in (0, 2]");
    const size_t np = (size_t)ctx->w * ctx->h;
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));   // no kernel may still read the prior about to be replaced
    if (!ctx->prior) {
        const int rc = dev_alloc(ctx, &ctx->prior, np);
        if (rc != TSAR_OK) { free_prior(ctx); upload_scene(ctx); return rc; }
    }
    {
        CallFrame f(ctx, __func__);
        const float *d = f.in(depth, np, mem), *n = f.in(normal_world, 3 * np, mem);
        if (f.ok()) f.take(launch_plane_prior(ctx, d, n, ctx->prior));
        const int rc = f.finish();
        if (rc != TSAR_OK) { free_prior(ctx); upload_scene(ctx); return rc; }   // the device block must not keep a half-written prior
    }
    DevScene& sc = ctx->hscene;
    sc.prior = ctx->prior;
    sc.prior_weight_depth = p->weight_depth;
    sc.prior_weight_normal = p->weight_normal;
    sc.prior_depth_clip = p->depth_clip;
    sc.prior_normal_clip = p->normal_clip;
    ctx->costs_voided();                   // scored without this term, or with another prior
    return upload_scene(ctx);
}

extern "C" int tsar_clear_plane_prior(tsar_ctx* ctx) {
    CHECK_CTX(ctx);
    if (!ctx->prior) return TSAR_OK;
    if (ctx->stream) TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    free_prior(ctx);
    ctx->costs_voided();                   // scored with the term
    return ctx->dscene ? upload_scene(ctx) : TSAR_OK;
}

extern "C" int tsar_get_plane_prior(tsar_ctx* ctx, float* prior_out, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (!prior_out) return fail(ctx, TSAR_ERR_INVALID, "tsar_get_plane_prior: prior_out is NULL");
    if (mem != TSAR_MEM_HOST && mem != TSAR_MEM_DEVICE) return fail(ctx, TSAR_ERR_INVALID, "tsar_get_plane_prior: mem must be TSAR_MEM_HOST or TSAR_MEM_DEVICE");
    if (!ctx->hscene.prior) return fail(ctx, TSAR_ERR_STATE, "tsar_get_plane_prior: no plane prior installed (tsar_set_plane_prior)");
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(prior_out, ctx->prior, (size_t)ctx->w * ctx->h * sizeof(float4), kind_from_dev(mem), ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}

// ---- a prior built from a checked depth map (plane_prior_build_kernels.hip) -------------------------------------------------------
extern "C" void tsar_default_plane_prior_build_params(tsar_plane_prior_build_params* p) {
    if (!p) return;
    p->cell = 4;                           // include/tsar.h says why, and that it is untuned
    p->max_levels = 0;
}

// Reads the map, the score and the reference camera, writes the caller's outputs and one temporary of the call: no transition of the
// plane state (tsar_dev.h) is involved, and nothing the context owns is written
extern "C" int tsar_build_plane_prior(tsar_ctx* ctx, const float* depth, const float* score, int mem, const tsar_plane_prior_build_params* p,
                                      float* depth_out, float* normal_world_out, uint8_t* level_out) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (!depth || !p) return fail(ctx, TSAR_ERR_INVALID, "tsar_build_plane_prior: depth or params is NULL");
    if (!depth_out && !normal_world_out && !level_out) return fail(ctx, TSAR_ERR_INVALID, "tsar_build_plane_prior: every output is NULL");
    if (mem != TSAR_MEM_HOST && mem != TSAR_MEM_DEVICE) return fail(ctx, TSAR_ERR_INVALID, "tsar_build_plane_prior: mem must be TSAR_MEM_HOST or TSAR_MEM_DEVICE");
    if (p->cell < 2 || p->cell > 256) return fail(ctx, TSAR_ERR_INVALID, "tsar_build_plane_prior: cell must be in 2..256");
    if (p->max_levels < 0 || p->max_levels > TSAR_PLANE_PRIOR_MAX_LEVELS) return fail(ctx, TSAR_ERR_INVALID, "tsar_build_plane_prior: max_levels must be in 0..16");
    if (ctx->w > 65535 || ctx->h > 65535) return fail(ctx, TSAR_ERR_INVALID, "tsar_build_plane_prior: the image is larger than 65535 pixels in a direction");
    const size_t keys = plane_prior_build_grid_keys(ctx->w, ctx->h, p->cell, p->max_levels);
    if (keys == 0) return fail(ctx, TSAR_ERR_INVALID, "tsar_build_plane_prior: the image is too small for one level (both sides must exceed cell)");
    const size_t np = (size_t)ctx->w * ctx->h;
    CallFrame f(ctx, __func__);
    const float *d = f.in(depth, np, mem), *s = f.in(score, np, mem);
    unsigned long long* grid = f.tmp<unsigned long long>(keys);
    float *od = f.out(depth_out, np, mem), *on = f.out(normal_world_out, 3 * np, mem);
    uint8_t* ol = f.out(level_out, np, mem);
    if (f.ok()) f.take(launch_plane_prior_build(ctx, d, s, p->cell, p->max_levels, grid, od, on, ol));
    return f.finish();
}

// buf[0]'s planes scored with the context's cost (invalid ones redrawn as tsar_pm_init draws) into buf[1], which becomes the state:
// the kernel's plane pointers are restrict-qualified, so it cannot run in place
static int rescore_state(tsar_ctx* ctx) {
    TRY(launch_pm_rescore(ctx, ctx->buf[0].n4, ctx->buf[1].c, ctx->buf[1].n4, ctx->beview, ctx->ratio));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    std::swap(ctx->buf[0], ctx->buf[1]);
    ctx->state_scored(true);               // every c[p] is n4[p]'s score under the context's cost, on the sweep window
    return TSAR_OK;
}

extern "C" int tsar_pm_rescore(tsar_ctx* ctx) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    NEED_SOURCES(ctx);
    NEED_STATE(ctx);
    return rescore_state(ctx);
}

extern "C" int tsar_get_geom_matrices(tsar_ctx* ctx, int view, float* forward, float* back) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (view < 0 || view >= ctx->n_views || !forward || !back) return fail(ctx, TSAR_ERR_INVALID, "tsar_get_geom_matrices: view out of range or NULL output");
    const DevView& dv = ctx->hscene.view[view];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) forward[4 * r + c] = dv.A[3 * r + c];
        forward[4 * r + 3] = dv.b[r];
    }
    for (int i = 0; i < 12; i++) back[i] = ctx->hscene.geom_back[view][i];
    return TSAR_OK;
}

// ---- the geometric-consistency pass coarse to fine ------------------------------------------------------------------------------
// `coarse` holds what tsar_pyramid_views installs from `fine`: ((w + 1) / 2, (h + 1) / 2) views of as many views, on the same device, with
// fine's cameras and their fx, fy, cx, cy halved
static bool is_pyramid_of(const tsar_ctx* coarse, const tsar_ctx* fine) {
    if (!fine->have_views || !is_level_below(coarse, fine)) return false;
    if (coarse->n_views != fine->n_views || coarse->cams.size() != fine->cams.size()) return false;
    for (size_t v = 0; v < fine->cams.size(); v++) {
        tsar_camera c = fine->cams[v];
        c.K[0] *= 0.5f; c.K[2] *= 0.5f; c.K[4] *= 0.5f; c.K[5] *= 0.5f;
        if (memcmp(&c, &coarse->cams[v], sizeof c) != 0) return false;
    }
    return true;
}

extern "C" int tsar_geom_pyramid(tsar_ctx* coarse, const tsar_ctx* fine_in) {
    CHECK_CTX(coarse);
    tsar_ctx* fine = const_cast<tsar_ctx*>(fine_in);   // its maps are only read; its stream is recorded on
    if (!is_other_ctx(coarse, fine)) return fail(coarse, TSAR_ERR_INVALID, "tsar_geom_pyramid: fine must be another context");
    if (!fine->hscene.geom_on) return fail(coarse, TSAR_ERR_STATE, "tsar_geom_pyramid: the fine context has no geometric-consistency term");
    if (!is_pyramid_of(coarse, fine))
        return fail(coarse, TSAR_ERR_INVALID, "tsar_geom_pyramid: the coarse context must hold fine's views one level down (tsar_pyramid_views)");
    const size_t np = (size_t)coarse->w * coarse->h;
    const DevScene& fs = fine->hscene;
    bool ordered = false;                  // coarse's stream after fine's, before the first map is read
    return install_geom_term(coarse, fs.geom_weight, fs.geom_clip /* the same number of pixels of this level */, [&](int v, float** map) -> int {
        if (!ordered) TRY(stream_after(coarse, fine));
        ordered = true;
        if (!fs.geom_depth[v]) return TSAR_OK;
        TRY(dev_alloc(coarse, map, np));
        return launch_geom_pyramid(coarse, fs.geom_depth[v], fine->w, fine->h, *map);
    });
}

extern "C" int tsar_pyramid_planes(tsar_ctx* coarse, const tsar_ctx* fine_in) {
    CHECK_CTX(coarse);
    tsar_ctx* fine = const_cast<tsar_ctx*>(fine_in);
    if (!is_other_ctx(coarse, fine)) return fail(coarse, TSAR_ERR_INVALID, "tsar_pyramid_planes: fine must be another context");
    if (!fine->have_state) return fail(coarse, TSAR_ERR_INVALID, "tsar_pyramid_planes: the fine context has no plane state");
    if (!is_level_below(coarse, fine))
        return fail(coarse, TSAR_ERR_INVALID, "tsar_pyramid_planes: the coarse context must hold views of ((w + 1) / 2, (h + 1) / 2) of the fine one on the same device");
    NEED_SOURCES(coarse);
    TRY(stream_after(coarse, fine));
    TRY(launch_pyramid_planes(coarse, fine->buf[0].n4, fine->w, fine->h, coarse->buf[0].n4));
    return rescore_state(coarse);
}

extern "C" int tsar_upsample_merge(tsar_ctx* fine, const tsar_ctx* coarse_in) {
    CHECK_CTX(fine);
    tsar_ctx* coarse = const_cast<tsar_ctx*>(coarse_in);
    if (!is_other_ctx(fine, coarse)) return fail(fine, TSAR_ERR_INVALID, "tsar_upsample_merge: coarse must be another context");
    if (!fine->have_state) return fail(fine, TSAR_ERR_INVALID, "tsar_upsample_merge: the fine context has no plane state");
    NEED_SOURCES(fine);
    if (!coarse->have_state || !is_level_below(coarse, fine))
        return fail(fine, TSAR_ERR_INVALID, "tsar_upsample_merge: the coarse context must hold a plane state of ((w + 1) / 2, (h + 1) / 2) on the same device");
    TRY(stream_after(fine, coarse));
    TRY(launch_pm_upsample_merge(fine, coarse->buf[0].n4, coarse->w, coarse->h));   // buf[0] -> buf[1]
    TSAR_HIP_TRY(fine, hipStreamSynchronize(fine->stream));
    std::swap(fine->buf[0], fine->buf[1]);
    fine->state_scored(true);              // every cost is its plane's score on the sweep window
    return TSAR_OK;
}

// ---- the geometric-consistency check on its own (geom_check_kernels.hip) ---------------------------------------------------------
extern "C" void tsar_default_geom_check_params(tsar_geom_check_params* p) {
    if (!p) return;
    p->reproj_error = 2.0f;                // tsar_default_fusion_params' values
    p->depth_diff = 0.01f;
    p->min_consistent = 2;
}

// Reads the map and the term, writes ctx->scale and the caller's outputs: no transition of the plane state (tsar_dev.h) is involved
extern "C" int tsar_geom_check(tsar_ctx* ctx, const float* depth, const tsar_geom_check_params* p, uint8_t* count_out, float* depth_out, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (!ctx->hscene.geom_on) return fail(ctx, TSAR_ERR_STATE, "tsar_geom_check: no geometric-consistency term installed (tsar_set_geom_depths supplies the source maps)");
    if (!p) return fail(ctx, TSAR_ERR_INVALID, "tsar_geom_check: params is NULL");
    if (!(p->reproj_error > 0.0f) || !(p->reproj_error <= 1048576.0f)) return fail(ctx, TSAR_ERR_INVALID, "tsar_geom_check: reproj_error must be in (0, 2^20] pixels");
    if (!(p->depth_diff > 0.0f) || !(p->depth_diff < __builtin_inff())) return fail(ctx, TSAR_ERR_INVALID, "tsar_geom_check: depth_diff must be finite and > 0");
    if (p->min_consistent < 1 || p->min_consistent > 31) return fail(ctx, TSAR_ERR_INVALID, "tsar_geom_check: min_consistent must be in 1..31");
    if (mem != TSAR_MEM_HOST && mem != TSAR_MEM_DEVICE) return fail(ctx, TSAR_ERR_INVALID, "tsar_geom_check: mem must be TSAR_MEM_HOST or TSAR_MEM_DEVICE");
    if (!depth && !(ctx->have_state && ctx->have_out)) return fail(ctx, TSAR_ERR_STATE, "tsar_geom_check: depth is NULL and the context has no result (call tsar_compute_disp / tsar_fill_textureless first)");
    const size_t np = (size_t)ctx->w * ctx->h;
    const float* own = (const float*)ctx->out4 + 3;        // the result plane is (n_world, depth) per pixel
    CallFrame f(ctx, __func__);
    const float* d = f.in(depth, np, mem);
    uint8_t* dc = f.out(count_out, np, mem);
    float* dd = f.out(depth_out, np, mem);
    if (f.ok()) f.take(launch_geom_check(ctx, depth ? d : own, depth ? 1 : 4, p, dc, dd));
    return f.finish();
}

// ---- the source views' maps rendered into the reference camera (geom_reproject_kernels.hip) ---------------------------------------
extern "C" void tsar_default_geom_reproject_params(tsar_geom_reproject_params* p) {
    if (!p) return;
    p->depth_diff = 0.01f;                 // tsar_default_geom_check_params' value
    p->min_views = 1;
}

// Reads the term's maps and matrices, writes the caller's outputs and two temporaries of the call: no transition of the plane state
// (tsar_dev.h) is involved, and lines->scale is left alone
extern "C" int tsar_geom_reproject(tsar_ctx* ctx, const tsar_geom_reproject_params* p, float* depth_out, uint8_t* count_out, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (!ctx->hscene.geom_on) return fail(ctx, TSAR_ERR_STATE, "tsar_geom_reproject: no geometric-consistency term installed (tsar_set_geom_depths supplies the source maps)");
    if (!p) return fail(ctx, TSAR_ERR_INVALID, "tsar_geom_reproject: params is NULL");
    if (!depth_out && !count_out) return fail(ctx, TSAR_ERR_INVALID, "tsar_geom_reproject: depth_out and count_out are both NULL");
    if (!(p->depth_diff > 0.0f) || !(p->depth_diff < __builtin_inff())) return fail(ctx, TSAR_ERR_INVALID, "tsar_geom_reproject: depth_diff must be finite and > 0");
    if (p->min_views < 1 || p->min_views > TSAR_MAX_VIEWS - 1) return fail(ctx, TSAR_ERR_INVALID, "tsar_geom_reproject: min_views must be in 1..63");
    if (mem != TSAR_MEM_HOST && mem != TSAR_MEM_DEVICE) return fail(ctx, TSAR_ERR_INVALID, "tsar_geom_reproject: mem must be TSAR_MEM_HOST or TSAR_MEM_DEVICE");
    const size_t np = (size_t)ctx->w * ctx->h;
    CallFrame f(ctx, __func__);
    float* dd = f.out(depth_out, np, mem);
    uint8_t* dc = f.out(count_out, np, mem);
    uint32_t* zbuf = f.tmp<uint32_t>(np);
    unsigned long long* mask = f.tmp<unsigned long long>(np);
    if (f.ok()) f.take(launch_geom_reproject(ctx, p, zbuf, mask, dd, dc));
    return f.finish();
}

// ---- a depth map offered to the matcher -----------------------------------------------------------------------------------------------
// The composition include/tsar.h states: rescore_state, the candidates, tsar_pm_cost_planes's launcher, the strict select
extern "C" int tsar_pm_merge_depths(tsar_ctx* ctx, const float* depth, int mem, int64_t* n_taken_out) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    NEED_SOURCES(ctx);
    NEED_STATE(ctx);
    if (!depth) return fail(ctx, TSAR_ERR_INVALID, "tsar_pm_merge_depths: depth is NULL");
    if (mem != TSAR_MEM_HOST && mem != TSAR_MEM_DEVICE) return fail(ctx, TSAR_ERR_INVALID, "tsar_pm_merge_depths: mem must be TSAR_MEM_HOST or TSAR_MEM_DEVICE");
    TRY(rescore_state(ctx));               // from here on the state is a scored one, whatever happens below
    const size_t np = (size_t)ctx->w * ctx->h;
    unsigned long long taken = 0;
    CallFrame f(ctx, __func__);
    const float* d = f.in(depth, np, mem);
    float4* cand = f.tmp<float4>(np);
    float* cand_c = f.tmp<float>(np);
    int32_t* cand_bv = f.tmp<int32_t>(np);
    float* cand_rt = f.tmp<float>(np);
    unsigned long long* dtaken = f.tmp<unsigned long long>(1);
    f.zero(dtaken, sizeof(unsigned long long));
    if (f.ok()) f.take(launch_merge_candidates(ctx, d, cand));
    if (f.ok()) f.take(launch_pm_cost_planes(ctx, cand, cand_c, cand_bv, cand_rt));
    if (f.ok()) f.take(launch_merge_select(ctx, cand, cand_c, cand_bv, cand_rt, dtaken));
    f.copy(&taken, dtaken, sizeof taken, hipMemcpyDeviceToHost);
    TRY(f.finish());                       // (synchronises: `taken` is complete)
    ctx->state_scored(true);               // every taken cost is the taken plane's score on the sweep window
    if (n_taken_out) *n_taken_out = (int64_t)taken;
    return TSAR_OK;
}

// ---- what the entries on point clouds share ---------------------------------------------------------------------------------------------
// The checks every one of them makes on its memory space and its clouds, in this order: mem, every n, every stride, every pointer.  The
// wording of an entry with one cloud is the default; tsar_cloud_distance, with two, passes its own.
struct CloudArg { const void* pts; int64_t n; int stride; };
static int check_clouds(tsar_ctx* ctx, const char* entry, int mem, std::initializer_list<CloudArg> clouds, const char* n_names = "n", const char* stride_names = "the stride",
                        const char* pts_names = "cloud") {
    std::string msg;
    if (mem != TSAR_MEM_HOST && mem != TSAR_MEM_DEVICE) msg = "mem must be TSAR_MEM_HOST or TSAR_MEM_DEVICE";
    for (const CloudArg& c : clouds)
        if (msg.empty() && (c.n < 0 || c.n > INT32_MAX)) msg = std::string(n_names) + " must be in 0..2^31-1";
    for (const CloudArg& c : clouds)
        if (msg.empty() && c.stride < 3) msg = std::string(stride_names) + " must be at least 3 floats (x y z first)";
    for (const CloudArg& c : clouds)
        if (msg.empty() && c.n > 0 && !c.pts) msg = std::string(pts_names) + " is NULL";
    return msg.empty() ? TSAR_OK : fail(ctx, TSAR_ERR_INVALID, (std::string(entry) + ": " + msg).c_str());
}

// *r2 = fl(R * R), one float32 product; false unless R and the product are finite and > 0
static bool cloud_radius2(float R, float* r2) {
    const volatile float r2v = R * R;
    *r2 = r2v;
    return fabsf(R) <= FLT_MAX && *r2 > 0.0f && *r2 <= FLT_MAX && R > 0.0f;
}

// tol2[k] = fl(tol[k] * tol[k]), one float32 product each; a tolerance outside (0, bound] refuses the call with `refusal`
static int square_tolerances(tsar_ctx* ctx, int n_tol, const float* tol, float bound, const char* refusal, std::vector<float>& tol2) {
    tol2.resize((size_t)n_tol);
    for (int k = 0; k < n_tol; k++) {
        if (!(tol[k] > 0.0f && tol[k] <= bound)) return fail(ctx, TSAR_ERR_INVALID, refusal);
        const volatile float t2 = tol[k] * tol[k];
        tol2[k] = t2;
    }
    return TSAR_OK;
}

// The context-free form of an entry: a context of its own for the duration of the call.
template <typename Call>
static int with_own_ctx(int device, Call call) {
    tsar_ctx* ctx = nullptr;
    const int rc0 = tsar_create(device, &ctx);
    if (rc0 != TSAR_OK) return rc0;
    const int rc = call(ctx);
    tsar_destroy(ctx);
    return rc;
}

// ---- cloud-to-cloud distances (cloud_distance_kernels.hip) ----------------------------------------------------------------------------
extern "C" void tsar_default_cloud_distance_params(tsar_cloud_distance_params* p) {
    if (!p) return;
    p->max_dist = 0.0f;                    // no default: the caller's scale
    p->max_pairs = (int64_t)1 << 40;
}

// Needs no views and no state, and writes nothing the context owns.  The frame does not grow the arena (tsar_dev.h ScratchScope, grow =
// false): the sort buffers of two large clouds are no size a matching context should keep; what does not fit is freed on exit.
extern "C" int tsar_cloud_distance_ctx(tsar_ctx* ctx, const float* query, int64_t n_query, int query_stride, const float* target, int64_t n_target,
                                       int target_stride, const tsar_cloud_distance_params* p, int n_tol, const float* tol, float* dist2_out, int32_t* index_out,
                                       int64_t* within_out, int64_t* n_valid_query_out, int64_t* pairs_out, int mem) {
    CHECK_CTX(ctx);
    if (!p) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_distance: params is NULL");
    TRY(check_clouds(ctx, "tsar_cloud_distance", mem, {{query, n_query, query_stride}, {target, n_target, target_stride}}, "n_query and n_target", "a stride",
                     "query or target"));
    const float R = p->max_dist;
    float r2;
    if (!cloud_radius2(R, &r2))
        return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_distance: max_dist must be finite and > 0, with max_dist * max_dist finite and > 0 in float32");
    if (p->max_pairs < 0) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_distance: max_pairs must be >= 0");
    if (n_tol < 0 || (n_tol > 0 && !tol)) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_distance: n_tol < 0, or tol is NULL");
    std::vector<float> tol2;
    TRY(square_tolerances(ctx, n_tol, tol, R, "tsar_cloud_distance: every tolerance must be finite, > 0 and <= max_dist", tol2));
    CallFrame f(ctx, "tsar_cloud_distance", nullptr, /*grow_arena=*/false);
    const float* q = f.in(query, (size_t)n_query * query_stride, mem);
    const float* t = (target == query && n_target == n_query && target_stride == query_stride) ? q : f.in(target, (size_t)n_target * target_stride, mem);
    float* d2 = f.out(dist2_out, (size_t)n_query, mem);
    int32_t* idx = f.out(index_out, (size_t)n_query, mem);
    if (!f.ok()) return f.finish();
    return run_cloud_distance(f, q, n_query, query_stride, t, n_target, target_stride, r2, (double)R * (1.0 + 1.0 / 1024.0), p->max_pairs, n_tol, tol2.data(), d2, idx,
                              within_out, n_valid_query_out, pairs_out);
}

// Context-free form (the evaluation tool's two calls per pair of clouds).
extern "C" int tsar_cloud_distance(int device, const float* query, int64_t n_query, int query_stride, const float* target, int64_t n_target, int target_stride,
                                   const tsar_cloud_distance_params* p, int n_tol, const float* tol, float* dist2_out, int32_t* index_out, int64_t* within_out,
                                   int64_t* n_valid_query_out, int64_t* pairs_out, int mem) {
    return with_own_ctx(device, [&](tsar_ctx* ctx) {
        return tsar_cloud_distance_ctx(ctx, query, n_query, query_stride, target, n_target, target_stride, p, n_tol, tol, dist2_out, index_out, within_out, n_valid_query_out,
                                       pairs_out, mem);
    });
}

// ---- a voxel grid over a cloud (cloud_voxel_kernels.hip) -------------------------------------------------------------------------------
extern "C" void tsar_default_cloud_voxels_params(tsar_cloud_voxels_params* p) {
    if (!p) return;
    p->voxel = 0.0f;                       // no default: the caller's scale
}

// Like tsar_cloud_distance_ctx: no views, no state, nothing of the context written, and a frame that does not grow the arena.
extern "C" int tsar_cloud_voxels_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_voxels_params* p, const float* dist2, int n_tol,
                                     const float* tol, int32_t* rank_out, int64_t cap, int32_t* rep_out, int32_t* count_out, int32_t* within_out, int64_t* n_voxels_out,
                                     int64_t* n_valid_out, int mem) {
    CHECK_CTX(ctx);
    if (!p) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_voxels: params is NULL");
    TRY(check_clouds(ctx, "tsar_cloud_voxels", mem, {{cloud, n, stride}}));
    const float V = p->voxel;
    if (!(fabsf(V) <= FLT_MAX) || !(V > 0.0f)) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_voxels: voxel must be finite and > 0");
    if (cap < 0) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_voxels: cap must be >= 0");
    if (n_tol < 0 || (n_tol > 0 && (!tol || (!dist2 && n > 0)))) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_voxels: n_tol < 0, or tolerances without tol or without dist2");
    if (n_tol == 0 && within_out) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_voxels: within_out needs tolerances (n_tol is 0)");
    std::vector<float> tol2;
    TRY(square_tolerances(ctx, n_tol, tol, FLT_MAX, "tsar_cloud_voxels: every tolerance must be finite and > 0", tol2));
    CallFrame f(ctx, "tsar_cloud_voxels", nullptr, /*grow_arena=*/false);
    const float* c = f.in(cloud, (size_t)n * stride, mem);
    const float* d2 = n_tol > 0 ? f.in(dist2, (size_t)n, mem) : nullptr;
    if (!f.ok()) return f.finish();
    return run_cloud_voxels(f, c, n, stride, (double)V, d2, n_tol, tol2.data(), rank_out, cap, rep_out, count_out, within_out, n_voxels_out, n_valid_out, mem);
}

// Context-free form (the fuser's thinning step).
extern "C" int tsar_cloud_voxels(int device, const float* cloud, int64_t n, int stride, const tsar_cloud_voxels_params* p, const float* dist2, int n_tol, const float* tol,
                                 int32_t* rank_out, int64_t cap, int32_t* rep_out, int32_t* count_out, int32_t* within_out, int64_t* n_voxels_out, int64_t* n_valid_out,
                                 int mem) {
    return with_own_ctx(device, [&](tsar_ctx* ctx) {
        return tsar_cloud_voxels_ctx(ctx, cloud, n, stride, p, dist2, n_tol, tol, rank_out, cap, rep_out, count_out, within_out, n_voxels_out, n_valid_out, mem);
    });
}

// ---- neighbourhood statistics of a cloud (cloud_neighbor_kernels.hip) -------------------------------------------------------------------
extern "C" void tsar_default_cloud_neighbors_params(tsar_cloud_neighbors_params* p) {
    if (!p) return;
    p->radius = 0.0f;                      // no default: the caller's scale
    p->k = 0;
    p->max_pairs = (int64_t)1 << 40;
}

// Like tsar_cloud_distance_ctx: no views, no state, nothing of the context written, and a frame that does not grow the arena.
extern "C" int tsar_cloud_neighbors_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_neighbors_params* p, int32_t* count_out,
                                        float* knn_dist2_out, int64_t* n_valid_out, int64_t* pairs_out, int mem) {
    CHECK_CTX(ctx);
    if (!p) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_neighbors: params is NULL");
    TRY(check_clouds(ctx, "tsar_cloud_neighbors", mem, {{cloud, n, stride}}));
    const float R = p->radius;
    float r2;
    if (!cloud_radius2(R, &r2))
        return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_neighbors: radius must be finite and > 0, with radius * radius finite and > 0 in float32");
    if (p->k < 0 || p->k > TSAR_CLOUD_KNN_MAX) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_neighbors: k must be in 0..TSAR_CLOUD_KNN_MAX (32)");
    if (p->k == 0 && knn_dist2_out) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_neighbors: knn_dist2_out needs k > 0");
    if (p->max_pairs < 0) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_neighbors: max_pairs must be >= 0");
    CallFrame f(ctx, "tsar_cloud_neighbors", nullptr, /*grow_arena=*/false);
    const float* c = f.in(cloud, (size_t)n * stride, mem);
    int32_t* cnt = f.out(count_out, (size_t)n, mem);
    float* knn = f.out(knn_dist2_out, (size_t)n * (size_t)p->k, mem);
    if (!f.ok()) return f.finish();
    return run_cloud_neighbors(f, c, n, stride, r2, (double)R * (1.0 + 1.0 / 1024.0), p->k, p->max_pairs, cnt, knn, n_valid_out, pairs_out);
}

// Context-free form (the fuser's cleaning step).
extern "C" int tsar_cloud_neighbors(int device, const float* cloud, int64_t n, int stride, const tsar_cloud_neighbors_params* p, int32_t* count_out, float* knn_dist2_out,
                                    int64_t* n_valid_out, int64_t* pairs_out, int mem) {
    return with_own_ctx(device, [&](tsar_ctx* ctx) { return tsar_cloud_neighbors_ctx(ctx, cloud, n, stride, p, count_out, knn_dist2_out, n_valid_out, pairs_out, mem); });
}

// ---- normals of a cloud; two sets of normals compared (cloud_normal_kernels.hip) -----------------------------------------------------------
extern "C" void tsar_default_cloud_normals_params(tsar_cloud_normals_params* p) {
    if (!p) return;
    p->radius = 0.0f;                      // no default: the caller's scale
    p->k = 16;
    p->min_neighbors = 5;
    p->orient = 0;
    p->viewpoint[0] = p->viewpoint[1] = p->viewpoint[2] = 0.0f;
    p->max_pairs = (int64_t)1 << 40;
}

// Like tsar_cloud_distance_ctx: no views, no state, nothing of the context written, and a frame that does not grow the arena.
extern "C" int tsar_cloud_normals_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_normals_params* p, int32_t* knn_index_out,
                                      int32_t* n_used_out, float* normal_out, float* curvature_out, double* cov_out, int64_t* n_valid_out, int64_t* n_normals_out,
                                      int64_t* pairs_out, int mem) {
    CHECK_CTX(ctx);
    if (!p) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normals: params is NULL");
    TRY(check_clouds(ctx, "tsar_cloud_normals", mem, {{cloud, n, stride}}));
    const float R = p->radius;
    float r2;
    if (!cloud_radius2(R, &r2))
        return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normals: radius must be finite and > 0, with radius * radius finite and > 0 in float32");
    if (p->k < 3 || p->k > TSAR_CLOUD_KNN_MAX) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normals: k must be in 3..TSAR_CLOUD_KNN_MAX (32)");
    if (p->min_neighbors < 2 || p->min_neighbors > p->k) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normals: min_neighbors must be in 2..k");
    if (p->orient < 0 || p->orient > 2) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normals: orient must be 0 (canonical), 1 (viewpoint) or 2 (the record's normal)");
    if (p->orient == 2 && stride < 6) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normals: orient 2 reads the record's floats 3..5: the stride must be at least 6");
    if (p->orient == 1 && !(fabsf(p->viewpoint[0]) <= FLT_MAX && fabsf(p->viewpoint[1]) <= FLT_MAX && fabsf(p->viewpoint[2]) <= FLT_MAX))
        return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normals: orient 1 needs a finite viewpoint");
    if (p->max_pairs < 0) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normals: max_pairs must be >= 0");
    CallFrame f(ctx, "tsar_cloud_normals", nullptr, /*grow_arena=*/false);
    const float* c = f.in(cloud, (size_t)n * stride, mem);
    int32_t* knn = f.out(knn_index_out, (size_t)n * (size_t)p->k, mem);
    int32_t* used = f.out(n_used_out, (size_t)n, mem);
    float* nrm = f.out(normal_out, (size_t)n * 3, mem);
    float* curv = f.out(curvature_out, (size_t)n, mem);
    double* cov = f.out(cov_out, (size_t)n * 6, mem);
    if (!f.ok()) return f.finish();
    return run_cloud_normals(f, c, n, stride, r2, (double)R * (1.0 + 1.0 / 1024.0), *p, knn, used, nrm, curv, cov, n_valid_out, n_normals_out, pairs_out);
}

// Context-free form (the evaluation tool's normals of the ground truth).
extern "C" int tsar_cloud_normals(int device, const float* cloud, int64_t n, int stride, const tsar_cloud_normals_params* p, int32_t* knn_index_out, int32_t* n_used_out,
                                  float* normal_out, float* curvature_out, double* cov_out, int64_t* n_valid_out, int64_t* n_normals_out, int64_t* pairs_out, int mem) {
    return with_own_ctx(device, [&](tsar_ctx* ctx) {
        return tsar_cloud_normals_ctx(ctx, cloud, n, stride, p, knn_index_out, n_used_out, normal_out, curvature_out, cov_out, n_valid_out, n_normals_out, pairs_out, mem);
    });
}

extern "C" int tsar_cloud_normal_compare_ctx(tsar_ctx* ctx, const float* normal_a, int stride_a, int64_t n, const float* normal_b, int stride_b, int64_t n_b,
                                             const int32_t* index, const float* dist2, float max_dist, int n_tol, const double* min_cos, int is_signed, float* cos_out,
                                             int64_t* within_out, int64_t* n_compared_out, int mem) {
    CHECK_CTX(ctx);
    TRY(check_clouds(ctx, "tsar_cloud_normal_compare", mem, {{normal_a, n, stride_a}, {normal_b, n_b, stride_b}}, "n and n_b", "a stride", "normal_a or normal_b"));
    if (n > 0 && !index) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normal_compare: index is NULL");
    if (n_tol < 0 || n_tol > TSAR_NORMAL_COMPARE_MAX_TOL || (n_tol > 0 && !min_cos))
        return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normal_compare: n_tol must be in 0..16, and min_cos not NULL with n_tol > 0");
    for (int k = 0; k < n_tol; k++)
        if (!(min_cos[k] >= -1.0 && min_cos[k] <= 1.0)) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normal_compare: every threshold must be in [-1, 1]");
    float md2 = 0.0f;
    if (dist2 && !cloud_radius2(max_dist, &md2))
        return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_normal_compare: with dist2, max_dist must be finite and > 0, with max_dist * max_dist finite and > 0 in float32");
    CallFrame f(ctx, "tsar_cloud_normal_compare", nullptr, /*grow_arena=*/false);
    const float* a = f.in(normal_a, (size_t)n * stride_a, mem);
    const float* b = (normal_b == normal_a && n_b == n && stride_b == stride_a) ? a : f.in(normal_b, (size_t)n_b * stride_b, mem);
    const int32_t* idx = f.in(index, (size_t)n, mem);
    const float* d2 = f.in(dist2, (size_t)n, mem);
    float* co = f.out(cos_out, (size_t)n, mem);
    if (!f.ok()) return f.finish();
    unsigned long long counters[1 + TSAR_NORMAL_COMPARE_MAX_TOL] = {0};
    TRY(run_cloud_normal_compare(f, a, stride_a, n, b, stride_b, n_b, idx, d2, md2, n_tol, min_cos, is_signed, co, counters));
    if (n_compared_out) *n_compared_out = (int64_t)counters[0];
    for (int k = 0; k < n_tol && within_out; k++) within_out[k] = (int64_t)counters[1 + k];
    return TSAR_OK;
}

extern "C" int tsar_cloud_normal_compare(int device, const float* normal_a, int stride_a, int64_t n, const float* normal_b, int stride_b, int64_t n_b, const int32_t* index,
                                         const float* dist2, float max_dist, int n_tol, const double* min_cos, int is_signed, float* cos_out, int64_t* within_out,
                                         int64_t* n_compared_out, int mem) {
    return with_own_ctx(device, [&](tsar_ctx* ctx) {
        return tsar_cloud_normal_compare_ctx(ctx, normal_a, stride_a, n, normal_b, stride_b, n_b, index, dist2, max_dist, n_tol, min_cos, is_signed, cos_out, within_out,
                                             n_compared_out, mem);
    });
}

// ---- a cloud rendered into a camera; a depth map scored against a map (cloud_render_kernels.hip) -----------------------------------------
extern "C" void tsar_default_cloud_render_params(tsar_cloud_render_params* p) {
    if (!p) return;
    p->radius = 0.0f;                      // no default: the caller's scale (0 renders without a footprint)
    p->max_px = 8;
    p->occlusion_diff = 0.02f;
    p->depth_diff = 0.01f;
    p->min_points = 1;
    p->max_splats = (int64_t)1 << 34;
}

// The checks and the view that tsar_cloud_render and tsar_cloud_render_oriented share, in the order the header lists the refusals; `entry`
// names the caller in the message, no_outputs is its "every output is NULL" refusal (null: the caller has an output).
static int cloud_render_view(tsar_ctx* ctx, const char* entry, const float* cloud, int64_t n, int stride, const tsar_camera* cam, int w, int h,
                             const tsar_cloud_render_params* p, const char* no_outputs, int mem, CrViewHost* vh) {
    const auto refuse = [&](const char* why) { return fail(ctx, TSAR_ERR_INVALID, (std::string(entry) + ": " + why).c_str()); };
    if (!p) return refuse("params is NULL");
    if (!cam) return refuse("cam is NULL");
    TRY(check_clouds(ctx, entry, mem, {{cloud, n, stride}}));
    if (no_outputs) return refuse(no_outputs);
    if (w < 1 || h < 1 || w + 2 >= (1 << 23) || h + 2 >= (1 << 23) || (int64_t)w * h > INT32_MAX)
        return refuse("w and h must be >= 1, with w + 2 and h + 2 < 2^23 (the 24-bit addressing limit) and w * h <= 2^31-1");
    const float radius = p->radius;
    const volatile float frv = cam->K[0] * radius;       // fl(K[0] * radius), one float32 product
    const float fr = frv;
    if (!(radius >= 0.0f && radius <= FLT_MAX)) return refuse("radius must be finite and >= 0");
    if (!(fr >= 0.0f && fr <= FLT_MAX)) return refuse("K[0] * radius must be finite and >= 0 in float32");
    if (p->max_px < 1 || p->max_px > 16) return refuse("max_px must be in 1..16");
    if (!(p->occlusion_diff >= 0.0f && p->occlusion_diff <= FLT_MAX)) return refuse("occlusion_diff must be finite and >= 0");
    if (!(p->depth_diff >= 0.0f && p->depth_diff <= FLT_MAX)) return refuse("depth_diff must be finite and >= 0");
    if (p->min_points < 1 || p->min_points > 255) return refuse("min_points must be in 1..255");
    if (p->max_splats < 0) return refuse("max_splats must be >= 0");
    for (int k = 0; k < 3; k++) {                         // P = K [R | t]: float64 products and sums of the float32 elements, rounded once
        const double k0 = cam->K[k * 3], k1 = cam->K[k * 3 + 1], k2 = cam->K[k * 3 + 2];
        for (int j = 0; j < 3; j++) vh->P[k * 4 + j] = (float)((k0 * (double)cam->R[j] + k1 * (double)cam->R[3 + j]) + k2 * (double)cam->R[6 + j]);
        vh->P[k * 4 + 3] = (float)((k0 * (double)cam->t[0] + k1 * (double)cam->t[1]) + k2 * (double)cam->t[2]);
    }
    vh->fr = radius > 0.0f ? fr : 0.0f;
    vh->foot = radius > 0.0f;
    vh->max_px = p->max_px;
    vh->w = w;
    vh->h = h;
    return TSAR_OK;
}

// Like tsar_cloud_distance_ctx: no views, no state, nothing of the context written, and a frame that does not grow the arena.
extern "C" int tsar_cloud_render_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_camera* cam, int w, int h, const tsar_cloud_render_params* p,
                                     float* depth_out, uint8_t* count_out, int32_t* index_out, int64_t* n_splats_out, int mem) {
    CHECK_CTX(ctx);
    CrViewHost vh;
    TRY(cloud_render_view(ctx, "tsar_cloud_render", cloud, n, stride, cam, w, h, p,
                          !depth_out && !count_out && !index_out ? "depth_out, count_out and index_out are all NULL" : nullptr, mem, &vh));
    CallFrame f(ctx, "tsar_cloud_render", nullptr, /*grow_arena=*/false);
    const size_t np = (size_t)w * h;
    const float* c = f.in(cloud, (size_t)n * stride, mem);
    float* dd = f.out(depth_out, np, mem);
    uint8_t* dc = f.out(count_out, np, mem);
    int32_t* di = f.out(index_out, np, mem);
    if (!f.ok()) return f.finish();
    return run_cloud_render(f, c, nullptr, n, stride, 0, vh, nullptr, p->occlusion_diff, p->depth_diff, p->min_points, p->max_splats, dd, dc, di, nullptr, n_splats_out, nullptr);
}

extern "C" int tsar_cloud_render(int device, const float* cloud, int64_t n, int stride, const tsar_camera* cam, int w, int h, const tsar_cloud_render_params* p,
                                 float* depth_out, uint8_t* count_out, int32_t* index_out, int64_t* n_splats_out, int mem) {
    return with_own_ctx(device, [&](tsar_ctx* ctx) { return tsar_cloud_render_ctx(ctx, cloud, n, stride, cam, w, h, p, depth_out, count_out, index_out, n_splats_out, mem); });
}

// The oriented occluder's host side (include/tsar.h): A = K R, M = A^-1 by cofactors and C = -R^T t in float64 from the float32 elements, each
// result rounded once.  false: A is singular, or an element of M or C is not finite.
static bool cloud_splat_view(const tsar_camera* cam, float radius, CsViewHost* sh) {
    double A[3][3], c[3][3];
    for (int k = 0; k < 3; k++)
        for (int j = 0; j < 3; j++)
            A[k][j] = (double)(float)(((double)cam->K[k * 3] * (double)cam->R[j] + (double)cam->K[k * 3 + 1] * (double)cam->R[3 + j]) +
                                      (double)cam->K[k * 3 + 2] * (double)cam->R[6 + j]);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
            c[i][j] = A[i1][j1] * A[i2][j2] - A[i1][j2] * A[i2][j1];
        }
    const double det = (A[0][0] * c[0][0] + A[0][1] * c[0][1]) + A[0][2] * c[0][2];
    if (det == 0.0) return false;
    bool finite = true;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            sh->M[j * 3 + i] = (float)(c[i][j] / det);
            finite = finite && fabsf(sh->M[j * 3 + i]) <= FLT_MAX;
        }
    for (int j = 0; j < 3; j++) {
        sh->C[j] = (float)-(((double)cam->R[j] * (double)cam->t[0] + (double)cam->R[3 + j] * (double)cam->t[1]) + (double)cam->R[6 + j] * (double)cam->t[2]);
        finite = finite && fabsf(sh->C[j]) <= FLT_MAX;
    }
    const volatile float r2v = radius * radius;          // fl(radius * radius), one float32 product
    sh->r2 = r2v;
    return finite;
}

// tsar_cloud_render_ctx with the normal-oriented occluder (the same driver of cloud_render_kernels.hip); the same frame rules.
extern "C" int tsar_cloud_render_oriented_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const float* normals, int normal_stride, const tsar_camera* cam,
                                              int w, int h, const tsar_cloud_render_params* p, float* depth_out, uint8_t* count_out, int32_t* index_out,
                                              float* occluder_out, int64_t* n_splats_out, int64_t* n_covered_out, int mem) {
    CHECK_CTX(ctx);
    CrViewHost vh;
    TRY(cloud_render_view(ctx, "tsar_cloud_render_oriented", cloud, n, stride, cam, w, h, p,
                          !depth_out && !count_out && !index_out && !occluder_out ? "depth_out, count_out, index_out and occluder_out are all NULL" : nullptr, mem, &vh));
    if (!normals && stride < 6)
        return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_render_oriented: normals is NULL, so the normal is the record's floats 3..5: the stride must be at least 6");
    if (normals && normal_stride < 3) return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_render_oriented: normal_stride must be at least 3 floats (the normal first)");
    CsViewHost sh;
    if (!cloud_splat_view(cam, p->radius, &sh))
        return fail(ctx, TSAR_ERR_INVALID, "tsar_cloud_render_oriented: K R is singular, or its inverse or the camera centre is not finite in float32");
    CallFrame f(ctx, "tsar_cloud_render_oriented", nullptr, /*grow_arena=*/false);
    const size_t np = (size_t)w * h;
    const float* c = f.in(cloud, (size_t)n * stride, mem);
    const float* nr = normals && n > 0 ? f.in(normals, (size_t)n * normal_stride, mem) : nullptr;
    float* dd = f.out(depth_out, np, mem);
    uint8_t* dc = f.out(count_out, np, mem);
    int32_t* di = f.out(index_out, np, mem);
    float* dz = f.out(occluder_out, np, mem);
    if (!f.ok()) return f.finish();
    // (n == 0: no lane reads a normal, and c may be null)
    return run_cloud_render(f, c, n > 0 ? (normals ? nr : c + 3) : nullptr, n, stride, normals ? normal_stride : stride, vh, &sh, p->occlusion_diff, p->depth_diff, p->min_points,
                            p->max_splats, dd, dc, di, dz, n_splats_out, n_covered_out);
}

extern "C" int tsar_cloud_render_oriented(int device, const float* cloud, int64_t n, int stride, const float* normals, int normal_stride, const tsar_camera* cam, int w, int h,
                                          const tsar_cloud_render_params* p, float* depth_out, uint8_t* count_out, int32_t* index_out, float* occluder_out,
                                          int64_t* n_splats_out, int64_t* n_covered_out, int mem) {
    return with_own_ctx(device, [&](tsar_ctx* ctx) {
        return tsar_cloud_render_oriented_ctx(ctx, cloud, n, stride, normals, normal_stride, cam, w, h, p, depth_out, count_out, index_out, occluder_out, n_splats_out,
                                              n_covered_out, mem);
    });
}

extern "C" int tsar_depth_compare_ctx(tsar_ctx* ctx, const float* depth, const float* gt, const uint8_t* mask, int64_t n, int n_tol, const float* tol, int64_t* n_gt_out,
                                      int64_t* n_both_out, int64_t* within_out, int64_t* n_front_out, int64_t* n_behind_out, float* error_out, int mem) {
    CHECK_CTX(ctx);
    TRY(check_clouds(ctx, "tsar_depth_compare", mem, {{depth, n, 3}, {gt, n, 3}}, "n", "", "depth or gt"));      // (maps: no stride to check)
    if (n_tol < 1 || n_tol > TSAR_DEPTH_COMPARE_MAX_TOL || !tol) return fail(ctx, TSAR_ERR_INVALID, "tsar_depth_compare: n_tol must be in 1..16, and tol not NULL");
    for (int k = 0; k < n_tol; k++)
        if (!(tol[k] >= 0.0f && tol[k] <= FLT_MAX)) return fail(ctx, TSAR_ERR_INVALID, "tsar_depth_compare: every tolerance must be finite and >= 0");
    CallFrame f(ctx, "tsar_depth_compare", nullptr, /*grow_arena=*/false);
    const float* d = f.in(depth, (size_t)n, mem);
    const float* g = f.in(gt, (size_t)n, mem);
    const uint8_t* m = f.in(mask, (size_t)n, mem);
    float* e = f.out(error_out, (size_t)n, mem);
    if (!f.ok()) return f.finish();
    unsigned long long counters[4 + TSAR_DEPTH_COMPARE_MAX_TOL] = {0};
    TRY(run_depth_compare(f, d, g, m, n, n_tol, tol, e, counters));
    if (n_gt_out) *n_gt_out = (int64_t)counters[0];
    if (n_both_out) *n_both_out = (int64_t)counters[1];
    if (n_front_out) *n_front_out = (int64_t)counters[2];
    if (n_behind_out) *n_behind_out = (int64_t)counters[3];
    for (int k = 0; k < n_tol && within_out; k++) within_out[k] = (int64_t)counters[4 + k];
    return TSAR_OK;
}

extern "C" int tsar_depth_compare(int device, const float* depth, const float* gt, const uint8_t* mask, int64_t n, int n_tol, const float* tol, int64_t* n_gt_out,
                                  int64_t* n_both_out, int64_t* within_out, int64_t* n_front_out, int64_t* n_behind_out, float* error_out, int mem) {
    return with_own_ctx(device, [&](tsar_ctx* ctx) {
        return tsar_depth_compare_ctx(ctx, depth, gt, mask, n, n_tol, tol, n_gt_out, n_both_out, within_out, n_front_out, n_behind_out, error_out, mem);
    });
}

extern "C" int tsar_depth_to_plane(tsar_ctx* ctx) {
    CHECK_CTX(ctx);
    NEED_STATE(ctx);
    ctx->costs_voided();
    TRY(launch_depth_to_plane(ctx));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}
extern "C" int tsar_get_result(tsar_ctx* ctx, float* depth, float* normal_world, float* cost, float* confid, int mem) {
    CHECK_CTX(ctx);
    NEED_STATE(ctx);
    if (!ctx->have_out) return fail(ctx, TSAR_ERR_STATE, "call tsar_compute_disp / tsar_fill_textureless first");
    const size_t np = (size_t)ctx->w * ctx->h;
    CallFrame f(ctx, __func__);
    float *dd = f.out(depth, np, mem), *dn = f.out(normal_world, 3 * np, mem);    // the result plane is split into maps of its own
    if ((depth || normal_world) && f.ok()) f.take(launch_split_out4(ctx, dd, dn));
    if (cost) f.copy(cost, ctx->buf[0].c, np * 4, kind_from_dev(mem));
    if (confid) f.copy(confid, ctx->confid, np * 4, kind_from_dev(mem));
    return f.finish();
}

// ---- TSAR refinement -----------------------------------------------------------------------------
extern "C" int tsar_set_reliable_mask(tsar_ctx* ctx, const float* scale, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (!scale) return fail(ctx, TSAR_ERR_INVALID, "scale is NULL");
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(ctx->scale, scale, (size_t)ctx->w * ctx->h * 4, kind_to_dev(mem), ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}
extern "C" int tsar_get_reliable_mask(tsar_ctx* ctx, float* scale, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (!scale) return fail(ctx, TSAR_ERR_INVALID, "scale is NULL");
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(scale, ctx->scale, (size_t)ctx->w * ctx->h * 4, kind_from_dev(mem), ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}
extern "C" int tsar_getview(tsar_ctx* ctx) {
    CHECK_CTX(ctx);
    NEED_STATE(ctx);
    TRY(launch_getview(ctx));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}
extern "C" int tsar_lrdiff(tsar_ctx* ctx) {
    CHECK_CTX(ctx);
    NEED_STATE(ctx);
    NEED_SOURCES(ctx);
    TRY(launch_lrdiff(ctx));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}
extern "C" int tsar_set_regions(tsar_ctx* ctx, const int32_t* labels, int n_regions, const float* region_text, const float* region_size, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    if (!labels || !region_text || n_regions < 1) return fail(ctx, TSAR_ERR_INVALID, "labels/region_text is NULL or n_regions < 1");
    const size_t np = (size_t)ctx->w * ctx->h;
    {
        // every label indexes the region tables in update_scale / fake_depth / the RANSAC kernels: check the range
        // before anything is installed (one pass; a bad label must give TSAR_ERR_INVALID, not a device fault)
        int32_t lo = 0, hi = 0;
        if (mem == TSAR_MEM_DEVICE) {
            TRY(launch_label_range(ctx, labels, np, &lo, &hi));
        } else {
            lo = hi = labels[0];
            for (size_t i = 1; i < np; i++) { lo = std::min(lo, labels[i]); hi = std::max(hi, labels[i]); }
        }
        if (lo < 0 || hi >= n_regions) return fail(ctx, TSAR_ERR_INVALID, "a label is outside [0, n_regions)");
    }
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(ctx->canny, labels, np * 4, kind_to_dev(mem), ctx->stream));
    TRY(install_regions(ctx, n_regions));
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(ctx->region_text, region_text, (size_t)n_regions * 4, kind_to_dev(mem), ctx->stream));
    if (region_size) TSAR_HIP_TRY(ctx, hipMemcpyAsync(ctx->region_size, region_size, (size_t)n_regions * 4, kind_to_dev(mem), ctx->stream));
    else TSAR_HIP_TRY(ctx, hipMemsetAsync(ctx->region_size, 0, (size_t)n_regions * 4, ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->n_regions = n_regions;
    return TSAR_OK;
}
extern "C" int tsar_set_region_planes(tsar_ctx* ctx, const float* region_planes) {
    CHECK_CTX(ctx);
    NEED_REGIONS(ctx);
    if (!region_planes) return fail(ctx, TSAR_ERR_INVALID, "region_planes is NULL");
    TSAR_HIP_TRY(ctx, hipMemcpyAsync(ctx->region_n4, region_planes, (size_t)ctx->n_regions * 16, hipMemcpyHostToDevice, ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}
extern "C" int tsar_fake_depth(tsar_ctx* ctx, float* fakedepth_out, int mem) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    NEED_REGIONS(ctx);
    TRY(launch_fake_depth(ctx));
    if (fakedepth_out) TSAR_HIP_TRY(ctx, hipMemcpyAsync(fakedepth_out, ctx->fakedepth, (size_t)ctx->w * ctx->h * 4, kind_from_dev(mem), ctx->stream));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return TSAR_OK;
}
extern "C" int tsar_fill_textureless(tsar_ctx* ctx) {   // gipuma_fill gipuma.cu:1819-1850
    CHECK_CTX(ctx);
    NEED_STATE(ctx);
    NEED_REGIONS(ctx);
    ctx->costs_voided();
    TRY(launch_update_scale(ctx));
    TRY(launch_compute_disp(ctx));
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->result_computed();
    return TSAR_OK;
}

// ---- pinned host buffers ---------------------------------------------------------------------------
// Host buffers handed to the library move over PCIe; from pageable memory the runtime stages them through its own
// bounce buffers (tsar_get_result of a 6048 x 4032 view: 51 ms), from page-locked memory the DMA engine reads / writes
// them directly.  The host side (tsar_gipuma, bench.py's host_boundary leg) allocates its image and result buffers here.
extern "C" void* tsar_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
extern "C" void tsar_host_free(void* p) {
    if (p) hipHostFree(p);
}

// ---- device buffers for a multi-GPU host (tsar_gipuma --all --fuse) -----------------------------------------
// One host process drives every GPU of the node (one worker thread + context per device).  Results that are to be fused
// stay on the device that produced them and travel to the fusing device directly over xGMI (peer copy) — the role the
// file system plays in the reference's per-view shell loop (scripts/courtyard.sh:29-48 -> Fusion.exe).  Inside one process
// a peer copy IS the point-to-point transfer a gather is made of; RCCL carries the same gather between the one-rank-per-GPU
// processes of bench.py (driver.gather_results).
extern "C" void* tsar_device_alloc(int device, size_t bytes) {
    void* p = nullptr;
    if (bytes == 0 || hipSetDevice(device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    return p;
}
extern "C" void tsar_device_free(int device, void* p) {
    if (p && hipSetDevice(device) == hipSuccess) hipFree(p);
}
extern "C" int tsar_device_write(int device, void* dst, const void* host_src, size_t bytes) {
    if (!dst || !host_src) return TSAR_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess || hipMemcpy(dst, host_src, bytes, hipMemcpyHostToDevice) != hipSuccess) return TSAR_ERR_HIP;
    return TSAR_OK;
}
extern "C" int tsar_device_read(int device, void* host_dst, const void* src, size_t bytes) {
    if (!host_dst || !src) return TSAR_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess || hipMemcpy(host_dst, src, bytes, hipMemcpyDeviceToHost) != hipSuccess) return TSAR_ERR_HIP;
    return TSAR_OK;
}
extern "C" int tsar_peer_copy(int dst_device, void* dst, int src_device, const void* src, size_t bytes) {
    if (!dst || !src) return TSAR_ERR_INVALID;
    if (hipSetDevice(dst_device) != hipSuccess) return TSAR_ERR_HIP;
    if (dst_device != src_device) {
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, dst_device, src_device) == hipSuccess && can) {
            const hipError_t e = hipDeviceEnablePeerAccess(src_device, 0);
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) return TSAR_ERR_HIP;
            (void)hipGetLastError();
        }
    }
    if (hipMemcpyPeer(dst, dst_device, src, src_device, bytes) != hipSuccess) return TSAR_ERR_HIP;   // synchronous: complete on return
    return TSAR_OK;
}

// ---- measurement ---------------------------------------------------------------------------------
extern "C" int tsar_enable_kernel_timing(tsar_ctx* ctx, int enable) {
    if (!ctx) return TSAR_ERR_INVALID;
    ctx->timing = enable != 0;
    return TSAR_OK;
}
extern "C" int tsar_reset_kernel_timing(tsar_ctx* ctx) {
    CHECK_CTX(ctx);
    hipStreamSynchronize(ctx->stream);
    drain_timers(ctx);
    ctx->timers.clear();
    return TSAR_OK;
}
extern "C" int tsar_get_kernel_timing(tsar_ctx* ctx, tsar_kernel_timing* out, int cap, int* n_out) {
    CHECK_CTX(ctx);
    if (!n_out) return fail(ctx, TSAR_ERR_INVALID, "n_out is NULL");
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    drain_timers(ctx);
    *n_out = (int)ctx->timers.size();
    for (int i = 0; i < *n_out && i < cap && out; i++) {
        memset(&out[i], 0, sizeof(out[i]));
        strncpy(out[i].name, ctx->timers[i].name.c_str(), sizeof(out[i].name) - 1);
        out[i].launches = ctx->timers[i].launches;
        out[i].total_ms = ctx->timers[i].total_ms;
    }
    return TSAR_OK;
}

// ---- self-tests (selftest_kernels.hip) ---------------------------------------------------------------------------------------
extern "C" int tsar_selftest_divide(tsar_ctx* ctx, const float* X, const float* Y, const float* Z, size_t n, float* u_out, float* v_out, int ieee) {
    CHECK_CTX(ctx);
    if (!X || !Y || !Z || !u_out || !v_out || n == 0 || n > ((size_t)1 << 28)) return fail(ctx, TSAR_ERR_INVALID, "NULL argument or n out of range (1..2^28)");
    CallFrame f(ctx, __func__);
    const float *x = f.in(X, n, TSAR_MEM_HOST), *y = f.in(Y, n, TSAR_MEM_HOST), *z = f.in(Z, n, TSAR_MEM_HOST);
    float *u = f.out(u_out, n, TSAR_MEM_HOST), *v = f.out(v_out, n, TSAR_MEM_HOST);
    if (f.ok()) f.take(launch_selftest_divide(ctx, x, y, z, n, u, v, ieee));
    return f.finish();
}
// The counter self-tests: n zeroed 64-bit device counters from the scratch arena, launch(counters), the counters copied to out[n].
template <typename Launch>
static int run_counters(tsar_ctx* ctx, int n, uint64_t* out, Launch launch) {
    CallFrame f(ctx, __func__);
    unsigned long long* dc = f.out((unsigned long long*)out, (size_t)n, TSAR_MEM_HOST);
    f.zero(dc, (size_t)n * sizeof(unsigned long long));
    if (f.ok()) f.take(launch(dc));
    return f.finish();
}
extern "C" int tsar_selftest_divide_random(tsar_ctx* ctx, int log2_triples, uint64_t seed, int mode, int guarded, uint64_t* mismatches_out,
                                           uint64_t* outside_guard_out) {
    CHECK_CTX(ctx);
    if (log2_triples < 6 || log2_triples > 36 || mode < 0 || mode > 2 || !mismatches_out) return fail(ctx, TSAR_ERR_INVALID, "log2_triples in 6..36, mode in 0..2");
    if (!guarded && mode == 2) return fail(ctx, TSAR_ERR_INVALID, "the unguarded form is only defined inside the guard (modes 0, 1)");
    uint64_t hc[2] = {0, 0};
    const int rc = run_counters(ctx, 2, hc, [&](unsigned long long* dc) {
        // launches of 2^30 triples at most (~0.1 s each)
        int rc = TSAR_OK;
        for (int done = 0; rc == TSAR_OK && done < (1 << (log2_triples > 30 ? log2_triples - 30 : 0)); done++)
            rc = launch_selftest_divide_random(ctx, log2_triples > 30 ? 30 : log2_triples, seed + 0x9E3779B97F4A7C15ull * (uint64_t)done, mode, guarded, dc);
        return rc;
    });
    *mismatches_out = hc[0];
    if (outside_guard_out) *outside_guard_out = hc[1];
    return rc;
}
extern "C" int tsar_selftest_sqrt(tsar_ctx* ctx, int mode, uint64_t seed, uint64_t* mismatches_out) {
    CHECK_CTX(ctx);
    if (mode < 0 || mode > 3 || !mismatches_out) return fail(ctx, TSAR_ERR_INVALID, "mode in 0..3");
    uint64_t hc = 0;
    const int rc = run_counters(ctx, 1, &hc, [&](unsigned long long* dc) { return launch_selftest_sqrt(ctx, mode, seed, dc); });
    *mismatches_out = hc;
    return rc;
}
int launch_sweep_repeat(tsar_ctx* ctx, int colour, unsigned long long* memo, unsigned long long* dout);
extern "C" int tsar_selftest_sweep_repeat(tsar_ctx* ctx, int colour, void* memo_dev, uint64_t* out8) {
    CHECK_CTX(ctx);
    if (!memo_dev || !out8) return fail(ctx, TSAR_ERR_INVALID, "memo_dev / out8 is NULL");
    NEED_VIEWS(ctx);
    NEED_STATE(ctx);
    return run_counters(ctx, 8, out8, [&](unsigned long long* dc) { return launch_sweep_repeat(ctx, colour & 1, (unsigned long long*)memo_dev, dc); });
}
extern "C" int tsar_selftest_sweep_census(tsar_ctx* ctx, int colour, uint64_t* out8) {
    CHECK_CTX(ctx);
    NEED_VIEWS(ctx);
    NEED_STATE(ctx);
    if (!out8) return fail(ctx, TSAR_ERR_INVALID, "out8 is NULL");
    return run_counters(ctx, 8, out8, [&](unsigned long long* dc) { return launch_sweep_census(ctx, colour & 1, dc); });
}
// Counters of the pruning kernels (pm_sweep_impl.h pruned_cost): on = 1 zeroes them and makes every following sweep launch of this
// context count; on = 0 hands them back (out32 may be NULL) and stops the counting.
extern "C" int tsar_selftest_prune_census(tsar_ctx* ctx, int on, uint32_t* out32) {
    CHECK_CTX(ctx);
    TSAR_HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (on) {
        if (!ctx->prune_counts) TSAR_HIP_TRY(ctx, hipMalloc((void**)&ctx->prune_counts, 32 * sizeof(uint32_t)));
        TSAR_HIP_TRY(ctx, hipMemset(ctx->prune_counts, 0, 32 * sizeof(uint32_t)));
        return TSAR_OK;
    }
    if (!ctx->prune_counts) return fail(ctx, TSAR_ERR_INVALID, "no prune census is running");
    if (out32) TSAR_HIP_TRY(ctx, hipMemcpy(out32, ctx->prune_counts, 32 * sizeof(uint32_t), hipMemcpyDeviceToHost));
    TSAR_HIP_TRY(ctx, hipFree(ctx->prune_counts));
    ctx->prune_counts = nullptr;
    return TSAR_OK;
}
