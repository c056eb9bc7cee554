// tsar_dev.h — device-visible scene description and the host context behind include/tsar.h.
// gfx950 only; no CUDA / multi-backend paths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/tsar.h"

#define TSAR_LUT_LINES 32         // box <= 63: at most 32 lines of at most 32 taps
#define TSAR_LUT_TAPS 40          // 32 rounded up to whole chunks of 4 / 5 / 6 taps, plus slack
#define TSAR_LUT_MAX_CLASSES 144  // (rows + 1) KiB of LDS: what fits beside the reference window in 160 KiB
#define TSAR_MAX_SELECTED 32   // views scored per hypothesis: the reference's costVector[32] (gipuma.cu:467-468)

// One source view as the kernels read it: pose relative to the reference camera (ref = K[I|0]),
// reference cameraGeometryUtils.h:270-302 / camera.h:9-33.
struct DevView {
    float K[9];
    float R[9];
    float t[3];
    float t_abs_lo;          // min |t[r]|, max |t[r]|: bounds of the nine products t[r] n[c] of the strict homography's operand guard
    float A[9];              // K R K_ref^-1  (fast-mode homography H = A - b m^T, m = K_ref^-T n / d)
    float b[3];              // K t
    float t_abs_hi;
    const float* img;        // [h][w] float gray
    const uint32_t* quad;    // [(h+2)][(w+2)] packed 2x2 texel quads (8-bit images only), see plane_kernels.hip build_quad_kernel
    const uint2* dquad;      // [(h+2)][(w+2)] the same quads as four halfs (t00, t10 - t00, t01 - t00, t11 - t10 - t01 + t00): fast mode's converged sweeps (pm_tap_r5.h MIX), else null
};

// Reference camera block (camera.h:9-33 for cameras[REFERENCE]).
struct DevRef {
    float K[9];
    float Kinv[9];
    float Minv[9];
    float Rorig[9];
    float RorigInv[9];
    float P34[3];
    float C[3];
    float fx, f, alpha, baseline, depthMin, depthMax;
};

// Everything a kernel needs besides the state planes.  Lives in device memory; every field is
// wave-uniform, so reads become scalar loads.
struct DevScene {
    int w, h;
    int n_sel;                 // viewSelectionSubsetNumber
    int hrad, vrad;            // (box-1)/2, gipuma.cu:858-859
    int n_best, cost_comb;
    int refine_steps;          // iterations of the deltaZ loop, gipuma.cu:644
    int quad_pitch;            // w + 2
    int use_quad;              // all views are integral 0..255 -> 1-load bilinear taps
    float min_disp, max_disp;
    uint32_t flags;
    uint32_t seed_lo, seed_hi;
    int k_sparse;              // every view's K is (fx 0 cx; 0 fy cy; 0 0 1) and K_ref^-1 has the same zero / one pattern (no skew):
                               // the strict homography then skips the products with those zeros (plane_homography, tsar_device_math.h)
    DevRef ref;
    int sel[TSAR_MAX_VIEWS];   // view indices in pair.txt order
    DevView view[TSAR_MAX_VIEWS];
    // Shared weight table of the general-window tap loop (pm_core_lut.h view_cost_lut; 8-bit imagery): the bilateral weight
    // exp(-sqrt(i^2 + j^2) / 50 - |r - centre| / 18) of a tap depends on its distance class (the distinct i^2 + j^2 of the
    // window) and on an integer 0..255, so a workgroup keeps one 256-entry row per class in LDS instead of S weights per thread.
    int lut_classes;                               // rows of the table; row lut_classes is all zero (padding taps of a line's last chunk)
    int lut_row_major;                             // 1: lines of the walk are window rows (fast mode), 0: window columns (the oracle's order)
    int lut_chunk;                                 // taps per chunk of a line: 4, 5 or 6 (the fewest padding slots)
    int lut_pad_taps;                              // taps per line rounded up to whole chunks: the stride of tap_row
    int lut_d2[TSAR_LUT_MAX_CLASSES];              // i^2 + j^2 per class
    uint32_t tap_row[TSAR_LUT_LINES * TSAR_LUT_TAPS + 8];   // [line * lut_pad_taps + tap of the line] -> byte offset of the tap's row in the
                                                   // table (padding slots -> the zero row); chunks are consecutive: a walk reads it linearly
    // Geometric-consistency term (include/tsar.h tsar_set_geom_depths; pm_core.h geom_term).  Appended last so that no field above
    // moves: the kernels without the term (variant bit 24 clear) compile to the same code as before it existed.
    const float* geom_depth[TSAR_MAX_VIEWS];       // view v's depth map [h][w] in its own camera (device, owned by the context); null = no term
    float geom_back[TSAR_MAX_VIEWS][12];           // [K_ref R^T K_v^-1 | -K_ref R^T t]: (c D_v, r D_v, D_v, 1) -> reference image (derive_cameras)
    float geom_weight, geom_clip, geom_clip_sq;    // lambda, tau, tau * tau
    int geom_on;                                   // a term is installed: the launchers pick the variant-bit-24 kernels
    // Plane-prior term (include/tsar.h tsar_set_plane_prior; pm_core.h prior_term), carried by the same variant-bit-24 kernels.
    const float4* prior;                           // [h][w] (q in reference-camera coordinates, Dp), all zero = no prior there (device, owned); null = no term
    float prior_weight_depth, prior_weight_normal, prior_depth_clip, prior_normal_clip;
};
// the launchers pick the variant-bit-24 kernels: a geometric term, a plane prior or both (a prior alone runs them with every map null)
static inline bool scene_has_terms(const DevScene& s) { return s.geom_on != 0 || s.prior != nullptr; }

// Variant bits of the tap loops beside the box-11 loop's own numbers (114 / 122 / 250, pm_tap_r5.h)
#define TSAR_V_LUT 1024           // bit 10: the general-window loop, weights from the shared table (pm_core_lut.h; chunk length in bits 11-13)
#define TSAR_V_BUF 131072         // bit 17: gathers as structured buffer loads (pm_tap_r5.h BUF)
#define TSAR_V_MIX 2097152        // bit 21, with TSAR_V_BUF: gathers from the half-float difference texture (pm_tap_r5.h MIX)
// Variant bits of the geometric-consistency kernels (the remaining bits name the tap loop as before)
#define TSAR_V_GEOM 16777216      // bit 24: multiview_cost adds lambda e to each view's cost (pm_core.h geom_term) and the plane-prior term to the result (add_prior_term)
#define TSAR_V_PRUNE 67108864     // bit 26, with 250 and its BUF / MIX forms, sweep only: wide refinement steps leave a view the partial-window bound proves rejected (pm_tap_r5.h PRUNE)
#define TSAR_V_PAIR 134217728     // bit 27, with 250 alone (pm_pair.hip): one 16-byte gather per pair of row taps (pm_tap_r5.h PAIR)
#define TSAR_V_RING 268435456     // bit 28, with 250 | TSAR_V_BUF | TSAR_V_MIX and its TSAR_V_PRUNE form, sweep only (pm_ring.hip): the unrolled clamp-free walk keeps six gathers in flight across a view's lines (pm_tap_r5.h RING)
#define TSAR_V_REDRAW 33554432    // bit 25, with INIT: pm_full_kernel keeps the given plane where it is a valid hypothesis (tsar_pm_rescore)

// State planes of one ping-pong buffer (linestate.h:12-13).
struct PlaneBuf {
    float* c;       // [h][w]
    float4* n4;     // [h][w] (n_x, n_y, n_z, d), n.X + d = 0 in reference-camera coordinates
};

struct KernelTimer {
    std::string name;
    int launches = 0;
    float total_ms = 0.f;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
};

// Device scratch of the calls that need temporaries or stage host buffers (CallFrame below; DESIGN.md lists them): one arena per
// context, grown to the largest call seen and kept, so that a worker refining view after view (tsar_gipuma --all --mode=tsar) does
// not pay ~18 hipMalloc + hipFree per operator and view (26 of the 59 ms of a RANSAC call at 24 MP were these).
struct ScratchArena {
    char* base = nullptr;
    size_t cap = 0;
    size_t wanted = 0;      // the largest call that did not fit so far: the arena is (re)built the second time one overflows, so a
                            // context that makes each call once (one view per process) never pays for an arena it would not reuse
};

struct tsar_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    tsar_params params{};
    bool have_params = false, have_views = false, have_state = false;
    int w = 0, h = 0, n_views = 0;
    DevScene hscene{};          // host copy
    DevScene* dscene = nullptr;  // device copy
    std::vector<float*> img;     // device images (owned)
    std::vector<uint32_t*> quad;
    std::vector<uint2*> dquad;   // half-float difference textures (fast mode, box-11 loop, buffer gathers), see DevView
    PlaneBuf buf[2]{};           // buf[0] is the canonical state outside tsar_pm_iterate
    float *ratio = nullptr, *depth = nullptr, *scale = nullptr, *lrdiff = nullptr, *confid = nullptr, *fakedepth = nullptr;
    int32_t *beview = nullptr, *canny = nullptr;
    float4* out4 = nullptr;      // result of compute_disp: (n_world, depth)
    bool have_out = false;
    // c[p] is the score of n4[p] under the context's current cost (views, subset, sweep window, geometric term) for every pixel: the
    // sweep then skips a neighbour that carries the pixel's own plane (pm_sweep_impl.h same_bits).  Left standing over a cost that is
    // not its plane's score, it makes the sweep skip what the reference scores and may accept.  Read by the sweep launcher and the
    // sweep census self-tests, all behind NEED_STATE, and written by both transitions that create a state: voiding needs no guard.
    bool cost_consistent = false;
    // regions (cannylines)
    int n_regions = 0;
    float *region_text = nullptr, *region_size = nullptr;
    float4* region_n4 = nullptr;
    int exact_sqrt_probe = 0;    // the cost tail's square root (sqrt_rsq_exact) on THIS device: 0 not probed yet, 1 holds, -1 failed
    int exact_div_probe = 0;     // strict mode's short exact division on THIS device: 0 not probed yet, 1 holds, -1 failed (probe_exact_divide)
    int sweeps_done = 0;         // RNG stream counter
    // Propagation memo (pm_sweep_impl.h SweepMemo): per pixel the eight candidates of its previous propagation launch, the number of
    // that launch, and the number of the last launch that changed the pixel's plane.  A candidate that is the same neighbour as last
    // time, with a plane unchanged since, was scored at this pixel then and rejected (or taken and since improved on): the pixel's cost
    // never rises, so it is rejected again and need not be scored — the reference's results, bit for bit, with fewer evaluations.
    // Valid among the launches of ONE sweep call only (tsar_pm_iterate, tsar_pm_iterate_final, tsar_pm_sweep; nothing else touches
    // the state in between): pm_sweeps (tsar_api.hip) voids it at the start of every call, and is the only writer of memo_valid_from
    // and the only allocator of the three buffers, which exist all or none (memo_cand non-null means all three do).
    int32_t* memo_cand = nullptr;     // [h][w][8]
    uint32_t* memo_seq = nullptr;     // [h][w]
    uint32_t* changed_seq = nullptr;  // [h][w]
    uint32_t launch_seq = 0;          // sweep launches of this context so far (never reset)
    uint32_t memo_valid_from = 1;     // memos written before this launch are void (read by launch_sweep_t, pm_sweep_impl.h)
    int call_launch = 0;              // launches since the current sweep call began
    int memo_mode = 1;                // TSAR_MEMO=0: off
    int compact_from = 6;             // TSAR_COMPACT_FROM=n (-1: never): from launch n of a call on, a wave packs its surviving hypotheses (pm_sweep_impl.h)
    // Partial-window pruning of the wide refinement steps (pm_tap_r5.h PRUNE; fast mode, best view only, no geometric / prior term)
    int prune = 1;                    // TSAR_PRUNE=0: off (the kernels without the check)
    int prune_steps = 2;              // TSAR_PRUNE_STEPS=n: refinement steps 0 .. n - 1 are checked
    int prune_from = 1;               // TSAR_PRUNE_FROM=n: from launch n of a call on
    // Paired gathers in the random-plane launches (pm_pair.hip, pm_tap_r5.h PAIR): TSAR_PAIR=0 neither, 1 the initialisation, 2 the
    // first sweep of a run (the plain global-load launches), 3 both
    int pair = 3;
    // The ring form of the difference-texture launches' unrolled walk (pm_ring.hip, pm_tap_r5.h RING): TSAR_RING=0 never, n >= 1 from
    // sweep n of a run on (1: every difference-texture launch).  Measured per launch (profiles/ring): sweep 1, whose planes have seen one
    // sweep and are still unrelated between neighbouring lanes, loses 5 ms to the ring (a row's six gathers no longer reach L1 together),
    // sweep 2 0.35 ms; every later one gains 0.3 - 1 ms.
    int ring = 3;
    uint32_t* prune_counts = nullptr; // tsar_selftest_prune_census: device counters while a census runs, else null
    // coarse-to-fine mode (tsar_pyramid_views / tsar_upsample_planes)
    std::vector<tsar_camera> cams;    // the cameras tsar_set_views was given (before cam_scale), from which a coarser level derives its own
    bool views_u8 = false;            // the views came through tsar_set_views_u8 (a coarser level is then an 8-bit decode too)
    float4* resize4 = nullptr;        // [h][w] the planes the last tsar_upsample_planes chose (the reference's lines->resize4, linestate.h:64)
    bool have_resize = false;
    const float* final_text = nullptr;   // device lines->text while tsar_pm_iterate_final runs (the kernels' `final` mode), else null
    // geometric consistency (tsar_set_geom_depths): the source views' depth maps, owned; hscene.geom_depth points into them
    std::vector<float*> geom_maps;
    // plane prior (tsar_set_plane_prior): owned; hscene.prior is this pointer while a prior is installed
    float4* prior = nullptr;
    // timing
    int variant = 2;             // TSAR_VARIANT=n: code-generation variant of the fast-mode tap loop (pm_tap_r5.h view_cost_r5); tsar_create picks 250 (med3/fract + D16 window loads + clamp-free loop for in-image windows + wave priority + SGPR-pinned texture base and line-top weight loads + row-wise window walk in fast mode; strict mode runs it as 122, the oracle's column order) when the D16 probe passes, else 114
    bool mix_gather = true;      // TSAR_MIX_GATHER=0: keep the byte texture for the buffer-load launches too (pm_tap_r5.h MIX off)
    bool buffer_gather = true;   // TSAR_BUFFER_GATHER=0: the fast tap loop's gathers as global loads + a shift instead of structured buffer loads
    int strip_w = -1;            // TSAR_STRIP=n: width in tiles of the strips the sweep walks (pm_core.h strip_tile), 0 = row-major,
                                 // -1 = automatic: one vertical band of the image per XCD (see strip_width)
    // The remaining environment knobs (DESIGN.md §4 lists them all).  Everything is read ONCE, by tsar_create (tsar_api.hip
    // read_knobs): a context never looks at the environment again, and no knob is latched in a function-local static.
    int buffer_from = 1;         // TSAR_BUFFER_FROM=n: fast mode's sweeps use buffer-load gathers on the difference texture from sweep n of a run on (default 1: only the first sweep, whose planes are random, keeps global loads on the byte texture; measured 0 / 1 / 2 -> 37.19 / 35.33 / 35.44 ms mean sweep, profiles/r04); strict mode from max(n, 2)
    int force_block = 0;         // TSAR_BLOCK=128|256: force the sweep's workgroup shape (0: by image size, SWEEP_SMALL_IMAGE_TILES)
    int lut_mode = 1;            // TSAR_LUT=0: one-tap loop for windows other than box 11; 2: box 11 through the general-window loop too
    int ransac_wgs = 8;          // TSAR_RANSAC_WGS: workgroups per region in RANSAC stage 2 (1 = the single-workgroup kernel)
    int ransac_chain = 8;        // TSAR_RANSAC_CHAIN=4|8|16: speculative steps per pass
    int ransac_lookahead = 0;    // TSAR_RANSAC_LOOKAHEAD=1|2|3: the history-tree kernel instead of the chain
    int ransac_poll_limit = 1 << 15;      // TSAR_RANSAC_POLL_LIMIT: polls (~0.3 us each) before a stage-2 workgroup gives up waiting
    bool ransac_cooperative = true;       // TSAR_RANSAC_COOPERATIVE=0: plain launch of the multi-workgroup stage 2
    bool ransac_force_fallback = false;   // TSAR_RANSAC_FORCE_FALLBACK=1: pre-set the give-up flag (tests of that path)
    bool trace_host = false;     // TSAR_TRACE_HOST=1: host-side steps of the refinement operators on stderr
    bool render_skip = true;     // TSAR_RENDER_SKIP=0: tsar_cloud_render[_oriented]'s footprint loop issues every minimum, without the plain load that lets a lane skip one
#ifdef TSAR_EXPERIMENTS
    size_t lds_pad = 0;          // TSAR_LDS_PAD=n: unused LDS per sweep workgroup (occupancy experiments)
#endif
    bool timing = false;
    std::vector<KernelTimer> timers;
    ScratchArena scratch;

    // ---- what a call does to the plane state: the only writers of have_state, have_out, cost_consistent and sweeps_done (beside
    // pm_sweeps' count and tsar_set_sweep_counter) ----
    // a state whose costs are its planes' scores (init, rescore, upsampling, merge); `consistent`: scored on the sweeps' window (false
    // only for tsar_pm_init on an even box, whose window is one tap ring larger).  The sweeps that follow draw like the first ones.
    void state_scored(bool consistent) { have_state = true; have_out = false; sweeps_done = 0; cost_consistent = consistent; }
    // a state the caller gave (planes with any costs): the sweep counter runs on
    void state_given() { have_state = true; have_out = false; cost_consistent = false; }
    // the stored costs are no longer the planes' scores: the cost changed (view subset, geometric term) or planes were rewritten
    void costs_voided() { cost_consistent = false; }
    // the result buffer (out4) follows / no longer follows the planes
    void result_computed() { have_out = true; }
    void result_voided() { have_out = false; }
    // new parameters or new views: nothing derived from the previous views stands
    void views_reset() { have_views = have_state = have_out = have_resize = false; }
};

// ---- entry guards of the C ABI (every extern "C" function that takes a context) ------------------------------------------------
static inline int fail(tsar_ctx* ctx, int code, const char* msg) { if (ctx) ctx->err = msg; return code; }
static inline int enter_ctx(tsar_ctx* ctx) {   // the calling thread works on the context's device from here on
    if (!ctx) return TSAR_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return fail(ctx, TSAR_ERR_HIP, "hipSetDevice failed");
    return TSAR_OK;
}
#define CHECK_CTX(ctx) TRY(enter_ctx(ctx))
#define NEED_VIEWS(ctx) if (!(ctx)->have_views) return fail(ctx, TSAR_ERR_STATE, "tsar_set_views has not been called")
// matching scores planes against source views; a context holding the reference view only serves the textureless-refinement
// operators (load_planes, weak-texture detection, region RANSAC, fill)
#define NEED_SOURCES(ctx) if ((ctx)->hscene.n_sel < 1) return fail(ctx, TSAR_ERR_STATE, "no source views: tsar_set_views was given the reference view only")
#define NEED_STATE(ctx) if (!(ctx)->have_state) return fail(ctx, TSAR_ERR_STATE, "no plane state: call tsar_pm_init, tsar_load_planes or tsar_set_plane first")
#define NEED_REGIONS(ctx) if ((ctx)->n_regions < 1) return fail(ctx, TSAR_ERR_STATE, "tsar_set_regions has not been called")
#define TRY(expr) do { int rc_ = (expr); if (rc_ != TSAR_OK) return rc_; } while (0)

template <typename T>
static int dev_alloc(tsar_ctx* ctx, T** p, size_t n) {
    if (*p) { hipFree(*p); *p = nullptr; }
    hipError_t e = hipMalloc((void**)p, n * sizeof(T));
    if (e != hipSuccess) { ctx->err = std::string("hipMalloc: ") + hipGetErrorString(e); return e == hipErrorOutOfMemory ? TSAR_ERR_NOMEM : TSAR_ERR_HIP; }
    return TSAR_OK;
}
// A device buffer that lives for one call: freed on every exit path unless release()d to a longer-lived owner.  (hipFree waits
// for the device, so work still queued on the buffer is complete before it goes.)
template <typename T>
struct DevTmp {
    T* p = nullptr;
    DevTmp() = default;
    DevTmp(const DevTmp&) = delete;
    DevTmp& operator=(const DevTmp&) = delete;
    ~DevTmp() { if (p) hipFree(p); }
    int alloc(tsar_ctx* ctx, size_t n) { return dev_alloc(ctx, &p, n); }
    T* release() { T* q = p; p = nullptr; return q; }
};

// One call's view of the arena: alloc() hands out 256-byte-aligned pieces; what does not fit is a plain hipMalloc for this call;
// the second time a call overflows, the arena is re-sized to the largest total seen, and calls of that size allocate nothing from
// then on.  grow = false: a call that must not grow what the context keeps (diagnostics, the few bytes of a probe) uses the arena
// space that is there and leaves `wanted` and the arena alone.
struct ScratchScope {
    tsar_ctx* ctx;
    bool grow;
    size_t used = 0, need = 0;
    std::vector<void*> extra;
    explicit ScratchScope(tsar_ctx* c, bool grow_arena = true) : ctx(c), grow(grow_arena) {}
    void* alloc(size_t bytes) {
        bytes = ((bytes ? bytes : 4) + 255) & ~(size_t)255;
        need += bytes;
        if (used + bytes <= ctx->scratch.cap) { void* p = ctx->scratch.base + used; used += bytes; return p; }
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
        extra.push_back(p);
        return p;
    }
    void release() {                       // the stream is idle (CallFrame synchronises first)
        for (void* p : extra) hipFree(p);
        extra.clear();
        if (grow && need > ctx->scratch.cap) {
            const bool again = ctx->scratch.wanted > ctx->scratch.cap;          // an earlier call overflowed this arena too
            if (need > ctx->scratch.wanted) ctx->scratch.wanted = need;
            if (again) {
                if (ctx->scratch.base) hipFree(ctx->scratch.base);
                ctx->scratch.base = nullptr;
                ctx->scratch.cap = 0;
                void* p = nullptr;
                if (hipMalloc(&p, ctx->scratch.wanted) == hipSuccess) { ctx->scratch.base = (char*)p; ctx->scratch.cap = ctx->scratch.wanted; }
            }
        }
        used = need = 0;
    }
    ~ScratchScope() { release(); }
};

// where a caller's buffer lies decides the kind of a copy to / from a context buffer
static inline hipMemcpyKind copy_kind(int mem, hipMemcpyKind host_kind) { return mem == TSAR_MEM_DEVICE ? hipMemcpyDeviceToDevice : host_kind; }
static inline hipMemcpyKind kind_to_dev(int mem) { return copy_kind(mem, hipMemcpyHostToDevice); }
static inline hipMemcpyKind kind_from_dev(int mem) { return copy_kind(mem, hipMemcpyDeviceToHost); }

// One ABI call's frame, created after the guards: its pieces of the arena, device views of the caller's buffers, a sticky status
// and the way out.  The first failure is recorded with its message; every later operation on a failed frame does nothing, so a
// function takes its pieces, queues its copies and looks at ok() once before it launches.  finish() (or the destructor, on an
// early return) synchronises the stream and releases the pieces: every exit leaves an idle stream and a released scope.
struct CallFrame {
    tsar_ctx* ctx;
    const char* entry;                     // names the call in allocation and HIP failure messages
    const char* tag;                       // "[ransac]": trace() lines on stderr when TSAR_TRACE_HOST is set, else null
    ScratchScope scratch;
    int rc = TSAR_OK;
    bool closed = false;
    struct Back { void* dst; const void* src; size_t bytes; };
    std::vector<Back> back;                // staged outputs that finish() copies to the caller's host buffers
    std::chrono::steady_clock::time_point t0;
    CallFrame(tsar_ctx* c, const char* entry_name, const char* trace_tag = nullptr, bool grow_arena = true)
        : ctx(c), entry(entry_name), tag(c->trace_host ? trace_tag : nullptr), scratch(c, grow_arena), t0(std::chrono::steady_clock::now()) {}
    CallFrame(const CallFrame&) = delete;
    CallFrame& operator=(const CallFrame&) = delete;
    ~CallFrame() { close(); }

    bool ok() const { return rc == TSAR_OK; }
    int fail(int code, const std::string& msg) { if (ok()) { rc = code; ctx->err = msg; } return rc; }
    void take(int code) { if (ok()) rc = code; }                      // a launcher's status (which has left its message in ctx->err)
    bool hip(hipError_t e, const char* what) {                          // as TSAR_HIP_TRY: TSAR_ERR_HIP with the name of the failing call
        if (e != hipSuccess) fail(TSAR_ERR_HIP, std::string(entry) + ": " + what + ": " + hipGetErrorString(e));
        return ok();
    }
    template <typename T>
    T* tmp(size_t n) {                                                  // a piece of the arena for this call
        if (!ok()) return nullptr;
        T* p = (T*)scratch.alloc(n * sizeof(T));
        if (!p) fail(TSAR_ERR_NOMEM, std::string(entry) + ": device allocation failed");
        return p;
    }
    template <typename T>
    const T* in(const T* src, size_t n, int mem) {                      // device view of a caller's input: host buffers are copied in
        if (!src || mem == TSAR_MEM_DEVICE) return src;
        T* d = tmp<T>(n);
        copy(d, src, n * sizeof(T), hipMemcpyHostToDevice);
        return d;
    }
    template <typename T>
    T* out(T* dst, size_t n, int mem) {                                 // device view of a caller's output: finish() fills host buffers
        if (!dst || mem == TSAR_MEM_DEVICE) return dst;
        T* d = tmp<T>(n);
        if (d) back.push_back({dst, d, n * sizeof(T)});
        return d;
    }
    void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        if (ok() && bytes) hip(hipMemcpyAsync(dst, src, bytes, kind, ctx->stream), "hipMemcpyAsync");
    }
    void zero(void* p, size_t bytes) {
        if (ok() && bytes) hip(hipMemsetAsync(p, 0, bytes, ctx->stream), "hipMemsetAsync");
    }
    bool launched() { return ok() && hip(hipGetLastError(), "kernel launch"); }
    bool sync() { return ok() && hip(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"); }   // where the host reads a value mid-call
    void trace(const char* what) {
        if (!tag) return;
        hipStreamSynchronize(ctx->stream);
        const auto n = std::chrono::steady_clock::now();
        fprintf(stderr, "%s %s %.3f ms\n", tag, what, std::chrono::duration<double, std::milli>(n - t0).count());
        t0 = n;
    }
    int finish() {                                                      // copy-backs only if all went well; one synchronise
        if (!closed)
            for (const Back& b : back) copy(b.dst, b.src, b.bytes, hipMemcpyDeviceToHost);
        close();
        return rc;
    }
    void close() {
        if (closed) return;
        closed = true;
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        hip(e, "hipStreamSynchronize");
        scratch.release();
    }
};

#define TSAR_HIP_TRY(ctx, expr)                                                                       \
    do {                                                                                              \
        hipError_t e_ = (expr);                                                                       \
        if (e_ != hipSuccess) {                                                                       \
            (ctx)->err = std::string(#expr) + ": " + hipGetErrorString(e_);                           \
            return TSAR_ERR_HIP;                                                                      \
        }                                                                                             \
    } while (0)

// The region tables (text, size, planes; n entries each), installed by tsar_set_regions and tsar_detect_weak_texture.  n_regions is
// 0 from before anything is freed until the caller, having filled the tables, sets it: a failure on the way leaves a context that
// NEED_REGIONS refuses.
static inline int install_regions(tsar_ctx* ctx, int n) {
    ctx->n_regions = 0;
    TRY(dev_alloc(ctx, &ctx->region_text, (size_t)n));
    TRY(dev_alloc(ctx, &ctx->region_size, (size_t)n));
    TRY(dev_alloc(ctx, &ctx->region_n4, (size_t)n));
    TSAR_HIP_TRY(ctx, hipMemsetAsync(ctx->region_n4, 0, (size_t)n * 16, ctx->stream));
    return TSAR_OK;
}

// RAII bracket that records a hipEvent pair around a launch when timing is enabled.
struct ScopedKernelTimer {
    tsar_ctx* ctx;
    int ti = -1;                // index into ctx->timers (timers may nest: the vector can grow between constructor and destructor)
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ScopedKernelTimer(tsar_ctx* c, const char* name);
    ~ScopedKernelTimer();
};

// ---- launchers implemented in the .hip files -----------------------------------------------------
int launch_build_quad(tsar_ctx* ctx, const float* img, uint32_t* quad, int w, int h, int* nonintegral_flag);
int launch_expand_u8(tsar_ctx* ctx, const uint8_t* in, float* out, size_t n);   // plane_kernels.hip
int launch_build_dquad(tsar_ctx* ctx, const uint32_t* quad, uint2* dquad, int w, int h);
int launch_pm_init(tsar_ctx* ctx);
int launch_pm_init_pair(tsar_ctx* ctx);    // pm_pair.hip: the plain fast box-11 configuration with paired gathers
int launch_pm_sweep_pair(tsar_ctx* ctx, int block, int colour, const PlaneBuf& same_in, const PlaneBuf& other, const PlaneBuf& same_out,
                         uint32_t stream_id, int do_prop, int do_refine);   // pm_pair.hip
int launch_pm_sweep_ring(tsar_ctx* ctx, int block, bool prune, int colour, const PlaneBuf& same_in, const PlaneBuf& other, const PlaneBuf& same_out,
                         uint32_t stream_id, int do_prop, int do_refine);   // pm_ring.hip
bool probe_d16_hi_zeroes(tsar_ctx* ctx);   // pm_sweep.hip
int launch_pm_sweep(tsar_ctx* ctx, int colour, const PlaneBuf& same_in, const PlaneBuf& other, const PlaneBuf& same_out,
                    uint32_t stream_id, int do_prop, int do_refine);
int launch_pm_sweep_lut(tsar_ctx* ctx, int colour, const PlaneBuf& same_in, const PlaneBuf& other, const PlaneBuf& same_out, uint32_t stream_id,
                        int do_prop, int do_refine);       // pm_sweep_lut.hip
int launch_pm_full_lut(tsar_ctx* ctx, bool init, bool redraw, const float4* planes, float* c, float4* n, int32_t* bv, float* rt);   // pm_init_lut.hip
int lut_chunk_taps(int taps_per_line);
// the general-window tap loop serves 8-bit imagery (quad textures), both filter modes, whose window has few enough
// distance classes for the LDS table; TSAR_LUT=0 switches it off (the one-tap-at-a-time loop then runs), TSAR_LUT=2 also sends
// the box-11 / two-best-views configuration through it instead of its own tap loop: A/B measurements
static inline bool lut_path_forced(const tsar_ctx* ctx) { return ctx->lut_mode == 2; }
static inline bool lut_path_applies(const tsar_ctx* ctx) {
    const bool off = ctx->lut_mode == 0;
    const DevScene& hs = ctx->hscene;
    // (its fast-mode loop loads window texels with ds_read_u16_d16_hi: only where tsar_create's probe found the register's
    // other half zeroed — variant bit 3)
    const bool d16_ok = (hs.flags & TSAR_FLAG_STRICT_DIV) || (ctx->variant & 8);
    return !off && d16_ok && hs.use_quad && hs.lut_classes > 0;
}
int launch_pm_sweep_experiment(tsar_ctx* ctx, int colour, const PlaneBuf& same_in, const PlaneBuf& other, const PlaneBuf& same_out, uint32_t stream_id,
                               int do_prop, int do_refine, int* launched);   // pm_sweep_experiments.hip (TSAR_EXPERIMENTS builds)
int launch_pm_cost_planes(tsar_ctx* ctx, const float4* planes, float* cost, int32_t* beview, float* ratio);
int launch_pm_rescore(tsar_ctx* ctx, const float4* planes, float* cost, float4* n, int32_t* beview, float* ratio);   // pm_init.hip
int launch_pm_upsample(tsar_ctx* ctx, const float4* coarse, int cw, int ch);                     // pm_upsample.hip
int launch_pm_upsample_merge(tsar_ctx* ctx, const float4* coarse, int cw, int ch);               // pm_upsample.hip (buf[0] -> buf[1])
int launch_pm_upsample_lut(tsar_ctx* ctx, bool merge, const float4* coarse, int cw, int ch);   // pm_upsample_lut.hip
int launch_pyr_down(tsar_ctx* ctx, const float* src, int w, int h, void* dst, bool u8);        // tsar_pyramid.hip
int launch_geom_pyramid(tsar_ctx* ctx, const float* src, int w, int h, float* dst);            // tsar_pyramid.hip
int launch_pyramid_planes(tsar_ctx* ctx, const float4* src, int w, int h, float4* dst);        // tsar_pyramid.hip
int launch_geom_check(tsar_ctx* ctx, const float* depth, int depth_stride, const tsar_geom_check_params* p, uint8_t* count_out,
                      float* depth_out);                                                       // geom_check_kernels.hip (writes ctx->scale)
int launch_geom_reproject(tsar_ctx* ctx, const tsar_geom_reproject_params* p, uint32_t* zbuf, unsigned long long* mask, float* depth_out,
                          uint8_t* count_out);                                                 // geom_reproject_kernels.hip
int launch_merge_candidates(tsar_ctx* ctx, const float* depth, float4* cand);                  // geom_reproject_kernels.hip (reads buf[0].n4)
int launch_merge_select(tsar_ctx* ctx, const float4* cand, const float* cand_c, const int32_t* cand_bv, const float* cand_rt,
                        unsigned long long* n_taken);                                          // geom_reproject_kernels.hip (writes buf[0], beview, ratio)
int launch_get_disp(tsar_ctx* ctx, const float* depth_in, const float* normal_world);
int launch_plane_prior(tsar_ctx* ctx, const float* depth_in, const float* normal_world, float4* prior);   // plane_kernels.hip
size_t plane_prior_build_grid_keys(int w, int h, int cell, int max_levels);                      // plane_prior_build_kernels.hip (0: no level fits)
int launch_plane_prior_build(tsar_ctx* ctx, const float* depth, const float* score, int cell, int max_levels, unsigned long long* grid,
                             float* depth_out, float* normal_out, uint8_t* level_out);          // plane_prior_build_kernels.hip
int run_cloud_distance(CallFrame& f, const float* query, long long n_query, int query_stride, const float* target, long long n_target, int target_stride,
                       float r2, double edge, long long max_pairs, int n_tol, const float* tol2, float* dist2_out, int32_t* index_out, int64_t* within_out,
                       int64_t* n_valid_out, int64_t* pairs_out);                                  // cloud_distance_kernels.hip (device pointers; finishes the frame)
int run_cloud_voxels(CallFrame& f, const float* cloud, long long n, int stride, double voxel, const float* dist2, int n_tol, const float* tol2, int32_t* rank_out,
                     long long cap, int32_t* rep_out, int32_t* count_out, int32_t* within_out, int64_t* n_voxels_out, int64_t* n_valid_out,
                     int mem);                                                                  // cloud_voxel_kernels.hip (cloud, dist2: device; outputs in `mem`; finishes the frame)
int run_cloud_neighbors(CallFrame& f, const float* cloud, long long n, int stride, float r2, double edge, int k, long long max_pairs, int32_t* count_out,
                        float* knn_out, int64_t* n_valid_out, int64_t* pairs_out);              // cloud_neighbor_kernels.hip (device pointers; finishes the frame)
int run_cloud_normals(CallFrame& f, const float* cloud, long long n, int stride, float r2, double edge, const tsar_cloud_normals_params& p, int32_t* knn_index_out,
                      int32_t* n_used_out, float* normal_out, float* curvature_out, double* cov_out, int64_t* n_valid_out, int64_t* n_normals_out,
                      int64_t* pairs_out);                                                          // cloud_normal_kernels.hip (device pointers; finishes the frame)
int run_cloud_normal_compare(CallFrame& f, const float* normal_a, int stride_a, long long n, const float* normal_b, int stride_b, long long n_b, const int32_t* index,
                             const float* dist2, float md2, int n_tol, const double* min_cos, int is_signed, float* cos_out,
                             unsigned long long* counters_out);                                   // cloud_normal_kernels.hip (counters: n_compared, within[16])
struct CrViewHost { float P[12]; float fr; int max_px, w, h; bool foot; };                       // tsar_cloud_render's view: P, fl(K[0] * radius), radius > 0
struct CsViewHost { float M[9]; float C[3]; float r2; };                                          // tsar_cloud_render_oriented's: (K R)^-1, -R^T t, fl(radius * radius)
int run_cloud_render(CallFrame& f, const float* cloud, const float* normals, long long n, int stride, int normal_stride, const CrViewHost& vh, const CsViewHost* sh,
                     float occlusion_diff, float depth_diff, int min_points, long long max_splats, float* depth_out, uint8_t* count_out, int32_t* index_out,
                     float* occluder_out, int64_t* n_splats_out, int64_t* n_covered_out);         // cloud_render_kernels.hip (device pointers; sh null: the square occluder; finishes the frame)
int run_depth_compare(CallFrame& f, const float* depth, const float* gt, const uint8_t* mask, long long n, int n_tol, const float* tol, float* error_out,
                      unsigned long long* counters_out);                                         // cloud_render_kernels.hip (counters: n_gt, n_both, n_front, n_behind, within[16])
int launch_compute_disp(tsar_ctx* ctx);
int launch_compute_disp_final(tsar_ctx* ctx, const float4* resize4, const float* text);
int launch_depth_to_plane(tsar_ctx* ctx);
int launch_getview(tsar_ctx* ctx);
int launch_lrdiff(tsar_ctx* ctx);
int launch_selftest_divide(tsar_ctx* ctx, const float* X, const float* Y, const float* Z, size_t n, float* u, float* v, int ieee);   // selftest_kernels.hip
int launch_sweep_census(tsar_ctx* ctx, int colour, unsigned long long* dout);
int launch_selftest_divide_random(tsar_ctx* ctx, int log2_pairs, uint64_t seed, int mode, int guarded, unsigned long long* dcounts);
int launch_selftest_sqrt(tsar_ctx* ctx, int mode, uint64_t seed, unsigned long long* dcounts);
int launch_update_scale(tsar_ctx* ctx);
int launch_fake_depth(tsar_ctx* ctx);
int launch_split_out4(tsar_ctx* ctx, float* depth, float* normal3);
int launch_label_range(tsar_ctx* ctx, const int32_t* labels, size_t n, int32_t* lo, int32_t* hi);   // min / max of a device label plane
