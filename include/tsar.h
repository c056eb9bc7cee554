/*
 * tsar.h — C ABI of the MI355X-native PatchMatch-MVS matcher (libtsar_hip.so).
 *
 * This is the drop-in boundary for the GPU operator layer of ZhenlongYuan/TSAR-MVS.
 * The reference crosses host→device at four C++ functions taking a CUDA-managed
 * `GlobalState&` (reference gipuma.h:2-6, bodies gipuma.cu:1700-1913) plus the gSLICr
 * `core_engine` (reference gSLICr_Lib/engines/gSLICr_core_engine.h:19-32).  A managed-memory
 * C++ object cannot cross an FFI, so the same operators are exported here as plain
 * `extern "C"` functions over an opaque context, plain pointers and sizes:
 *
 *   reference operator (file:line)                      this header
 *   --------------------------------------------------  ---------------------------------------
 *   GlobalState ctor + LineState::resize                 tsar_create / tsar_destroy
 *     (globalstate.h:41-53, linestate.h:71-110)
 *   getCameraParameters + addImageToTextureFloatGray     tsar_set_views
 *     (cameraGeometryUtils.h:174-364, main.cpp:1190-1228)
 *   AlgorithmParameters fill (main.cpp:1386-1416)        tsar_set_params
 *   viewSelectionSubset fill (main.cpp:1351-1384)        tsar_set_view_subset
 *   gipuma_init_cu2            (gipuma.cu:678-729)       tsar_pm_init
 *   red/black prop+refine loop (gipuma.cu:1744-1754,     tsar_pm_iterate
 *     bodies :846-1138)
 *   the same kernels with `final == true`                tsar_pm_iterate_final
 *     (gipuma.cu:856,1063,559-562,669-672; lines->text)
 *   pmCostMultiview_cu on a given plane map              tsar_pm_cost_planes (test / diagnostics hook)
 *     (gipuma.cu:455-518)
 *   host fill of norm4/depth/c + firstcuda               tsar_load_planes
 *     (main.cpp:1479-1493, gipuma_get_disp gipuma.cu:731-755)
 *   weak.png → lines->scale (main.cpp:1499-1514)         tsar_set_reliable_mask / tsar_get_reliable_mask
 *   gipuma_getlrdiff           (gipuma.cu:1160-1186)     tsar_lrdiff
 *   sliccuda → gipuma_getview  (gipuma.cu:1188-1213)     tsar_getview
 *   gipuma_WMF / gipuma_WMF_Final (gipuma.cu:1294-1698)  tsar_wmf
 *   texture() output canny[]/text[] (main.cpp:559-593)   tsar_set_regions
 *   texture() itself (main.cpp:365-596, CPU + OpenCV)     tsar_detect_weak_texture
 *   CPU RANSAC per region      (main.cpp:1520-1730)      tsar_ransac_regions
 *   fakecuda → gipuma_update_scale_2 (gipuma.cu:1261-92) tsar_fake_depth
 *   fillcuda → gipuma_update_scale + gipuma_compute_disp tsar_fill_textureless
 *     (gipuma.cu:1215-1259, 810-844)
 *   gipuma_compute_disp alone  (gipuma.cu:810-844)       tsar_compute_disp
 *   gipuma_compute_disp_final  (gipuma.cu:757-808)       tsar_compute_disp_final
 *   gipuma_dptow               (gipuma.cu:1140-1158)     tsar_depth_to_plane
 *   copy-out of norm4 (main.cpp:1785-1795)               tsar_get_result / tsar_get_plane
 *   gSLICr core_engine::Process_Frame + Get_Seg_Res      tsar_slic
 *   Fusion.exe (binary only; flags x/1.sh:20-30)         tsar_fuse
 *   (none: the reference ships no evaluation)            tsar_cloud_distance
 *   (none: the reference's fuser thins nothing)          tsar_cloud_voxels
 *   (none: the reference's fuser cleans nothing)         tsar_cloud_neighbors
 *   (none: the reference estimates no cloud normals)     tsar_cloud_normals / tsar_cloud_normal_compare
 *   (none: the reference renders no cloud)               tsar_cloud_render / tsar_depth_compare
 *   (none: nor one with oriented occluders)              tsar_cloud_render_oriented
 *
 * Conventions
 *   - every function returns an int status (TSAR_OK = 0, negative = error) and never exits the
 *     process (the reference's checkCudaErrors calls exit(), helper_cuda.h);
 *     tsar_last_error() returns a human-readable message for the last failure on that context.
 *   - the caller owns every buffer it passes; the library owns all device memory inside tsar_ctx.
 *   - `mem` arguments say where caller buffers live: TSAR_MEM_HOST or TSAR_MEM_DEVICE (HIP device
 *     pointer on the context's device).  No unified memory.
 *   - one tsar_ctx per device and per host thread; all work of a context is issued on one HIP
 *     stream (tsar_get_stream) and the call returns after that work is complete unless the
 *     function says it is asynchronous.
 *   - TSAR_MEM_DEVICE inputs are read on the context's own (non-blocking) stream, which is not ordered against
 *     any other stream: the work that produces them (a kernel on another stream, an RCCL collective, a copy)
 *     must be COMPLETE before the call, e.g. by synchronising the producing stream or by making it wait
 *     on an event the caller then synchronises.  TSAR_MEM_DEVICE outputs are complete when the call returns.
 *   - host buffers from tsar_host_alloc are page-locked: copies to and from them run at PCIe rate without the
 *     runtime's bounce buffers.  Any other host memory works too, slower.
 *   - images are row-major float32 gray, values as produced by an 8-bit decode (0..255); planes are
 *     row-major float32 [h][w] (or [h][w][3]/[h][w][4]).
 */
#ifndef TSAR_H_
#define TSAR_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSAR_MAX_VIEWS 64        /* reference MAX_IMAGES 512 (config.h:2); ≤32 views are ever selected */
#define TSAR_MAXCOST 2.0f        /* reference config.h:22 */

/* status codes */
#define TSAR_OK 0
#define TSAR_ERR_INVALID (-1)    /* bad argument */
#define TSAR_ERR_HIP (-2)        /* HIP runtime failure */
#define TSAR_ERR_STATE (-3)      /* call order violated (e.g. iterate before set_views) */
#define TSAR_ERR_NOMEM (-4)

#define TSAR_MEM_HOST 0
#define TSAR_MEM_DEVICE 1

/* cost combination, reference algorithmparameters.h:17 */
#define TSAR_COMB_ALL 0
#define TSAR_COMB_BEST_N 1
#define TSAR_COMB_ANGLE 2   /* accepted like the reference: only BEST_N is distinguished on the GPU path (gipuma.cu:496-499), */
#define TSAR_COMB_GOOD 3    /* so ANGLE and GOOD average all valid views exactly as ALL does */

/* behaviour flags (tsar_params.flags).  Default 0 = the reference's behaviour wherever it is
 * well defined. */
#define TSAR_FLAG_FIX_DOWN_FAR_SEED  (1u << 0) /* seed the down_far arm's minimum with c[down_far]
                                                  (reference seeds with c[up_far], gipuma.cu:906) */
#define TSAR_FLAG_FIX_RIGHT_FAR_CMP  (1u << 1) /* right_far arm picks the minimum
                                                  (reference comparison is inverted, gipuma.cu:943) */
#define TSAR_FLAG_STRICT_DIV         (1u << 2) /* the reference's arithmetic, operation for operation: IEEE divisions in the per-tap
                                                  perspective divide, the tap position as (m0 x + m1 y) + m2 (getCorrespondingPoint_cu
                                                  gipuma.cu:161-171), (w r) s, window columns, the reference's homography and blend
                                                  (bit-exact against the CPU oracle; ~28 % slower than the default arithmetic, whose
                                                  seven rounding-level liberties oracle/tsar_oracle.c S7 lists) */
#define TSAR_FLAG_FIX_PLANE_FIT      (1u << 3) /* tsar_ransac_regions: the plane through three points with its first component
                                                   as the cross product has it, (y2-y1)(z3-z1) - (z2-z1)(y3-y1).  The reference's
                                                   calcLinePara writes (y3-y1) in both products (main.cpp:159); default off. */
#define TSAR_FLAG_NO_LINE_CLOSING    (1u << 4) /* tsar_detect_weak_texture: skip the Hough boundary closing of large regions
                                                  (main.cpp:385-435; on by default like the reference's HoughLinesP step) */

#define TSAR_FLAG_TEX_FILTER_8BIT    (1u << 5) /* bilinear fractions rounded to 8 fractional bits before the blend, as the CUDA
                                                  texture unit the reference samples through stores them (linear filtering with
                                                  1.8 fixed-point weights, main.cpp:1215-1219); the unit's rounding rule is
                                                  unpublished: round-to-nearest-even here.  Runs the general-window tap loop at every box
                                                  (box 11: ~15 % below the default filter). */

#define TSAR_FLAG_FIX_INIT_RADIUS     (1u << 6) /* tsar_pm_init on the sweeps' window, radius (box - 1) / 2.  The reference's
                                                  gipuma_init_cu2 uses box / 2 (gipuma.cu:693-694), every other kernel
                                                  (box - 1) / 2 (:858-859): an even box initialises on a larger window.
                                                  Reproduced by default. */

typedef struct tsar_ctx tsar_ctx;

/* One calibrated view as read from an MVSNet-style cams/%08d_cam.txt (reference
 * fileIoUtils.h:117-153): intrinsics and world→camera extrinsics.  Row-major. */
typedef struct tsar_camera {
    float K[9];
    float R[9];
    float t[3];
} tsar_camera;

/* Subset of the reference's AlgorithmParameters (algorithmparameters.h:54-88) that the GPU path
 * reads.  Zero-initialise, then tsar_default_params(). */
typedef struct tsar_params {
    int32_t box_hsize;    /* --blocksize (scripts pass 11; default 19).  1..63.  tsar_set_views refuses (TSAR_ERR_INVALID, with the
                             reason in tsar_last_error) a box above 23 when the shared weight table of the general-window loop
                             cannot serve it: images that are not an 8-bit decode; rectangular boxes with more than 144 distinct
                             tap distances (radii of mixed parity, e.g. 63 x 61); fast mode on a device whose D16 LDS-load probe
                             failed.  An even box initialises on radius box / 2 and sweeps on (box - 1) / 2 like the reference
                             (TSAR_FLAG_FIX_INIT_RADIUS); a context holding the reference view alone takes any box. */
    int32_t box_vsize;
    int32_t n_best;       /* --n_best (scripts 1; default 2) */
    int32_t cost_comb;    /* --cost_comb: TSAR_COMB_* */
    float depth_min;      /* from the reference view's cam file */
    float depth_max;
    float cam_scale;      /* --cam_scale: K is divided by it (cameraGeometryUtils.h:143-154) */
    uint32_t flags;       /* TSAR_FLAG_* */
    uint64_t seed;        /* RNG stream seed (the reference seeds with clock64(), gipuma.cu:700) */
} tsar_params;

/* gSLICr settings actually set by the reference (main.cpp:608-615). */
typedef struct tsar_slic_settings {
    int32_t spixel_size;      /* 20 */
    int32_t no_iters;         /* 5 */
    float coh_weight;         /* 5.0 */
    int32_t do_enforce_connectivity; /* 0 in the reference */
    int32_t color_space;      /* 0 = CIELAB (reference), 1 = XYZ, 2 = RGB */
} tsar_slic_settings;

/* Per-kernel timing record (tsar_get_kernel_timing). */
typedef struct tsar_kernel_timing {
    char name[48];
    int32_t launches;
    float total_ms;           /* sum of hipEventElapsedTime over the launches */
} tsar_kernel_timing;

/* ---- lifecycle ------------------------------------------------------------------------- */
int tsar_create(int device, tsar_ctx** out);
int tsar_destroy(tsar_ctx* ctx);
const char* tsar_last_error(const tsar_ctx* ctx);
const char* tsar_version(void);
/* the HIP stream (hipStream_t) all kernels of this context are launched on */
int tsar_get_stream(tsar_ctx* ctx, void** stream_out);
int tsar_synchronize(tsar_ctx* ctx);

/* ---- inputs ---------------------------------------------------------------------------- */
void tsar_default_params(tsar_params* p);
int tsar_set_params(tsar_ctx* ctx, const tsar_params* p);
/* views[0] is the reference view, views[1..n-1] the source views, in the order of the reference's
 * argv image list.  gray[i] points at w*h float32.  Cameras are re-origined so that the reference
 * camera is K[I|0] (cameraGeometryUtils.h:270-302).  Must follow tsar_set_params.
 * n_views = 1 (the reference view alone) is enough for the textureless-refinement operators (tsar_load_planes, weak-texture
 * detection, region RANSAC, fill — none of them reads a source image); the matching entry points (tsar_pm_*, tsar_lrdiff)
 * then return TSAR_ERR_STATE. */
int tsar_set_views(tsar_ctx* ctx, int n_views, int w, int h, const float* const* gray, int mem,
                   const tsar_camera* cams);
/* The same with the 8-bit decode itself: gray[i] points at w*h bytes, widened to float on the device — bit for bit what
 * tsar_set_views does with (float)gray[i][p], which is how the reference fills its textures (imread(..., GRAYSCALE) ->
 * convertTo(CV_32F), main.cpp:1302,1423).  A quarter of the bytes cross PCIe and the caller holds no float copies of its images
 * (1.07 GB at ETH3D size with ten sources): what tsar_gipuma hands over. */
int tsar_set_views_u8(tsar_ctx* ctx, int n_views, int w, int h, const uint8_t* const* gray, int mem,
                      const tsar_camera* cams);
/* indices (1..n_views-1) of the source views used for matching, in pair.txt order; at most 32 (the reference's
 * costVector[32], gipuma.cu:467).  Default after tsar_set_views: the first min(n_views - 1, 32) source views.
 * Changing the subset invalidates the stored costs' meaning: the next sweep re-scores neighbours it would otherwise skip. */
int tsar_set_view_subset(tsar_ctx* ctx, int n, const int32_t* view_idx);

/* ---- PatchMatch (the north-star path) --------------------------------------------------- */
int tsar_pm_init(tsar_ctx* ctx);
/* `iters` red/black iterations; each = black (prop+refine) then red (prop+refine). */
int tsar_pm_iterate(tsar_ctx* ctx, int iters);
/* The same loop with the kernels' `final` argument true (dormant in the reference: nothing passes true).
 * text [h][w] = lines->text: pixels with text == -1 keep their plane and cost (gipuma.cu:856, :1063) and
 * accepted hypotheses do not update ratio / best view (gipuma.cu:559-562, :669-672). */
int tsar_pm_iterate_final(tsar_ctx* ctx, int iters, const float* text, int mem);
/* Diagnostics: multi-view cost of caller-supplied planes.  planes = [h][w][4] (n_x,n_y,n_z,d) in
 * reference-camera coordinates; outputs [h][w]; beview/ratio may be NULL. */
int tsar_pm_cost_planes(tsar_ctx* ctx, const float* planes, int mem, float* cost_out,
                        int32_t* beview_out, float* ratio_out);
/* Diagnostics: overwrite / read the raw matcher state: planes [h][w][4] + cost [h][w]. */
int tsar_set_plane(tsar_ctx* ctx, const float* planes, const float* cost, int mem);
/* Diagnostics: ONE half-iteration (colour 0 = black: (x+y) even, 1 = red), optionally only its
 * propagation or only its refinement half (the reference's four kernels gipuma.cu:1096-1138), and
 * the RNG stream counter (number of half-iterations done so far) that keys the refinement draws. */
int tsar_pm_sweep(tsar_ctx* ctx, int colour, int do_prop, int do_refine);
int tsar_set_sweep_counter(tsar_ctx* ctx, int n);
int tsar_get_plane(tsar_ctx* ctx, float* planes, float* cost, int32_t* beview, float* ratio, int mem);

/* ---- plane <-> depth (reference gipuma.cu:731-844, 1140-1158) ---------------------------- */
/* depth [h][w], normal_world [h][w][3]: planes from an external MVS; cost is set to 1. */
int tsar_load_planes(tsar_ctx* ctx, const float* depth, const float* normal_world, int mem);
int tsar_compute_disp(tsar_ctx* ctx);
int tsar_compute_disp_final(tsar_ctx* ctx, const float* resize_planes, const float* text, int mem);
int tsar_depth_to_plane(tsar_ctx* ctx);

/* ---- coarse-to-fine PatchMatch (the remedy of the ACMM / APD line for textureless regions) ------------------------------ */
/* Installs on `coarse` the 1 + N views of `fine`, each downsampled by 2 on the device (no host round trip; `fine` keeps its views,
 * so the call chains for further levels).  The filter is OpenCV's pyrDown, which the reference uses (main.cpp:377-379, 621-622):
 *   - kernel [1 4 6 4 1]^T [1 4 6 4 1] / 256, its centre on source pixel (2x, 2y);
 *   - border BORDER_REFLECT_101;
 *   - output size ((w + 1) / 2, (h + 1) / 2);
 *   - views from tsar_set_views_u8: integer sum s of the weighted texels, (s + 128) >> 8 (pyrDown on CV_8U), so the coarse level is an
 *     8-bit decode again (its tap loops, box limits and TSAR_FLAG_TEX_FILTER_8BIT apply as at the fine level);
 *   - views from tsar_set_views: float32 without rounding, per source row r_j = (((t0 + 4 t1) + 6 t2) + 4 t3) + t4, then
 *     (((r0 + 4 r1) + 6 r2) + 4 r3) + r4, times 1/256, each operation rounded in that order (no fused multiply-add).
 * Cameras: the coarse K is the fine K with fx, fy, cx, cy halved (exact for a filter centred on (2x, 2y); --cam_scale's convention,
 * cameraGeometryUtils.h:143-154); R, t and the depth range stay; everything else is derived as tsar_set_views derives it.  `coarse`
 * takes `fine`'s params (box, n_best, cost_comb, flags, seed, cam_scale) and view subset.  TSAR_ERR_INVALID, with the reason in
 * tsar_last_error(coarse): contexts on different devices, `fine` without views, a coarse side smaller than the window (or than 8).
 * The contexts' streams are ordered by an event. */
int tsar_pyramid_views(tsar_ctx* coarse, const tsar_ctx* fine);
/* Starts `fine`'s plane state from `coarse`'s (planes (n, d) are metric and independent of K, getD_cu gipuma.cu:71-90).  Fine pixel
 * (x, y) scores the coarse planes at (x / 2 + i, y / 2 + j), i, j in {0, 1}, clamped to the coarse image, in the order (0,0), (1,0),
 * (0,1), (1,1), with its own multi-view cost (tsar_pm_cost_planes's, in the context's arithmetic, window, best-N and subset); the
 * lowest cost wins, the first on a tie.  The winner's plane, cost, best view and ratio become the state the next tsar_pm_iterate
 * starts from (like tsar_pm_init's: the sweep counter restarts at 0), and the winning planes are kept as the context's upsampled
 * planes (the reference's lines->resize4, linestate.h:64, which its snapshot allocates and never fills).  TSAR_ERR_INVALID unless
 * coarse holds a plane state of ((w + 1) / 2, (h + 1) / 2) on the same device.  Timed as "pm_upsample". */
int tsar_upsample_planes(tsar_ctx* fine, const tsar_ctx* coarse);
/* tsar_compute_disp_final with resize4 = the planes the last tsar_upsample_planes kept (TSAR_ERR_INVALID if there are none).
 * text [h][w] is lines->text, which the reference never fills; here it is the region text of the pixel's weak-texture label,
 * text[p] = region_text[labels[p]] from tsar_detect_weak_texture (main.cpp:575-589): -1 textureless, 1 otherwise. */
int tsar_compute_disp_final_upsampled(tsar_ctx* ctx, const float* text, int mem);
/* Diagnostics: the image of view `view` as the context holds it, [h][w] float32 (a pyramid level's views included). */
int tsar_get_view_image(tsar_ctx* ctx, int view, float* out, int mem);

/* ---- geometric consistency ----------------------------------------------------------------- */
/* A second PatchMatch pass whose cost also asks whether the source views' depth maps agree (the ACMM / APD family's geometric
 * consistency).  With maps installed, view v's cost of hypothesis plane n4 at reference pixel (x, y) becomes c_v + lambda e_v.  Validity
 * (c_v < MAXCOST, gipuma.cu:506-510) is decided on the photometric c_v before the term is added; best-N, best view and ratio then
 * proceed as without the term, on the summed costs.  A view without a map (NULL entry) adds nothing.
 * e_v, in float32, every operation one IEEE-754 operation rounded to nearest (no fused multiply-add), in exactly this order:
 *   D  = the hypothesis's depth at (x, y) (getDepthFromPlane3_cu, gipuma.cu:436-453; once per hypothesis);  X = float(x), Y = float(y)
 *   F  = [A | b] of view v: A = K_v R K_ref^-1, b = K_v t, the float32 matrices the context holds for the fast homography (rounded
 *        once from float64: tsar_set_views), so that F (x D, y D, D, 1) is K_v (R (D K_ref^-1 (x, y, 1)) + t);
 *        xd = X * D, yd = Y * D;  a_r = ((F[r][0] * xd + F[r][1] * yd) + F[r][2] * D) + F[r][3]  for r = 0, 1, 2 -> (a, b, s)
 *   u = a / s, v = b / s (correctly rounded quotients);  c = floor(u + 0.5), r = floor(v + 0.5) (the sum rounded first)
 *   inside = s > 0 and 0 <= c <= w - 1 and 0 <= r <= h - 1;  D_v = depth_v[r][c] if inside, else 0
 *   B  = the 3 x 4 matrix [K_ref R^T K_v^-1 | -K_ref R^T t] of view v, formed in float64 from the float64 K_ref, K_v, R, t from which
 *        tsar_set_views rounds its float32 cameras (K_v^-1 by the adjugate, then the products (K_ref R^T) K_v^-1 and -(K_ref R^T) t,
 *        each entry a sum over k in increasing order), each entry rounded once to float32.  It takes (c D_v, r D_v, D_v, 1) to the
 *        reference image: cd = c * D_v, rd = r * D_v;  p_r = ((B[r][0] * cd + B[r][1] * rd) + B[r][2] * D_v) + B[r][3]
 *   x' = p_0 / p_2, y' = p_1 / p_2 (correctly rounded);  dx = x' - X, dy = y' - Y;  e2 = dx * dx + dy * dy
 *   e  = tau if not (inside and D_v > 0 and p_2 > 0 and e2 < tau * tau) (this covers every non-finite intermediate: NaN fails each
 *        comparison); else 0 if e2 < 2^-100; else min(sqrt(e2), tau), the square root correctly rounded
 *   the view's cost: c_v + (lambda * e)
 * tsar_get_geom_matrices returns F and B as the kernels read them (row-major 3 x 4).  Defaults lambda = 0.2, tau = 3 px are ACMM's
 * (not the reference's, whose live path reads such a pass's output from a closed binary, main.cpp:1462-1474).
 *
 * tsar_set_geom_depths: depth[v], v >= 1, is view v's depth map [h][w] in its own camera (what tsar_get_result / TSAR_disp.dmb hold;
 * <= 0 = no estimate); depth[0] is ignored; NULL = no term for that view.  The maps are copied into memory the context owns.  Voids the
 * stored costs and the propagation memo (like tsar_set_view_subset).  TSAR_ERR_INVALID: n_views other than the context's, depth NULL,
 * weight < 0 or not finite, clip not in (0, 2^20]; TSAR_ERR_STATE: a context without source views.  tsar_set_views removes the term.
 * With a term installed every plane-scoring entry includes it (tsar_pm_init, tsar_pm_iterate[_final], tsar_pm_sweep,
 * tsar_pm_cost_planes, tsar_pm_rescore, tsar_pyramid_planes, tsar_upsample_merge; the sweeps are timed as "pm_sweep_geom");
 * tsar_pyramid_views and tsar_upsample_planes return TSAR_ERR_STATE (the pass runs coarse to fine through the three entries below).
 * tsar_clear_geom: removes the term and frees the maps.
 * tsar_pm_rescore: scores the current planes with the context's cost (the term included when installed) and writes cost, best view and
 * ratio.  A pixel whose plane is not a valid hypothesis — its depth not finite or outside [depth_min, depth_max], as the depth-0
 * pixels of a loaded map are — instead gets the hypothesis tsar_pm_init draws there, with its score.  Afterwards every stored cost is
 * its plane's score (the sweeps' memo holds), and the sweep counter restarts at 0 as after tsar_pm_init, so a pass does not depend on
 * what the context ran before.  Timed as "pm_rescore". */
int tsar_set_geom_depths(tsar_ctx* ctx, int n_views, const float* const* depth, int mem, float weight, float clip);
int tsar_clear_geom(tsar_ctx* ctx);
int tsar_pm_rescore(tsar_ctx* ctx);
int tsar_get_geom_matrices(tsar_ctx* ctx, int view, float* forward, float* back);   /* forward[12], back[12], row-major 3 x 4 */

/* The geometric-consistency pass coarse to fine (ACMM's multi-scale geometric consistency).  Build every level first with
 * tsar_pyramid_views while no term is installed anywhere, then install the term level by level with these entries:
 *   fine: tsar_load_planes, tsar_set_geom_depths;  each coarser level: tsar_geom_pyramid, tsar_pyramid_planes;
 *   coarsest: tsar_pm_iterate;  each finer level, down to the full resolution: tsar_upsample_merge, tsar_pm_iterate.
 * Coarse pixel (x, y) lies on fine pixel (2x, 2y) (tsar_pyramid_views halves fx, fy, cx, cy exactly).
 *
 * tsar_geom_pyramid: installs on `coarse` a term with fine's weight and clip.  The clip keeps its value, now in pixels of the coarser
 * level (ACMM keeps tau per scale).  Each source map of `fine` is carried one level down, without arithmetic:
 *   Dc[y][x] = Df[2y][2x] if that is > 0; otherwise the first value > 0 among Df[2y][2x+1], Df[2y+1][2x], Df[2y+1][2x+1], counting only
 *   pixels inside the image; otherwise 0 (no estimate).
 * A NULL map stays NULL.  The coarse context owns its maps (tsar_clear_geom frees them), and it may be the `fine` of the next level.
 * Voids coarse's stored costs and memo like tsar_set_geom_depths.  TSAR_ERR_STATE if `fine` has no term; TSAR_ERR_INVALID unless
 * `coarse` holds ((w + 1) / 2, (h + 1) / 2) views of as many views, on the same device, with fine's cameras and their fx, fy, cx, cy
 * halved (what tsar_pyramid_views installs).  The contexts' streams are ordered by an event.  Timed as "geom_pyramid".
 * tsar_pyramid_planes: coarse plane (x, y) = fine plane (2x, 2y), bit for bit (planes are metric, getD_cu); then the coarse planes
 * are scored as tsar_pm_rescore scores them, with the coarse context's own cost, its term included: a plane that is not a valid
 * hypothesis there gets tsar_pm_init's draw, every stored cost is its plane's score, and the sweep counter restarts at 0.
 * TSAR_ERR_INVALID if `fine` has no plane state or `coarse` holds no views of ((w + 1) / 2, (h + 1) / 2) on the same device.  Timed as
 * "pm_pyramid_planes" (the copy) and "pm_rescore".
 * tsar_upsample_merge: like tsar_upsample_planes, with the pixel's own plane kept as a candidate (in place of ACMM's detail restorer).
 * Fine pixel (x, y) scores five planes with its full multi-view cost (tsar_pm_cost_planes's: arithmetic, window, best-N, subset, and
 * the term when one is installed): 1. its own current plane; 2.-5. the coarse planes at (x / 2 + i, y / 2 + j), clamped, in the order
 * (0,0), (1,0), (0,1), (1,1).  The lowest cost wins, the earlier candidate on a tie (so the own plane wins ties).  Plane, cost, best view
 * and ratio are written as tsar_upsample_planes writes them; afterwards every stored cost is its plane's score and the sweep counter
 * is 0.  Allowed with or without a term on either context.  The planes kept for tsar_compute_disp_final_upsampled are not touched.
 * TSAR_ERR_INVALID if `fine` has no plane state, or `coarse` has no plane state of ((w + 1) / 2, (h + 1) / 2) on the same device.
 * Timed as "pm_upsample_merge". */
int tsar_geom_pyramid(tsar_ctx* coarse, const tsar_ctx* fine);
int tsar_pyramid_planes(tsar_ctx* coarse, const tsar_ctx* fine);
int tsar_upsample_merge(tsar_ctx* fine, const tsar_ctx* coarse);

/* The geometric-consistency check on its own: which pixels of a depth map of the reference view do the source views' maps confirm?
 * What tsar_fuse decides per point, as a per-pixel count, a mask and a filtered map (the reference's pipeline reads such a mask, weak.png,
 * from a closed binary, main.cpp:1499-1514).  Needs views and an installed term: tsar_set_geom_depths supplies the source maps and the
 * two matrices (a weight of 0 installs maps for checking only).
 * depth [h][w]: the map to check; NULL = the context's own result (tsar_get_result's depth: tsar_compute_disp or tsar_fill_textureless
 * must have run, TSAR_ERR_STATE otherwise).  count_out [h][w] uint8 and depth_out [h][w] float32 may each be NULL (depth_out may be
 * `depth` itself); `mem` applies to all three pointers.  The call always writes lines->scale, 1 where the pixel is kept, else 0
 * (tsar_get_reliable_mask returns it: what tsar_set_reliable_mask would install), and changes nothing else: planes, stored costs, the
 * propagation memo, the sweep counter, the result planes and the term stay as they are.  Timed as "geom_check".
 * The arithmetic, the same in both arithmetic modes: float32, every operation one IEEE-754 operation rounded to nearest (no fused
 * multiply-add).  For pixel (x, y) with D = depth[y][x]:
 *   candidate = D > 0 and D < inf (NaN fails both); a pixel that is no candidate gets count 0
 *   for every view v = 1 .. n_views - 1 that has a map, in view order (the view subset does not matter): the chain of
 *   tsar_set_geom_depths above with this D, the F and B tsar_get_geom_matrices returns, exactly as written there, up to inside, D_v,
 *   p_0, p_1, p_2, x', y' and e2 (no square root);  r2 = reproj_error * reproj_error;  dd = depth_diff * D;
 *     ok_v = inside and D_v > 0 and p_2 > 0 and e2 < r2 and |p_2 - D| < dd      (p_2: the source point's depth in the reference camera)
 *   count = sum of ok_v;  keep = count >= min_consistent;  depth_out = keep ? D : 0;  scale = keep ? 1 : 0
 * TSAR_ERR_STATE: no term installed.  TSAR_ERR_INVALID: p NULL; reproj_error or depth_diff not finite or <= 0; reproj_error > 2^20;
 * min_consistent outside [1, 31]. */
typedef struct tsar_geom_check_params {
    float reproj_error;       /* px,       default 2.0  (tsar_fusion_params' value) */
    float depth_diff;         /* relative, default 0.01 (tsar_fusion_params' value) */
    int32_t min_consistent;   /* default 2, in [1, 31] */
} tsar_geom_check_params;
void tsar_default_geom_check_params(tsar_geom_check_params* p);
int tsar_geom_check(tsar_ctx* ctx, const float* depth, const tsar_geom_check_params* p, uint8_t* count_out, float* depth_out, int mem);

/* The source views' depth maps rendered into the reference camera: what do the sources see at each pixel of the reference view, and how
 * many of them agree on it?  The way OpenMVS and the learned pipelines start a view from its neighbours; the complement of tsar_geom_check,
 * which can only say that the sources do not confirm a depth.  Needs views and an installed term, like tsar_geom_check: tsar_set_geom_depths
 * supplies the maps and B (a weight of 0 installs maps for this call only).  depth_out [h][w] float32 and count_out [h][w] uint8 may each be
 * NULL, not both; `mem` applies to both.  The call writes nothing in the context: lines->scale, planes, stored costs, the propagation
 * memo, the sweep counter, the result planes and the term stay as they are.  Timed as "geom_reproject" (three launches).
 * The arithmetic, the same in both arithmetic modes: float32, every operation one IEEE-754 operation rounded to nearest (no fused
 * multiply-add).  For every view v = 1 .. n_views - 1 that has a map, in any order (the view subset does not matter), and every pixel
 * (c, r) of it, with D_v = depth_v[r][c]:
 *   candidate = D_v > 0 and D_v < inf (NaN fails both)
 *   C = float(c), R = float(r);  cd = C * D_v, rd = R * D_v
 *   B  = view v's back-projection as tsar_get_geom_matrices returns it;  p_k = ((B[k][0] * cd + B[k][1] * rd) + B[k][2] * D_v) + B[k][3], k = 0, 1, 2
 *   x' = p_0 / p_2, y' = p_1 / p_2 (correctly rounded);  xi = floor(x' + 0.5), yi = floor(y' + 0.5) (the sum rounded first)
 *   lands = candidate and p_2 > 0 and p_2 < inf and 0 <= xi <= w - 1 and 0 <= yi <= h - 1 (NaN fails every comparison): the pixel
 *           lands on reference pixel (xi, yi) at depth p_2
 * and then for every reference pixel:
 *   Z     = the minimum of p_2 over all landings of all views there (the front-most surface); a pixel nothing lands on has no Z
 *   dd    = depth_diff * Z;  view v supports the pixel when at least one of its landings there has |p_2 - Z| <= dd (the front-most
 *           landing always supports itself);  count = the number of supporting views
 *   count_out = count where something landed, else 0;  depth_out = Z where something landed and count >= min_views, else 0
 * A minimum and a set of views do not depend on the order of arrival: the outputs are the same bits in every run.
 * TSAR_ERR_STATE: no term installed.  TSAR_ERR_INVALID: p NULL; both outputs NULL; depth_diff not finite or <= 0; min_views outside
 * [1, 63]; mem unknown. */
typedef struct tsar_geom_reproject_params {
    float depth_diff;         /* relative, default 0.01: a view supports a pixel's front-most depth Z when one of its landings there is within depth_diff * Z of Z */
    int32_t min_views;        /* default 1, in [1, 63]: depth_out is Z only where at least this many views support it */
} tsar_geom_reproject_params;
void tsar_default_geom_reproject_params(tsar_geom_reproject_params* p);
int tsar_geom_reproject(tsar_ctx* ctx, const tsar_geom_reproject_params* p, float* depth_out, uint8_t* count_out, int mem);

/* Offers a depth map of the reference view (tsar_geom_reproject's, say) to the matcher: each pixel takes the plane with its own normal
 * through the offered depth where that plane scores lower.  Needs views, sources and a plane state.  The result is this composition of
 * existing entries, bit for bit:
 *   1. the state is rescored exactly as tsar_pm_rescore does (invalid planes get tsar_pm_init's draw): planes P, costs C, best views, ratios;
 *   2. the candidate of pixel (x, y), D = depth[y][x]: where D is finite and depth_min <= D <= depth_max, Q = (P's normal, d) with d the
 *      offset of the plane with that normal through the pixel at depth D (getD_cu gipuma.cu:71-86, what tsar_load_planes computes);
 *      elsewhere Q = P;
 *   3. Q is scored as tsar_pm_cost_planes scores it (the context's arithmetic, window, best-N, subset and term);
 *   4. where cost(Q) < C, strictly (the own plane wins ties), the pixel takes Q's plane, cost, best view and ratio.
 * Afterwards every stored cost is its plane's score, the sweep counter is 0 and the result is void, as after tsar_pm_rescore.
 * *n_taken_out (may be NULL): the number of pixels that took Q.  TSAR_ERR_INVALID: depth NULL, mem unknown; TSAR_ERR_STATE as
 * tsar_pm_rescore.  Timed as "pm_rescore", tsar_pm_cost_planes's name for the scoring, and "pm_merge_depths" (two launches). */
int tsar_pm_merge_depths(tsar_ctx* ctx, const float* depth, int mem, int64_t* n_taken_out);

/* ---- plane prior ------------------------------------------------------------------------------ */
/* A per-pixel prior plane and a truncated penalty on a hypothesis's deviation from it, added to the multi-view cost (ACMP's planar
 * prior, used softly: the photometric and geometric costs arbitrate).  The prior may be a region plane, a coarser result, a filled map
 * of the textureless refinement, anything external, or what tsar_build_plane_prior below builds from a checked depth map.
 * The prior the context holds, per pixel (q_x, q_y, q_z, Dp): Dp is the caller's depth[y][x], unchanged; q is the caller's
 * normal_world[y][x] taken to reference-camera coordinates exactly as tsar_load_planes takes it (the same device function, bit for bit).
 * A pixel has a prior iff Dp > 0 and Dp < inf and the three normal components are finite; otherwise the held entry is (0, 0, 0, 0).
 * Normals are used as given: the caller supplies unit normals.  tsar_get_plane_prior returns the held entries [h][w][4].
 * The term, the same in both arithmetic modes: float32, every operation one IEEE-754 operation rounded to nearest, no fused
 * multiply-add, quotients correctly rounded.  For a hypothesis n4 = (n_x, n_y, n_z, d) at (x, y):
 *   c = its multi-view cost as without a prior: after best-N, with the geometric term inside it when one is installed
 *   if no view was valid (c is TSAR_MAXCOST, best view -1) the result is c;  if the pixel has no prior the result is c;  otherwise
 *   D   = the hypothesis's depth at (x, y) (getDepthFromPlane3_cu; the value the geometric term uses, once per hypothesis)
 *   a   = |D - Dp|;  rel = a / Dp
 *   r_d = rel / depth_clip if rel < depth_clip, else 1 (NaN fails the comparison: 1)
 *   s   = 1 - ((n_x * q_x + n_y * q_y) + n_z * q_z);  s0 = 0 if s < 0, else s
 *   r_n = s0 / normal_clip if s < normal_clip, else 1
 *   t   = (weight_depth * r_d) + (weight_normal * r_n)
 *   the result: c + t
 * Best view and ratio are not touched.  The penalty is truncated on purpose: far from a wrong prior every hypothesis pays the same
 * constant, so the data decide there.  As with the geometric term, a valid hypothesis's cost may now exceed TSAR_MAXCOST; only the
 * invalid one equals it by construction.
 *
 * tsar_set_plane_prior: depth [h][w], normal_world [h][w][3] (what tsar_get_result returns), copied into memory the context owns.  Voids
 * the stored costs and the propagation memo, like tsar_set_geom_depths; works with or without a geometric term; tsar_set_views removes
 * the prior.  TSAR_ERR_INVALID: a NULL pointer; unknown mem; a weight negative or not finite; depth_clip not finite or <= 0; normal_clip
 * outside (0, 2].  TSAR_ERR_STATE: no source views.
 * With a prior installed every plane-scoring entry includes the term: tsar_pm_init, tsar_pm_iterate[_final], tsar_pm_sweep,
 * tsar_pm_cost_planes, tsar_pm_rescore, tsar_pm_merge_depths, and tsar_upsample_merge on the fine context (the kernels are those of the
 * geometric term, timed under its names: "pm_sweep_geom").  tsar_pyramid_views and tsar_upsample_planes return TSAR_ERR_STATE for a context
 * with a prior, as with the geometric term.  A prior never moves to another context: tsar_pyramid_planes / tsar_geom_pyramid score the
 * coarse context with the coarse context's own cost.  tsar_lrdiff, the check, the reprojection and the refinement operators do not score
 * planes this way and are unchanged.
 * tsar_clear_plane_prior: removes the prior (voids the stored costs).  tsar_get_plane_prior: TSAR_ERR_STATE without a prior.
 * Timed as "plane_prior" (the conversion). */
typedef struct tsar_plane_prior_params {
    float weight_depth;   /* default 0.1  */
    float weight_normal;  /* default 0.05 */
    float depth_clip;     /* relative, default 0.02 */
    float normal_clip;    /* 1 - cos(angle), default 1 - cos(30 deg) rounded once from float64 */
} tsar_plane_prior_params;
void tsar_default_plane_prior_params(tsar_plane_prior_params* p);
int tsar_set_plane_prior(tsar_ctx* ctx, const float* depth, const float* normal_world, int mem, const tsar_plane_prior_params* p);
int tsar_clear_plane_prior(tsar_ctx* ctx);
int tsar_get_plane_prior(tsar_ctx* ctx, float* prior_out /* [h][w][4] as held */, int mem);

/* A plane prior built from the pixels of a depth map that a check confirmed (ACMP builds its prior from a triangulation of such pixels):
 * a hierarchical lattice triangulation, exact integer geometry up to the choice of a triangle, then one float64 solve per pixel.  No
 * sort, no floating-point atomics, no data-dependent loop bound: every output bit is the same in every run and in both arithmetic modes.
 * depth [h][w] float32: the filtered map, 0 where a pixel was dropped (tsar_geom_check's depth_out).  score [h][w] float32 or NULL: lower
 * is better (a stored cost; ACMP's "most credible point").  Needs views: the reference camera, and w, h <= 65535.
 *   candidate: depth > 0 and depth < inf (NaN and -0.0 fail), and, with a score, score >= 0 and score < inf (NaN fails; a score of -0.0
 *     is a candidate and counts as +0.0)
 *   levels: level l has cells of edge s_l = cell << l on a grid of ceil(w / s_l) x ceil(h / s_l) cells (the last column and row may be
 *     partial); it exists while both grid dimensions are >= 2, l < max_levels (max_levels = 0: all that fit) and l < 16
 *   support point of a cell: its candidate with the smallest (score, raster index), lexicographic, scores compared as their bit
 *     patterns (the order of non-negative floats); without a score the smallest raster index.  A cell without a candidate is empty.
 *     (A coarser cell's support point is the minimum over its four children: a minimum, so no order of arrival can matter.)
 *   quads: cells (a, b), (a+1, b), (a, b+1), (a+1, b+1) of one level form a quad when all four exist and none is empty; their support
 *     points are P00, P10, P01, P11.  orient(A, B, C) = (Bx - Ax)(Cy - Ay) - (By - Ay)(Cx - Ax), in integers.  The quad is split along
 *     P00-P11 when orient(P00, P11, P10) and orient(P00, P11, P01) have strictly opposite signs: triangles (P00, P10, P11), (P00, P11, P01);
 *     otherwise along P10-P01: triangles (P00, P10, P01), (P10, P11, P01).  A triangle (A, B, C) with area2 = orient(A, B, C) = 0 is skipped;
 *     a pixel P is inside when orient(A, B, P), orient(B, C, P), orient(C, A, P) are each zero or of area2's sign (edges and vertices inside).
 *   the triangle of pixel (x, y): levels from 0 upwards; at level l, with the pixel in cell (i, j) = (x / s_l, y / s_l), the quads with
 *     origin (i-1, j-1), (i, j-1), (i-1, j), (i, j) in that order, each quad's two triangles in the order above; the first triangle that
 *     contains the pixel is taken, l is its level.  At most 8 triangles per level are tried.  A pixel no level covers has no prior.
 *   the plane of (A, B, C), float64, every operation one IEEE-754 operation rounded to nearest (no fused multiply-add), quotients and the
 *     square root correctly rounded; integers and float32 values enter exactly:
 *       wA = 1 / depth[A], wB, wC likewise;  dB = wB - wA;  dC = wC - wA          (the inverse depth of a plane is affine in the pixel)
 *       gx = (dB * (Cy - Ay) - dC * (By - Ay)) / area2;   gy = (dC * (Bx - Ax) - dB * (Cx - Ax)) / area2
 *       wp = (wA + gx * (x - Ax)) + gy * (y - Ay);   no prior unless wp > 0 (it is, whenever the three depths are of comparable size)
 *       c0 = (wA - gx * Ax) - gy * Ay;   m_k = (K[0][k] * gx + K[1][k] * gy) + K[2][k] * c0, k = 0, 1, 2   (K: the reference camera's, as
 *            the kernels hold it: float32 after cam_scale)
 *       len = sqrt((m_0 * m_0 + m_1 * m_1) + m_2 * m_2);   q_k = -m_k / len        (the unit normal in reference-camera coordinates, facing
 *            the camera)
 *       normal_world_k = float32((R[0][k] * q_0 + R[1][k] * q_1) + R[2][k] * q_2)   (R: the reference camera's world->camera rotation; the
 *            convention of tsar_get_result's normal_world, so the map can go straight into tsar_set_plane_prior)
 *       depth = float32(1 / wp)
 * Outputs, each may be NULL, not all three: depth_out [h][w] float32 and normal_world_out [h][w][3] float32, 0 where there is no prior;
 * level_out [h][w] uint8, the level used, 255 where there is no prior.  `mem` applies to every pointer; with device pointers nothing
 * touches the host.  The call changes nothing in the context: planes, stored costs, the propagation memo, the sweep counter, lines->scale,
 * the result planes, the term and any prior the context holds stay as they are.  The grids are temporaries of the call.  Timed as
 * "plane_prior_build" (the per-pixel look-up and solve), "plane_prior_build_supports" (level 0) and "plane_prior_build_levels" (the
 * coarser levels, one timed bracket around their launches).
 * TSAR_ERR_STATE: no views.  TSAR_ERR_INVALID: depth or p NULL; all three outputs NULL; mem unknown; cell outside [2, 256]; max_levels
 * outside [0, 16]; an image too small for one level (w <= cell or h <= cell) or larger than 65535 in either direction. */
#define TSAR_PLANE_PRIOR_MAX_LEVELS 16
typedef struct tsar_plane_prior_build_params {
    int32_t cell;         /* level-0 cell edge in pixels, in [2, 256]; default 4: ACMP's spacing is 5, and on the 160 x 120 simulated scene of
                             DESIGN.md section 8 a cell of 4 did better than 8.  Untuned on real scenes. */
    int32_t max_levels;   /* default 0 = every level that fits; in [0, 16] */
} tsar_plane_prior_build_params;
void tsar_default_plane_prior_build_params(tsar_plane_prior_build_params* p);
int tsar_build_plane_prior(tsar_ctx* ctx, const float* depth, const float* score /* may be NULL */, int mem,
                           const tsar_plane_prior_build_params* p, float* depth_out, float* normal_world_out, uint8_t* level_out);

/* After tsar_compute_disp: depth [h][w] (0 where cost == MAXCOST), normal_world [h][w][3],
 * cost [h][w], confid [h][w]; any may be NULL. */
int tsar_get_result(tsar_ctx* ctx, float* depth, float* normal_world, float* cost, float* confid,
                    int mem);

/* ---- TSAR textureless refinement (reference gipuma.cu:1160-1698, main.cpp:1499-1783) ------ */
int tsar_set_reliable_mask(tsar_ctx* ctx, const float* scale, int mem);          /* lines->scale */
int tsar_get_reliable_mask(tsar_ctx* ctx, float* scale, int mem);                /* lines->scale as tsar_wmf leaves it */
int tsar_lrdiff(tsar_ctx* ctx);
int tsar_getview(tsar_ctx* ctx);
int tsar_wmf(tsar_ctx* ctx, int iters, int final_pass);
/* labels [h][w] = region id per pixel (lines->canny); region_text[n_regions] = -1 for textureless
 * regions (cannylines->text).  Every label must lie in [0, n_regions): checked, TSAR_ERR_INVALID otherwise. */
int tsar_set_regions(tsar_ctx* ctx, const int32_t* labels, int n_regions, const float* region_text,
                     const float* region_size, int mem);
/* Weak-texture region detection of the reference view on the GPU (reference texture(), main.cpp:365-596):
 * computes lines->canny / cannylines->text / size and installs them like tsar_set_regions.  labels_out
 * [h][w] int32, text_out/size_out [cap] may be NULL.  The boundary closing of large regions (main.cpp:385-435) runs a
 * deterministic Hough transform with the reference's parameters in place of OpenCV's randomised HoughLinesP, whose
 * arithmetic is not in the reference's sources (parity unpinned for that step; TSAR_FLAG_NO_LINE_CLOSING skips it). */
int tsar_detect_weak_texture(tsar_ctx* ctx, int32_t* labels_out, int mem, int* n_regions_out, float* text_out,
                             float* size_out, int cap);
/* GPU replacement of the per-region CPU RANSAC; region_planes_out [n_regions][4] may be NULL */
int tsar_ransac_regions(tsar_ctx* ctx, float* region_planes_out, float* inlier_ratio_out);
int tsar_set_region_planes(tsar_ctx* ctx, const float* region_planes);            /* host [n][4] */
int tsar_fake_depth(tsar_ctx* ctx, float* fakedepth_out, int mem);
int tsar_fill_textureless(tsar_ctx* ctx);

/* ---- gSLICr superpixels ------------------------------------------------------------------ */
void tsar_default_slic_settings(tsar_slic_settings* s);
/* bgra: [h][w][4] uint8 (the reference feeds a 1/4-resolution BGR image, main.cpp:617-640);
 * labels_out [h][w] int32. */
int tsar_slic(tsar_ctx* ctx, const uint8_t* bgra, int w, int h, const tsar_slic_settings* s,
              int32_t* labels_out, int mem);

/* ---- depth-map fusion (row N3; the reference ships it only as Fusion.exe, flags x/1.sh:20-30) ----- */
typedef struct tsar_fusion_params {
    int32_t num_consistent;   /* --num_consistent=  (scripts: 1) */
    float reproj_error;       /* --reproj_error=    (2 px) */
    float depth_diff;         /* --depth_diff=      (0.01 relative) */
    float angle_deg;          /* --angle=           (15 degrees between normals) */
    int32_t used_list;        /* --used_list=       (1: pixels that contributed to a point are not fused again) */
} tsar_fusion_params;
void tsar_default_fusion_params(tsar_fusion_params* p);
/* Fuses n_views depth/normal maps (what tsar_get_result exports: depth [h][w], world normals [h][w][3]) into
 * one point cloud.  cams: K and world->camera R, t per view; gray: the views' images (point colour).  The
 * source views of view v are src_idx[src_off[v] .. src_off[v+1]) (pair.txt as CSR).  points_out: up to `cap`
 * records of 9 floats (x y z, nx ny nz, gray, number of agreeing views, reference view), in view order then
 * raster order; *n_points_out is the number found (may exceed cap).
 * `mem` names where the maps lie, and points_out with them: host maps deliver into a host buffer, device maps into a device
 * buffer (the copy into points_out is issued as device-to-host or device-to-device accordingly).
 * tsar_fuse_ctx runs on the context's device and stream and takes every temporary from the context's scratch arena (no device
 * allocation from the second call of a size on); tsar_fuse is the context-free form for a one-shot fuser process: it creates a
 * context on `device` for the duration of the call. */
int tsar_fuse_ctx(tsar_ctx* ctx, int n_views, int w, int h, const tsar_camera* cams, const float* const* depth,
                  const float* const* normal_world, const float* const* gray, int mem, const int32_t* src_off,
                  const int32_t* src_idx, const tsar_fusion_params* params, float* points_out, int64_t cap,
                  int64_t* n_points_out);
int tsar_fuse(int device, int n_views, int w, int h, const tsar_camera* cams, const float* const* depth,
              const float* const* normal_world, const float* const* gray, int mem, const int32_t* src_off,
              const int32_t* src_idx, const tsar_fusion_params* params, float* points_out, int64_t cap,
              int64_t* n_points_out);

/* ---- cloud-to-cloud distances (what an accuracy / completeness evaluation of a fused cloud against a scan is made of) ----------- */
/* For every query point the squared distance to its nearest target point within a radius R, and that target's index.  Records are
 * `stride` float32 each (>= 3), x y z first, so tsar_fuse's 9-float records go in as they are.  `mem` names where query, target,
 * dist2_out and index_out lie; tol, within_out, n_valid_query_out and pairs_out are host memory.  query and target may be one cloud.
 * The arithmetic, the same in both arithmetic modes: float32, every operation one IEEE-754 operation rounded to nearest, no fused
 * multiply-add.
 *   candidate: a record whose x, y and z are all finite
 *   for a candidate query i and a candidate target j:  dx = qx - tx, dy = qy - ty, dz = qz - tz;  d2(i, j) = (dx * dx + dy * dy) + dz * dz
 *   R2 = fl(R * R), one float32 product
 *   dist2[i] = the minimum of d2(i, j) over all candidate j, if that minimum is <= R2;  index[i] = the smallest j that attains it
 *   otherwise dist2[i] = +inf and index[i] = -1: also for a query that is no candidate, and when no target is a candidate (n_target == 0)
 *   within[k] = the number of i with dist2[i] <= fl(tol[k] * tol[k])
 *   n_valid_query = the number of candidate queries
 *   pairs = the number of (i, j) the call evaluated (below)
 * This is the brute-force definition; a minimum and a count do not depend on an order of arrival, so the outputs are the same bits in
 * every run.  How the pairs are found changes none of them: a uniform grid over the candidate targets, with
 *   origin o = the per-axis minimum over the candidate targets (exact in any order);  cell edge e = (double)R * (1 + 2^-10);
 *   cell coordinate of a point, per axis: floor(((double)p - (double)o) / e), in float64, the quotient correctly rounded.
 * Two points whose float32 d2 is <= R2 are less than R (1 + 2^-10) apart on every axis (d2's rounding errors are a few 2^-24 of it), so
 * their cell coordinates differ by at most 1: the 27 cells around the query's hold every such target, and the minimum over them is the
 * minimum over all whenever that is <= R2.  pairs counts, over the candidate queries, the candidate targets in those 27 cells.
 * TSAR_ERR_INVALID, with the reason in tsar_last_error: p NULL; mem unknown; a stride below 3; a count negative or above 2^31 - 1; max_dist
 * not finite, or fl(R * R) not finite or not > 0; a tolerance not finite, not > 0 or above max_dist; a grid of 2^20 cells or more on an
 * axis (max_dist is too small for the targets' extent); more than max_pairs pairs — then *pairs_out is still filled and nothing else is
 * written: an R as large as the scene is a brute-force n_query x n_target launch, which is refused, not run.
 * tsar_cloud_distance_ctx needs no views and no state, runs on the context's stream and changes nothing in the context; its temporaries
 * (sort buffers of both clouds) are pieces of the call's frame that never grow the context's scratch arena: what the arena does not hold
 * is allocated for the call and freed on exit.  tsar_cloud_distance is the context-free form, like tsar_fuse.
 * Timed as "cloud_bounds", "cloud_keys", "cloud_sort" (both sorts), "cloud_gather", "cloud_pairs" and "cloud_distance" (the search). */
typedef struct tsar_cloud_distance_params {
    float max_dist;       /* R: the search radius; finite, fl(R * R) finite and > 0.  No default (0): the caller's scale */
    int64_t max_pairs;    /* a call that would evaluate more (query, target) pairs than this is refused; default 1 << 40 */
} tsar_cloud_distance_params;
void tsar_default_cloud_distance_params(tsar_cloud_distance_params* p);
int tsar_cloud_distance_ctx(tsar_ctx* ctx, const float* query, int64_t n_query, int query_stride, const float* target, int64_t n_target,
                            int target_stride, const tsar_cloud_distance_params* p, int n_tol, const float* tol /* host, may be NULL with n_tol 0 */,
                            float* dist2_out /* [n_query] or NULL */, int32_t* index_out /* [n_query] or NULL */,
                            int64_t* within_out /* host [n_tol] or NULL */, int64_t* n_valid_query_out, int64_t* pairs_out /* host, may be NULL */,
                            int mem);
int tsar_cloud_distance(int device, const float* query, int64_t n_query, int query_stride, const float* target, int64_t n_target,
                        int target_stride, const tsar_cloud_distance_params* p, int n_tol, const float* tol, float* dist2_out, int32_t* index_out,
                        int64_t* within_out, int64_t* n_valid_query_out, int64_t* pairs_out, int mem);

/* ---- a voxel grid over a cloud (thinning a fused cloud; the voxel-averaged accuracy / completeness of an evaluation) -------------- */
/* Per occupied voxel of edge V: the number of its points, one representative point and, per tolerance, how many of its points have a
 * dist2 (tsar_cloud_distance's output for the same cloud) within it; per point the number of its voxel.  Records are `stride` float32
 * each (>= 3), x y z first.  `mem` names where cloud, dist2, rank_out, rep_out, count_out and within_out lie; tol, n_voxels_out and
 * n_valid_out are host memory.  The arithmetic, the same in both arithmetic modes: every operation one IEEE-754 operation rounded to
 * nearest, no fused multiply-add.
 *   candidate: a record whose x, y and z are all finite (tsar_cloud_distance's rule)
 *   origin o = the per-axis float32 minimum over the candidates (exact in any order)
 *   cell of a point, per axis: floor(((double)p - (double)o) / (double)V), in float64, the quotient correctly rounded (the cell function
 *     of tsar_cloud_distance with e = V); a cloud of 2^21 cells or more on an axis is refused
 *   voxel key = z << 42 | y << 21 | x;  the occupied voxels are numbered 0 .. n_voxels - 1 in ascending key order
 *   rank[i]  = the number of point i's voxel, -1 for a record that is no candidate
 *   count[v] = the number of candidates in voxel v
 *   rep[v]   = the index of the candidate of v nearest the cell's centre: per axis c = (double)o + ((double)cell + 0.5) * (double)V (one
 *     product, then one sum), d = (double)p - c;  d2 = (dx * dx + dy * dy) + dz * dz in float64;  d2f = (float)d2;  the winner has the
 *     minimal 64-bit code bits(d2f) << 32 | i: the smallest d2f, then the smallest index.  A real input point: row rep[v] of the cloud
 *     keeps its whole record (normal, colour)
 *   within[v][k] = the number of candidates i of v with dist2[i] <= fl(tol[k] * tol[k]) (one float32 product; NaN and +inf never pass)
 *   n_valid  = the number of candidates
 * The per-voxel outputs hold `cap` voxels: *n_voxels_out is the number found and may exceed cap; then the first cap voxels are written
 * and the call still succeeds (like tsar_fuse).  Entries from min(n_voxels, cap) on are not written.  Minima and integer counts of
 * bit-defined quantities: no output depends on an order of arrival, and every run gives the same bits.  n == 0 or no candidate: zero
 * voxels, every rank -1, success.
 * TSAR_ERR_INVALID, with the reason in tsar_last_error: p NULL; mem unknown; a stride below 3; n negative or above 2^31 - 1; voxel not
 * finite or not > 0; 2^21 cells or more on an axis; n_tol > 0 with dist2 or tol NULL, or with a tolerance not finite or not > 0;
 * within_out given with n_tol == 0; cap < 0.
 * tsar_cloud_voxels_ctx needs no views and no state, runs on the context's stream and changes nothing in the context; its temporaries
 * never grow the context's scratch arena.  tsar_cloud_voxels is the context-free form.  Timed as "cloud_bounds", "voxel_keys",
 * "cloud_sort", "voxel_heads", "voxel_scan", "voxel_reduce" and "voxel_finish". */
typedef struct tsar_cloud_voxels_params {
    float voxel;          /* V: the voxel edge; finite and > 0.  No default (0): the caller's scale */
} tsar_cloud_voxels_params;
void tsar_default_cloud_voxels_params(tsar_cloud_voxels_params* p);
int tsar_cloud_voxels_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_voxels_params* p,
                          const float* dist2 /* [n] or NULL */, int n_tol, const float* tol /* host; NULL with n_tol 0 */,
                          int32_t* rank_out /* [n] or NULL */, int64_t cap, int32_t* rep_out /* [cap] or NULL */,
                          int32_t* count_out /* [cap] or NULL */, int32_t* within_out /* [cap][n_tol] or NULL */,
                          int64_t* n_voxels_out, int64_t* n_valid_out /* host, may be NULL */, int mem);
int tsar_cloud_voxels(int device, const float* cloud, int64_t n, int stride, const tsar_cloud_voxels_params* p, const float* dist2,
                      int n_tol, const float* tol, int32_t* rank_out, int64_t cap, int32_t* rep_out, int32_t* count_out,
                      int32_t* within_out, int64_t* n_voxels_out, int64_t* n_valid_out, int mem);

/* ---- neighbourhood statistics of a cloud (removing stray points from a fused cloud before it is thinned or scored) ----------------- */
/* Per point of one cloud: how many other points lie within a radius R, and the k smallest squared distances among those.  Records are
 * `stride` float32 each (>= 3), x y z first.  `mem` names where cloud, count_out and knn_dist2_out lie; n_valid_out and pairs_out are host
 * memory.  The arithmetic, the same in both arithmetic modes: float32, every operation one IEEE-754 operation rounded to nearest, no
 * fused multiply-add.
 *   candidate: a record whose x, y and z are all finite (tsar_cloud_distance's rule)
 *   for candidates i and j:  dx = xi - xj, dy = yi - yj, dz = zi - zj;  d2(i, j) = (dx * dx + dy * dy) + dz * dz (tsar_cloud_distance's)
 *   R2 = fl(R * R), one float32 product
 *   count[i] = the number of candidates j != i with d2(i, j) <= R2.  The point itself is excluded by its index, not by its distance: a
 *     duplicate of the point counts, with d2 = +0.  count[i] = -1 for a record that is no candidate
 *   knn_dist2[i][0 .. k) = the k smallest values, ascending, of the multiset { d2(i, j) : j != i, j a candidate, d2(i, j) <= R2 }, padded
 *     with +inf where the multiset has fewer than k values; all +inf for a record that is no candidate.  A multiset of values: ties
 *     need no index rule
 *   n_valid = the number of candidates
 *   pairs = the number of (i, j) the call looked at: the sum over the candidates i of the candidates in the 27 cells around i's, the
 *     point itself included
 * Integer counts and order statistics of bit-defined values: no output depends on an order of arrival, and every run gives the same
 * bits.  How the pairs are found changes none of them: tsar_cloud_distance's grid over the candidates (origin = their per-axis minimum,
 * cell edge (double)R * (1 + 2^-10), the float64 cell function), and the argument written there carries over: two points with d2 <= R2
 * lie in cells that differ by at most 1 per axis, so the 27 cells hold every pair that counts.
 * n == 0 or no candidate: success, every count -1, n_valid 0, pairs 0.
 * TSAR_ERR_INVALID, with the reason in tsar_last_error: p NULL; mem unknown; a stride below 3; n negative or above 2^31 - 1; radius not
 * finite, or fl(R * R) not finite or not > 0; k outside 0 .. TSAR_CLOUD_KNN_MAX; knn_dist2_out given with k == 0; max_pairs negative; a
 * grid of 2^20 cells or more on an axis (radius is too small for the cloud's extent); more than max_pairs pairs — then *pairs_out is
 * still filled and nothing else is written.
 * tsar_cloud_neighbors_ctx needs no views and no state, runs on the context's stream and changes nothing in the context; its temporaries
 * (24 bytes per point, 16 per candidate and the sort's scratch) are pieces of the call's frame that never grow the context's scratch arena.  tsar_cloud_neighbors is
 * the context-free form, like tsar_cloud_voxels.  Timed as "cloud_bounds", "cloud_keys", "cloud_sort", "cloud_gather", "cloud_pairs" and
 * "cloud_neighbors" (the search, and the pass that marks the records that are no candidates). */
#define TSAR_CLOUD_KNN_MAX 32
typedef struct tsar_cloud_neighbors_params {
    float radius;         /* R: finite, fl(R * R) finite and > 0.  No default (0): the caller's scale */
    int32_t k;            /* 0 .. TSAR_CLOUD_KNN_MAX: how many nearest neighbours' distances to return; 0 = counts only */
    int64_t max_pairs;    /* as tsar_cloud_distance: a call that would look at more pairs is refused; default 1 << 40 */
} tsar_cloud_neighbors_params;
void tsar_default_cloud_neighbors_params(tsar_cloud_neighbors_params* p);
int tsar_cloud_neighbors_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_neighbors_params* p,
                             int32_t* count_out /* [n] or NULL */, float* knn_dist2_out /* [n][k] or NULL */,
                             int64_t* n_valid_out, int64_t* pairs_out /* host, may be NULL */, int mem);
int tsar_cloud_neighbors(int device, const float* cloud, int64_t n, int stride, const tsar_cloud_neighbors_params* p, int32_t* count_out,
                         float* knn_dist2_out, int64_t* n_valid_out, int64_t* pairs_out, int mem);

/* ---- normals of a cloud (a scan has none: this gives a reconstruction's normals something to be judged against) -------------------- */
/* tsar_cloud_normals: per point of one cloud the indices of its k nearest neighbours within a radius R, and the PCA normal and surface
 * variation of that neighbourhood.  Records are `stride` float32 each (>= 3), x y z first.  `mem` names where cloud and the five per-point
 * outputs lie; n_valid_out, n_normals_out and pairs_out are host memory.  Every output may be NULL.  The arithmetic, the same in both
 * arithmetic modes: every operation one IEEE-754 operation rounded to nearest, no fused multiply-add; float64 `/` and sqrt correctly
 * rounded.
 * Neighbours (float32):
 *   candidate, d2(i, j) and R2 = fl(R * R): those of tsar_cloud_neighbors
 *   point i's neighbour list = the candidates j != i with d2(i, j) <= R2, ordered by the 64-bit code bits(d2) << 32 | j (the smallest d2
 *     first, then the smallest index), cut at k.  m = its length.  The point itself is excluded by its index: a duplicate counts
 *   knn_index[i][s] = the s-th j for s < m, -1 from m on;  n_used[i] = m.  A record that is no candidate: n_used -1, every index -1
 * Moments (float64, relative to the point, in list order s = 0 .. m - 1):
 *   u = (double)p_j - (double)p_i per axis;  S_a += u_a;  Q_ab += u_a * u_b (one product, one sum), both from 0
 *   M = (double)(m + 1): the point itself is part of its neighbourhood, with u = 0
 *   mu_a = S_a / M;  C_ab = Q_ab / M - mu_a * mu_b;  cov = C_xx C_xy C_xz C_yy C_yz C_zz
 * Eigenvectors (float64): cyclic Jacobi on a = C, V = I, exactly 6 sweeps; a sweep is the rotations (p, q, r) = (0, 1, 2), (0, 2, 1),
 * (1, 2, 0); a rotation is skipped iff a_pq == 0, otherwise
 *   theta = (a_qq - a_pp) / (2 * a_pq);  t = (theta < 0 ? -1 : 1) / (|theta| + sqrt(theta * theta + 1));  c = 1 / sqrt(t * t + 1);  s = t * c
 *   h = t * a_pq;  a_pp = a_pp - h;  a_qq = a_qq + h;  a_pq = 0
 *   (a_rp, a_rq) <- (c * a_rp - s * a_rq, s * a_rp + c * a_rq);  for each row k of V: (v_kp, v_kq) <- (c * v_kp - s * v_kq, s * v_kp + c * v_kq)
 *   lambda0 = the smallest diagonal entry of a, the lowest index on ties;  v = that column of V
 * Orientation: first the canonical sign: if the component of v with the largest magnitude (the lowest index on ties) is < 0, v = -v.
 *   orient 1: w = (double)viewpoint - (double)p_i;  d = (v_x * w_x + v_y * w_y) + v_z * w_z;  v = -v iff d < 0
 *   orient 2: the same with w = the record's floats 3 .. 5 widened (its own normal); a NaN d leaves the canonical sign
 *   normal = (float)v per component, not renormalised
 * Curvature (surface variation): sum = (a_00 + a_11) + a_22;  curvature = (float)((lambda0 > 0 ? lambda0 : 0) / sum) if sum > 0, else 0
 * No normal: a record that is no candidate, or a point with m < min_neighbors: normal 0 0 0, curvature -1, cov 0 (knn_index and n_used are
 * still the list's).  n_normals = the number of points that have a normal; n_valid = the number of candidates; pairs as tsar_cloud_neighbors.
 * An order statistic of bit-defined codes, sums in list order and a fixed number of rotations: no output depends on an order of arrival,
 * and every run gives the same bits.  The pairs are found as in tsar_cloud_neighbors (the grid, the 27 cells).
 * TSAR_ERR_INVALID, with the reason in tsar_last_error: tsar_cloud_neighbors' refusals (p NULL; mem unknown; a stride below 3; n negative or
 * above 2^31 - 1; radius; max_pairs negative; 2^20 cells or more on an axis; more than max_pairs pairs, with *pairs_out still filled and
 * nothing else written); k outside 3 .. TSAR_CLOUD_KNN_MAX; min_neighbors outside 2 .. k; orient outside 0 .. 2; orient 2 with a stride
 * below 6; orient 1 with a viewpoint that is not finite.
 * tsar_cloud_normals_ctx needs no views and no state, runs on the context's stream and changes nothing in the context; its temporaries are
 * pieces of the call's frame that never grow the context's scratch arena.  tsar_cloud_normals is the context-free form.  Timed as
 * "cloud_bounds", "cloud_keys", "cloud_sort", "cloud_gather", "cloud_pairs" and "cloud_normals" (search, moments and Jacobi in one kernel,
 * and the pass that marks the records that are no candidates).
 * This is the plain PCA normal over the k nearest neighbours within R: no orientation is propagated across the cloud, nothing is meshed. */
typedef struct tsar_cloud_normals_params {
    float radius;          /* R: finite, fl(R * R) finite and > 0.  No default (0): the caller's scale */
    int32_t k;             /* 3 .. TSAR_CLOUD_KNN_MAX: the neighbours used at most; default 16 */
    int32_t min_neighbors; /* 2 .. k: a point with fewer neighbours within R gets no normal; default 5 */
    int32_t orient;        /* 0 the canonical sign (default), 1 towards viewpoint, 2 along the record's own normal (floats 3 .. 5; stride >= 6) */
    float viewpoint[3];    /* read with orient 1 */
    int64_t max_pairs;     /* as tsar_cloud_neighbors; default 1 << 40 */
} tsar_cloud_normals_params;
void tsar_default_cloud_normals_params(tsar_cloud_normals_params* p);
int tsar_cloud_normals_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_normals_params* p,
                           int32_t* knn_index_out /* [n][k] or NULL */, int32_t* n_used_out /* [n] or NULL */, float* normal_out /* [n][3] or NULL */,
                           float* curvature_out /* [n] or NULL */, double* cov_out /* [n][6] or NULL */, int64_t* n_valid_out,
                           int64_t* n_normals_out, int64_t* pairs_out /* host, may be NULL */, int mem);
int tsar_cloud_normals(int device, const float* cloud, int64_t n, int stride, const tsar_cloud_normals_params* p, int32_t* knn_index_out,
                       int32_t* n_used_out, float* normal_out, float* curvature_out, double* cov_out, int64_t* n_valid_out,
                       int64_t* n_normals_out, int64_t* pairs_out, int mem);

/* tsar_cloud_normal_compare: the agreement of the normals of cloud a with those of cloud b, as integer counts.  normal_a: n rows of stride_a
 * float32 (>= 3), the normal first; normal_b: n_b rows of stride_b; index [n] int32: per row of a the row of b it is compared with, or -1
 * (tsar_cloud_distance's index_out); dist2 [n] float32 or NULL, with max_dist.  These and cos_out lie in `mem`; min_cos (n_tol thresholds,
 * 0 .. 16, each in [-1, 1]) and the int64 outputs are host memory.  Row i is compared iff
 *   0 <= index[i] < n_b;  dist2 is NULL or dist2[i] <= fl(max_dist * max_dist) (one float32 product; NaN fails);  all six components finite;
 *   aa = (a_x * a_x + a_y * a_y) + a_z * a_z > 0 and bb likewise, in float64 on the widened floats
 * and then c = ((a_x * b_x + a_y * b_y) + a_z * b_z) / sqrt(aa * bb) in float64, c = |c| unless is_signed.
 *   cos_out[i] = (float)c, NaN for a row that is not compared;  within[k] = the compared rows with c >= min_cos[k];  n_compared
 * No angle is formed: a caller turns degrees into min_cos with one host cos.  Integer sums: the same in every run.
 * TSAR_ERR_INVALID: mem unknown; n or n_b negative or above 2^31 - 1; a stride below 3; normal_a or index NULL with n > 0, normal_b NULL with
 * n_b > 0; n_tol outside 0 .. 16, or min_cos NULL with n_tol > 0; a threshold outside [-1, 1]; with dist2, max_dist not finite or
 * fl(max_dist * max_dist) not finite or not > 0.  The _ctx form needs no views and no state and changes nothing in the context; timed as
 * "cloud_normal_compare". */
#define TSAR_NORMAL_COMPARE_MAX_TOL 16
int tsar_cloud_normal_compare_ctx(tsar_ctx* ctx, const float* normal_a, int stride_a, int64_t n, const float* normal_b, int stride_b, int64_t n_b,
                                  const int32_t* index, const float* dist2 /* [n] or NULL */, float max_dist, int n_tol,
                                  const double* min_cos /* host */, int is_signed, float* cos_out /* [n] or NULL */,
                                  int64_t* within_out /* host [n_tol] or NULL */, int64_t* n_compared_out /* host, may be NULL */, int mem);
int tsar_cloud_normal_compare(int device, const float* normal_a, int stride_a, int64_t n, const float* normal_b, int stride_b, int64_t n_b,
                              const int32_t* index, const float* dist2, float max_dist, int n_tol, const double* min_cos, int is_signed,
                              float* cos_out, int64_t* within_out, int64_t* n_compared_out, int mem);

/* ---- a cloud rendered into a camera, and a depth map scored against such a map ------------------------------------------------------- */
/* tsar_cloud_render: a point cloud (a scan, a fused cloud) rendered into one calibrated view as a depth map, occlusion by the cloud's own
 * points handled: per pixel the depth of the front-most point that lands on it, how many points support that depth, and which point it is.
 * Records are `stride` float32 each (>= 3), x y z first, so tsar_fuse's 9-float records go in as they are.  `mem` names where cloud,
 * depth_out, count_out and index_out lie; cam, p and n_splats_out are host memory.
 * Two buffers, because one is not enough: a pixel's depth comes only from points that land ON that pixel (a splat of constant depth over a
 * footprint would pull every slanted surface forward), while the footprint of a point only OCCLUDES: it hides what lies clearly behind it
 * on the neighbouring pixels, so that a thin cloud does not show the background through the holes of its foreground.
 * The arithmetic, the same in both arithmetic modes: float32, every operation one IEEE-754 operation rounded to nearest, no fused
 * multiply-add.
 *   P (3 x 4), formed on the host in float64 from the float32 K, R, t and rounded once to float32 per element:
 *     P[k][j] = (K[k][0] * R[0][j] + K[k][1] * R[1][j]) + K[k][2] * R[2][j], j = 0, 1, 2;   P[k][3] = (K[k][0] * t[0] + K[k][1] * t[1]) + K[k][2] * t[2]
 *   candidate: a record whose x, y and z are all finite
 *   p_k = ((P[k][0] * x + P[k][1] * y) + P[k][2] * z) + P[k][3], k = 0, 1, 2
 *   x' = p_0 / p_2, y' = p_1 / p_2 (correctly rounded);  xi = floor(x' + 0.5), yi = floor(y' + 0.5) (the sum rounded first)
 *   lands = candidate and p_2 > 0 and p_2 < inf and 0 <= xi <= w - 1 and 0 <= yi <= h - 1 (NaN fails every comparison): the point lands
 *           on pixel (xi, yi) at depth p_2 (tsar_geom_reproject's chain from p_k on)
 *   footprint half-width: fr = fl(K[0] * radius), one float32 product;  s = (int)min(floor(fr / p_2 + 0.5), max_px) in float32 (the
 *           quotient correctly rounded, the sum rounded first); radius == 0 gives s = 0.  The footprint of a point that lands is the square
 *           [xi - s, xi + s] x [yi - s, yi + s] clipped to the image.  A point whose centre is outside the image does not land and takes
 *           no part at all: its footprint does not reach in from outside.
 * and then for every pixel:
 *   Zc, index = the minimal 64-bit code bits(p_2) << 32 | i over the points i that land on it: the front-most depth, and the smallest index
 *           among the front-most (positive finite floats order like their bits)
 *   Zo    = the minimum of p_2 over the points whose footprint covers the pixel (the centre pixel is covered: Zo <= Zc)
 *   visible = something landed and Zc - Zo <= occlusion_diff * Zo
 *   count = the number of points landing on the pixel with |p_2 - Zc| <= depth_diff * Zc (the winner counts itself)
 *   kept  = visible and count >= min_points
 *   count_out = min(count, 255) where something landed, else 0;  depth_out = Zc where kept, else 0;  index_out = index where kept, else -1
 *   n_splats = the sum over the points that land of their clipped footprint's size (n_landing when radius == 0): the scatter's atomics
 * Minima, integer sums and bit-defined comparisons: no output depends on the order of arrival, and every run gives the same bits.
 * A call with n_splats > max_splats is refused before anything is written, with *n_splats_out still filled (max_pairs' rule of
 * tsar_cloud_distance): a radius as large as the scene is 1089 atomics per point at max_px = 16.
 * TSAR_ERR_INVALID, with the reason in tsar_last_error: cam or p NULL; cloud NULL with n > 0; all three outputs NULL; mem unknown; a stride
 * below 3; n negative or above 2^31 - 1; w or h below 1, w + 2 or h + 2 not below 2^23 (the context's 24-bit addressing limit) or w * h
 * above 2^31 - 1; radius negative or not finite, or fl(K[0] * radius) negative or not finite; max_px outside [1, 16]; occlusion_diff or
 * depth_diff negative or not finite; min_points outside [1, 255]; max_splats negative; more than max_splats splats.
 * tsar_cloud_render_ctx needs no views and no state, runs on the context's stream and changes nothing in the context; its temporaries (the
 * two z-buffers and the counts) are pieces of the call's frame that never grow the context's scratch arena.  tsar_cloud_render is the
 * context-free form.  Timed as "cloud_render_count", "cloud_render_scatter", "cloud_render_support" and "cloud_render_resolve". */
typedef struct tsar_cloud_render_params {
    float radius;             /* world units: the half-width of a point's occluder footprint; 0 = no footprint (a plain one-pixel z-buffer).  No default (0): the caller's scale */
    int32_t max_px;           /* caps the footprint half-width in pixels; default 8, in [1, 16] */
    float occlusion_diff;     /* relative, default 0.02: a pixel whose front-most landing lies further than this behind the occluder buffer is hidden */
    float depth_diff;         /* relative, default 0.01: a landing supports the pixel's depth Zc when it is within depth_diff * Zc of it */
    int32_t min_points;       /* default 1, in [1, 255]: depth_out is Zc only where at least this many landings support it */
    int64_t max_splats;       /* a call that would issue more footprint atomics than this is refused; default 1 << 34 */
} tsar_cloud_render_params;
void tsar_default_cloud_render_params(tsar_cloud_render_params* p);
int tsar_cloud_render_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_camera* cam, int w, int h,
                          const tsar_cloud_render_params* p, float* depth_out /* [h][w] or NULL */, uint8_t* count_out /* [h][w] or NULL */,
                          int32_t* index_out /* [h][w] or NULL */, int64_t* n_splats_out /* host, may be NULL */, int mem);
int tsar_cloud_render(int device, const float* cloud, int64_t n, int stride, const tsar_camera* cam, int w, int h,
                      const tsar_cloud_render_params* p, float* depth_out, uint8_t* count_out, int32_t* index_out, int64_t* n_splats_out, int mem);

/* tsar_cloud_render_oriented: tsar_cloud_render with a normal-oriented occluder.  The square footprint at the constant depth p_2 stands in
 * front of a slanted surface's own neighbouring pixels: from a slope of about 2 on, a surface hides itself.  Here a point occludes as its
 * tangent disc of world radius `radius`: the depth of its plane along each pixel's ray, only where that ray meets the disc, cut to the
 * square that s allows.  It is still a square-clipped disc per point: nothing is meshed, and a point whose centre is outside the image
 * still takes no part.
 * Everything is tsar_cloud_render's (P, candidate, lands, s, the clipped square, n_splats, Zc and index, visible, count, kept and the three
 * outputs) except the value a point writes into the occluder buffer.  float32, every operation one IEEE-754 operation, no fused
 * multiply-add, unless stated.  The normal of point i is normals[i * normal_stride + 0..2], or with normals NULL the record's floats 3..5.
 *   on the host, in float64 from float32 elements, each element of A, M and C rounded once to float32:
 *     A = K R: A[k][j] = (K[k][0] * R[0][j] + K[k][1] * R[1][j]) + K[k][2] * R[2][j]  (P's first three columns); the cofactors below are
 *         float64 operations on the rounded A
 *     M = A^-1 by cofactors: c[i][j] = A[i1][j1] * A[i2][j2] - A[i1][j2] * A[i2][j1] with i1 = (i + 1) mod 3, i2 = (i + 2) mod 3 and j1, j2
 *         likewise;  det = (A[0][0] * c[0][0] + A[0][1] * c[0][1]) + A[0][2] * c[0][2];  M[j][i] = c[i][j] / det
 *     C[j] = -((R[0][j] * t[0] + R[1][j] * t[1]) + R[2][j] * t[2])  (the camera centre);   r2 = fl(radius * radius), one float32 product
 *   per point that lands, with its position X and normal n:
 *     oriented = n_0, n_1 and n_2 are all finite and not all zero
 *     a_k = X_k - C_k;   num = (n_0 * a_0 + n_1 * a_1) + n_2 * a_2;   g_j = (M[0][j] * n_0 + M[1][j] * n_1) + M[2][j] * n_2
 *   the centre pixel (xi, yi): covered, with the value p_2, always (so Zo <= Zc still holds)
 *   every other pixel (u, v) of the clipped square, u and v as float32:
 *     den = g_0 * u + (g_1 * v + g_2);   z = num / den (correctly rounded);   d_k = M[k][0] * u + (M[k][1] * v + M[k][2])
 *     e_k = z * d_k - a_k;   q = (e_0 * e_0 + e_1 * e_1) + e_2 * e_2
 *     an oriented point covers the pixel iff z > 0 and z < inf and q <= r2 (NaN fails every comparison), with the value z
 *     a point that is not oriented covers the whole clipped square with the value p_2: tsar_cloud_render's rule
 *   Zo = the float whose bits are the minimum of bits(value) over the points that cover the pixel (values are positive and finite)
 *   occluder_out = Zo where something covers the pixel, else 0
 *   n_covered = the number of (point, pixel) pairs that cover, centres included: an integer sum, the same whatever TSAR_RENDER_SKIP says;
 *           n_splats (the pixels examined) is tsar_cloud_render's, and max_splats bounds it in the same way, before anything is written
 * The result does not depend on the sign of n (num and den change sign together).  radius == 0 is allowed: s = 0, only centres cover, and
 * the result is the one-pixel render.  Minima and integer sums: every run gives the same bits.
 * `mem` names where cloud, normals and the four planes lie; cam, p, n_splats_out and n_covered_out (filled when the call succeeds; both may
 * be NULL) are host memory.
 * TSAR_ERR_INVALID: tsar_cloud_render's refusals, with all FOUR planes NULL in place of three; normals NULL with a stride below 6; normals
 * given with normal_stride below 3; det == 0, or an element of M or C that is not finite.
 * The _ctx form needs no views and no state and changes nothing in the context, like tsar_cloud_render_ctx.  Timed as "cloud_splat_count",
 * "cloud_splat_scatter", "cloud_splat_support" and "cloud_splat_resolve". */
int tsar_cloud_render_oriented_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride,
                                   const float* normals /* [n][normal_stride], the normal first; NULL: the record's floats 3..5 */, int normal_stride,
                                   const tsar_camera* cam, int w, int h, const tsar_cloud_render_params* p, float* depth_out /* [h][w] or NULL */,
                                   uint8_t* count_out /* [h][w] or NULL */, int32_t* index_out /* [h][w] or NULL */, float* occluder_out /* [h][w] or NULL */,
                                   int64_t* n_splats_out /* host, may be NULL */, int64_t* n_covered_out /* host, may be NULL */, int mem);
int tsar_cloud_render_oriented(int device, const float* cloud, int64_t n, int stride, const float* normals, int normal_stride, const tsar_camera* cam,
                               int w, int h, const tsar_cloud_render_params* p, float* depth_out, uint8_t* count_out, int32_t* index_out,
                               float* occluder_out, int64_t* n_splats_out, int64_t* n_covered_out, int mem);

/* tsar_depth_compare: a depth map scored against a ground-truth map (tsar_cloud_render's, say) with the per-pixel bars: how many pixels
 * lie within each relative tolerance, how many in front, how many behind.  depth [n], gt [n] float32, mask [n] uint8 (NULL: every pixel)
 * and error_out [n] float32 (may be NULL) lie in `mem`; tol (n_tol relative tolerances, 1 <= n_tol <= 16) and the int64 outputs are host
 * memory; each output may be NULL.  float32, one IEEE operation per operator, no fused multiply-add.  With D = depth[i], G = gt[i]:
 *   ground-truth pixel: G > 0 and G < inf (NaN fails both) and mask[i] != 0
 *   n_gt      = the number of ground-truth pixels
 *   n_both    = the ground-truth pixels with D > 0 and D < inf
 *   within[k] = the n_both pixels with |D - G| <= fl(tol[k] * G)
 *   n_front   = the n_both pixels with D - G < -fl(tol[0] * G);  n_behind = those with D - G > fl(tol[0] * G)
 *   error_out[i] = (D - G) / G (correctly rounded) on the n_both pixels, NaN elsewhere
 * Only integer counts come back; a caller forms the ratios in float64: accuracy = within / n_both, completeness = within / n_gt, cover =
 * n_both / n_gt.  Integer sums: the same in every run.
 * TSAR_ERR_INVALID: depth, gt or tol NULL (depth and gt with n > 0); n negative or above 2^31 - 1; n_tol outside [1, 16]; a tolerance
 * negative or not finite; mem unknown.  The _ctx form needs no views and no state and changes nothing in the context; timed as
 * "depth_compare". */
#define TSAR_DEPTH_COMPARE_MAX_TOL 16
int tsar_depth_compare_ctx(tsar_ctx* ctx, const float* depth, const float* gt, const uint8_t* mask /* or NULL */, int64_t n, int n_tol,
                           const float* tol /* host */, int64_t* n_gt_out, int64_t* n_both_out, int64_t* within_out /* host [n_tol] */,
                           int64_t* n_front_out, int64_t* n_behind_out, float* error_out /* [n] or NULL */, int mem);
int tsar_depth_compare(int device, const float* depth, const float* gt, const uint8_t* mask, int64_t n, int n_tol, const float* tol,
                       int64_t* n_gt_out, int64_t* n_both_out, int64_t* within_out, int64_t* n_front_out, int64_t* n_behind_out,
                       float* error_out, int mem);

/* ---- page-locked host buffers --------------------------------------------------------------- */
/* NULL on failure.  Replaces the reference's cudaMallocManaged host-visible planes (managed.h:7-15) on the host side of the
 * boundary: the caller's image / result buffers, allocated here, are DMA targets. */
void* tsar_host_alloc(size_t bytes);
void tsar_host_free(void* p);

/* ---- device buffers for a multi-GPU host -------------------------------------------------------- */
/* Plain device memory on `device` (NULL on failure) and a synchronous device-to-device copy between two devices of the node
 * (xGMI peer copy; also valid with dst_device == src_device).  tsar_gipuma --all --fuse keeps each view's result on the GPU
 * that matched it and gathers them to the fusing GPU with these, where the reference's pipeline goes through files
 * (scripts/courtyard.sh:29-48, x/1.sh:30). */
void* tsar_device_alloc(int device, size_t bytes);
void tsar_device_free(int device, void* p);
int tsar_device_write(int device, void* dst, const void* host_src, size_t bytes);     /* synchronous host -> device copy */
int tsar_device_read(int device, void* host_dst, const void* src, size_t bytes);      /* synchronous device -> host copy */
int tsar_peer_copy(int dst_device, void* dst, int src_device, const void* src, size_t bytes);

/* ---- measurement ------------------------------------------------------------------------- */
/* When enabled every kernel launch is bracketed by hipEvents on the context's stream. */
int tsar_enable_kernel_timing(tsar_ctx* ctx, int enable);
int tsar_reset_kernel_timing(tsar_ctx* ctx);
/* fills up to `cap` records, returns the number of distinct kernels in *n_out */
int tsar_get_kernel_timing(tsar_ctx* ctx, tsar_kernel_timing* out, int cap, int* n_out);

/* ---- self-tests ---------------------------------------------------------------------------- */
/* TSAR_FLAG_STRICT_DIV's perspective divide u = X / Z, v = Y / Z (getCorrespondingPoint_cu gipuma.cu:161-171, vecdiv4) is computed
 * with one v_rcp_f32 + Newton step and one residual correction per quotient instead of the compiler's IEEE division sequence, behind
 * an operand guard that falls back to the latter.  These run that code path on caller-supplied or device-generated operands so a
 * test can compare it with IEEE division (the host's `/`, or the device's) bit for bit.
 *   tsar_selftest_divide: host arrays in / out; ieee = 1 returns the device's IEEE quotients instead, ieee = 2 the fast mode's
 *   X * v_rcp_f32(Z) (with X = 1: the device's reciprocal itself, which the CPU oracle's restatement of the fast arithmetic reads).
 *   tsar_selftest_divide_random: 2^log2_triples (X, Y, Z) triples generated on the device (mode 0: like the tap loop's operands;
 *   1: any mantissa / sign, exponents across the guard range; 2: any bit pattern); guarded = 0 runs the form without the guard (the
 *   clamp-free tap loops; modes 0 and 1).  Returns the number of quotients that differ from `/` and of triples outside the guard. */
/* tsar_selftest_sqrt: the square root of the matching cost's tail (tsar_device_math.h sqrt_rsq_exact: v_rsq_f32 + one fused residual
 * correction instead of the compiler's IEEE sequence) against sqrtf on the device; mode 0 = every mantissa of two adjacent binades
 * (both exponent parities, 2^24 inputs: the enumeration), mode 1 = 2^24 random inputs with exponents across [2^-100, 2^100], mode 2 =
 * the control (the same inputs as mode 0 without the correction step: must report mismatches), mode 3 = 2^24 random mantissas spread over
 * the 67 binades the cost tail's operands can reach ([1e-10, 4.3e9]).  tsar_set_views runs modes 0 and 3 once per context before it
 * accepts 8-bit imagery, and REFUSES the views (TSAR_ERR_HIP) on a mismatch; there is no fallback to sqrtf. */
int tsar_selftest_sqrt(tsar_ctx* ctx, int mode, uint64_t seed, uint64_t* mismatches_out);
int tsar_selftest_divide(tsar_ctx* ctx, const float* X, const float* Y, const float* Z, size_t n, float* u_out, float* v_out, int ieee);
int tsar_selftest_divide_random(tsar_ctx* ctx, int log2_triples, uint64_t seed, int mode, int guarded, uint64_t* mismatches_out,
                                uint64_t* outside_guard_out);
/* Census of the propagation arms of the NEXT half-sweep of `colour` on the current state (nothing is modified): how many multi-view
 * evaluations the wave-uniform hypothesis loop of the sweep kernel runs, against what lane-local candidate queues would run
 * (gipuma.cu:553-555 early-outs; selftest_kernels.hip documents the eight counters). */
int tsar_selftest_sweep_census(tsar_ctx* ctx, int colour, uint64_t* out8);
/* Census behind the propagation memo: for the half-sweep of `colour` about to run, how many alive arms carry the plane the pixel
 * tried in the previous call of this function (memo_dev: w * h * 8 uint64 on the device, zeroed before the first call, updated by
 * each).  out8: [0] alive arms, [1] repeating the same arm's plane, [2] any arm's, [3] (wave, arm) pairs with an alive lane,
 * [4] of those, pairs in which every alive lane repeats, [5] sum over waves of max-over-lanes alive arms, [6] ... of fresh ones,
 * [7] sum over waves of ceil(fresh pairs of the wave / 64) = the propagation trips of the packed form. */
int tsar_selftest_sweep_repeat(tsar_ctx* ctx, int colour, void* memo_dev, uint64_t* out8);
/* Census of the sweep's partial-window pruning (kernels with variant bit 26): on = 1 starts counting in every
 * following sweep launch of this context, on = 0 stops and returns out32 = [refinement step 0..7][4]: (wave, hypothesis) pairs
 * checked, (wave, view) pairs they had, (wave, view) pairs left early, hypotheses scored a second time in full because a lane
 * accepted.  Launches that run no pruning kernel, or check no step, count nothing. */
int tsar_selftest_prune_census(tsar_ctx* ctx, int on, uint32_t* out32);
/* One stage of tsar_slic on caller-supplied HOST arrays, so that a test can hold every SLIC kernel to the outputs of the reference's
 * own per-pixel functions (gSLICr_seg_engine_shared.h:7-204, host-compiled from the reference where it lies: tests/golden/slic_ref.npz).
 * Centres are 32-byte records laid out like the reference's spixel_info (gSLICr_spixel_info.h:11-17: center 2 f32, color_info
 * 4 f32, id i32, no_pixels i32).  Uses s->spixel_size, s->coh_weight, s->color_space.
 *   stage 0  Cvt_Img_Space:            in0 = bgra u8[h*w*4]                          inout = float4[h*w]         (out)
 *   stage 1  Init_Cluster_Centers:     in0 = float4[h*w]                             inout = centres[mw*mh]      (out)
 *   stage 2  Find_Center_Association:  in0 = float4[h*w], in1 = centres[mw*mh]       inout = labels i32[h*w]     (in: previous, out)
 *   stage 3  Update_Cluster_Center + Finalize_Reduction_Result (mw = w / S, mh = h / S):
 *                                      in0 = float4[h*w], in1 = labels i32[h*w]      inout = centres[mw*mh]      (out)
 *   stage 4  Enforce_Connectivity, one pass: in0 = labels i32[h*w]                   inout = labels i32[h*w]     (out) */
int tsar_selftest_slic_stage(tsar_ctx* ctx, int stage, int w, int h, int mw, int mh, const tsar_slic_settings* s, const void* in0,
                             const void* in1, void* inout);

#ifdef __cplusplus
}
#endif
#endif /* TSAR_H_ */
