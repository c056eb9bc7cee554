/*
 * tsar_oracle.c — CPU ORACLE.  TEST INFRASTRUCTURE ONLY.
 *
 * A plain-C restatement of the PatchMatch / TSAR hot path of ZhenlongYuan/TSAR-MVS
 * (reference gipuma.cu, main.cpp).  Nothing under oracle/ is linked, imported or executed by the
 * product (libtsar_hip.so, tsar_mvs_amd/); only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may use it, and only as the checker / the reported CPU baseline.
 *
 * PARITY: UNPINNED for everything restated from gipuma.cu / main.cpp.  The reference ships no tests, golden vectors or sample
 * outputs, and those two files cannot be built in this image (they need nvcc, the CUDA headers/runtime, cuRAND and
 * OpenCV; none are present and stand-ins for them are not allowed).  This file is therefore pinned by analytic known answers
 * authored in tests/ (a plane that truly generated the images scores ~0, homography of a fronto-parallel plane is the expected
 * translation, plane<->depth round trips, etc.), not by outputs of gipuma.cu — and by a second restatement written from the
 * reference's text in another language and loop structure (tests/test_oracle_independent_float64.py: the matching cost, numpy
 * float64; tests/test_oracle_independent_sweep.py: init, the eight arms, the accept tests and the refinement steps, numpy float32,
 * bit for bit against this file built with -DORC_NO_FMA).
 * PINNED BY THE REFERENCE ITSELF are the two pieces of it that a host compiler takes as they stand (oracle/Makefile `ref`,
 * built from the sources where they lie; outputs recorded by tests/golden/make_slic_ref_golden.py):
 *   - config.h:60-240, the 3x3 array macros getHomography_cu is made of (outer_product, matdivide, matmatsub2, matmul_cu,
 *     matvecmul): mat3mul / mat3vec / homography below, built with -DORC_NO_FMA, reproduce them BIT FOR BIT
 *     (tests/test_reference_macros_golden.py) — operand order and the element-wise division by d are the reference's;
 *   - gSLICr_Lib/engines/gSLICr_seg_engine_shared.h:7-204 — see tsar_oracle_slic.c.
 *
 * Each function cites the reference lines it restates.  Where the reference is non-deterministic
 * or undefined, the deterministic semantics chosen are:
 *   S1 RNG: stateless Philox4x32-10, key = seed, counter = (pixel, stream, step, 0); the reference
 *      re-seeds XORWOW with clock64() in every kernel (gipuma.cu:700,1077).
 *   S2 propagation reads neighbours from the state as it was when the launch started (Jacobi);
 *      the reference races on same-colour neighbours (gipuma.cu:958-1034).
 *   S3 image reads: clamp-to-edge addressing, exact fp32 bilinear weights (CUDA uses 8 fractional
 *      bits; tex2D does not exist on gfx950).  S3' (ORC_FLAG_TEX_FILTER_8BIT): the two filter
 *      fractions are rounded to 8 fractional bits first, as the CUDA texture unit stores them
 *      (1.8 fixed point); its rounding rule is unpublished, round-to-nearest-even is used here.
 *   S4 fused multiply-adds appear exactly where fmaf() is written here; everything else is a
 *      single IEEE operation (compile with -ffp-contract=off).  rsqrtf -> 1/sqrtf, exp -> the
 *      polynomial orc_expf below (both sides of the parity check implement the same polynomial).
 *   S5 reference quirks 1,2 (down_far seed, inverted right_far compare) are reproduced unless the
 *      FIX flags are set; the out-of-bounds read of quirk 1 (y<3) is defined as c[down_far].
 *   S6 ratio = c0/c1 needs two selected views; with one it is defined as 0 (reference reads an
 *      uninitialised slot, gipuma.cu:505).
 *
 * The geometric-consistency term (geom_term, orc_set_geom, orc_pm_rescore) is not in the reference: it is restated from its
 * statement in include/tsar.h (tsar_set_geom_depths, tsar_pm_rescore), not from the kernels.  The plane-prior term (prior_term,
 * orc_set_plane_prior) is not in the reference either, and is restated the same way: from the text of include/tsar.h
 * (tsar_set_plane_prior), one IEEE operation per operator of that text, not from the kernels.  It takes the prior as the context holds
 * it (tsar_get_plane_prior), so the world-to-camera conversion of the normals stays orc_load_planes's.
 *
 * Build: see oracle/Makefile (gcc -O2 -ffp-contract=off -mfma -fopenmp -shared).
 */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

/* -DORC_NO_FMA (oracle/Makefile: libtsar_oracle_nofma.so) writes every fmaf(a, b, c) of S4 as a * b + c, two roundings: the build
 * that can be held BIT FOR BIT to the reference's own config.h macros compiled by g++ without contraction
 * (tests/test_reference_macros_golden.py) — it pins which operands meet in which order; where nvcc fuses is S4's assumption. */
#ifdef ORC_NO_FMA
#define fmaf(a, b, c) ((a) * (b) + (c))
#endif

#define ORC_MAX_VIEWS 64
#define ORC_MAXCOST 2.0f
#define ORC_FLAG_FIX_DOWN_FAR_SEED (1u << 0)
#define ORC_FLAG_FIX_RIGHT_FAR_CMP (1u << 1)
#define ORC_FLAG_TEX_FILTER_8BIT (1u << 5)
#define ORC_FLAG_FIX_INIT_RADIUS (1u << 6) /* gipuma_init_cu2 on the sweeps' window instead of its own box / 2 (gipuma.cu:693-694) */
/* S7: the arithmetic of the HIP library's default ("fast") mode, restated so that the mode bench.py times can be checked bit for
 * bit too, not only statistically.  It is the reference's algorithm with seven ROUNDING liberties, none of which changes which
 * operations are done on which data:
 *   (1) the per-tap perspective divide is one reciprocal and two multiplies, u = X * rcp(Z), v = Y * rcp(Z), where rcp is the
 *       GPU's v_rcp_f32 (1 ulp) — a hardware function, so the oracle evaluates it from a table of its 2^23 mantissa results that the
 *       test reads from the device once (orc_set_rcp_table; the exponent is handled exactly);
 *   (2) the plane homography as H = A - b m^T with A = K R K_ref^-1 and b = K t folded per view in double precision on the host,
 *       m = K_ref^-T n * rcp(d);
 *   (3) the cross sum accumulates (w s) r instead of (w r) s;
 *   (4) positions are clamped to [0, w - 1] x [0, h - 1] instead of [-1, w] x [-1, h] — the same sample bit for bit (edge
 *       replication), so the oracle's bilinear() serves both;
 *   (5) ORC_FLAG_ROW_ORDER: the three source sums run over the window row by row (x fastest) instead of column by column
 *       (what the 8-bit-imagery kernels do; float imagery keeps columns);
 *   (6) the bilinear blend as (t00 + ax d1) + ay (d2 + ax d3) over the texel differences d1 = t10 - t00, d2 = t01 - t00,
 *       d3 = t11 - t10 - t01 + t00 (bilinear_qd): the reference's top-row interpolation as it stands, and "bottom row minus top row"
 *       formed as ONE fused multiply-add on the differences where the reference interpolates the bottom row and subtracts
 *       (gipuma's tex2D blend: three roundings there, one here).  Three FMAs per tap.
 *   (7) the tap position as m[1] y + (m[0] x + m[2]), two fused operations per coordinate with the inner one shared by a window
 *       line, where getCorrespondingPoint_cu's matvecmul4noz (config.h:150-162) adds the constant LAST, (m[0] x + m[1] y) + m[2].
 *       (Rounds 1-5 evaluated the strict mode this way too — a reassociation nobody had stated; the second, independent restatement
 *       of the cost, tests/test_oracle_independent_sweep.py, found it at the end of round 5 and strict mode now keeps the text's.)
 * The strict mode (no flag) remains the restatement of the reference; this mode is pinned to it only through the tolerances
 * stated in tests/test_gpu_fast_mode.py. */
#define ORC_FLAG_FAST_ARITH (1u << 7)
#define ORC_FLAG_ROW_ORDER (1u << 8)

typedef struct {
    float K[9], Kinv[9], R[9], t[3]; /* pose relative to the reference camera (ref = K[I|0]) */
    float Minv[9], P34[3], C[3];     /* of P = K_ref [R|t] (cameraGeometryUtils.h:302-356) */
    float Rorig[9], RorigInv[9];
    float fx, fy, f, alpha, baseline, depthMin, depthMax;
    float A[9], b[3];                /* S7 (2): K R K_ref^-1 and K t */
} orc_camera;

typedef struct {
    int w, h, n_views;
    const float *img[ORC_MAX_VIEWS];
    orc_camera cam[ORC_MAX_VIEWS];
    int n_sel, sel[ORC_MAX_VIEWS];
    int hrad, vrad, n_best, cost_comb;
    int box_hsize, box_vsize;   /* as given: gipuma_init_cu2 derives its own radius from them */
    float min_disp, max_disp;
    uint32_t flags;
    uint64_t seed;
    /* LineState planes (linestate.h:12-47) */
    float *c, *norm4, *ratio, *depth, *scale, *lrdiff, *confid, *fakedepth;
    int32_t *beview, *canny;
    /* cannylines */
    int n_regions;
    float *region_text, *region_norm4, *region_size;
    int launch; /* number of red/black launches so far (RNG stream) */
    const float *rcp_table; /* S7 (1): v_rcp_f32 of 1 + m 2^-23 for m = 0 .. 2^23 - 1, borrowed */
    int rcp_out_of_range;   /* S7 (1): operands the table could not serve (zero, denormal, inf, nan, result not normal): must stay 0 */
    /* geometric-consistency term (include/tsar.h, tsar_set_geom_depths): off unless geom_on */
    int geom_on;
    float geom_weight, geom_clip;
    const float *geom_depth[ORC_MAX_VIEWS];          /* view v's depth map [h][w], borrowed; NULL = no term for v */
    float geom_F[ORC_MAX_VIEWS][12], geom_B[ORC_MAX_VIEWS][12];   /* row-major 3 x 4, as given (tsar_get_geom_matrices) */
    /* plane-prior term (include/tsar.h, tsar_set_plane_prior): off unless prior != NULL */
    const float *prior;                              /* [h][w][4] = (q_x, q_y, q_z, Dp) as the context holds it, borrowed */
    float prior_wd, prior_wn, prior_dc, prior_nc;    /* weight_depth, weight_normal, depth_clip, normal_clip */
} orc_state;

/* ------------------------------------------------------------------------------------------ */
/* small algebra (config.h:36-241)                                                              */
static inline float dot3f(const float *a, const float *b) { return fmaf(a[2], b[2], fmaf(a[1], b[1], a[0] * b[0])); }
static inline void mat3vec(const float *m, const float *v, float *o) {
    o[0] = dot3f(m, v);
    o[1] = dot3f(m + 3, v);
    o[2] = dot3f(m + 6, v);
}
static inline void mat3mul(const float *a, const float *b, float *o) { /* matmul_cu config.h:204-240 */
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++)
            o[r * 3 + c] = fmaf(a[r * 3 + 2], b[6 + c], fmaf(a[r * 3 + 1], b[3 + c], a[r * 3] * b[c]));
}

/* exp() for x <= 0 (bilateral weight, gipuma.cu:268): Cody-Waite reduction + Cephes polynomial. */
float orc_expf(float x) {
    x = fmaxf(x, -87.0f);
    float k = rintf(x * 1.44269504f);
    float r = fmaf(k, -0.693145752f, x);
    r = fmaf(k, -1.42860677e-6f, r);
    float p = 1.9875691500e-4f;
    p = fmaf(p, r, 1.3981999507e-3f);
    p = fmaf(p, r, 8.3334519073e-3f);
    p = fmaf(p, r, 4.1665795894e-2f);
    p = fmaf(p, r, 1.6666665459e-1f);
    p = fmaf(p, r, 5.0000001201e-1f);
    float y = fmaf(p, r * r, r) + 1.0f;
    union { uint32_t u; float f; } s;
    s.u = (uint32_t)((int32_t)k + 127) << 23;
    return y * s.f;
}

/* Philox4x32-10 (Salmon et al. 2011), S1 */
static inline void philox4x32(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
    for (int r = 0; r < 10; r++) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
/* (0,1] like curand_uniform */
static inline float u01(uint32_t x) { return (float)((x >> 8) + 1u) * 5.9604644775390625e-8f; }
static inline void rng4(const orc_state *s, uint32_t pixel, uint32_t stream, uint32_t step, float u[4]) {
    uint32_t r[4];
    philox4x32(pixel, stream, step, 0u, (uint32_t)s->seed, (uint32_t)(s->seed >> 32), r);
    for (int i = 0; i < 4; i++) u[i] = u01(r[i]);
}
void orc_rng4(uint64_t seed, uint32_t pixel, uint32_t stream, uint32_t step, float *u) {
    orc_state s;
    s.seed = seed;
    rng4(&s, pixel, stream, step, u);
}
/* curand_between gipuma.cu:113-116 */
static inline float between(float u, float lo, float hi) { return fmaf(u, hi - lo, lo); }

/* ------------------------------------------------------------------------------------------ */
/* image access, S3                                                                            */
static inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
static inline float texel(const float *img, int w, int h, int x, int y) {
    return img[(size_t)clampi(y, 0, h - 1) * w + clampi(x, 0, w - 1)];
}
/* tex2D<float>(tex, u+0.5, v+0.5) with linear filtering, clamp addressing (main.cpp:1215-1219) */
static inline float bilinear_qd(const float *img, int w, int h, float u, float v, int q8, int diff);
static inline float bilinear_q(const float *img, int w, int h, float u, float v, int q8) { return bilinear_qd(img, w, h, u, v, q8, 0); }
/* diff (S7 (6), fast arithmetic only): the blend as (t00 + ax d1) + ay (d2 + ax d3) over the texel differences d1 = t10 - t00,
 * d2 = t01 - t00, d3 = (t11 - t01) - d1 (exact integers on 8-bit imagery), three FMAs */
static inline float bilinear_qd(const float *img, int w, int h, float u, float v, int q8, int diff) {
    u = fminf(fmaxf(u, -1.0f), (float)w);
    v = fminf(fmaxf(v, -1.0f), (float)h);
    float fu = floorf(u), fv = floorf(v);
    float ax = u - fu, ay = v - fv;
    if (q8) { ax = rintf(ax * 256.0f) * 0.00390625f; ay = rintf(ay * 256.0f) * 0.00390625f; } /* S3' */
    int x0 = (int)fu, y0 = (int)fv;
    float t00 = texel(img, w, h, x0, y0), t10 = texel(img, w, h, x0 + 1, y0);
    float t01 = texel(img, w, h, x0, y0 + 1), t11 = texel(img, w, h, x0 + 1, y0 + 1);
    if (diff) {
        const float d1 = t10 - t00, d2 = t01 - t00, d3 = (t11 - t01) - d1;
        return fmaf(ay, fmaf(ax, d3, d2), fmaf(ax, d1, t00));
    }
    float top = fmaf(ax, t10 - t00, t00);
    float bot = fmaf(ax, t11 - t01, t01);
    return fmaf(ay, bot - top, top);
}
static inline float bilinear(const float *img, int w, int h, float u, float v) { return bilinear_q(img, w, h, u, v, 0); }
float orc_bilinear(const float *img, int w, int h, float u, float v) { return bilinear(img, w, h, u, v); }
float orc_bilinear_q8(const float *img, int w, int h, float u, float v) { return bilinear_q(img, w, h, u, v, 1); }

/* ------------------------------------------------------------------------------------------ */
/* camera derivation (cameraGeometryUtils.h:270-356), double precision then rounded            */
static void inv3d(const double *m, double *o) {
    double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
    double id = 1.0 / det;
    o[0] = (m[4] * m[8] - m[5] * m[7]) * id;
    o[1] = (m[2] * m[7] - m[1] * m[8]) * id;
    o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = (m[5] * m[6] - m[3] * m[8]) * id;
    o[4] = (m[0] * m[8] - m[2] * m[6]) * id;
    o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = (m[3] * m[7] - m[4] * m[6]) * id;
    o[7] = (m[1] * m[6] - m[0] * m[7]) * id;
    o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}
static void mul3d(const double *a, const double *b, double *o) {
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) o[r * 3 + c] = a[r * 3] * b[c] + a[r * 3 + 1] * b[3 + c] + a[r * 3 + 2] * b[6 + c];
}
/* K,R,t: n_views x (9,9,3) floats, world->camera; view 0 is the reference */
void orc_derive_cameras(orc_state *s, int n_views, const float *K, const float *R, const float *t, float cam_scale,
                        float depth_min, float depth_max) {
    double R0[9], t0[3], K0[9];
    for (int i = 0; i < 9; i++) { R0[i] = R[i]; K0[i] = K[i]; }
    for (int i = 0; i < 3; i++) t0[i] = t[i];
    /* scaleK cameraGeometryUtils.h:143-154 */
    K0[0] /= cam_scale; K0[4] /= cam_scale; K0[2] /= cam_scale; K0[5] /= cam_scale;
    s->n_views = n_views;
    for (int v = 0; v < n_views; v++) {
        orc_camera *cm = &s->cam[v];
        double Kv[9], Rv[9], tv[3], Rrel[9], trel[3], R0t[9];
        for (int i = 0; i < 9; i++) { Kv[i] = K[v * 9 + i]; Rv[i] = R[v * 9 + i]; }
        for (int i = 0; i < 3; i++) tv[i] = t[v * 3 + i];
        Kv[0] /= cam_scale; Kv[4] /= cam_scale; Kv[2] /= cam_scale; Kv[5] /= cam_scale;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) R0t[r * 3 + c] = R0[c * 3 + r];
        mul3d(Rv, R0t, Rrel); /* [R|t] * [R0|t0]^-1 */
        for (int r = 0; r < 3; r++) trel[r] = tv[r] - (Rrel[r * 3] * t0[0] + Rrel[r * 3 + 1] * t0[1] + Rrel[r * 3 + 2] * t0[2]);
        if (v == 0) { /* exactly K[I|0] */
            for (int i = 0; i < 9; i++) Rrel[i] = (i % 4 == 0) ? 1.0 : 0.0;
            trel[0] = trel[1] = trel[2] = 0.0;
        }
        double Kvi[9], M[9], Mi[9], P34[3];
        inv3d(Kv, Kvi);
        mul3d(K0, Rrel, M); /* P built with the reference K for every camera (cameraGeometryUtils.h:302) */
        inv3d(M, Mi);
        for (int r = 0; r < 3; r++) P34[r] = K0[r * 3] * trel[0] + K0[r * 3 + 1] * trel[1] + K0[r * 3 + 2] * trel[2];
        for (int i = 0; i < 9; i++) {
            cm->K[i] = (float)Kv[i]; cm->Kinv[i] = (float)Kvi[i]; cm->R[i] = (float)Rrel[i]; cm->Minv[i] = (float)Mi[i];
            cm->Rorig[i] = (float)Rv[i];
        }
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) cm->RorigInv[r * 3 + c] = (float)Rv[c * 3 + r];
        for (int r = 0; r < 3; r++) {
            cm->t[r] = (float)trel[r];
            cm->P34[r] = (float)P34[r];
            cm->C[r] = (float)(-(Rrel[r] * trel[0] + Rrel[3 + r] * trel[1] + Rrel[6 + r] * trel[2]));
        }
        {   /* S7 (2): A = K R K_ref^-1, b = K t, in the library's own expression order (cofactors first, det along the first row) */
            double Ki[9], KR[9], A[9];
            const double c00 = K0[4] * K0[8] - K0[5] * K0[7], c01 = K0[5] * K0[6] - K0[3] * K0[8], c02 = K0[3] * K0[7] - K0[4] * K0[6];
            const double sdet = 1.0 / (K0[0] * c00 + K0[1] * c01 + K0[2] * c02);
            Ki[0] = c00 * sdet; Ki[1] = (K0[2] * K0[7] - K0[1] * K0[8]) * sdet; Ki[2] = (K0[1] * K0[5] - K0[2] * K0[4]) * sdet;
            Ki[3] = c01 * sdet; Ki[4] = (K0[0] * K0[8] - K0[2] * K0[6]) * sdet; Ki[5] = (K0[2] * K0[3] - K0[0] * K0[5]) * sdet;
            Ki[6] = c02 * sdet; Ki[7] = (K0[1] * K0[6] - K0[0] * K0[7]) * sdet; Ki[8] = (K0[0] * K0[4] - K0[1] * K0[3]) * sdet;
            mul3d(Kv, Rrel, KR);
            mul3d(KR, Ki, A);
            for (int i = 0; i < 9; i++) cm->A[i] = (float)A[i];
            for (int r = 0; r < 3; r++) cm->b[r] = (float)(Kv[r * 3] * trel[0] + Kv[r * 3 + 1] * trel[1] + Kv[r * 3 + 2] * trel[2]);
        }
        cm->fx = (float)K0[0]; cm->fy = (float)K0[4]; cm->f = (float)K0[0];
        cm->alpha = (float)K0[0] / (float)K0[4];
        cm->baseline = 1.0f; /* cameraGeometryUtils.h:309 */
        cm->depthMin = depth_min; cm->depthMax = depth_max;
    }
    /* main.cpp:1393-1398 */
    s->min_disp = s->cam[0].f * s->cam[0].baseline / depth_max;
    s->max_disp = s->cam[0].f * s->cam[0].baseline / depth_min;
}

/* ------------------------------------------------------------------------------------------ */
/* geometry helpers                                                                            */
/* -v through the sign bit.  Written as `-fmaf(a, b, c)` the compiler may emit ONE fused negate-multiply-subtract, (-a b) - c, which
 * differs from -(a b + c) in the sign of an exact zero (a b = +0, c = -0: -(+0) = -0, but (-0) - (-0) = +0).  A plane offset of
 * exactly +-0 (a plane through a point at depth 0: the weighted median filter at a tap whose lines->depth is infinite) then gives
 * a depth of -+0 and a disparity of -+inf, and inf - inf against inf + inf decides a pixel's reliability. */
static inline float neg_exact(float v) {
    uint32_t u;
    memcpy(&u, &v, 4);
    u ^= 0x80000000u;
    memcpy(&v, &u, 4);
    return v;
}
/* getD_cu gipuma.cu:71-86 */
static inline float getD(const float *n, int x, int y, float depth, const orc_camera *cm) {
    float pt[3], X[3];
    pt[0] = depth * (float)x - cm->P34[0];
    pt[1] = depth * (float)y - cm->P34[1];
    pt[2] = depth - cm->P34[2];
    mat3vec(cm->Minv, pt, X);
    return neg_exact(dot3f(n, X));
}
/* getDepthFromPlane3_cu / getDisparity_cu gipuma.cu:436-453 */
static inline float depth_from_plane(const orc_camera *cm, const float *n4, int x, int y) {
    float d = n4[3];
    if (d != d) return 1000.0f;
    float den = fmaf(n4[2], cm->fx, fmaf(n4[1] * ((float)y - cm->K[5]), cm->alpha, n4[0] * ((float)x - cm->K[2])));
    return (-d * cm->fx) / den;
}
/* getViewVector_cu gipuma.cu:97-105 (+ get3Dpoint_cu1 :57-67, normalize_cu :88-95) */
static inline void view_vector(const orc_camera *cm, int x, int y, float *v) {
    float pt[3], X[3];
    pt[0] = (float)x - cm->P34[0];
    pt[1] = (float)y - cm->P34[1];
    pt[2] = 1.0f - cm->P34[2];
    mat3vec(cm->Minv, pt, X);
    X[0] -= cm->C[0]; X[1] -= cm->C[1]; X[2] -= cm->C[2];
    float inv = 1.0f / sqrtf(dot3f(X, X));
    v[0] = X[0] * inv; v[1] = X[1] * inv; v[2] = X[2] * inv;
}
float orc_getD(const orc_state *s, const float *n, int x, int y, float depth) { return getD(n, x, y, depth, &s->cam[0]); }
float orc_depth_from_plane(const orc_state *s, const float *n4, int x, int y) { return depth_from_plane(&s->cam[0], n4, x, y); }
void orc_view_vector(const orc_state *s, int x, int y, float *v) { view_vector(&s->cam[0], x, y, v); }
/* depth_from_plane of planes[y][x] at (x, y), the whole image at once */
void orc_depth_from_planes(const orc_state *s, const float *planes, float *depth) {
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            depth[p] = depth_from_plane(&s->cam[0], planes + 4 * p, x, y);
        }
}

/* getHomography_cu gipuma.cu:207-224: H = K_to * ((R - t n^T / d) * K_ref^-1) */
static inline void homography(const orc_camera *ref, const orc_camera *to, const float *n4, float *H) {
    float M[9], T[9];
    for (int r = 0; r < 3; r++)   /* outer_product4, then matdivide: every element divided by d (config.h:139-148) */
        for (int c = 0; c < 3; c++) M[r * 3 + c] = to->R[r * 3 + c] - (to->t[r] * n4[c]) / n4[3];
    mat3mul(M, ref->Kinv, T);
    mat3mul(to->K, T, H);
}
void orc_homography(const orc_state *s, int view, const float *n4, float *H) { homography(&s->cam[0], &s->cam[view], n4, H); }
/* the same on bare arrays (tests/test_reference_macros_golden.py: against the reference's own config.h macros compiled on the host) */
void orc_homography_arrays(const float *K1_inv, const float *K2, const float *R, const float *t, const float *n4, float *H) {
    orc_camera ref, to;
    memcpy(ref.Kinv, K1_inv, 36); memcpy(to.K, K2, 36); memcpy(to.R, R, 36); memcpy(to.t, t, 12);
    homography(&ref, &to, n4, H);
}
void orc_mat3mul(const float *a, const float *b, float *o) { mat3mul(a, b, o); }
void orc_mat3vec(const float *m, const float *v, float *o) { mat3vec(m, v, o); }

/* S7 (1): v_rcp_f32 from the device's mantissa table; the exponent and sign are exact */
static inline float rcp_gpu(const orc_state *s, float x) {
    union { float f; uint32_t u; } a, r;
    a.f = x;
    const uint32_t e = (a.u >> 23) & 0xffu, m = a.u & 0x7fffffu;
    if (!s->rcp_table || e == 0 || e == 255) { ((orc_state *)s)->rcp_out_of_range = 1; return 1.0f / x; }
    r.f = s->rcp_table[m];                       /* in (0.5, 1]: exponent field 126, or 127 for m = 0 */
    const int re = (int)((r.u >> 23) & 0xffu) + 127 - (int)e;
    if (re <= 0 || re >= 255) { ((orc_state *)s)->rcp_out_of_range = 1; return 1.0f / x; }
    r.u = (a.u & 0x80000000u) | ((uint32_t)re << 23) | (r.u & 0x7fffffu);
    return r.f;
}
/* S7 (2): plane_homography_fast of the HIP library (tsar_device_math.h) */
static inline void homography_fast(const orc_state *s, const orc_camera *ref, const orc_camera *to, const float *n4, float *H) {
    const float inv_d = rcp_gpu(s, n4[3]);
    float m[3];
    for (int c = 0; c < 3; c++) m[c] = fmaf(n4[2], ref->Kinv[6 + c], fmaf(n4[1], ref->Kinv[3 + c], n4[0] * ref->Kinv[c])) * inv_d;
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) H[r * 3 + c] = fmaf(-to->b[r], m[c], to->A[r * 3 + c]);
}
/* pmCost in the fast arithmetic (S7).  The reference terms (weights, sum w, sum w r, sum w r^2) are the strict ones in the strict
 * order — the kernels hoist them per pixel in both modes; only the three source sums follow the liberties. */
static float pm_cost_fast(const orc_state *s, int view, int x, int y, const float *n4) {
    const float *l = s->img[0], *r = s->img[view];
    const int w = s->w, h = s->h;
    const int q8 = (s->flags & ORC_FLAG_TEX_FILTER_8BIT) != 0, rows = (s->flags & ORC_FLAG_ROW_ORDER) != 0;
    float H[9];
    homography_fast(s, &s->cam[0], &s->cam[view], n4, H);
    const float cen = texel(l, w, h, x, y);
    float sum_ref = 0, sum_ref_ref = 0, wsum = 0;
    for (int i = -s->hrad; i < s->hrad + 1; i += 2)
        for (int j = -s->vrad; j < s->vrad + 1; j += 2) {
            const float ref_pix = texel(l, w, h, x + i, y + j);
            const float wt = orc_expf(-sqrtf((float)(i * i + j * j)) / 50.0f - fabsf(ref_pix - cen) / 18.0f);
            const float wr = wt * ref_pix;
            sum_ref += wr;
            sum_ref_ref = fmaf(wr, ref_pix, sum_ref_ref);
            wsum += wt;
        }
    float sum_src = 0, sum_src_src = 0, sum_ref_src = 0;
    const int ro = rows ? s->vrad : s->hrad, ri = rows ? s->hrad : s->vrad;      /* radius of the outer / inner loop */
    for (int a = -ro; a < ro + 1; a += 2) {
        const float fa = (float)((rows ? y : x) + a);
        const float bx = fmaf(H[rows ? 1 : 0], fa, H[2]), by = fmaf(H[rows ? 4 : 3], fa, H[5]), bz = fmaf(H[rows ? 7 : 6], fa, H[8]);
        for (int b = -ri; b < ri + 1; b += 2) {
            const float fb = (float)((rows ? x : y) + b);
            const float X = fmaf(H[rows ? 0 : 1], fb, bx), Y = fmaf(H[rows ? 3 : 4], fb, by), Z = fmaf(H[rows ? 6 : 7], fb, bz);
            const int i = rows ? b : a, j = rows ? a : b;                      /* x and y offset of this tap */
            const float ref_pix = texel(l, w, h, x + i, y + j);
            const float wt = orc_expf(-sqrtf((float)(i * i + j * j)) / 50.0f - fabsf(ref_pix - cen) / 18.0f);
            const float rz = rcp_gpu(s, Z);
            const float src_pix = bilinear_qd(r, w, h, X * rz, Y * rz, q8, 1);
            const float ws = wt * src_pix;
            sum_src += ws;
            sum_src_src = fmaf(ws, src_pix, sum_src_src);
            sum_ref_src = fmaf(ws, ref_pix, sum_ref_src);
        }
    }
    const float inv = 1.0f / wsum;
    sum_ref *= inv; sum_ref_ref *= inv; sum_src *= inv; sum_src_src *= inv; sum_ref_src *= inv;
    const float var_ref = sum_ref_ref - sum_ref * sum_ref;
    const float var_src = sum_src_src - sum_src * sum_src;
    if (var_ref < 1e-5f || var_src < 1e-5f) return ORC_MAXCOST;
    const float covar = sum_ref_src - sum_ref * sum_src;
    const float vrs = sqrtf(var_ref * var_src);
    return fmaxf(0.0f, fminf(ORC_MAXCOST, 1.0f - covar / vrs));
}

/* ------------------------------------------------------------------------------------------ */
/* pmCost gipuma.cu:229-298: bilateral-weighted NCC over the dilated window                     */
static float pm_cost(const orc_state *s, int view, int x, int y, const float *n4) {
    if (s->flags & ORC_FLAG_FAST_ARITH) return pm_cost_fast(s, view, x, y, n4);
    const float *l = s->img[0], *r = s->img[view];
    const int w = s->w, h = s->h;
    float H[9];
    homography(&s->cam[0], &s->cam[view], n4, H);
    float cen = texel(l, w, h, x, y);
    float sum_ref = 0, sum_ref_ref = 0, sum_src = 0, sum_src_src = 0, sum_ref_src = 0, wsum = 0;
    for (int i = -s->hrad; i < s->hrad + 1; i += 2) {
        float xi = (float)(x + i);
        /* getCorrespondingPoint_cu gipuma.cu:161-171 = matvecmul4noz (config.h:150-162): (m[0] x + m[1] y) + m[2], the constant LAST
         * (S4: mul, fma, add); the x products are the same for a window column */
        float mx = H[0] * xi, my = H[3] * xi, mz = H[6] * xi;
        for (int j = -s->vrad; j < s->vrad + 1; j += 2) {
            float yj = (float)(y + j);
            float ref_pix = texel(l, w, h, x + i, y + j);
            float X = fmaf(H[1], yj, mx) + H[2], Y = fmaf(H[4], yj, my) + H[5], Z = fmaf(H[7], yj, mz) + H[8];
            float src_pix = bilinear_q(r, w, h, X / Z, Y / Z, (s->flags & ORC_FLAG_TEX_FILTER_8BIT) != 0);
            float sd = sqrtf((float)(i * i + j * j));
            float cd = fabsf(ref_pix - cen);
            float wt = orc_expf(-sd / 50.0f - cd / 18.0f);
            float wr = wt * ref_pix, ws = wt * src_pix;
            sum_ref += wr;
            sum_ref_ref = fmaf(wr, ref_pix, sum_ref_ref);
            sum_src += ws;
            sum_src_src = fmaf(ws, src_pix, sum_src_src);
            sum_ref_src = fmaf(wr, src_pix, sum_ref_src);
            wsum += wt;
        }
    }
    float inv = 1.0f / wsum;
    sum_ref *= inv; sum_ref_ref *= inv; sum_src *= inv; sum_src_src *= inv; sum_ref_src *= inv;
    float var_ref = sum_ref_ref - sum_ref * sum_ref;
    float var_src = sum_src_src - sum_src * sum_src;
    if (var_ref < 1e-5f || var_src < 1e-5f) return ORC_MAXCOST;
    float covar = sum_ref_src - sum_ref * sum_src;
    float vrs = sqrtf(var_ref * var_src);
    return fmaxf(0.0f, fminf(ORC_MAXCOST, 1.0f - covar / vrs));
}
float orc_pm_cost(const orc_state *s, int view, int x, int y, const float *n4) { return pm_cost(s, view, x, y, n4); }

/* sort_small gipuma.cu:425-434 */
static void sort_small(float *d, int n) {
    for (int i = 1; i < n; i++) {
        float tmp = d[i];
        int j;
        for (j = i; j >= 1 && tmp < d[j - 1]; j--) d[j] = d[j - 1];
        d[j] = tmp;
    }
}
/* The geometric-consistency term lambda e of view v for a hypothesis of depth D at (x, y), restated from the statement in
 * include/tsar.h (tsar_set_geom_depths): plain float operations, each one IEEE operation (-ffp-contract=off, no fmaf: the same in
 * every build of this file), the quotients '/', the root sqrtf, and the header's comparisons (NaN fails each one). */
static float geom_term(const orc_state *s, int view, int x, int y, float D) {
    const float *dm = s->geom_depth[view];
    if (!dm) return 0.0f;
    const float *F = s->geom_F[view], *B = s->geom_B[view];
    const float X = (float)x, Y = (float)y, tau = s->geom_clip;
    const float xd = X * D, yd = Y * D;
    const float a = ((F[0] * xd + F[1] * yd) + F[2] * D) + F[3];
    const float b = ((F[4] * xd + F[5] * yd) + F[6] * D) + F[7];
    const float sz = ((F[8] * xd + F[9] * yd) + F[10] * D) + F[11];
    const float u = a / sz, v = b / sz;
    const float c = floorf(u + 0.5f), r = floorf(v + 0.5f);
    const int inside = sz > 0.0f && c >= 0.0f && c <= (float)(s->w - 1) && r >= 0.0f && r <= (float)(s->h - 1);
    const float Dv = inside ? dm[(size_t)(int)r * s->w + (int)c] : 0.0f;
    const float cd = c * Dv, rd = r * Dv;
    const float p0 = ((B[0] * cd + B[1] * rd) + B[2] * Dv) + B[3];
    const float p1 = ((B[4] * cd + B[5] * rd) + B[6] * Dv) + B[7];
    const float p2 = ((B[8] * cd + B[9] * rd) + B[10] * Dv) + B[11];
    const float xq = p0 / p2, yq = p1 / p2;
    const float dx = xq - X, dy = yq - Y;
    const float e2 = dx * dx + dy * dy;
    float e;
    if (!(inside && Dv > 0.0f && p2 > 0.0f && e2 < tau * tau)) e = tau;
    else if (e2 < 0x1p-100f) e = 0.0f;
    else e = fminf(sqrtf(e2), tau);
    return s->geom_weight * e;
}
float orc_geom_term(const orc_state *s, int view, int x, int y, float D) { return geom_term(s, view, x, y, D); }

/* The plane-prior term t of a hypothesis n4 of depth D at (x, y), restated from the statement in include/tsar.h
 * (tsar_set_plane_prior) the way geom_term is: plain float operations, each one IEEE operation (-ffp-contract=off, no fmaf: the same
 * in every build of this file and in both arithmetic modes), the three quotients '/', the header's comparisons (NaN fails each one).
 * 0 where the pixel has no prior (the held entry is all zero there: Dp > 0 fails). */
static float prior_term(const orc_state *s, int x, int y, const float *n4, float D) {
    const float *q = s->prior + 4 * ((size_t)y * s->w + x);
    const float Dp = q[3];
    if (!(Dp > 0.0f)) return 0.0f;
    const float a = fabsf(D - Dp);
    const float rel = a / Dp;
    const float r_d = rel < s->prior_dc ? rel / s->prior_dc : 1.0f;
    const float sn = 1.0f - ((n4[0] * q[0] + n4[1] * q[1]) + n4[2] * q[2]);
    const float s0 = sn < 0.0f ? 0.0f : sn;
    const float r_n = sn < s->prior_nc ? s0 / s->prior_nc : 1.0f;
    return (s->prior_wd * r_d) + (s->prior_wn * r_n);
}

/* pmCostMultiview_cu gipuma.cu:455-518.  With a geometric term installed, view v's cost becomes c_v + lambda e_v after the validity
 * test (include/tsar.h); D is the hypothesis's depth at (x, y), once per hypothesis.  With a plane prior installed, a valid
 * hypothesis's cost becomes c + t after the best-N division at pixels that have a prior; best view and ratio are not touched. */
static float pm_cost_multiview(const orc_state *s, int x, int y, const float *n4, int *beview, float *ratio) {
    float cv[ORC_MAX_VIEWS], ov[ORC_MAX_VIEWS];
    int num = s->n_sel, valid = 0;
    const float D = (s->geom_on || s->prior) ? depth_from_plane(&s->cam[0], n4, x, y) : 0.0f;
    for (int i = 0; i < num; i++) {
        float c = pm_cost(s, s->sel[i], x, y, n4);
        if (c < ORC_MAXCOST) valid++; else c = ORC_MAXCOST;
        if (s->geom_on) c = c + geom_term(s, s->sel[i], x, y, D);
        cv[i] = c; ov[i] = c;
    }
    sort_small(cv, num);
    int nb = valid;
    if (s->cost_comb == 1) nb = nb < s->n_best ? nb : s->n_best;
    float cost;
    if (nb > 0) {
        cost = 0.0f;
        for (int i = 0; i < nb; i++) cost += cv[i];
        cost = cost / (float)nb;
        *ratio = num >= 2 ? cv[0] / cv[1] : 0.0f; /* S6 */
        *beview = -1;
        for (int i = 0; i < num; i++)
            if (cv[0] == ov[i]) *beview = s->sel[i];
        if (s->prior && s->prior[4 * ((size_t)y * s->w + x) + 3] > 0.0f) cost = cost + prior_term(s, x, y, n4, D);
    } else {
        cost = ORC_MAXCOST; *ratio = 0.0f; *beview = -1;
    }
    return cost;
}
float orc_pm_cost_multiview(const orc_state *s, int x, int y, const float *n4, int *beview, float *ratio) {
    return pm_cost_multiview(s, x, y, n4, beview, ratio);
}
void orc_pm_cost_planes(const orc_state *s, const float *planes, float *cost, int32_t *beview, float *ratio) {
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            int bv; float rt;
            cost[p] = pm_cost_multiview(s, x, y, planes + 4 * p, &bv, &rt);
            if (beview) beview[p] = bv;
            if (ratio) ratio[p] = rt;
        }
}

/* ------------------------------------------------------------------------------------------ */
/* gipuma_init_cu2 gipuma.cu:678-729: the random hypothesis of pixel (x, y) */
static void draw_plane(const orc_state *s, int x, int y, float *n4) {
    const orc_camera *cm = &s->cam[0];
    size_t p = (size_t)y * s->w + x;
    float vv[3], u[4];
    view_vector(cm, x, y, vv);
    rng4(s, (uint32_t)p, 0u, 0u, u);
    float disp = between(u[0], s->min_disp, s->max_disp);
    /* rndUnitVectorSphereMarsaglia_cu gipuma.cu:118-132 */
    float a = between(u[1], -1.0f, 1.0f), b = between(u[2], -1.0f, 1.0f);
    float sum = fmaf(a, a, b * b);
    for (uint32_t call = 1; sum >= 1.0f && call < 16; call++) {
        rng4(s, (uint32_t)p, 0u, call, u);
        a = between(u[0], -1.0f, 1.0f); b = between(u[1], -1.0f, 1.0f);
        sum = fmaf(a, a, b * b);
        if (sum >= 1.0f) {
            a = between(u[2], -1.0f, 1.0f); b = between(u[3], -1.0f, 1.0f);
            sum = fmaf(a, a, b * b);
        }
    }
    if (sum >= 1.0f) { a = 0.0f; b = 0.0f; sum = 0.0f; }
    float sq = sqrtf(1.0f - sum);
    n4[0] = 2.0f * a * sq; n4[1] = 2.0f * b * sq; n4[2] = 1.0f - 2.0f * sum;
    if (dot3f(n4, vv) > 0.0f) { n4[0] = -n4[0]; n4[1] = -n4[1]; n4[2] = -n4[2]; } /* vecOnHemisphere_cu :106-112 */
    float depth = cm->f * cm->baseline / disp;
    n4[3] = getD(n4, x, y, depth, cm);
}
static void init_pixel(orc_state *s, int x, int y) {
    size_t p = (size_t)y * s->w + x;
    float n4[4];
    draw_plane(s, x, y, n4);
    memcpy(s->norm4 + 4 * p, n4, sizeof n4);
    int bv; float rt;
    s->c[p] = pm_cost_multiview(s, x, y, n4, &bv, &rt);
}
void orc_pm_init(orc_state *s) {
    /* gipuma_init_cu2 takes box / 2 as its window radius (gipuma.cu:693-694); the propagation, refinement and lrdiff kernels
     * take (box - 1) / 2 (:858-859, :1065-1066, :1175-1176).  They differ for even boxes. */
    const int hr = s->hrad, vr = s->vrad;
    if (!(s->flags & ORC_FLAG_FIX_INIT_RADIUS)) { s->hrad = s->box_hsize / 2; s->vrad = s->box_vsize / 2; }
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) init_pixel(s, x, y);
    s->hrad = hr; s->vrad = vr;
    s->launch = 0;
}
/* tsar_pm_rescore (include/tsar.h): a plane whose depth at (x, y) is finite and inside [depthMin, depthMax] stays, any other pixel
 * gets the hypothesis init draws there; every pixel is scored on the sweeps' window (not init's box / 2) with cost, best view and
 * ratio written, and the launch counter restarts as after orc_pm_init. */
void orc_pm_rescore(orc_state *s) {
    const orc_camera *cm = &s->cam[0];
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            float *n4 = s->norm4 + 4 * p;
            const float d = depth_from_plane(cm, n4, x, y);
            if (!(d >= cm->depthMin && d <= cm->depthMax)) draw_plane(s, x, y, n4);
            int bv; float rt;
            s->c[p] = pm_cost_multiview(s, x, y, n4, &bv, &rt);
            s->beview[p] = bv;
            s->ratio[p] = rt;
        }
    s->launch = 0;
}

/* candidate selection of gipuma_checkerboard_spatialProp_cu gipuma.cu:874-1042; out[8] = pixel
 * index per arm (up_far, down_far, left_far, right_far, up_near, down_near, left_near, right_near)
 * or -1 when the arm is skipped.  c = cost plane of the launch-start snapshot (S2). */
static void select_candidates(const orc_state *s, const float *c, int x, int y, int32_t *out) {
    const int col = s->w, row = s->h;
    const int p = y * col + x;
    const int left_near = p - 1, left_far = p - 3, right_near = p + 1, right_far = p + 3;
    const int up_near = p - col, up_far = p - 3 * col, down_near = p + col, down_far = p + 3 * col;
    float cmin; int cp;
    for (int k = 0; k < 8; k++) out[k] = -1;
    if (y > 2) { /* up_far :889-902 */
        cmin = c[up_far]; cp = up_far;
        for (int i = 1; i < 11; ++i)
            if (y > 2 + 2 * i) { int q = up_far - 2 * i * col; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
        out[0] = cp;
    }
    if (y < row - 3) { /* down_far :905-918, quirk 1 */
        if ((s->flags & ORC_FLAG_FIX_DOWN_FAR_SEED) || y <= 2) cmin = c[down_far]; else cmin = c[up_far];
        cp = down_far;
        for (int i = 1; i < 11; ++i)
            if (y < row - 3 - 2 * i) { int q = down_far + 2 * i * col; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
        out[1] = cp;
    }
    if (x > 2) { /* left_far :921-934 */
        cmin = c[left_far]; cp = left_far;
        for (int i = 1; i < 11; ++i)
            if (x > 2 + 2 * i) { int q = left_far - 2 * i; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
        out[2] = cp;
    }
    if (x < col - 3) { /* right_far :937-950, quirk 2 */
        cmin = c[right_far]; cp = right_far;
        for (int i = 1; i < 11; ++i)
            if (x < col - 3 - 2 * i) {
                int q = right_far + 2 * i;
                int take = (s->flags & ORC_FLAG_FIX_RIGHT_FAR_CMP) ? (c[q] < cmin) : (cmin < c[q]);
                if (take) { cmin = c[q]; cp = q; }
            }
        out[3] = cp;
    }
    if (y > 0) { /* up_near :953-973 */
        cmin = c[up_near]; cp = up_near;
        for (int i = 0; i < 3; ++i) {
            if (y > 1 + i && x > i) { int q = up_near - (1 + i) * col - i; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
            if (y > 1 + i && x < col - 1 - i) { int q = up_near - (1 + i) * col + i; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
        }
        out[4] = cp;
    }
    if (y < row - 1) { /* down_near :976-996 */
        cmin = c[down_near]; cp = down_near;
        for (int i = 0; i < 3; ++i) {
            if (y < row - 2 - i && x > i) { int q = down_near + (1 + i) * col - i; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
            if (y < row - 2 - i && x < col - 1 - i) { int q = down_near + (1 + i) * col + i; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
        }
        out[5] = cp;
    }
    if (x > 0) { /* left_near :999-1019 */
        cmin = c[left_near]; cp = left_near;
        for (int i = 0; i < 3; ++i) {
            if (x > 1 + i && y > i) { int q = left_near - (1 + i) - i * col; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
            if (x > 1 + i && y < row - 1 - i) { int q = left_near - (1 + i) + i * col; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
        }
        out[6] = cp;
    }
    if (x < col - 1) { /* right_near :1022-1042 */
        cmin = c[right_near]; cp = right_near;
        for (int i = 0; i < 3; ++i) {
            if (x < col - 2 - i && y > i) { int q = right_near + (1 + i) - i * col; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
            if (x < col - 2 - i && y < row - 1 - i) { int q = right_near + (1 + i) + i * col; if (c[q] < cmin) { cmin = c[q]; cp = q; } }
        }
        out[7] = cp;
    }
}
void orc_select_candidates(const orc_state *s, const float *c, int x, int y, int32_t *out) { select_candidates(s, c, x, y, out); }

typedef struct { float cost, n4[4], depth, ratio; int beview, wrote; } pix_t;

/* gipuma_checkerboard_spatialProp_cu :846-1050 + spatialPropagation_cu :524-566 */
static void propagate_pixel(const orc_state *s, const float *c_snap, const float *n_snap, int x, int y, pix_t *px) {
    const orc_camera *cm = &s->cam[0];
    int32_t cand[8];
    select_candidates(s, c_snap, x, y, cand);
    for (int k = 0; k < 8; k++) {
        if (cand[k] < 0) continue;
        const float *nb = n_snap + 4 * (size_t)cand[k];
        float depth_b = depth_from_plane(cm, nb, x, y);
        int bv; float rt;
        float cost_b = pm_cost_multiview(s, x, y, nb, &bv, &rt);
        if (depth_b >= cm->depthMin && depth_b <= cm->depthMax && cost_b < px->cost) {
            px->depth = depth_b; memcpy(px->n4, nb, 16); px->cost = cost_b;
            px->ratio = rt; px->beview = bv; px->wrote = 1;
        }
    }
}
/* gipuma_checkerboard_planeRefinement_cu :1053-1094, planeRefinement_cu :621-676,
 * getRndDispAndUnitVector_cu :582-619 */
static void refine_pixel(const orc_state *s, int x, int y, uint32_t stream, pix_t *px) {
    const orc_camera *cm = &s->cam[0];
    size_t p = (size_t)y * s->w + x;
    float vv[3];
    view_vector(cm, x, y, vv);
    float deltaN = 1.0f;
    const float maxdisp = s->max_disp / 2.0f;
    uint32_t step = 0;
    for (float deltaZ = maxdisp; deltaZ >= 0.01f; deltaZ = deltaZ / 10.0f, step++) {
        float u[4], nt[4];
        rng4(s, (uint32_t)p, stream, step, u);
        float disp = cm->f * cm->baseline / px->depth;
        float minDelta = -fminf(deltaZ, s->min_disp + disp); /* quirk 5: plus, as written (:601) */
        float maxDelta = fminf(deltaZ, s->max_disp - disp);
        float dz = between(u[0], minDelta, maxDelta);
        float dispOut = fminf(fmaxf(disp + dz, s->min_disp), s->max_disp);
        float depthOut = cm->f * cm->baseline / dispOut;
        nt[0] = px->n4[0] + between(u[1], -deltaN, deltaN);
        nt[1] = px->n4[1] + between(u[2], -deltaN, deltaN);
        nt[2] = px->n4[2] + between(u[3], -deltaN, deltaN);
        float inv = 1.0f / sqrtf(dot3f(nt, nt));
        nt[0] *= inv; nt[1] *= inv; nt[2] *= inv;
        if (dot3f(nt, vv) > 0.0f) { nt[0] = -nt[0]; nt[1] = -nt[1]; nt[2] = -nt[2]; }
        nt[3] = getD(nt, x, y, depthOut, cm);
        int bv; float rt;
        float ct = pm_cost_multiview(s, x, y, nt, &bv, &rt);
        if (ct < px->cost) {
            px->cost = ct; px->depth = depthOut; memcpy(px->n4, nt, 16);
            px->ratio = rt; px->beview = bv; px->wrote = 1;
        }
        deltaN = deltaN / 4.0f;
    }
}
int orc_refine_steps(const orc_state *s) {
    int n = 0;
    for (float deltaZ = s->max_disp / 2.0f; deltaZ >= 0.01f; deltaZ = deltaZ / 10.0f) n++;
    return n;
}

/* one launch = propagation then refinement of every pixel of one colour.
 * colour 0 = "black": (x + y) even  (gipuma.cu:1099-1103: even x -> even y, odd x -> odd y),
 * colour 1 = "red".  do_prop / do_refine allow testing the halves separately.
 * final_text != NULL is the kernels' `final == true` mode: pixels whose lines->text is -1 are left
 * untouched (gipuma.cu:856, :1063) and accepted hypotheses do not write ratio / beview
 * (gipuma.cu:559-562, :669-672). */
static void pm_sweep_impl_rects(orc_state *s, int colour, int do_prop, int do_refine, const float *final_text, int n_rects, const int32_t *rects);
static void pm_sweep_impl(orc_state *s, int colour, int do_prop, int do_refine, const float *final_text) {
    pm_sweep_impl_rects(s, colour, do_prop, do_refine, final_text, 0, NULL);
}
/* n_rects > 0: only the pixels inside one of the rectangles rects[4 k .. 4 k + 3] = (x0, y0, x1, y1), x1 / y1 exclusive, are
 * updated (every read still sees the launch-start state of the whole image): what lets a test check a full-size launch of the
 * GPU path on windows of it in seconds instead of minutes. */
static void pm_sweep_impl_rects(orc_state *s, int colour, int do_prop, int do_refine, const float *final_text, int n_rects, const int32_t *rects) {
    const size_t np = (size_t)s->w * s->h;
    float *c_snap = (float *)malloc(np * sizeof(float));
    float *n_snap = (float *)malloc(np * 4 * sizeof(float));
    memcpy(c_snap, s->c, np * sizeof(float));
    memcpy(n_snap, s->norm4, np * 4 * sizeof(float));
    const uint32_t stream = 1u + (uint32_t)s->launch;
#pragma omp parallel for schedule(dynamic, 2)
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            if (((x + y) & 1) != colour) continue;
            if (n_rects > 0) {
                int inside = 0;
                for (int k = 0; k < n_rects && !inside; k++)
                    inside = x >= rects[4 * k] && y >= rects[4 * k + 1] && x < rects[4 * k + 2] && y < rects[4 * k + 3];
                if (!inside) continue;
            }
            size_t p = (size_t)y * s->w + x;
            if (final_text && final_text[p] == -1.0f) continue;
            pix_t px;
            px.cost = c_snap[p]; memcpy(px.n4, n_snap + 4 * p, 16);
            px.depth = depth_from_plane(&s->cam[0], px.n4, x, y);
            px.wrote = 0; px.ratio = 0; px.beview = 0;
            if (do_prop) propagate_pixel(s, c_snap, n_snap, x, y, &px);
            if (do_refine) refine_pixel(s, x, y, stream, &px);
            s->c[p] = px.cost; memcpy(s->norm4 + 4 * p, px.n4, 16);
            if (px.wrote && !final_text) { s->ratio[p] = px.ratio; s->beview[p] = px.beview; }
        }
    free(c_snap); free(n_snap);
    s->launch++;
}
void orc_pm_sweep(orc_state *s, int colour, int do_prop, int do_refine) { pm_sweep_impl(s, colour, do_prop, do_refine, NULL); }
void orc_pm_sweep_rects(orc_state *s, int colour, int do_prop, int do_refine, int n_rects, const int32_t *rects) {
    pm_sweep_impl_rects(s, colour, do_prop, do_refine, NULL, n_rects, rects);
}
/* host loop of gipuma_first gipuma.cu:1744-1754 */
void orc_pm_iterate(orc_state *s, int iters) {
    for (int it = 0; it < iters; it++) {
        pm_sweep_impl(s, 0, 1, 1, NULL);
        pm_sweep_impl(s, 1, 1, 1, NULL);
    }
}
/* the same loop with the kernels' `final` argument true; text [h][w] = lines->text */
void orc_pm_iterate_final(orc_state *s, int iters, const float *text) {
    for (int it = 0; it < iters; it++) {
        pm_sweep_impl(s, 0, 1, 1, text);
        pm_sweep_impl(s, 1, 1, 1, text);
    }
}

/* ------------------------------------------------------------------------------------------ */
/* plane <-> depth kernels                                                                     */
/* host fill main.cpp:1479-1490 + gipuma_get_disp gipuma.cu:731-755 */
void orc_load_planes(orc_state *s, const float *depth, const float *normal_world) {
    const orc_camera *cm = &s->cam[0];
#pragma omp parallel for
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            float n[4];
            mat3vec(cm->Rorig, normal_world + 3 * p, n);
            s->c[p] = 1.0f;
            float disp = cm->f * cm->baseline / depth[p];    /* lines->depth holds f*b/depth (main.cpp:1488) */
            s->depth[p] = disp;
            float disp_new = cm->f * cm->baseline / disp;      /* gipuma.cu:751-752 */
            n[3] = getD(n, x, y, disp_new, cm);
            memcpy(s->norm4 + 4 * p, n, 16);
        }
}
/* gipuma_compute_disp gipuma.cu:810-844: out4 = (n_world, depth or 0) */
void orc_compute_disp(const orc_state *s, float *out4) {
    const orc_camera *cm = &s->cam[0];
#pragma omp parallel for
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            const float *n = s->norm4 + 4 * p;
            float o[4];
            mat3vec(cm->RorigInv, n, o);
            o[3] = (s->c[p] != ORC_MAXCOST) ? depth_from_plane(cm, n, x, y) : 0.0f;
            memcpy(out4 + 4 * p, o, 16);
        }
}
/* gipuma_dptow gipuma.cu:1140-1158 */
void orc_depth_to_plane(orc_state *s) {
    const orc_camera *cm = &s->cam[0];
#pragma omp parallel for
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            float disp = cm->f * cm->baseline / s->depth[p];
            s->norm4[4 * p + 3] = getD(s->norm4 + 4 * p, x, y, disp, cm);
        }
}
/* gipuma_compute_disp_final gipuma.cu:757-808; resize4 [h][w][4], text [h][w]; out4 as compute_disp;
 * also updates s->norm4 (camera-frame plane after merge/clamp) and s->depth */
void orc_compute_disp_final(orc_state *s, const float *resize4, const float *text, float *out4) {
    const orc_camera *cm = &s->cam[0];
#pragma omp parallel for
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            float n[4];
            memcpy(n, s->norm4 + 4 * p, 16);
            float depth_now = depth_from_plane(cm, n, x, y);
            float disp_now = cm->f * cm->baseline / depth_now;
            float depth_org = depth_from_plane(cm, resize4 + 4 * p, x, y);
            float disp_org = cm->f * cm->baseline / depth_org;
            if ((fabsf(disp_now - disp_org) > 6.0f && text[p] == 1.0f) || text[p] == -1.0f) memcpy(n, resize4 + 4 * p, 16);
            float d = depth_from_plane(cm, n, x, y);
            if (d > cm->depthMax) n[3] = getD(n, x, y, cm->depthMax, cm);
            if (d < cm->depthMin) n[3] = getD(n, x, y, cm->depthMin, cm);
            s->depth[p] = depth_from_plane(cm, n, x, y);
            memcpy(s->norm4 + 4 * p, n, 16);
            float o[4];
            mat3vec(cm->RorigInv, n, o);
            o[3] = (s->c[p] != ORC_MAXCOST) ? depth_from_plane(cm, n, x, y) : 0.0f;
            memcpy(out4 + 4 * p, o, 16);
        }
}

/* ------------------------------------------------------------------------------------------ */
/* TSAR refinement kernels                                                                     */
/* rlCost gipuma.cu:300-392 */
static float rl_cost(const orc_state *s, int view, int x, int y, const float *n4) {
    const float *l = s->img[0], *r = s->img[view];
    const int w = s->w, h = s->h;
    float H[9], V[9];
    homography(&s->cam[0], &s->cam[view], n4, H);
    float det = H[0] * H[4] * H[8] + H[1] * H[5] * H[6] + H[2] * H[3] * H[7] - H[2] * H[4] * H[6] - H[1] * H[3] * H[8] - H[0] * H[5] * H[7];
    V[0] = (H[4] * H[8] - H[5] * H[7]) / det;
    V[1] = -(H[1] * H[8] - H[2] * H[7]) / det;
    V[2] = (H[1] * H[5] - H[2] * H[4]) / det;
    V[3] = -(H[3] * H[8] - H[5] * H[6]) / det;
    V[4] = (H[0] * H[8] - H[2] * H[6]) / det;
    V[5] = -(H[0] * H[5] - H[2] * H[3]) / det;
    V[6] = (H[3] * H[7] - H[4] * H[6]) / det;
    V[7] = -(H[0] * H[7] - H[1] * H[6]) / det;
    V[8] = (H[0] * H[4] - H[1] * H[3]) / det;
    float xf = (float)x, yf = (float)y;
    /* getCorrespondingPoint_cu :161-171 (matvecmul4noz: the two products first, the constant last; S4: mul, fma, add) */
    float Zc = fmaf(H[7], yf, H[6] * xf) + H[8];
    float pcx = (fmaf(H[1], yf, H[0] * xf) + H[2]) / Zc, pcy = (fmaf(H[4], yf, H[3] * xf) + H[5]) / Zc;
    float cen = bilinear_q(r, w, h, pcx, pcy, (s->flags & ORC_FLAG_TEX_FILTER_8BIT) != 0);
    float sum_ref = 0, sum_ref_ref = 0, sum_src = 0, sum_src_src = 0, sum_ref_src = 0, wsum = 0;
    for (int i = -s->hrad; i < s->hrad + 1; i += 2)
        for (int j = -s->vrad; j < s->vrad + 1; j += 2) {
            /* make_int2(pt_c.x + i, pt_c.y + j): float -> int truncation (:355) */
            float fx_ = fminf(fmaxf(pcx + (float)i, -2.0e9f), 2.0e9f), fy_ = fminf(fmaxf(pcy + (float)j, -2.0e9f), 2.0e9f);
            int plx = (int)fx_, ply = (int)fy_;
            float ref_pix = texel(r, w, h, plx, ply);
            float qx = (float)plx, qy = (float)ply;
            float Z = fmaf(V[7], qy, V[6] * qx) + V[8];
            float X = fmaf(V[1], qy, V[0] * qx) + V[2], Y = fmaf(V[4], qy, V[3] * qx) + V[5];
            float u_ = X / Z, v_ = Y / Z;
            if (s->flags & ORC_FLAG_FAST_ARITH) { const float rz = rcp_gpu(s, Z); u_ = X * rz; v_ = Y * rz; }   /* S7 (1): the one liberty lrdiff takes */
            float src_pix = bilinear_q(l, w, h, u_, v_, (s->flags & ORC_FLAG_TEX_FILTER_8BIT) != 0);
            float sd = sqrtf((float)(i * i + j * j));
            float cd = fabsf(ref_pix - cen);
            float wt = orc_expf(-sd / 50.0f - cd / 18.0f);
            float wr = wt * ref_pix, ws = wt * src_pix;
            sum_ref += wr;
            sum_ref_ref = fmaf(wr, ref_pix, sum_ref_ref);
            sum_src += ws;
            sum_src_src = fmaf(ws, src_pix, sum_src_src);
            sum_ref_src = fmaf(wr, src_pix, sum_ref_src);
            wsum += wt;
        }
    float inv = 1.0f / wsum;
    sum_ref *= inv; sum_ref_ref *= inv; sum_src *= inv; sum_src_src *= inv; sum_ref_src *= inv;
    float var_ref = sum_ref_ref - sum_ref * sum_ref;
    float var_src = sum_src_src - sum_src * sum_src;
    if (var_ref < 1e-5f || var_src < 1e-5f) return ORC_MAXCOST;
    float covar = sum_ref_src - sum_ref * sum_src;
    return fmaxf(0.0f, fminf(ORC_MAXCOST, 1.0f - covar / sqrtf(var_ref * var_src)));
}
/* gipuma_getlrdiff gipuma.cu:1160-1186; pixels whose beview is not a valid source view keep lrdiff */
void orc_lrdiff(orc_state *s) {
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            int v = s->beview[p];
            if (v < 1 || v >= s->n_views) continue;
            float d = fabsf(s->c[p] - rl_cost(s, v, x, y, s->norm4 + 4 * p));
            s->lrdiff[p] = d > 1.0f ? 1.0f : d;
        }
}
/* gipuma_getview gipuma.cu:1188-1213 */
void orc_getview(orc_state *s) {
    const orc_camera *cm = &s->cam[0];
#pragma omp parallel for
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            s->confid[p] = ((2.0f - s->c[p]) / 2.0f + (1.0f - s->lrdiff[p])) / 2.0f;
            float d = depth_from_plane(cm, s->norm4 + 4 * p, x, y);
            s->depth[p] = cm->f * cm->baseline / d;
        }
}
/* shared by update_scale / update_scale_2: region plane oriented towards the camera */
static inline void region_plane(const orc_state *s, int region, int x, int y, float *n4) {
    float vv[3];
    view_vector(&s->cam[0], x, y, vv);
    memcpy(n4, s->region_norm4 + 4 * (size_t)region, 16);
    float dp = n4[0] * vv[0] + n4[1] * vv[1] + n4[2] * vv[2];
    if (dp > 0.0f) { n4[0] *= -1; n4[1] *= -1; n4[2] *= -1; n4[3] *= -1; }
}
/* gipuma_update_scale_2 gipuma.cu:1261-1292 */
void orc_fake_depth(orc_state *s) {
#pragma omp parallel for
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            int rg = s->canny[p];
            if (s->region_text[rg] == -1.0f) {
                float n4[4];
                region_plane(s, rg, x, y, n4);
                s->fakedepth[p] = depth_from_plane(&s->cam[0], n4, x, y);
            }
        }
}
/* gipuma_update_scale gipuma.cu:1215-1259 */
void orc_update_scale(orc_state *s) {
    const orc_camera *cm = &s->cam[0];
#pragma omp parallel for
    for (int y = 0; y < s->h; y++)
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            int rg = s->canny[p];
            if (s->region_text[rg] == -1.0f) {
                float n4[4];
                s->c[p] = 0.0f;
                s->scale[p] = 1.0f;
                region_plane(s, rg, x, y, n4);
                memcpy(s->norm4 + 4 * p, n4, 16);
            }
            float d = depth_from_plane(cm, s->norm4 + 4 * p, x, y);
            s->depth[p] = cm->f * cm->baseline / d;
        }
}

/* ------------------------------------------------------------------------------------------ */
/* state plumbing for ctypes                                                                   */
orc_state *orc_create(int w, int h) {
    orc_state *s = (orc_state *)calloc(1, sizeof(orc_state));
    size_t np = (size_t)w * h;
    s->w = w; s->h = h;
    s->c = (float *)calloc(np, 4); s->norm4 = (float *)calloc(np, 16); s->ratio = (float *)calloc(np, 4);
    s->depth = (float *)calloc(np, 4); s->scale = (float *)calloc(np, 4); s->lrdiff = (float *)calloc(np, 4);
    s->confid = (float *)calloc(np, 4); s->fakedepth = (float *)calloc(np, 4);
    s->beview = (int32_t *)calloc(np, 4); s->canny = (int32_t *)calloc(np, 4);
    s->n_best = 1; s->cost_comb = 1; s->hrad = 5; s->vrad = 5; s->box_hsize = 11; s->box_vsize = 11;
    return s;
}
void orc_destroy(orc_state *s) {
    if (!s) return;
    free(s->c); free(s->norm4); free(s->ratio); free(s->depth); free(s->scale); free(s->lrdiff);
    free(s->confid); free(s->fakedepth); free(s->beview); free(s->canny);
    free(s->region_text); free(s->region_norm4); free(s->region_size);
    free(s);
}
void orc_set_image(orc_state *s, int view, const float *img) { s->img[view] = img; } /* borrowed */
void orc_set_params(orc_state *s, int box_hsize, int box_vsize, int n_best, int cost_comb, uint32_t flags, uint64_t seed) {
    s->hrad = (box_hsize - 1) / 2; s->vrad = (box_vsize - 1) / 2; /* gipuma.cu:858-859 */
    s->box_hsize = box_hsize; s->box_vsize = box_vsize;
    s->n_best = n_best; s->cost_comb = cost_comb; s->flags = flags; s->seed = seed;
}
void orc_set_rcp_table(orc_state *s, const float *table) { s->rcp_table = table; s->rcp_out_of_range = 0; } /* S7 (1); borrowed */
int orc_rcp_out_of_range(const orc_state *s) { return s->rcp_out_of_range; }
/* the geometric-consistency term: view's depth map (borrowed; NULL = no term for that view) and its F, B (12 floats each, row-major
 * 3 x 4, passed in as the library reports them); weight lambda and clip tau; orc_clear_geom removes the term */
void orc_set_geom(orc_state *s, int view, const float *depth, const float *F, const float *B) {
    s->geom_depth[view] = depth;
    memcpy(s->geom_F[view], F, sizeof s->geom_F[view]);
    memcpy(s->geom_B[view], B, sizeof s->geom_B[view]);
    s->geom_on = 1;
}
void orc_set_geom_params(orc_state *s, float weight, float clip) { s->geom_weight = weight; s->geom_clip = clip; }
void orc_clear_geom(orc_state *s) {
    s->geom_on = 0;
    s->geom_weight = 0.0f; s->geom_clip = 0.0f;
    memset(s->geom_depth, 0, sizeof s->geom_depth);
    memset(s->geom_F, 0, sizeof s->geom_F);
    memset(s->geom_B, 0, sizeof s->geom_B);
}
/* the plane-prior term: held = the [h][w][4] array the context holds (tsar_get_plane_prior: the normal in reference-camera
 * coordinates and the depth, all zero where there is no prior), borrowed like the geometric maps; orc_clear_plane_prior removes it */
void orc_set_plane_prior(orc_state *s, const float *held, float weight_depth, float weight_normal, float depth_clip, float normal_clip) {
    s->prior = held;
    s->prior_wd = weight_depth; s->prior_wn = weight_normal; s->prior_dc = depth_clip; s->prior_nc = normal_clip;
}
void orc_clear_plane_prior(orc_state *s) {
    s->prior = NULL;
    s->prior_wd = 0.0f; s->prior_wn = 0.0f; s->prior_dc = 0.0f; s->prior_nc = 0.0f;
}
float orc_rcp_gpu(const orc_state *s, float x) { return rcp_gpu(s, x); }
void orc_set_subset(orc_state *s, int n, const int32_t *idx) {
    s->n_sel = n;
    for (int i = 0; i < n; i++) s->sel[i] = idx[i];
}
void orc_set_regions(orc_state *s, const int32_t *labels, int n_regions, const float *text, const float *size) {
    memcpy(s->canny, labels, (size_t)s->w * s->h * 4);
    free(s->region_text); free(s->region_norm4); free(s->region_size);
    s->n_regions = n_regions;
    s->region_text = (float *)malloc((size_t)n_regions * 4);
    s->region_size = (float *)calloc((size_t)n_regions, 4);
    s->region_norm4 = (float *)calloc((size_t)n_regions, 16);
    memcpy(s->region_text, text, (size_t)n_regions * 4);
    if (size) memcpy(s->region_size, size, (size_t)n_regions * 4);
}
void orc_set_region_planes(orc_state *s, const float *planes) { memcpy(s->region_norm4, planes, (size_t)s->n_regions * 16); }
float *orc_plane_c(orc_state *s) { return s->c; }
float *orc_plane_norm4(orc_state *s) { return s->norm4; }
float *orc_plane_ratio(orc_state *s) { return s->ratio; }
int32_t *orc_plane_beview(orc_state *s) { return s->beview; }
float *orc_plane_depth(orc_state *s) { return s->depth; }
float *orc_plane_scale(orc_state *s) { return s->scale; }
float *orc_plane_lrdiff(orc_state *s) { return s->lrdiff; }
float *orc_plane_confid(orc_state *s) { return s->confid; }
float *orc_plane_fakedepth(orc_state *s) { return s->fakedepth; }
const orc_camera *orc_camera_ptr(const orc_state *s, int view) { return &s->cam[view]; }
int orc_camera_sizeof(void) { return (int)sizeof(orc_camera); }
float orc_min_disp(const orc_state *s) { return s->min_disp; }
float orc_max_disp(const orc_state *s) { return s->max_disp; }
void orc_set_launch(orc_state *s, int launch) { s->launch = launch; }

/* raw Philox block for the published known-answer vectors (Random123 kat_vectors) */
void orc_philox_raw(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t *out) {
    philox4x32(c0, c1, c2, c3, k0, k1, out);
}

/* ------------------------------------------------------------------------------------------ */
/* weighted median filter, gipuma_WMF (gipuma.cu:1499-1698) and gipuma_WMF_Final (:1294-1497).
 * Restated literally, including the bubble sort whose inner loop touches index `num` (one
 * zero-initialised slot takes part and the largest element drops out of the first `num`, SURVEY
 * quirk 12).  Neighbours are read from the launch-start copies (S2).  Where the reference would
 * leave norm_mid uninitialised (cumulative weight never reaches wSum/2 in one of the normal
 * component scans) the last sorted element is used.  exp -> orc_expf. */
#define WMF_CAP 145
typedef struct { float w[WMF_CAP], d[WMF_CAP], x[WMF_CAP], y[WMF_CAP], z[WMF_CAP], w1[WMF_CAP], w2[WMF_CAP], w3[WMF_CAP]; int n[WMF_CAP]; int num; } wmf_buf;

static void wmf_sort(wmf_buf *b) {
    const int num = b->num;
    for (int i = 0; i < num; i++)
        for (int j = 0; j < num - i; j++) {
            if (b->d[j] > b->d[j + 1]) {
                float t = b->w[j]; b->w[j] = b->w[j + 1]; b->w[j + 1] = t;
                t = b->d[j]; b->d[j] = b->d[j + 1]; b->d[j + 1] = t;
                int nn = b->n[j]; b->n[j] = b->n[j + 1]; b->n[j + 1] = nn;
            }
            if (b->x[j] > b->x[j + 1]) { float t = b->x[j]; b->x[j] = b->x[j + 1]; b->x[j + 1] = t; t = b->w1[j]; b->w1[j] = b->w1[j + 1]; b->w1[j + 1] = t; }
            if (b->y[j] > b->y[j + 1]) { float t = b->y[j]; b->y[j] = b->y[j + 1]; b->y[j + 1] = t; t = b->w2[j]; b->w2[j] = b->w2[j + 1]; b->w2[j + 1] = t; }
            if (b->z[j] > b->z[j + 1]) { float t = b->z[j]; b->z[j] = b->z[j + 1]; b->z[j + 1] = t; t = b->w3[j]; b->w3[j] = b->w3[j + 1]; b->w3[j + 1] = t; }
        }
}
static float wmf_median(const float *v, const float *w, int num, float half) {
    float acc = 0.f;
    for (int i = 0; i < num; i++) {
        acc += w[i];
        if (acc >= half) return v[i];
    }
    return v[num - 1];
}
/* gathers the taps; returns wSum; fills the plane through the weighted-median-depth pixel */
static int wmf_collect(const orc_state *s, const float *scale_in, const float *depth_in, const float *n_in, int x, int y,
                       int radius, int gap, float sdiv, wmf_buf *b) {
    const float *img = s->img[0];
    memset(b, 0, sizeof(*b));
    const float cen = texel(img, s->w, s->h, x, y);
    int num = 0;
    for (int i = -radius; i <= radius; i += gap)
        for (int j = -radius; j <= radius; j += gap) {
            int px = x + i, py = y + j;
            if (px < 0 || px >= s->w || py < 0 || py >= s->h) continue;
            size_t q = (size_t)py * s->w + px;
            if (scale_in[q] != 1.0f) continue;
            float cd = fabsf(img[q] - cen);
            float sd = sqrtf((float)(i * i + j * j)) / sdiv;
            float wt = orc_expf(-sd / 4.0f) * orc_expf(-cd / 9.0f);   /* sigma_spatial 2, sigma_color 3 */
            b->w[num] = b->w1[num] = b->w2[num] = b->w3[num] = wt;
            b->d[num] = depth_in[q]; b->n[num] = (int)q;
            b->x[num] = n_in[4 * q]; b->y[num] = n_in[4 * q + 1]; b->z[num] = n_in[4 * q + 2];
            num++;
        }
    b->num = num;
    return num;
}
static int wmf_plane(const orc_state *s, const float *depth_in, wmf_buf *b, float *nm) {
    const orc_camera *cm = &s->cam[0];
    const int num = b->num;
    wmf_sort(b);
    float wSum = 0.f;
    for (int i = 0; i < num; i++) wSum += b->w[i];
    const float half = wSum / 2.f;
    nm[0] = wmf_median(b->x, b->w1, num, half);
    nm[1] = wmf_median(b->y, b->w2, num, half);
    nm[2] = wmf_median(b->z, b->w3, num, half);
    float acc = 0.f;
    for (int i = 0; i < num; i++) {
        acc += b->w[i];
        if (acc >= half) {
            int weimid = b->n[i];
            float depth_mid = cm->f * cm->baseline / depth_in[weimid];
            double nrm = (double)sqrtf(dot3f(nm, nm));
            nm[0] = (float)((double)nm[0] / nrm); nm[1] = (float)((double)nm[1] / nrm); nm[2] = (float)((double)nm[2] / nrm);
            nm[3] = getD(nm, weimid % s->w, weimid / s->w, depth_mid, cm);
            return 1;
        }
    }
    return 0;
}
/* one gipuma_WMF launch: marks every pixel reliable / unreliable */
void orc_wmf_detect(orc_state *s, int iter) {
    const orc_camera *cm = &s->cam[0];
    const size_t np = (size_t)s->w * s->h;
    const int po = 1 << iter, repo = 1 << (3 - iter);
    const int radius = 80 / po, gap = 16 / po, ths = 24 / po;
    float *scale_in = (float *)malloc(np * 4);
    memcpy(scale_in, s->scale, np * 4);
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = 0; y < s->h; y++) {
        wmf_buf b;
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            float nm[4];
            int num = wmf_collect(s, scale_in, s->depth, s->norm4, x, y, radius, gap, (float)repo, &b);
            if (num > 0 && wmf_plane(s, s->depth, &b, nm)) {
                float depth_now = depth_from_plane(cm, nm, x, y);
                float disp_now = cm->f * cm->baseline / depth_now;
                float depth_org = depth_from_plane(cm, s->norm4 + 4 * p, x, y);
                float disp_org = cm->f * cm->baseline / depth_org;
                s->scale[p] = (fabsf(disp_now - disp_org) > (float)ths) ? 0.0f : 1.0f;   /* DEPTH_THS_MIN/MAX are 0 (:38-39) */
            } else {
                s->scale[p] = 0.0f;
            }
        }
    }
    free(scale_in);
}
/* one gipuma_WMF_Final launch: fills unreliable pixels of textured regions */
void orc_wmf_fill(orc_state *s, int iter) {
    const orc_camera *cm = &s->cam[0];
    const size_t np = (size_t)s->w * s->h;
    const int po = 1 << iter;
    const int radius = 5 * po, gap = po, ths = 32 / po;
    float *scale_in = (float *)malloc(np * 4), *depth_in = (float *)malloc(np * 4), *n_in = (float *)malloc(np * 16);
    memcpy(scale_in, s->scale, np * 4); memcpy(depth_in, s->depth, np * 4); memcpy(n_in, s->norm4, np * 16);
#pragma omp parallel for schedule(dynamic, 4)
    for (int y = 0; y < s->h; y++) {
        wmf_buf b;
        for (int x = 0; x < s->w; x++) {
            size_t p = (size_t)y * s->w + x;
            if (!(s->region_text[s->canny[p]] == 1.0f && scale_in[p] == 0.0f)) continue;
            float nm[4];
            int num = wmf_collect(s, scale_in, depth_in, n_in, x, y, radius, gap, (float)po, &b);
            if (num < ths || num == 0) continue;
            if (!wmf_plane(s, depth_in, &b, nm)) continue;
            memcpy(s->norm4 + 4 * p, nm, 16);
            float depth_now = depth_from_plane(cm, nm, x, y);
            float disp = cm->f * cm->baseline / depth_now;
            if (disp <= s->min_disp || disp >= s->max_disp) { s->scale[p] = 0.0f; s->depth[p] = s->min_disp; }
            else { s->scale[p] = 1.0f; s->depth[p] = disp; }
        }
    }
    free(scale_in); free(depth_in); free(n_in);
}

/* ------------------------------------------------------------------------------------------ */
/* region plane RANSAC, main.cpp:1520-1730 (+ calcLinePara :147-164).  Double precision as in the
 * reference.  Deterministic choices (the reference uses rand() and a time-seeded shuffle):
 *   - points are listed in raster order; regions with more than 50000 reliable pixels keep an
 *     evenly spaced subset of 49999 (reference: random shuffle, then pop to < 50000);
 *   - random indices / perturbations come from Philox: stage 1 draw k uses counter
 *     (k, 0x52414E53, region, 0), stage 2 draw (round*4+scale) uses (.., 0x52414E54, region, 0);
 *   - calcLinePara's first component is reproduced as written unless ORC_FLAG_FIX_PLANE_FIT. */
#define ORC_FLAG_FIX_PLANE_FIT (1u << 3)
static inline uint32_t rnd_index(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }
static int count_inliers(const float *pts, int n, double a, double b, double c, double d, double thr) {
    int cnt = 0;
    for (int i = 0; i < n; i++) {
        double resid = fabs((double)pts[3 * i] * a + (double)pts[3 * i + 1] * b + (double)pts[3 * i + 2] * c + d);
        if (resid < thr) cnt++;
    }
    return cnt;
}
/* pts: n x 3 floats.  out: plane (a,b,c,d) as floats + inlier count */
int orc_ransac_points(const float *pts, int n, float region_size, uint64_t seed, uint32_t region, uint32_t flags, float *plane_out) {
    double a = 0, b = 0, c = 1, d = -1;
    int maximum = 0;
    /* `float depth_abs = 0.0003 * sqrtf(size / 20)` (:1551-1552): double product rounded to float;
     * every later `depth_abs += 0.0001` is a double add rounded back to float */
    float depth_abs_f = (float)(0.0003 * (double)sqrtf(region_size / 20));
    double depth_abs = depth_abs_f;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (n <= 0) { plane_out[0] = 0; plane_out[1] = 0; plane_out[2] = 1; plane_out[3] = -1; return 0; }
    for (int k = 0; k < 10000; k++) {
        uint32_t r[4];
        philox4x32((uint32_t)k, 0x52414E53u, region, 0u, k0, k1, r);
        const float *p1 = pts + 3 * rnd_index(r[0], (uint32_t)n), *p2 = pts + 3 * rnd_index(r[1], (uint32_t)n), *p3 = pts + 3 * rnd_index(r[2], (uint32_t)n);
        double x1 = p1[0], y1 = p1[1], z1 = p1[2], x2 = p2[0], y2 = p2[1], z2 = p2[2], x3 = p3[0], y3 = p3[1], z3 = p3[2];
        double ta = (flags & ORC_FLAG_FIX_PLANE_FIT) ? (y2 - y1) * (z3 - z1) - (z2 - z1) * (y3 - y1)
                                                    : (y3 - y1) * (z3 - z1) - (z2 - z1) * (y3 - y1);
        double tb = (x3 - x1) * (z2 - z1) - (x2 - x1) * (z3 - z1);
        double tc = (x2 - x1) * (y3 - y1) - (x3 - x1) * (y2 - y1);
        double td = -(ta * x1 + tb * y1 + tc * z1);
        double sq = sqrt(ta * ta + tb * tb + tc * tc);
        ta /= sq; tb /= sq; tc /= sq; td /= sq;
        int cnt = count_inliers(pts, n, ta, tb, tc, td, depth_abs);
        if (cnt >= maximum) { a = ta; b = tb; c = tc; d = td; maximum = cnt; }
        if (k % 1000 == 0) {
            double rat = (double)maximum / (double)n;
            if (rat < 0.3 && depth_abs < 0.003) {
                depth_abs_f = (float)((double)depth_abs_f + 0.0001); depth_abs = depth_abs_f;
            } else {
                int max2 = count_inliers(pts, n, a, b, c, d, (double)depth_abs_f + 0.0001);
                if ((double)max2 > (double)maximum + (double)n * 0.02) { depth_abs_f = (float)((double)depth_abs_f + 0.0001); depth_abs = depth_abs_f; maximum = max2; }
            }
        }
    }
    for (int round = 0; round < 1000; round++) {
        int sc = 0;
        for (int j = 2000; j >= 2; j /= 10, sc++) {
            uint32_t r[4];
            philox4x32((uint32_t)(round * 4 + sc), 0x52414E54u, region, 0u, k0, k1, r);
            int med = j / 2;
            double da = (double)((int)rnd_index(r[0], (uint32_t)j) - med) / 10000;
            double db = (double)((int)rnd_index(r[1], (uint32_t)j) - med) / 10000;
            double dc = (double)((int)rnd_index(r[2], (uint32_t)j) - med) / 10000;
            double dd = (double)((int)rnd_index(r[3], (uint32_t)j) - med) / 1000;
            double ra = a + da, rb = b + db, rc = c + dc, rd = d + dd;
            double sq = sqrt(ra * ra + rb * rb + rc * rc);
            ra /= sq; rb /= sq; rc /= sq; rd /= sq;
            int cnt = count_inliers(pts, n, ra, rb, rc, rd, depth_abs);
            if (cnt >= maximum) { a = ra; b = rb; c = rc; d = rd; maximum = cnt; }
        }
    }
    plane_out[0] = (float)a; plane_out[1] = (float)b; plane_out[2] = (float)c; plane_out[3] = (float)d;
    return maximum;
}
/* gather (main.cpp:1527-1594) + fit for every textureless region; planes -> region_norm4 */
void orc_ransac_regions(orc_state *s, float *inlier_ratio) {
    const orc_camera *cm = &s->cam[0];
    const size_t np = (size_t)s->w * s->h;
    for (int rg = 0; rg < s->n_regions; rg++) {
        if (inlier_ratio) inlier_ratio[rg] = 0.f;
        if (s->region_text[rg] != -1.0f) continue;
        int total = 0;
        for (size_t p = 0; p < np; p++)
            if (s->canny[p] == rg && s->scale[p] == 1.0f) total++;
        int keep = total > 50000 ? 49999 : total;
        float *pts = (float *)malloc((size_t)(keep > 0 ? keep : 1) * 12);
        int i = 0, m = 0;
        for (size_t p = 0; p < np; p++) {
            if (!(s->canny[p] == rg && s->scale[p] == 1.0f)) continue;
            int take = total > 50000 ? (int)(((int64_t)(i + 1) * keep) / total) > (int)(((int64_t)i * keep) / total) : 1;
            i++;
            if (!take) continue;
            int x = (int)(p % s->w), y = (int)(p / s->w);
            float depth = cm->f * cm->baseline / s->depth[p];
            float pt[3] = {depth * (float)x - cm->P34[0], depth * (float)y - cm->P34[1], depth - cm->P34[2]};
            /* main.cpp:1583-1591 writes the products out without fma */
            pts[3 * m] = cm->Minv[0] * pt[0] + cm->Minv[1] * pt[1] + cm->Minv[2] * pt[2];
            pts[3 * m + 1] = cm->Minv[3] * pt[0] + cm->Minv[4] * pt[1] + cm->Minv[5] * pt[2];
            pts[3 * m + 2] = cm->Minv[6] * pt[0] + cm->Minv[7] * pt[1] + cm->Minv[8] * pt[2];
            m++;
        }
        int best = orc_ransac_points(pts, m, s->region_size[rg], s->seed, (uint32_t)rg, s->flags, s->region_norm4 + 4 * (size_t)rg);
        if (inlier_ratio) inlier_ratio[rg] = m > 0 ? (float)best / (float)m : 0.f;
        free(pts);
    }
}
float *orc_region_planes(orc_state *s) { return s->region_norm4; }
