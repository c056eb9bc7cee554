// cloud_render_dev.h — the landing and the clipped footprint of a point (include/tsar.h tsar_cloud_render), shared by the units that render
// a cloud: cloud_render_kernels.hip (the square occluder) and cloud_splat_kernels.hip (the normal-oriented one).
#pragma once
#include <float.h>
#include <math.h>

#include "tsar_device_math.h"

#define CR_BLOCK 256
#define CR_EMPTY32 0xFFFFFFFFu             // an occluder entry nothing covers (no float that lands has these bits: they are a NaN's)
#define CR_EMPTY64 0xFFFFFFFFFFFFFFFFull   // a centre entry nothing landed on

struct CrView {
    float P[12];          // K [R | t], float64 products rounded once
    float fr;             // fl(K[0] * radius); 0 with radius 0
    float max_px;         // (float)max_px
    int w, h;
};

struct CrLanding {
    bool lands;
    int xi, yi, s;        // valid when lands
    float p2;
};

template <bool FOOT>
DEVFN CrLanding cr_land(const float* __restrict__ pts, long long i, int stride, const CrView& v) {
    const float* p = pts + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    const bool candidate = fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX;   // (NaN fails)
    const float p0 = ((v.P[0] * x + v.P[1] * y) + v.P[2] * z) + v.P[3];
    const float p1 = ((v.P[4] * x + v.P[5] * y) + v.P[6] * z) + v.P[7];
    const float p2 = ((v.P[8] * x + v.P[9] * y) + v.P[10] * z) + v.P[11];
    const float xq = p0 / p2, yq = p1 / p2;
    const float xi = floorf(xq + 0.5f), yi = floorf(yq + 0.5f);
    CrLanding l;
    // (NaN fails every comparison: a non-finite projection does not land, so xi and yi stay inside the planes)
    l.lands = candidate && p2 > 0.0f && p2 < __builtin_inff() && xi >= 0.0f && xi <= (float)(v.w - 1) && yi >= 0.0f && yi <= (float)(v.h - 1);
    l.xi = l.lands ? (int)xi : 0;
    l.yi = l.lands ? (int)yi : 0;
    l.p2 = p2;
    // (p_2 > 0 and fr >= 0, both finite: the quotient is in [0, inf], never NaN, and the minimum is in [0, max_px])
    l.s = FOOT && l.lands ? (int)fminf(floorf(v.fr / p2 + 0.5f), v.max_px) : 0;
    return l;
}

// the footprint clipped to the image: [x0, x1] x [y0, y1]
DEVFN void cr_clip(const CrLanding& l, const CrView& v, int& x0, int& x1, int& y0, int& y1) {
    x0 = l.xi - l.s < 0 ? 0 : l.xi - l.s;
    x1 = l.xi + l.s > v.w - 1 ? v.w - 1 : l.xi + l.s;
    y0 = l.yi - l.s < 0 ? 0 : l.yi - l.s;
    y1 = l.yi + l.s > v.h - 1 ? v.h - 1 : l.yi + l.s;
}

static inline unsigned cr_blocks(long long n) { return (unsigned)((n + CR_BLOCK - 1) / CR_BLOCK); }
