// tsar_outliers.h — the stray-point rules of api.remove_outliers for the command-line tools (tsar_fusion --outlier_*, tsar_evaluate
// --clean_*): the switches' values, their refusals, and the keep mask from one tsar_cloud_neighbors_ctx call.
//   radius rule:           count >= N
//   k-th-neighbour rule:   s = knn_dist2[i][K - 1];  med = the lower median of the finite s (element (m - 1) / 2 of the m finite values in
//                          ascending order, std::nth_element);  kept iff s <= fl(fl(Q * Q) * med), two float32 products; m = 0: nothing passes
// A record is kept iff it is a candidate and passes every rule given: an order statistic and two products, the same mask as the Python
// binding's and the numpy restatement's.  The entries are referred to weakly: a tool still links against, and runs with, a library that
// lacks them, and refuses the switch there.
#pragma once
#include <float.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/tsar.h"

extern "C" {
void tsar_default_cloud_neighbors_params(tsar_cloud_neighbors_params* p) __attribute__((weak));
int tsar_cloud_neighbors_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_neighbors_params* p, int32_t* count_out, float* knn_dist2_out,
                             int64_t* n_valid_out, int64_t* pairs_out, int mem) __attribute__((weak));
}

struct OutlierSettings {
    const char* prefix;           // "--outlier_" or "--clean_": names the switches in the messages
    bool have_radius = false, have_ratio = false;
    float radius = 0.0f, ratio = 2.0f;
    int min_neighbors = 0, knn = 0;        // 0: the rule is off
    explicit OutlierSettings(const char* p) : prefix(p) {}
    bool on() const { return have_radius; }
    std::string opt(const char* name) const { return std::string(prefix) + name; }

    // One switch's value.  what: 'r' radius, 'n' min_neighbors, 'k' knn, 'q' ratio.  An empty string, or the one-line refusal.
    std::string parse(char what, const char* v) {
        char* end = nullptr;
        if (what == 'r' || what == 'q') {
            const double t = strtod(v, &end);
            const bool good = end != v && *end == '\0' && t > 0.0 && (float)t <= FLT_MAX && (float)t > 0.0f;
            if (!good) return opt(what == 'r' ? "radius=R" : "ratio=Q") + " must be a finite number > 0";
            if (what == 'r') { radius = (float)t; have_radius = true; }
            else { ratio = (float)t; have_ratio = true; }
            return "";
        }
        const long t = strtol(v, &end, 10);
        const bool good = end != v && *end == '\0';
        if (what == 'n') {
            if (!good || t < 1 || t > INT32_MAX) return opt("min_neighbors=N") + " must be an integer >= 1";
            min_neighbors = (int)t;
        } else {
            if (!good || t < 1 || t > TSAR_CLOUD_KNN_MAX) return opt("knn=K") + " must be an integer in 1.." + std::to_string(TSAR_CLOUD_KNN_MAX);
            knn = (int)t;
        }
        return "";
    }
    // After the last switch: an empty string, or the one-line refusal.
    std::string check() const {
        if (!have_radius && (min_neighbors || knn || have_ratio)) return opt("min_neighbors=, ") + opt("knn= and ") + opt("ratio= need ") + opt("radius=R");
        if (have_radius && !min_neighbors && !knn) return opt("radius=R needs ") + opt("min_neighbors=N, ") + opt("knn=K or both");
        if (have_ratio && !knn) return opt("ratio=Q needs ") + opt("knn=K");
        if (have_radius && (!tsar_cloud_neighbors_ctx || !tsar_default_cloud_neighbors_params)) return opt("radius: this libtsar_hip.so has no tsar_cloud_neighbors");
        return "";
    }
    std::string json() const {
        char b[160];
        snprintf(b, sizeof b, "{\"radius\": %.9g, \"min_neighbors\": %s, \"k\": %s, \"ratio\": %.9g}", (double)radius,
                 min_neighbors ? std::to_string(min_neighbors).c_str() : "null", knn ? std::to_string(knn).c_str() : "null", (double)ratio);
        return b;
    }
};

// keep[i] = 1 for the records of `cloud` (n records of `stride` floats, host memory) that stay.  false: the library's message is in
// tsar_last_error(ctx).
static inline bool outlier_keep_mask(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const OutlierSettings& s, std::vector<uint8_t>& keep) {
    tsar_cloud_neighbors_params np;
    tsar_default_cloud_neighbors_params(&np);
    np.radius = s.radius;
    np.k = s.knn;
    std::vector<int32_t> count((size_t)n + 1);
    std::vector<float> knn(s.knn ? (size_t)n * (size_t)s.knn + 1 : 0);
    if (tsar_cloud_neighbors_ctx(ctx, cloud, n, stride, &np, count.data(), s.knn ? knn.data() : nullptr, nullptr, nullptr, TSAR_MEM_HOST) != TSAR_OK) return false;
    keep.assign((size_t)n, 0);
    for (int64_t i = 0; i < n; i++) keep[(size_t)i] = count[(size_t)i] >= s.min_neighbors;      // (-1: no candidate)
    if (s.knn) {
        std::vector<float> finite;
        for (int64_t i = 0; i < n; i++) {
            const float v = knn[(size_t)i * s.knn + (s.knn - 1)];
            if (v <= FLT_MAX) finite.push_back(v);
        }
        if (finite.empty()) {
            keep.assign((size_t)n, 0);
        } else {
            const size_t mid = (finite.size() - 1) / 2;
            std::nth_element(finite.begin(), finite.begin() + mid, finite.end());
            const volatile float q2 = s.ratio * s.ratio;       // two float32 products, each rounded
            const volatile float T = q2 * finite[mid];
            for (int64_t i = 0; i < n; i++) keep[(size_t)i] = keep[(size_t)i] && knn[(size_t)i * s.knn + (s.knn - 1)] <= T;
        }
    }
    return true;
}
