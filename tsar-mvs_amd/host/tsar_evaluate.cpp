// tsar_evaluate — accuracy and completeness of a reconstructed cloud against a ground-truth cloud, on the GPU:
//   tsar_evaluate RECON.ply GT.ply --tolerances=0.01,0.02,0.05 [--max_pairs=N] [--device=D] [--json=FILE] [--voxel=V] [--crop=x0,y0,z0,x1,y1,z1]
//                 [--clean_radius=R [--clean_min_neighbors=N] [--clean_knn=K [--clean_ratio=Q]]]
//                 [--normals=K --normal_radius=R [--normal_min_neighbors=N] [--normal_tolerances=D1,D2,...] [--normal_signed]]
// accuracy(tau) = the share of RECON's points with a GT point within tau; completeness(tau) = the share of GT's points with a RECON point
// within tau; f1 = their harmonic mean: the point-wise precision / recall / F-score.  Not ETH3D's or DTU's evaluation program: nothing is
// masked or aligned, and without the two switches below nothing is down-sampled or cropped.  Two tsar_cloud_distance_ctx calls with max_dist = the largest tolerance (include/tsar.h);
// points with a non-finite coordinate take no part.  Prints one table and one JSON line; --json=FILE gets the same line.
// --voxel=V adds the voxel-averaged figures (a grid of edge V over each cloud, tsar_cloud_voxels_ctx: per occupied voxel the share of its
// points within tau, averaged over the voxels in ascending voxel order, one float64 term after another), --crop= first makes every point
// outside the closed box a non-candidate.  In the manner of the benchmarks, still not their programs: no alignment, no observation masks.
// --clean_radius=R with --clean_min_neighbors=N and / or --clean_knn=K first removes RECON's stray points (host/tsar_outliers.h: the rules of
// api.remove_outliers, one tsar_cloud_neighbors_ctx call), before the crop and before any scoring; GT is left as it is.
// --normals=K --normal_radius=R also scores RECON's normals (its nx ny nz) against normals estimated from GT's points: the plain PCA normal
// over the K nearest neighbours within R with the canonical sign (tsar_cloud_normals_ctx, after the crop), and one
// tsar_cloud_normal_compare_ctx of every RECON point with the GT point nearest to it within the largest tolerance.  No orientation is
// propagated across the cloud and nothing is meshed: not a benchmark's program either.
#include <math.h>
#include <stdlib.h>

#include <chrono>

#include "tsar_io.h"
#include "tsar_outliers.h"

// The entries that only --voxel calls are referred to weakly: the tool still links against, and runs with, a library that lacks them, and
// refuses the switch there.
extern "C" {
void tsar_default_cloud_voxels_params(tsar_cloud_voxels_params* p) __attribute__((weak));
int tsar_cloud_voxels_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_voxels_params* p, const float* dist2, int n_tol, const float* tol,
                          int32_t* rank_out, int64_t cap, int32_t* rep_out, int32_t* count_out, int32_t* within_out, int64_t* n_voxels_out, int64_t* n_valid_out,
                          int mem) __attribute__((weak));
void tsar_default_cloud_normals_params(tsar_cloud_normals_params* p) __attribute__((weak));
int tsar_cloud_normals_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_normals_params* p, int32_t* knn_index_out, int32_t* n_used_out,
                           float* normal_out, float* curvature_out, double* cov_out, int64_t* n_valid_out, int64_t* n_normals_out, int64_t* pairs_out,
                           int mem) __attribute__((weak));
int tsar_cloud_normal_compare_ctx(tsar_ctx* ctx, const float* normal_a, int stride_a, int64_t n, const float* normal_b, int stride_b, int64_t n_b, const int32_t* index,
                                  const float* dist2, float max_dist, int n_tol, const double* min_cos, int is_signed, float* cos_out, int64_t* within_out,
                                  int64_t* n_compared_out, int mem) __attribute__((weak));
}

static int refuse(const std::string& msg) {
    fprintf(stderr, "%s\n", msg.c_str());
    return 1;
}

static std::string json_string(const std::string& s) {
    std::string o = "\"";
    for (const char ch : s) {
        if (ch == '"' || ch == '\\') { o += '\\'; o += ch; }
        else if ((unsigned char)ch < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", ch); o += b; }
        else o += ch;
    }
    return o + "\"";
}

template <typename T, typename Fmt>
static std::string json_list(const std::vector<T>& v, Fmt fmt) {
    std::string o = "[";
    for (size_t k = 0; k < v.size(); k++) o += (k ? ", " : "") + fmt(v[k]);
    return o + "]";
}

int main(int argc, char** argv) {
    (void)write_cloud_ply;                         // (tsar_io.h's writer, unused here)
    const char* usage = "usage: tsar_evaluate RECON.ply GT.ply --tolerances=T1[,T2...] [--max_pairs=N] [--device=D] [--json=FILE] [--voxel=V]\n"
                        "                     [--crop=x0,y0,z0,x1,y1,z1] [--clean_radius=R [--clean_min_neighbors=N] [--clean_knn=K [--clean_ratio=Q]]]\n"
                        "                     [--normals=K --normal_radius=R [--normal_min_neighbors=N] [--normal_tolerances=D1,D2,...] [--normal_signed]]\n"
                        "       point-wise accuracy / completeness / F-score of RECON against GT at each tolerance; --voxel=V adds the figures averaged\n"
                        "       over the occupied voxels of edge V, --crop= drops the points outside the closed box first (not ETH3D's or DTU's\n"
                        "       program: no masks, no alignment); --clean_radius=R first removes RECON's points with fewer than N others within R and / or\n"
                        "       whose K-th neighbour within R lies beyond Q (2) times the median K-th-neighbour distance; --normals=K also scores RECON's\n"
                        "       normals against the plain PCA normals of GT's points (K nearest neighbours within R, at least N (5) of them; no orientation\n"
                        "       propagated, nothing meshed) at each angle in degrees (10,30): lines are compared, with --normal_signed directions\n";
    if (argc >= 2 && (!strcmp(argv[1], "-h") || !strcmp(argv[1], "--help"))) { printf("%s", usage); return 0; }
    std::vector<std::string> paths;
    std::vector<float> tol;
    bool have_tol = false;
    long long max_pairs = -1;
    int device = 0;
    std::string json_path;
    bool have_voxel = false, have_crop = false;
    float voxel = 0.0f;
    float crop[6] = {0, 0, 0, 0, 0, 0};
    OutlierSettings clean("--clean_");
    bool have_normals = false, have_nradius = false, have_nmin = false, have_ntol = false, nsigned = false;
    int nk = 0, nmin = 5;
    float nradius = 0.0f;
    std::vector<double> ndeg = {10.0, 30.0};
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&](const char* opt) -> const char* { const size_t n = strlen(opt); return a.compare(0, n, opt) == 0 ? argv[i] + n : nullptr; };
        const char* v;
        std::string why;
        if ((v = value("--tolerances="))) {
            have_tol = true;
            const char* s = v;
            while (true) {
                char* end = nullptr;
                const double t = strtod(s, &end);
                if (end == s || !(t > 0.0) || !((float)t <= FLT_MAX)) return refuse("--tolerances=T1[,T2...]: every tolerance must be a finite number > 0");
                tol.push_back((float)t);
                if (*end == '\0') break;
                if (*end != ',') return refuse("--tolerances=T1[,T2...]: every tolerance must be a finite number > 0");
                s = end + 1;
            }
        } else if ((v = value("--max_pairs="))) {
            char* end = nullptr;
            max_pairs = strtoll(v, &end, 10);
            if (end == v || *end != '\0' || max_pairs < 0) return refuse("--max_pairs=N must be an integer >= 0");
        } else if ((v = value("--device="))) {
            char* end = nullptr;
            device = (int)strtol(v, &end, 10);
            if (end == v || *end != '\0' || device < 0) return refuse("--device=D must be an integer >= 0");
        } else if ((v = value("--voxel="))) {
            char* end = nullptr;
            const double t = strtod(v, &end);
            if (end == v || *end != '\0' || !(t > 0.0) || !((float)t <= FLT_MAX) || !((float)t > 0.0f)) return refuse("--voxel=V must be a finite number > 0");
            voxel = (float)t;
            have_voxel = true;
        } else if ((v = value("--crop="))) {
            const char* msg = "--crop=x0,y0,z0,x1,y1,z1 must be six finite numbers with x0 <= x1, y0 <= y1 and z0 <= z1";
            const char* s = v;
            for (int k = 0; k < 6; k++) {
                char* end = nullptr;
                const double t = strtod(s, &end);
                if (end == s || !(fabs(t) <= FLT_MAX) || *end != (k < 5 ? ',' : '\0')) return refuse(msg);
                crop[k] = (float)t;
                s = end + 1;
            }
            for (int a = 0; a < 3; a++)
                if (!(crop[a] <= crop[3 + a])) return refuse(msg);
            have_crop = true;
        } else if ((v = value("--clean_radius="))) {
            if (!(why = clean.parse('r', v)).empty()) return refuse(why);
        } else if ((v = value("--clean_min_neighbors="))) {
            if (!(why = clean.parse('n', v)).empty()) return refuse(why);
        } else if ((v = value("--clean_knn="))) {
            if (!(why = clean.parse('k', v)).empty()) return refuse(why);
        } else if ((v = value("--clean_ratio="))) {
            if (!(why = clean.parse('q', v)).empty()) return refuse(why);
        } else if ((v = value("--normals="))) {
            char* end = nullptr;
            const long k = strtol(v, &end, 10);
            if (end == v || *end != '\0' || k < 3 || k > TSAR_CLOUD_KNN_MAX) return refuse("--normals=K must be an integer in 3..32");
            nk = (int)k;
            have_normals = true;
        } else if ((v = value("--normal_radius="))) {
            char* end = nullptr;
            const double t = strtod(v, &end);
            if (end == v || *end != '\0' || !(t > 0.0) || !((float)t <= FLT_MAX) || !((float)t > 0.0f)) return refuse("--normal_radius=R must be a finite number > 0");
            nradius = (float)t;
            have_nradius = true;
        } else if ((v = value("--normal_min_neighbors="))) {
            char* end = nullptr;
            const long m = strtol(v, &end, 10);
            if (end == v || *end != '\0' || m < 2 || m > TSAR_CLOUD_KNN_MAX) return refuse("--normal_min_neighbors=N must be an integer in 2..K");
            nmin = (int)m;
            have_nmin = true;
        } else if ((v = value("--normal_tolerances="))) {
            const char* msg = "--normal_tolerances=D1[,D2...]: up to 16 angles in degrees, each a number in [0, 180]";
            ndeg.clear();
            have_ntol = true;
            const char* s = v;
            while (true) {
                char* end = nullptr;
                const double t = strtod(s, &end);
                if (end == s || !(t >= 0.0 && t <= 180.0) || ndeg.size() == 16) return refuse(msg);
                ndeg.push_back(t);
                if (*end == '\0') break;
                if (*end != ',') return refuse(msg);
                s = end + 1;
            }
        } else if (a == "--normal_signed") {
            nsigned = true;
        } else if ((v = value("--json="))) {
            json_path = v;
        } else if (a.compare(0, 2, "--") == 0) {
            return refuse("unknown option " + a);
        } else {
            paths.push_back(a);
        }
    }
    if (paths.size() != 2) { fprintf(stderr, "%s", usage); return 1; }
    if (!have_tol || tol.empty()) return refuse("--tolerances=T1[,T2...] is required");
    if (have_voxel && (!tsar_cloud_voxels_ctx || !tsar_default_cloud_voxels_params)) return refuse("--voxel: this libtsar_hip.so has no tsar_cloud_voxels");
    { const std::string why = clean.check(); if (!why.empty()) return refuse(why); }
    if (!have_normals && (have_nradius || have_nmin || have_ntol || nsigned))
        return refuse("--normal_radius=, --normal_min_neighbors=, --normal_tolerances= and --normal_signed need --normals=K");
    if (have_normals && !have_nradius) return refuse("--normals=K needs --normal_radius=R");
    if (have_normals && nmin > nk) return refuse("--normal_min_neighbors=N must be an integer in 2..K");
    if (have_normals && (!tsar_cloud_normals_ctx || !tsar_default_cloud_normals_params || !tsar_cloud_normal_compare_ctx))
        return refuse("--normals: this libtsar_hip.so has no tsar_cloud_normals");
    const int stride[2] = {have_normals ? 6 : 3, 3};      // with --normals RECON is read with its normals: records of 6 floats
    std::vector<float> cloud[2];
    int64_t n[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        std::string why;
        if (!(stride[k] == 6 ? read_cloud_ply_normals(paths[k], cloud[k], n[k], why) : read_cloud_ply(paths[k], cloud[k], n[k], why))) return refuse(why);
        if (n[k] > INT32_MAX) return refuse(paths[k] + ": more than 2^31 - 1 points");
    }
    tsar_ctx* ctx = nullptr;
    if (tsar_create(device, &ctx) != TSAR_OK) return refuse("tsar_create failed (is a HIP device visible?)");
    int64_t cleaned = 0;
    if (clean.on()) {                               // RECON's stray points become non-candidates, before the crop and the scoring
        std::vector<uint8_t> keep;
        if (!outlier_keep_mask(ctx, cloud[0].data(), n[0], stride[0], clean, keep)) {
            fprintf(stderr, "%s\n", tsar_last_error(ctx));
            tsar_destroy(ctx);
            return 1;
        }
        for (int64_t i = 0; i < n[0]; i++) {
            float* p = cloud[0].data() + (size_t)stride[0] * i;
            if (keep[(size_t)i] || !(fabsf(p[0]) <= FLT_MAX && fabsf(p[1]) <= FLT_MAX && fabsf(p[2]) <= FLT_MAX)) continue;
            p[0] = p[1] = p[2] = NAN;
            cleaned++;
        }
    }
    int64_t cropped[2] = {0, 0};
    for (int k = 0; k < 2 && have_crop; k++)        // a point outside the closed box becomes a non-candidate
        for (int64_t i = 0; i < n[k]; i++) {
            float* p = cloud[k].data() + (size_t)stride[k] * i;
            if (!(fabsf(p[0]) <= FLT_MAX && fabsf(p[1]) <= FLT_MAX && fabsf(p[2]) <= FLT_MAX)) continue;
            if (p[0] >= crop[0] && p[0] <= crop[3] && p[1] >= crop[1] && p[1] <= crop[4] && p[2] >= crop[2] && p[2] <= crop[5]) continue;
            p[0] = p[1] = p[2] = NAN;
            cropped[k]++;
        }
    tsar_cloud_distance_params prm;
    tsar_default_cloud_distance_params(&prm);
    for (const float t : tol) prm.max_dist = t > prm.max_dist ? t : prm.max_dist;
    if (max_pairs >= 0) prm.max_pairs = max_pairs;
    // direction 0: RECON against GT (accuracy); direction 1: GT against RECON (completeness)
    std::vector<int64_t> within[2] = {std::vector<int64_t>(tol.size(), 0), std::vector<int64_t>(tol.size(), 0)};
    int64_t valid[2] = {0, 0}, pairs[2] = {0, 0};
    double ms[2] = {0, 0};
    std::vector<float> dist2[2];
    std::vector<int32_t> vcount[2], vwithin[2];
    int64_t voxels[2] = {0, 0};
    std::vector<int32_t> nindex;
    for (int k = 0; k < 2; k++) {
        const auto t0 = std::chrono::steady_clock::now();
        const bool want_d2 = have_voxel || (have_normals && k == 0);         // the accuracy direction also gives --normals its dist2 and index
        if (want_d2) dist2[k].resize((size_t)n[k] + 1);
        if (have_normals && k == 0) nindex.resize((size_t)n[0] + 1);
        int rc = tsar_cloud_distance_ctx(ctx, cloud[k].data(), n[k], stride[k], cloud[1 - k].data(), n[1 - k], stride[1 - k], &prm, (int)tol.size(), tol.data(),
                                         want_d2 ? dist2[k].data() : nullptr, have_normals && k == 0 ? nindex.data() : nullptr, within[k].data(), &valid[k], &pairs[k],
                                         TSAR_MEM_HOST);
        if (rc == TSAR_OK && have_voxel) {          // the cloud's voxels: per voxel its points and how many of them lie within each tolerance
            tsar_cloud_voxels_params vp;
            tsar_default_cloud_voxels_params(&vp);
            vp.voxel = voxel;
            vcount[k].resize((size_t)n[k] + 1);
            vwithin[k].resize((size_t)n[k] * tol.size() + 1);
            rc = tsar_cloud_voxels_ctx(ctx, cloud[k].data(), n[k], stride[k], &vp, dist2[k].data(), (int)tol.size(), tol.data(), nullptr, n[k], nullptr, vcount[k].data(),
                                       vwithin[k].data(), &voxels[k], nullptr, TSAR_MEM_HOST);
        }
        ms[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc != TSAR_OK) {
            fprintf(stderr, "%s\n", tsar_last_error(ctx));
            tsar_destroy(ctx);
            return 1;
        }
    }
    // --normals: GT's normals from GT's points (after the crop), then every RECON point with a GT point within the largest tolerance scored
    std::vector<double> nmin_cos(ndeg.size()), nacc(ndeg.size(), 0.0);
    std::vector<int64_t> nwithin(ndeg.size(), 0);
    int64_t n_gt_normals = 0, n_compared = 0;
    if (have_normals) {
        tsar_cloud_normals_params np;
        tsar_default_cloud_normals_params(&np);
        np.radius = nradius;
        np.k = nk;
        np.min_neighbors = nmin;
        if (max_pairs >= 0) np.max_pairs = max_pairs;
        std::vector<float> gt_normal((size_t)n[1] * 3 + 1), recon_normal((size_t)n[0] * 3 + 1);
        for (int64_t i = 0; i < n[0]; i++) memcpy(&recon_normal[(size_t)i * 3], &cloud[0][(size_t)i * 6 + 3], 12);
        for (size_t k = 0; k < ndeg.size(); k++) nmin_cos[k] = cos(ndeg[k] * (M_PI / 180.0));      // one host cos per angle
        int rc = tsar_cloud_normals_ctx(ctx, cloud[1].data(), n[1], 3, &np, nullptr, nullptr, gt_normal.data(), nullptr, nullptr, nullptr, &n_gt_normals, nullptr,
                                        TSAR_MEM_HOST);
        if (rc == TSAR_OK)
            rc = tsar_cloud_normal_compare_ctx(ctx, recon_normal.data(), 3, n[0], gt_normal.data(), 3, n[1], nindex.data(), dist2[0].data(), prm.max_dist,
                                               (int)nmin_cos.size(), nmin_cos.data(), nsigned ? 1 : 0, nullptr, nwithin.data(), &n_compared, TSAR_MEM_HOST);
        if (rc != TSAR_OK) {
            fprintf(stderr, "%s\n", tsar_last_error(ctx));
            tsar_destroy(ctx);
            return 1;
        }
        for (size_t k = 0; k < ndeg.size(); k++) nacc[k] = n_compared ? (double)nwithin[k] / (double)n_compared : 0.0;
    }
    tsar_destroy(ctx);
    std::vector<double> acc(tol.size()), com(tol.size()), f1(tol.size());
    for (size_t k = 0; k < tol.size(); k++) {       // float64 ratios of the integer counts
        acc[k] = valid[0] ? (double)within[0][k] / (double)valid[0] : 0.0;
        com[k] = valid[1] ? (double)within[1][k] / (double)valid[1] : 0.0;
        f1[k] = acc[k] + com[k] > 0.0 ? 2.0 * acc[k] * com[k] / (acc[k] + com[k]) : 0.0;
    }
    // the voxel-averaged shares: per voxel one float64 division, the terms added one after another in ascending voxel order
    std::vector<double> vshare[2] = {std::vector<double>(tol.size(), 0.0), std::vector<double>(tol.size(), 0.0)}, vf1(tol.size(), 0.0);
    for (int d = 0; d < 2 && have_voxel; d++)
        for (size_t k = 0; k < tol.size(); k++) {
            double sum = 0.0;
            for (int64_t v = 0; v < voxels[d]; v++) sum += (double)vwithin[d][(size_t)v * tol.size() + k] / (double)vcount[d][(size_t)v];
            vshare[d][k] = voxels[d] ? sum / (double)voxels[d] : 0.0;
        }
    for (size_t k = 0; k < tol.size(); k++) vf1[k] = vshare[0][k] + vshare[1][k] > 0.0 ? 2.0 * vshare[0][k] * vshare[1][k] / (vshare[0][k] + vshare[1][k]) : 0.0;
    printf("%12s %12s %12s %12s %14s %14s", "tolerance", "accuracy", "completeness", "f1", "n_accurate", "n_complete");
    if (have_voxel) printf(" %14s %18s %12s", "accuracy_voxel", "completeness_voxel", "f1_voxel");
    printf("\n");
    for (size_t k = 0; k < tol.size(); k++) {
        printf("%12.9g %12.6f %12.6f %12.6f %14lld %14lld", (double)tol[k], acc[k], com[k], f1[k], (long long)within[0][k], (long long)within[1][k]);
        if (have_voxel) printf(" %14.6f %18.6f %12.6f", vshare[0][k], vshare[1][k], vf1[k]);
        printf("\n");
    }
    if (have_normals) {
        printf("normals: the plain PCA normal over the %d nearest neighbours within %.9g (no orientation propagated, nothing meshed; not a benchmark's program);\n"
               "         %lld GT normals, %lld RECON points compared (%s)\n", nk, (double)nradius, (long long)n_gt_normals, (long long)n_compared,
               nsigned ? "directions" : "lines");
        printf("%12s %16s %14s\n", "angle_deg", "normal_accuracy", "n_within");
        for (size_t k = 0; k < ndeg.size(); k++) printf("%12.9g %16.6f %14lld\n", ndeg[k], nacc[k], (long long)nwithin[k]);
    }
    auto f9 = [](float v) { char b[32]; snprintf(b, sizeof b, "%.9g", (double)v); return std::string(b); };
    auto f17 = [](double v) { char b[40]; snprintf(b, sizeof b, "%.17g", v); return std::string(b); };
    auto i64 = [](int64_t v) { return std::to_string((long long)v); };
    char head[256];
    snprintf(head, sizeof head, "\"n_recon\": %lld, \"n_gt\": %lld, \"n_recon_valid\": %lld, \"n_gt_valid\": %lld, ", (long long)n[0], (long long)n[1],
             (long long)valid[0], (long long)valid[1]);
    char tail[256];
    snprintf(tail, sizeof tail, "\"pairs_accuracy\": %lld, \"pairs_completeness\": %lld, \"ms_accuracy\": %.3f, \"ms_completeness\": %.3f", (long long)pairs[0],
             (long long)pairs[1], ms[0], ms[1]);
    std::string more;
    if (have_voxel)
        more += ", \"voxel\": " + f9(voxel) + ", \"n_recon_voxels\": " + i64(voxels[0]) + ", \"n_gt_voxels\": " + i64(voxels[1]) + ", \"accuracy_voxel\": " +
                json_list(vshare[0], f17) + ", \"completeness_voxel\": " + json_list(vshare[1], f17) + ", \"f1_voxel\": " + json_list(vf1, f17);
    if (have_crop)
        more += ", \"crop\": " + json_list(std::vector<float>(crop, crop + 6), f9) + ", \"n_recon_cropped\": " + i64(cropped[0]) + ", \"n_gt_cropped\": " + i64(cropped[1]);
    if (clean.on()) more += ", \"clean\": " + clean.json() + ", \"n_recon_cleaned\": " + i64(cleaned);
    if (have_normals)
        more += ", \"normals\": {\"k\": " + std::to_string(nk) + ", \"radius\": " + f9(nradius) + ", \"min_neighbors\": " + std::to_string(nmin) + ", \"signed\": " +
                (nsigned ? "true" : "false") + "}, \"normal_tolerances_deg\": " + json_list(ndeg, f17) + ", \"n_gt_normals\": " + i64(n_gt_normals) +
                ", \"n_normal_compared\": " + i64(n_compared) + ", \"n_normal_within\": " + json_list(nwithin, i64) + ", \"normal_accuracy\": " + json_list(nacc, f17);
    const std::string rec = "{\"recon\": " + json_string(paths[0]) + ", \"gt\": " + json_string(paths[1]) + ", " + head + "\"tolerances\": " + json_list(tol, f9) +
                            ", \"n_accurate\": " + json_list(within[0], i64) + ", \"n_complete\": " + json_list(within[1], i64) + ", \"accuracy\": " + json_list(acc, f17) +
                            ", \"completeness\": " + json_list(com, f17) + ", \"f1\": " + json_list(f1, f17) + ", " + tail + more + "}";
    printf("%s\n", rec.c_str());
    if (!json_path.empty()) {
        FILE* f = fopen(json_path.c_str(), "w");
        if (!f || fprintf(f, "%s\n", rec.c_str()) < 0 || fclose(f) != 0) return refuse("cannot write " + json_path);
    }
    return 0;
}
