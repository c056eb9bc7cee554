// tsar_evaluate — accuracy and completeness of a reconstructed cloud against a ground-truth cloud, on the GPU:
//   tsar_evaluate RECON.ply GT.ply --tolerances=0.01,0.02,0.05 [--max_pairs=N] [--device=D] [--json=FILE]
// accuracy(tau) = the share of RECON's points with a GT point within tau; completeness(tau) = the share of GT's points with a RECON point
// within tau; f1 = their harmonic mean: the point-wise precision / recall / F-score.  Not ETH3D's or DTU's evaluation program: nothing is
// down-sampled, masked, cropped or aligned.  Two tsar_cloud_distance_ctx calls with max_dist = the largest tolerance (include/tsar.h);
// points with a non-finite coordinate take no part.  Prints one table and one JSON line; --json=FILE gets the same line.
#include <stdlib.h>

#include <chrono>

#include "tsar_io.h"

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
    const char* usage = "usage: tsar_evaluate RECON.ply GT.ply --tolerances=T1[,T2...] [--max_pairs=N] [--device=D] [--json=FILE]\n"
                        "       point-wise accuracy / completeness / F-score of RECON against GT at each tolerance (not ETH3D's or DTU's program:\n"
                        "       no voxel averaging, masks, cropping or alignment)\n";
    if (argc >= 2 && (!strcmp(argv[1], "-h") || !strcmp(argv[1], "--help"))) { printf("%s", usage); return 0; }
    std::vector<std::string> paths;
    std::vector<float> tol;
    bool have_tol = false;
    long long max_pairs = -1;
    int device = 0;
    std::string json_path;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&](const char* opt) -> const char* { const size_t n = strlen(opt); return a.compare(0, n, opt) == 0 ? argv[i] + n : nullptr; };
        const char* v;
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
    std::vector<float> cloud[2];
    int64_t n[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        std::string why;
        if (!read_cloud_ply(paths[k], cloud[k], n[k], why)) return refuse(why);
        if (n[k] > INT32_MAX) return refuse(paths[k] + ": more than 2^31 - 1 points");
    }
    tsar_cloud_distance_params prm;
    tsar_default_cloud_distance_params(&prm);
    for (const float t : tol) prm.max_dist = t > prm.max_dist ? t : prm.max_dist;
    if (max_pairs >= 0) prm.max_pairs = max_pairs;
    tsar_ctx* ctx = nullptr;
    if (tsar_create(device, &ctx) != TSAR_OK) return refuse("tsar_create failed (is a HIP device visible?)");
    // direction 0: RECON against GT (accuracy); direction 1: GT against RECON (completeness)
    std::vector<int64_t> within[2] = {std::vector<int64_t>(tol.size(), 0), std::vector<int64_t>(tol.size(), 0)};
    int64_t valid[2] = {0, 0}, pairs[2] = {0, 0};
    double ms[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = tsar_cloud_distance_ctx(ctx, cloud[k].data(), n[k], 3, cloud[1 - k].data(), n[1 - k], 3, &prm, (int)tol.size(), tol.data(), nullptr, nullptr,
                                               within[k].data(), &valid[k], &pairs[k], TSAR_MEM_HOST);
        ms[k] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (rc != TSAR_OK) {
            fprintf(stderr, "%s\n", tsar_last_error(ctx));
            tsar_destroy(ctx);
            return 1;
        }
    }
    tsar_destroy(ctx);
    std::vector<double> acc(tol.size()), com(tol.size()), f1(tol.size());
    for (size_t k = 0; k < tol.size(); k++) {       // float64 ratios of the integer counts
        acc[k] = valid[0] ? (double)within[0][k] / (double)valid[0] : 0.0;
        com[k] = valid[1] ? (double)within[1][k] / (double)valid[1] : 0.0;
        f1[k] = acc[k] + com[k] > 0.0 ? 2.0 * acc[k] * com[k] / (acc[k] + com[k]) : 0.0;
    }
    printf("%12s %12s %12s %12s %14s %14s\n", "tolerance", "accuracy", "completeness", "f1", "n_accurate", "n_complete");
    for (size_t k = 0; k < tol.size(); k++)
        printf("%12.9g %12.6f %12.6f %12.6f %14lld %14lld\n", (double)tol[k], acc[k], com[k], f1[k], (long long)within[0][k], (long long)within[1][k]);
    auto f9 = [](float v) { char b[32]; snprintf(b, sizeof b, "%.9g", (double)v); return std::string(b); };
    auto f17 = [](double v) { char b[40]; snprintf(b, sizeof b, "%.17g", v); return std::string(b); };
    auto i64 = [](int64_t v) { return std::to_string((long long)v); };
    char head[256];
    snprintf(head, sizeof head, "\"n_recon\": %lld, \"n_gt\": %lld, \"n_recon_valid\": %lld, \"n_gt_valid\": %lld, ", (long long)n[0], (long long)n[1],
             (long long)valid[0], (long long)valid[1]);
    char tail[256];
    snprintf(tail, sizeof tail, "\"pairs_accuracy\": %lld, \"pairs_completeness\": %lld, \"ms_accuracy\": %.3f, \"ms_completeness\": %.3f", (long long)pairs[0],
             (long long)pairs[1], ms[0], ms[1]);
    const std::string rec = "{\"recon\": " + json_string(paths[0]) + ", \"gt\": " + json_string(paths[1]) + ", " + head + "\"tolerances\": " + json_list(tol, f9) +
                            ", \"n_accurate\": " + json_list(within[0], i64) + ", \"n_complete\": " + json_list(within[1], i64) + ", \"accuracy\": " + json_list(acc, f17) +
                            ", \"completeness\": " + json_list(com, f17) + ", \"f1\": " + json_list(f1, f17) + ", " + tail + "}";
    printf("%s\n", rec.c_str());
    if (!json_path.empty()) {
        FILE* f = fopen(json_path.c_str(), "w");
        if (!f || fprintf(f, "%s\n", rec.c_str()) < 0 || fclose(f) != 0) return refuse("cannot write " + json_path);
    }
    return 0;
}
