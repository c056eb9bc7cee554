// tsar_evaluate_maps — a scene's depth maps scored per pixel against a scan rendered into their own cameras, on the GPU:
//   tsar_evaluate_maps D/ GT.ply --tolerances=0.001,0.01 --radius=R [--maps=STEM] [--max_px=N] [--occlusion_diff=REL] [--depth_diff=REL]
//                      [--min_points=N] [--views=id,id,...] [--write_gt=STEM] [--device=D] [--json=FILE]
//                      [--oriented [--normals=K] [--normal_radius=R] [--normal_min_neighbors=N]]
// Reads D/pair.txt and D/cams/%08d_cam.txt the way tsar_fusion does, GT.ply with tsar_io.h's reader, and for every view
// D/APD/%08d/STEM_disp.dmb (STEM: TSAR by default).  The cloud is uploaded once; per view it is rendered at the map's own size
// (tsar_cloud_render_ctx: occlusion by the cloud's own points, at the footprint --radius names in world units) and the map is compared
// with the render (tsar_depth_compare_ctx): the share of the pixels within each relative tolerance, in front and behind.  A view without a
// map is named and skipped.  Prints one table row per view, a total row (the counts added first, the ratios formed afterwards) and one
// JSON line; --json=FILE gets the same line.  --write_gt=STEM also writes each rendered map as D/APD/%08d/STEM_disp.dmb.
// --oriented renders with the normal-oriented occluder (tsar_cloud_render_oriented_ctx: a point occludes as its tangent disc, so a slanted
// surface does not hide itself), with GT.ply's nx ny nz, or with --normal_radius=R with the plain PCA normals of its points, estimated once
// on the device (tsar_cloud_normals_ctx: the K (16) nearest neighbours within R, at least N (5) of them); a point that gets no normal keeps
// the square occluder.
// These are the project's own per-pixel bars against a rendered scan, not ETH3D's or DTU's program: no observation masks, no alignment.
#include <math.h>
#include <stdlib.h>

#include <chrono>

#include "tsar_io.h"

// The entries that only --oriented calls are referred to weakly: the tool still links against, and runs with, a library that lacks them, and
// says so in one line when --oriented asks for them.
extern "C" {
int tsar_cloud_render_oriented_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const float* normals, int normal_stride, const tsar_camera* cam, int w, int h,
                                   const tsar_cloud_render_params* p, float* depth_out, uint8_t* count_out, int32_t* index_out, float* occluder_out, int64_t* n_splats_out,
                                   int64_t* n_covered_out, int mem) __attribute__((weak));
void tsar_default_cloud_normals_params(tsar_cloud_normals_params* p) __attribute__((weak));
int tsar_cloud_normals_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_normals_params* p, int32_t* knn_index_out, int32_t* n_used_out,
                           float* normal_out, float* curvature_out, double* cov_out, int64_t* n_valid_out, int64_t* n_normals_out, int64_t* pairs_out,
                           int mem) __attribute__((weak));
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

struct Counts {
    int64_t n_gt = 0, n_both = 0, n_front = 0, n_behind = 0, n_splats = 0, n_covered = 0;     // (n_covered: --oriented only)
    std::vector<int64_t> within;
};

static std::string f9(float v) { char b[32]; snprintf(b, sizeof b, "%.9g", (double)v); return b; }
static std::string f17(double v) { char b[40]; snprintf(b, sizeof b, "%.17g", v); return b; }
static std::string i64(int64_t v) { return std::to_string((long long)v); }

// the counts and the float64 ratios formed from them (0 where a denominator is 0)
static std::string counts_json(const Counts& c, bool oriented) {
    std::vector<double> acc(c.within.size()), com(c.within.size());
    for (size_t k = 0; k < c.within.size(); k++) {
        acc[k] = c.n_both ? (double)c.within[k] / (double)c.n_both : 0.0;
        com[k] = c.n_gt ? (double)c.within[k] / (double)c.n_gt : 0.0;
    }
    return "\"n_gt\": " + i64(c.n_gt) + ", \"n_both\": " + i64(c.n_both) + ", \"within\": " + json_list(c.within, i64) + ", \"n_front\": " + i64(c.n_front) +
           ", \"n_behind\": " + i64(c.n_behind) + ", \"n_splats\": " + i64(c.n_splats) + (oriented ? ", \"n_covered\": " + i64(c.n_covered) : std::string()) + ", \"accuracy\": " + json_list(acc, f17) + ", \"completeness\": " +
           json_list(com, f17) + ", \"cover\": " + f17(c.n_gt ? (double)c.n_both / (double)c.n_gt : 0.0);
}

static void print_row(const char* name, const Counts& c) {
    printf("%10s %10lld %10lld %8.6f %10lld %10lld", name, (long long)c.n_gt, (long long)c.n_both, c.n_gt ? (double)c.n_both / (double)c.n_gt : 0.0, (long long)c.n_front,
           (long long)c.n_behind);
    for (const int64_t wk : c.within) printf(" %10lld %8.6f", (long long)wk, c.n_both ? (double)wk / (double)c.n_both : 0.0);
    printf("\n");
}

int main(int argc, char** argv) {
    (void)write_cloud_ply;                         // (tsar_io.h's writer, unused here)
    const char* usage = "usage: tsar_evaluate_maps D/ GT.ply --tolerances=T1[,T2...] --radius=R [--maps=STEM] [--max_px=N] [--occlusion_diff=REL] [--depth_diff=REL]\n"
                        "                          [--min_points=N] [--views=id,id,...] [--write_gt=STEM] [--device=D] [--json=FILE]\n"
                        "                          [--oriented [--normals=K] [--normal_radius=R] [--normal_min_neighbors=N]]\n"
                        "       every D/APD/%08d/STEM_disp.dmb (STEM: TSAR) compared per pixel with GT.ply rendered into the view's camera, occlusion by the cloud's\n"
                        "       own points at a footprint of R world units; --write_gt=STEM also writes the rendered maps.  The project's own per-pixel bars\n"
                        "       against a rendered scan, not ETH3D's or DTU's program: no observation masks, no alignment.  --oriented: a point occludes as\n"
                        "       its tangent disc of radius R (still cut to the square), with GT.ply's nx ny nz, or with --normal_radius=R with PCA normals\n"
                        "       estimated from its points (the K (16) nearest within R, at least N (5)); a point without a normal keeps the square\n";
    if (argc >= 2 && (!strcmp(argv[1], "-h") || !strcmp(argv[1], "--help"))) { printf("%s", usage); return 0; }
    std::vector<std::string> paths;
    std::vector<float> tol;
    bool have_tol = false, have_radius = false, have_views = false;
    tsar_cloud_render_params prm;
    tsar_default_cloud_render_params(&prm);
    int device = 0;
    std::string json_path, stem = "TSAR", write_gt;
    bool have_write_gt = false;
    std::vector<int> only;
    bool oriented = false, have_nk = false, have_nradius = false, have_nmin = false;
    int nk = 16, nmin = 5;
    float nradius = 0.0f;
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        auto value = [&](const char* opt) -> const char* { const size_t n = strlen(opt); return a.compare(0, n, opt) == 0 ? argv[i] + n : nullptr; };
        auto number = [](const char* v, double& t) { char* end = nullptr; t = strtod(v, &end); return end != v && *end == '\0'; };
        auto integer = [](const char* v, long& t) { char* end = nullptr; t = strtol(v, &end, 10); return end != v && *end == '\0'; };
        const char* v;
        double t;
        long k;
        if ((v = value("--tolerances="))) {
            const char* msg = "--tolerances=T1[,T2...]: 1 to 16 tolerances, every one a finite number > 0";
            have_tol = true;
            const char* s = v;
            while (true) {
                char* end = nullptr;
                t = strtod(s, &end);
                if (end == s || !(t > 0.0) || !((float)t <= FLT_MAX) || !((float)t > 0.0f) || tol.size() == TSAR_DEPTH_COMPARE_MAX_TOL) return refuse(msg);
                tol.push_back((float)t);
                if (*end == '\0') break;
                if (*end != ',') return refuse(msg);
                s = end + 1;
            }
        } else if ((v = value("--radius="))) {
            if (!number(v, t) || !(t >= 0.0) || !((float)t <= FLT_MAX)) return refuse("--radius=R must be a finite number >= 0");
            prm.radius = (float)t;
            have_radius = true;
        } else if ((v = value("--max_px="))) {
            if (!integer(v, k) || k < 1 || k > 16) return refuse("--max_px=N must be an integer in 1..16");
            prm.max_px = (int32_t)k;
        } else if ((v = value("--occlusion_diff="))) {
            if (!number(v, t) || !(t >= 0.0) || !((float)t <= FLT_MAX)) return refuse("--occlusion_diff=REL must be a finite number >= 0");
            prm.occlusion_diff = (float)t;
        } else if ((v = value("--depth_diff="))) {
            if (!number(v, t) || !(t >= 0.0) || !((float)t <= FLT_MAX)) return refuse("--depth_diff=REL must be a finite number >= 0");
            prm.depth_diff = (float)t;
        } else if ((v = value("--min_points="))) {
            if (!integer(v, k) || k < 1 || k > 255) return refuse("--min_points=N must be an integer in 1..255");
            prm.min_points = (int32_t)k;
        } else if ((v = value("--views="))) {
            const char* msg = "--views=id[,id...]: every id must be an integer >= 0";
            have_views = true;
            const char* s = v;
            while (true) {
                char* end = nullptr;
                k = strtol(s, &end, 10);
                if (end == s || k < 0 || k > 99999999) return refuse(msg);
                only.push_back((int)k);
                if (*end == '\0') break;
                if (*end != ',') return refuse(msg);
                s = end + 1;
            }
        } else if ((v = value("--maps="))) {
            stem = v;
            if (stem.empty() || stem.find('/') != std::string::npos) return refuse("--maps=STEM must not be empty or contain a path separator");
        } else if ((v = value("--write_gt="))) {
            write_gt = v;
            have_write_gt = true;
            if (write_gt.empty() || write_gt.find('/') != std::string::npos) return refuse("--write_gt=STEM must not be empty or contain a path separator");
            if (write_gt == "TSAR" || write_gt == "TSAR_geom" || write_gt == "TSAR_filtered") return refuse("--write_gt=" + write_gt + " would overwrite the matcher's own maps");
        } else if ((v = value("--device="))) {
            if (!integer(v, k) || k < 0) return refuse("--device=D must be an integer >= 0");
            device = (int)k;
        } else if (a == "--oriented") {
            oriented = true;
        } else if ((v = value("--normals="))) {
            if (!integer(v, k) || k < 3 || k > TSAR_CLOUD_KNN_MAX) return refuse("--normals=K must be an integer in 3..32");
            nk = (int)k;
            have_nk = true;
        } else if ((v = value("--normal_radius="))) {
            if (!number(v, t) || !(t > 0.0) || !((float)t <= FLT_MAX) || !((float)t > 0.0f)) return refuse("--normal_radius=R must be a finite number > 0");
            nradius = (float)t;
            have_nradius = true;
        } else if ((v = value("--normal_min_neighbors="))) {
            if (!integer(v, k) || k < 2 || k > TSAR_CLOUD_KNN_MAX) return refuse("--normal_min_neighbors=N must be an integer in 2..K");
            nmin = (int)k;
            have_nmin = true;
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
    if (!have_radius) return refuse("--radius=R is required (world units; 0 renders without a footprint)");
    if (have_write_gt && write_gt == stem) return refuse("--write_gt=" + write_gt + " would overwrite the maps it is compared with");
    if (!oriented && (have_nk || have_nradius || have_nmin)) return refuse("--normals=, --normal_radius= and --normal_min_neighbors= need --oriented");
    if ((have_nk || have_nmin) && !have_nradius) return refuse("--normals=K and --normal_min_neighbors=N need --normal_radius=R");
    if (have_nradius && nmin > nk) return refuse("--normal_min_neighbors=N must be an integer in 2..K");
    if (oriented && (!tsar_cloud_render_oriented_ctx || (have_nradius && (!tsar_cloud_normals_ctx || !tsar_default_cloud_normals_params))))
        return refuse("--oriented: this libtsar_hip.so has no tsar_cloud_render_oriented");
    const int stride = oriented && !have_nradius ? 6 : 3;       // --oriented without an estimate reads GT.ply with its normals: records of 6 floats
    std::string dir = paths[0];
    if (dir.back() != '/') dir += '/';
    std::map<int, std::vector<int>> pairs;
    if (!read_pairs(dir + "pair.txt", pairs)) return refuse("cannot read " + dir + "pair.txt");
    std::vector<int> ids;
    if (have_views) {
        for (const int id : only) {
            if (!pairs.count(id)) return refuse("--views: view " + std::to_string(id) + " is not in pair.txt");
            ids.push_back(id);
        }
    } else {
        for (auto& kv : pairs) ids.push_back(kv.first);
    }
    std::vector<float> cloud;
    int64_t n = 0;
    {
        std::string why;
        if (!(stride == 6 ? read_cloud_ply_normals(paths[1], cloud, n, why) : read_cloud_ply(paths[1], cloud, n, why)))
            return refuse(stride == 6 && why.find("has no property n") != std::string::npos
                              ? "--oriented: " + paths[1] + " has no nx ny nz: give --normal_radius=R (and --normals=K) to estimate them from its points" : why);
        if (n > INT32_MAX) return refuse(paths[1] + ": more than 2^31 - 1 points");
    }
    tsar_ctx* ctx = nullptr;
    if (tsar_create(device, &ctx) != TSAR_OK) return refuse("tsar_create failed (is a HIP device visible?)");
    // the cloud goes to the device once; per view the map goes up, the render and the comparison stay there
    float* d_cloud = n ? (float*)tsar_device_alloc(device, (size_t)n * stride * sizeof(float)) : nullptr;
    float* d_normals = n && have_nradius ? (float*)tsar_device_alloc(device, (size_t)n * 3 * sizeof(float)) : nullptr;
    float *d_map = nullptr, *d_gt = nullptr;
    size_t map_cap = 0;
    auto leave = [&](const std::string& msg) {
        tsar_device_free(device, d_cloud);
        tsar_device_free(device, d_normals);
        tsar_device_free(device, d_map);
        tsar_device_free(device, d_gt);
        const std::string m = msg.empty() ? std::string(tsar_last_error(ctx)) : msg;
        tsar_destroy(ctx);
        return refuse(m);
    };
    if (n && (!d_cloud || tsar_device_write(device, d_cloud, cloud.data(), (size_t)n * stride * sizeof(float)) != TSAR_OK)) return leave("cannot upload the cloud");
    int64_t n_gt_normals = 0;
    if (have_nradius) {                             // the scan's normals, once, on the device; 0 0 0 where a point gets none
        if (n && !d_normals) return leave("cannot allocate the normals on the device");
        tsar_cloud_normals_params np;
        tsar_default_cloud_normals_params(&np);
        np.radius = nradius;
        np.k = nk;
        np.min_neighbors = nmin;
        if (tsar_cloud_normals_ctx(ctx, d_cloud, n, 3, &np, nullptr, nullptr, d_normals, nullptr, nullptr, nullptr, &n_gt_normals, nullptr, TSAR_MEM_DEVICE) != TSAR_OK)
            return leave("");
    }
    std::vector<Counts> per_view;
    std::vector<int> done, sizes_w, sizes_h, skipped;
    std::vector<double> ms;
    Counts total;
    total.within.assign(tol.size(), 0);
    std::vector<float> map, rendered;
    for (const int id : ids) {
        char name[32];
        snprintf(name, sizeof name, "%08d", id);
        int h = 0, w = 0, nb = 0;
        const std::string rel = std::string("APD/") + name + "/" + stem + "_disp.dmb";
        if (!read_dmb(dir + rel, map, h, w, nb) || nb != 1 || w < 1 || h < 1) {
            printf("view %s: no %s, skipped\n", name, rel.c_str());
            skipped.push_back(id);
            continue;
        }
        CamFile cf;
        if (!read_cam(dir + "cams/" + name + "_cam.txt", cf)) return leave(std::string("cannot read camera of view ") + name);
        const auto t0 = std::chrono::steady_clock::now();
        const size_t np = (size_t)w * h;
        if (np > map_cap) {
            tsar_device_free(device, d_map);
            tsar_device_free(device, d_gt);
            d_map = (float*)tsar_device_alloc(device, np * sizeof(float));
            d_gt = (float*)tsar_device_alloc(device, np * sizeof(float));
            map_cap = d_map && d_gt ? np : 0;
            if (!map_cap) return leave("cannot allocate the maps on the device");
        }
        if (tsar_device_write(device, d_map, map.data(), np * sizeof(float)) != TSAR_OK) return leave("cannot upload the map of view " + std::string(name));
        Counts c;
        c.within.assign(tol.size(), 0);
        if ((oriented ? tsar_cloud_render_oriented_ctx(ctx, d_cloud, n, stride, d_normals, 3, &cf.cam, w, h, &prm, d_gt, nullptr, nullptr, nullptr, &c.n_splats, &c.n_covered,
                                                       TSAR_MEM_DEVICE)
                      : tsar_cloud_render_ctx(ctx, d_cloud, n, 3, &cf.cam, w, h, &prm, d_gt, nullptr, nullptr, &c.n_splats, TSAR_MEM_DEVICE)) != TSAR_OK)
            return leave("");
        if (tsar_depth_compare_ctx(ctx, d_map, d_gt, nullptr, (int64_t)np, (int)tol.size(), tol.data(), &c.n_gt, &c.n_both, c.within.data(), &c.n_front, &c.n_behind, nullptr,
                                   TSAR_MEM_DEVICE) != TSAR_OK)
            return leave("");
        ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        if (have_write_gt) {
            rendered.resize(np);
            if (tsar_device_read(device, rendered.data(), d_gt, np * sizeof(float)) != TSAR_OK) return leave("cannot read back the rendered map of view " + std::string(name));
            const std::string out = dir + "APD/" + name + "/" + write_gt + "_disp.dmb";
            if (!write_dmb(out, rendered.data(), h, w, 1)) return leave("cannot write " + out);
        }
        total.n_gt += c.n_gt; total.n_both += c.n_both; total.n_front += c.n_front; total.n_behind += c.n_behind; total.n_splats += c.n_splats;
        total.n_covered += c.n_covered;
        for (size_t k = 0; k < tol.size(); k++) total.within[k] += c.within[k];
        per_view.push_back(c);
        done.push_back(id);
        sizes_w.push_back(w);
        sizes_h.push_back(h);
    }
    tsar_device_free(device, d_cloud);
    tsar_device_free(device, d_normals);
    tsar_device_free(device, d_map);
    tsar_device_free(device, d_gt);
    tsar_destroy(ctx);
    if (done.empty()) return refuse("no view has a map APD/%08d/" + stem + "_disp.dmb under " + dir);
    printf("%10s %10s %10s %8s %10s %10s", "view", "n_gt", "n_both", "cover", "n_front", "n_behind");
    for (const float t : tol) { char b[32]; snprintf(b, sizeof b, "<=%g", (double)t); printf(" %10s %8s", b, "share"); }
    printf("\n");
    for (size_t k = 0; k < done.size(); k++) {
        char name[32];
        snprintf(name, sizeof name, "%08d", done[k]);
        print_row(name, per_view[k]);
    }
    print_row("total", total);
    std::string views = "[";
    for (size_t k = 0; k < done.size(); k++) {
        char ms_txt[32];
        snprintf(ms_txt, sizeof ms_txt, "%.3f", ms[k]);
        views += std::string(k ? ", " : "") + "{\"id\": " + std::to_string(done[k]) + ", \"w\": " + std::to_string(sizes_w[k]) + ", \"h\": " + std::to_string(sizes_h[k]) + ", " +
                 counts_json(per_view[k], oriented) + ", \"ms\": " + ms_txt + "}";
    }
    views += "]";
    auto id_txt = [](int v) { return std::to_string(v); };
    const std::string rec = "{\"dir\": " + json_string(paths[0]) + ", \"gt\": " + json_string(paths[1]) + ", \"maps\": " + json_string(stem) + ", \"n_points\": " + i64(n) +
                            ", \"tolerances\": " + json_list(tol, f9) + ", \"radius\": " + f9(prm.radius) + ", \"max_px\": " + std::to_string(prm.max_px) +
                            ", \"occlusion_diff\": " + f9(prm.occlusion_diff) + ", \"depth_diff\": " + f9(prm.depth_diff) + ", \"min_points\": " + std::to_string(prm.min_points) +
                            (oriented ? std::string(", \"oriented\": true") : std::string()) +
                            (have_nradius ? ", \"normals\": {\"k\": " + std::to_string(nk) + ", \"radius\": " + f9(nradius) + ", \"min_neighbors\": " + std::to_string(nmin) +
                                                "}, \"n_gt_normals\": " + i64(n_gt_normals)
                                          : std::string()) +
                            (have_write_gt ? ", \"write_gt\": " + json_string(write_gt) : std::string()) + ", \"skipped\": " + json_list(skipped, id_txt) + ", \"views\": " + views +
                            ", \"total\": {" + counts_json(total, oriented) + "}}";
    printf("%s\n", rec.c_str());
    if (!json_path.empty()) {
        FILE* f = fopen(json_path.c_str(), "w");
        if (!f || fprintf(f, "%s\n", rec.c_str()) < 0 || fclose(f) != 0) return refuse("cannot write " + json_path);
    }
    return 0;
}
