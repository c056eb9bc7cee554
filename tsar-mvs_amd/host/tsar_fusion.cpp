// tsar_fusion — C++ host tool with the command line of the reference's fuser
// (x/1.sh:30:  Fusion <mslp_dir> --num_consistent= 1 --reproj_error= 2 --depth_diff= 0.01 --angle= 15 --used_list= 1 ;
// note the blank after '=' in the reference's scripts — both spellings are accepted).
// Reads <dir>/pair.txt, <dir>/cams/%08d_cam.txt, <dir>/images/%08d.pgm (else the .jpg of that name) and, per view,
// <dir>/APD/%08d/TSAR_disp.dmb + TSAR_normals.dmb (what tsar_gipuma / the reference write), fuses them on
// the GPU (tsar_fuse) and writes <dir>/APD/APD_TSAR.ply (binary little-endian: x y z nx ny nz red green blue).
// --voxel=V thins the fused cloud before it is written: a grid of edge V over it (tsar_cloud_voxels), and per occupied voxel the record of
// the point nearest the voxel's centre, whole, in the cloud's own order.
// --outlier_radius=R with --outlier_min_neighbors=N and / or --outlier_knn=K [--outlier_ratio=Q] removes the fused cloud's stray points
// first (host/tsar_outliers.h: the rules of api.remove_outliers, one tsar_cloud_neighbors_ctx call): before --voxel thins and before the
// cloud is written.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <future>
#include <memory>

#include "tsar_io.h"
#include "tsar_jpeg.h"
#include "tsar_outliers.h"

// The entries that only --voxel calls are referred to weakly: the tool still links against, and runs with, a library that lacks them, and
// refuses the switch there.
extern "C" {
void tsar_default_cloud_voxels_params(tsar_cloud_voxels_params* p) __attribute__((weak));
int tsar_cloud_voxels_ctx(tsar_ctx* ctx, const float* cloud, int64_t n, int stride, const tsar_cloud_voxels_params* p, const float* dist2, int n_tol, const float* tol,
                          int32_t* rank_out, int64_t cap, int32_t* rep_out, int32_t* count_out, int32_t* within_out, int64_t* n_voxels_out, int64_t* n_valid_out,
                          int mem) __attribute__((weak));
}

int main(int argc, char** argv) {
    if (argc < 2 || !strcmp(argv[1], "-h") || !strcmp(argv[1], "--help")) {
        printf("usage: tsar_fusion <mslp_dir> [--num_consistent= N] [--reproj_error= PX] [--depth_diff= REL] [--angle= DEG] [--used_list= 0|1] [--gpu=K] [--geom] [--voxel=V]\n"
               "                  [--outlier_radius=R [--outlier_min_neighbors=N] [--outlier_knn=K [--outlier_ratio=Q]]]\n"
               "       --geom: fuse APD/%%08d/TSAR_geom_disp.dmb + TSAR_geom_normals.dmb instead of TSAR_disp.dmb + TSAR_normals.dmb\n"
               "       --voxel=V: write one point per occupied voxel of edge V (the one nearest the voxel's centre, its whole record)\n"
               "       --outlier_radius=R: first drop the points with fewer than N others within R and / or whose K-th neighbour within R lies\n"
               "                           beyond Q (2) times the median K-th-neighbour distance\n");
        return argc < 2 ? 1 : 0;
    }
    std::string dir = argv[1];
    if (dir.back() != '/') dir += '/';
    tsar_fusion_params prm;
    tsar_default_fusion_params(&prm);
    int gpu = 0;
    float voxel = 0.0f;         // --voxel=V: thin the fused cloud (0: off)
    OutlierSettings outlier("--outlier_");
    bool geom = false;          // --geom: the geometric-consistency pass's maps (tsar_gipuma --all --geom_consistency)
    std::string why;            // the one-line refusal of an --outlier_ switch
    for (int i = 2; i < argc; i++) {
        const char* a = argv[i];
        auto value = [&](const char* opt) -> const char* {      // "--opt=VALUE" or "--opt= VALUE"
            const size_t n = strlen(opt);
            if (strncmp(a, opt, n) != 0) return nullptr;
            if (a[n] != '\0') return a + n;
            return i + 1 < argc ? argv[++i] : "";
        };
        const char* v;
        if ((v = value("--num_consistent="))) prm.num_consistent = atoi(v);
        else if ((v = value("--reproj_error="))) prm.reproj_error = (float)atof(v);
        else if ((v = value("--depth_diff="))) prm.depth_diff = (float)atof(v);
        else if ((v = value("--angle="))) prm.angle_deg = (float)atof(v);
        else if ((v = value("--used_list="))) prm.used_list = atoi(v);
        else if ((v = value("--gpu="))) gpu = atoi(v);
        else if (!strcmp(a, "--geom")) geom = true;
        else if ((v = value("--voxel="))) {
            char* end = nullptr;
            const double t = strtod(v, &end);
            if (end == v || *end != '\0' || !(t > 0.0) || !((float)t <= FLT_MAX) || !((float)t > 0.0f)) { fprintf(stderr, "--voxel=V must be a finite number > 0\n"); return 1; }
            voxel = (float)t;
            if (!tsar_cloud_voxels_ctx || !tsar_default_cloud_voxels_params) { fprintf(stderr, "--voxel: this libtsar_hip.so has no tsar_cloud_voxels\n"); return 1; }
        }
        else if ((v = value("--outlier_radius="))) { if (!(why = outlier.parse('r', v)).empty()) break; }
        else if ((v = value("--outlier_min_neighbors="))) { if (!(why = outlier.parse('n', v)).empty()) break; }
        else if ((v = value("--outlier_knn="))) { if (!(why = outlier.parse('k', v)).empty()) break; }
        else if ((v = value("--outlier_ratio="))) { if (!(why = outlier.parse('q', v)).empty()) break; }
        else printf("Command-line parameter warning: unknown option %s\n", a);
    }
    if (why.empty()) why = outlier.check();
    if (!why.empty()) { fprintf(stderr, "%s\n", why.c_str()); return 1; }
    printf("num_consistent: %d\nreproj_error: %g\ndepth_diff: %g\nangle: %g\nused_list: %d\n", prm.num_consistent, prm.reproj_error, prm.depth_diff, prm.angle_deg, prm.used_list);
    const std::string depth_file = geom ? "TSAR_geom_disp.dmb" : "TSAR_disp.dmb", normal_file = geom ? "TSAR_geom_normals.dmb" : "TSAR_normals.dmb";
    std::map<int, std::vector<int>> pairs;
    if (!read_pairs(dir + "pair.txt", pairs)) { fprintf(stderr, "cannot read %spair.txt\n", dir.c_str()); return 1; }
    std::vector<int> ids;
    for (auto& kv : pairs) ids.push_back(kv.first);
    std::map<int, int> slot;
    for (size_t k = 0; k < ids.size(); k++) slot[ids[k]] = (int)k;
    const int n = (int)ids.size();
    std::vector<tsar_camera> cams(n);
    std::vector<std::vector<float>> depth(n), normal(n), gray(n);
    std::vector<const float*> pd(n), pn(n), pg(n);
    int w = 0, h = 0;
    // every view's three files are read by its own helper thread (0.39 GB of maps per full-size view)
    std::vector<int> vw(n, 0), vh(n, 0);
    std::vector<std::string> problem(n);
    auto load = [&](int k) {
        char name[32];
        snprintf(name, sizeof name, "%08d", ids[k]);
        CamFile cf;
        if (!read_cam(dir + "cams/" + name + "_cam.txt", cf)) { problem[k] = std::string("cannot read camera of view ") + name; return; }
        cams[k] = cf.cam;
        int hh, ww, nb;
        if (!read_dmb(dir + "APD/" + name + "/" + depth_file, depth[k], hh, ww, nb) || nb != 1) { problem[k] = std::string("cannot read APD/") + name + "/" + depth_file; return; }
        vw[k] = ww; vh[k] = hh;
        int h2, w2;
        if (!read_dmb(dir + "APD/" + name + "/" + normal_file, normal[k], h2, w2, nb) || nb != 3 || w2 != ww || h2 != hh) { problem[k] = std::string("cannot read APD/") + name + "/" + normal_file; return; }
        int iw, ih;
        bool have = read_pgm(dir + "images/" + name + ".pgm", gray[k], iw, ih);
        for (const char* ext : {".jpg", ".JPG", ".jpeg", ".JPEG"}) {          // the scene's own JPEG (host/tsar_jpeg.h), like tsar_gipuma
            if (have) break;
            std::vector<uint8_t> px;
            if (tsar_jpeg::read(dir + "images/" + name + ext, tsar_jpeg::LUMA, px, iw, ih)) { gray[k].assign(px.begin(), px.end()); have = true; }
        }
        if (!have || iw != ww || ih != hh) gray[k].assign((size_t)ww * hh, 128.f);   // colour is cosmetic
        pd[k] = depth[k].data(); pn[k] = normal[k].data(); pg[k] = gray[k].data();
    };
    {
        const int par = 8;                                   // views in flight
        for (int k0 = 0; k0 < n; k0 += par) {
            std::vector<std::future<void>> jobs;
            for (int k = k0; k < n && k < k0 + par; k++) jobs.push_back(std::async(std::launch::async, load, k));
            for (auto& j : jobs) j.get();
        }
    }
    for (int k = 0; k < n; k++) {
        if (!problem[k].empty()) { fprintf(stderr, "%s\n", problem[k].c_str()); return 1; }
        if (k == 0) { w = vw[0]; h = vh[0]; }
        if (vw[k] != w || vh[k] != h) { fprintf(stderr, "view %08d has a different size\n", ids[k]); return 1; }
    }
    std::vector<int32_t> off(n + 1, 0), idx;
    for (int k = 0; k < n; k++) {
        for (int s : pairs[ids[k]])
            if (slot.count(s)) idx.push_back(slot[s]);
        off[k + 1] = (int32_t)idx.size();
    }
    if (idx.empty()) idx.push_back(0);
    const int64_t cap = (int64_t)n * w * h;
    std::unique_ptr<float[]> pts(new float[(size_t)cap * 9]);   // not zero-filled: only the fused points' pages are ever touched
    int64_t cnt = 0;
    const int rc = tsar_fuse(gpu, n, w, h, cams.data(), pd.data(), pn.data(), pg.data(), TSAR_MEM_HOST, off.data(), idx.data(), &prm, pts.get(), cap, &cnt);
    if (rc != TSAR_OK) { fprintf(stderr, "tsar_fuse failed: %d\n", rc); return 1; }
    if (cnt > cap) cnt = cap;
    if (outlier.on()) {
        if (cnt > INT32_MAX) { fprintf(stderr, "--outlier_radius: more than 2^31 - 1 fused points\n"); return 1; }
        std::vector<uint8_t> keep;
        tsar_ctx* ctx = nullptr;
        if (tsar_create(gpu, &ctx) != TSAR_OK) { fprintf(stderr, "tsar_create failed\n"); return 1; }
        const bool ok = outlier_keep_mask(ctx, pts.get(), cnt, 9, outlier, keep);
        if (!ok) fprintf(stderr, "%s\n", tsar_last_error(ctx));
        tsar_destroy(ctx);
        if (!ok) return 1;
        int64_t kept = 0;                                     // the kept records in the cloud's own order, moved towards the front in place
        for (int64_t i = 0; i < cnt; i++) {
            if (!keep[(size_t)i]) continue;
            if (kept != i) memmove(pts.get() + 9 * (size_t)kept, pts.get() + 9 * (size_t)i, 9 * sizeof(float));
            kept++;
        }
        printf("--outlier_radius=%g: %lld points -> %lld points\n", (double)outlier.radius, (long long)cnt, (long long)kept);
        cnt = kept;
    }
    if (voxel > 0.0f) {
        if (cnt > INT32_MAX) { fprintf(stderr, "--voxel: more than 2^31 - 1 fused points\n"); return 1; }
        tsar_cloud_voxels_params vp;
        tsar_default_cloud_voxels_params(&vp);
        vp.voxel = voxel;
        std::vector<int32_t> rep((size_t)cnt + 1);
        int64_t n_voxels = 0;
        tsar_ctx* ctx = nullptr;
        if (tsar_create(gpu, &ctx) != TSAR_OK) { fprintf(stderr, "tsar_create failed\n"); return 1; }
        const int vrc = tsar_cloud_voxels_ctx(ctx, pts.get(), cnt, 9, &vp, nullptr, 0, nullptr, nullptr, cnt, rep.data(), nullptr, nullptr, &n_voxels, nullptr, TSAR_MEM_HOST);
        if (vrc != TSAR_OK) fprintf(stderr, "%s\n", tsar_last_error(ctx));
        tsar_destroy(ctx);
        if (vrc != TSAR_OK) return 1;
        // the representatives in the cloud's own order: ascending indices, so the records move towards the front in place
        std::sort(rep.begin(), rep.begin() + n_voxels);
        for (int64_t v = 0; v < n_voxels; v++)
            if ((int64_t)rep[(size_t)v] != v) memmove(pts.get() + 9 * (size_t)v, pts.get() + 9 * (size_t)rep[(size_t)v], 9 * sizeof(float));
        printf("--voxel=%g: %lld points -> %lld voxels\n", (double)voxel, (long long)cnt, (long long)n_voxels);
        cnt = n_voxels;
    }
    const std::string out = dir + "APD/APD_TSAR.ply";
    if (!write_cloud_ply(out, pts.get(), cnt)) { fprintf(stderr, "cannot write %s\n", out.c_str()); return 1; }
    printf("%lld points -> %s\n", (long long)cnt, out.c_str());
    return 0;
}
