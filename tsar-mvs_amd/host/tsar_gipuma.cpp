// tsar_gipuma — C++ host driver above the C ABI (include/tsar.h), keeping the reference's
// process-level contract (reference main.cpp:708-1009 flags, :1351-1376 pair.txt,
// fileIoUtils.h:111-163 cam files, :333-381 .dmb) so that the per-view shell loop
// (reference scripts/courtyard.sh:29-48) and the fuser (x/1.sh:30) keep working:
//
//   tsar_gipuma <ref.pgm> <src.pgm...> -images_folder D/images/ -mslp_folder D/ -krt_file X
//               -output_folder O --cam_scale=1 --iterations=8 --blocksize=11 --cost_comb=best_n --n_best=1
//
// writes D/APD/<id>/TSAR_disp.dmb (depth) and TSAR_normals.dmb (world normals), the two files
// Fusion reads.  Beyond the reference:
//   --all [--gpus=N]   process every reference view of pair.txt, dealt round-robin to N GPUs, one host
//                      thread + one tsar_ctx per GPU (replaces the shell loop)
//   --mode=tsar is the reference's live path (external planes + weak.png -> region RANSAC -> plane fill);
//   --mode=patchmatch  (default) random init + iterations; --mode=load starts from
//                      APD/<id>/depths_geom.dmb + normals.dmb like the reference snapshot (main.cpp:1462-1490)
//   --all --fuse       after matching, every view's depth / normal map is gathered from the GPU that produced it to GPU 0
//                      over xGMI (tsar_peer_copy) and fused there (tsar_fuse) into D/APD/APD_TSAR.ply — the fuser of
//                      x/1.sh:30 without the round trip through .dmb files (which are still written)
//   --all --geom_consistency [--geom_iterations=N (2)] [--geom_weight=W (0.2)] [--geom_clip=PX (3)]   phase 2 after every view's phase 1:
//                      each view starts from its own TSAR_disp.dmb + TSAR_normals.dmb, installs its pair.txt sources' TSAR_disp.dmb as
//                      the geometric-consistency term (include/tsar.h tsar_set_geom_depths), rescores, runs N iterations at full
//                      resolution and writes TSAR_geom_disp.dmb + TSAR_geom_normals.dmb + TSAR_geom.txt (its settings); resumed only
//                      when that record matches and no input is newer than the outputs; with --fuse the geom maps are fused
//     [--geom_multi_scale=L (0) [--geom_coarse_iterations=N (--geom_iterations)]]   phase 2 coarse to fine (ACMM): the view's own maps
//                      and the term go down L pyramid levels (tsar_pyramid_views, tsar_geom_pyramid, tsar_pyramid_planes), N iterations
//                      run at the coarsest, then each finer level merges the coarser planes into its own (tsar_upsample_merge) and runs
//                      --geom_iterations iterations; each worker keeps its coarse contexts across views; TSAR_geom.txt gains a line
//                      with the two settings when L >= 1.  L = 0: the single-scale pass above
//     [--geom_cross_view[=K (2)] [--geom_cross_view_depth_diff=REL (0.01)]]   phase 2 also takes hypotheses from its sources: their maps
//                      are rendered into the view (tsar_geom_reproject, kept where K sources agree within REL) and offered to the
//                      matcher (tsar_pm_merge_depths, in device memory), in place of the rescore at L = 0 and right after the term is
//                      installed at L >= 1; TSAR_geom.txt gains a line with the two settings only when the switch is on
//     [--geom_plane_prior=STEM [--geom_prior_weight_depth=W (0.1)] [--geom_prior_weight_normal=W (0.05)] [--geom_prior_depth_clip=REL (0.02)]
//      [--geom_prior_angle_clip=DEG (30)]]   phase 2 of a view reads APD/<id>/STEM_disp.dmb + STEM_normals.dmb (a copy of a --mode=tsar
//                      run's filled maps, say) as its plane prior (include/tsar.h tsar_set_plane_prior), installed on the full-resolution
//                      context right after the term; a view lacking either file runs without a prior and is named on stdout;
//                      TSAR_geom.txt gains a line with STEM and the four settings only when the switch is on, and a view whose prior
//                      files are newer than its outputs is recomputed
//     [--geom_build_prior[=CELL (4)] [--geom_build_prior_levels=N (0: all)]]   phase 2 builds the view's plane prior itself, on the device,
//                      right after the term is installed: rescore, the stored cost as the score, the view's own depth checked against
//                      its sources' maps (tsar_geom_check at its defaults), tsar_build_plane_prior on the kept depths with level-0
//                      cells of CELL pixels, tsar_set_plane_prior with the four --geom_prior_* settings, rescore; TSAR_geom.txt gains
//                      a line with the settings only when the switch is on.  Not together with --geom_plane_prior=STEM
//   --all --consistency_filter[=K (2)] [--filter_reproj_error=PX (2)] [--filter_depth_diff=REL (0.01)]   a last phase after the matching
//                      phases, before --fuse: each view's depth map of the phase that ran last (TSAR_geom_disp.dmb with
//                      --geom_consistency, else TSAR_disp.dmb) is checked against its pair.txt sources' maps of the same phase
//                      (include/tsar.h tsar_geom_check: the maps are installed with weight 0); a pixel is kept when at least K sources
//                      confirm it.  Writes TSAR_filtered_disp.dmb (0 where dropped), TSAR_consistent.png (8-bit gray, 255 where kept:
//                      read_reliable_mask / --check-mask= decode it to exactly the mask, so it can serve as a weak.png) and
//                      TSAR_filter.txt (the settings and the maps checked); resumed only when that record matches and no input map is
//                      newer than the outputs.  --fuse fuses what it fuses without the switch
//   --all resumes: a view whose APD/<id>/TSAR_disp.dmb and TSAR_normals.dmb are complete (the reference's header, main.cpp:1817-1860 /
//                      fileIoUtils.h:333-381, and exactly h*w*nb floats behind it) is skipped — the output files are the per-view
//                      checkpoints; --force recomputes.  A view that fails on one GPU is retried once on the next
//                      GPU's worker with a fresh context; the exit status is non-zero if any view's outputs are still missing.
//   --num_consistent= --reproj_error= --depth_diff= --angle= --used_list=   the fuser's options (x/1.sh:20-30), for --fuse
//   --seed=S, --strict, --fix-quirks, --texture-filter-8bit (TSAR_FLAG_TEX_FILTER_8BIT)
//   --multi_scale=L [--coarse_iterations=N] [--textureless_merge]   (--mode=patchmatch) coarse-to-fine: L pyramid levels
//                      (tsar_pyramid_views), init + N iterations (default --iterations) at the coarsest, then per finer level
//                      tsar_upsample_planes + --iterations iterations; --textureless_merge ends with the reference view's weak-texture
//                      regions and tsar_compute_disp_final_upsampled instead of tsar_compute_disp.  L = 0 (default): single scale.
//                      --all keeps each worker's coarse contexts across views; APD/<id>/TSAR_multiscale.txt records the settings of a
//                      multi-scale view's maps, and the resume skips a view only when that record matches the run's settings
// Images: the scene's JPEGs as they are (host/tsar_jpeg.h: libjpeg's grayscale output = what the reference's imread returns,
// main.cpp:1302; bit-identical to libjpeg-turbo, tests/test_jpeg_decode.py), or binary PGM / PPM.  A name is looked up as the same
// stem + .pgm (.ppm with -color_processing) first — a user's own conversion wins — then as the JPEG of that stem.
//   --decode-image=IN[:OUT.pgm]   no GPU: decode one image the way a run would (after -color_processing: the blue channel), print
//                                 its size and checksums, optionally write it as PGM
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <fstream>
#include <functional>
#include <future>
#include <map>
#include <math.h>
#include <memory>
#include <mutex>
#include <sstream>
#include <unistd.h>

#include <string>
#include <thread>
#include <vector>

#include "../../include/tsar.h"

// Entries that only --geom_build_prior calls are referred to weakly: the tool still links against, and runs with, a library that
// lacks them (the recording stand-in of tests/test_cli_phases_cpu.py), and refuses the switch there.
extern "C" {
void tsar_default_plane_prior_build_params(tsar_plane_prior_build_params* p) __attribute__((weak));
int tsar_build_plane_prior(tsar_ctx* ctx, const float* depth, const float* score, int mem, const tsar_plane_prior_build_params* p, float* depth_out,
                           float* normal_world_out, uint8_t* level_out) __attribute__((weak));
int tsar_get_plane(tsar_ctx* ctx, float* planes, float* cost, int32_t* beview, float* ratio, int mem) __attribute__((weak));
}

struct Options {
    std::vector<std::string> images;
    std::string images_folder, mslp_folder, krt_file, output_folder;
    int iterations = 8, blocksize = 19, n_best = 2, cost_comb = TSAR_COMB_BEST_N;   // algorithmparameters.h:21-52
    float cam_scale = 1.0f, depth_min = -1.f, depth_max = -1.f;
    bool all = false, strict = false, fix_quirks = false, color = false, display_outputs = false, fuse = false, tex8 = false, timing = false, force = false;
    tsar_fusion_params fusion{};
    int gpus = 1, workers = 1;      // --all: worker threads per GPU; each overlaps its file output with the next view's kernels
    uint64_t seed = 0;
    std::string mode = "patchmatch";
    int multi_scale = 0, coarse_iterations = -1;     // -1: --iterations
    bool coarse_iterations_set = false, textureless_merge = false;
    bool geom = false;                               // --geom_consistency: phase 2 of --all (run_geom_view)
    int geom_iterations = 2;
    int geom_multi_scale = 0, geom_coarse_iterations = -1;   // --geom_multi_scale / --geom_coarse_iterations (-1: --geom_iterations)
    bool geom_coarse_iterations_set = false;
    float geom_weight = 0.2f, geom_clip = 3.0f;      // ACMM's lambda and tau (include/tsar.h tsar_set_geom_depths)
    bool geom_cross_view = false;                    // --geom_cross_view[=K]: phase 2 takes hypotheses from its sources' maps (tsar_geom_reproject + tsar_pm_merge_depths)
    bool geom_cross_view_option_set = false;         // --geom_cross_view_depth_diff was given
    tsar_geom_reproject_params cross{};              // --geom_cross_view_depth_diff, K
    std::string geom_prior_stem;                     // --geom_plane_prior=STEM: phase 2 reads APD/<id>/STEM_disp.dmb + STEM_normals.dmb as its plane prior
    bool geom_prior = false, geom_prior_option_set = false;   // the switch was given; one of its four settings was
    tsar_plane_prior_params prior{};                 // --geom_prior_weight_depth / _weight_normal / _depth_clip; normal_clip from the angle
    double geom_prior_angle = 30.0;                  // --geom_prior_angle_clip, degrees
    bool geom_build = false;                         // --geom_build_prior[=CELL]: phase 2 builds its plane prior (tsar_build_plane_prior)
    int geom_build_cell = 0, geom_build_levels = 0;  // CELL (0: the library's default), --geom_build_prior_levels
    bool geom_build_levels_set = false;
    tsar_plane_prior_build_params build{};           // what the builder is called with
    tsar_geom_check_params build_check{};            // the check that chooses the builder's candidates: the library's defaults
    bool filter = false;                             // --consistency_filter[=K]: the last phase of --all (run_filter_view)
    bool filter_option_set = false;                  // a --filter_* switch was given
    tsar_geom_check_params check{};                  // K, --filter_reproj_error, --filter_depth_diff (include/tsar.h tsar_geom_check)
};

#include "tsar_io.h"
#include "tsar_jpeg.h"

// The result buffers (depth / normal maps out) are page-locked (tsar_host_alloc): the DMA engine then writes them directly
// instead of going through the runtime's bounce buffers (a 6048 x 4032 view's results: 9 ms instead of 30), and one set serves
// every view of a worker.  Decoded images stay BYTES on the host (round 5: tsar_set_views_u8 widens them on the device) and are
// not page-locked: each is uploaded once per GPU (DeviceImageCache).
// Falls back to ordinary memory when page-locking fails.
static bool g_pin_results = false;     // set by main() for --all
template <class T>
struct PinnedAllocator {
    typedef T value_type;
    PinnedAllocator() = default;
    template <class U> PinnedAllocator(const PinnedAllocator<U>&) {}
    // never destroyed: buffers owned by objects with static storage (the image cache) are released after main() returns
    static std::mutex& mu() { static std::mutex* m = new std::mutex; return *m; }
    static std::map<void*, bool>& pinned() { static std::map<void*, bool>* s = new std::map<void*, bool>; return *s; }
    T* allocate(size_t n) {
        // page-locked only where a buffer is reused (--all: one set per worker for every view).  One view per process: page-locking
        // 0.39 GB on a helper thread beside the kernels contends with the runtime while pm_init's code object loads (that step
        // 13 -> 81 ms) to save 5 ms of copy: pageable there (profiles/r05/cli_single_view_breakdown.txt).  TSAR_GIPUMA_PIN=0/1 overrides.
        static const char* knob = getenv("TSAR_GIPUMA_PIN");
        const bool pin = knob ? knob[0] != '0' : g_pin_results;
        void* p = pin ? tsar_host_alloc(n * sizeof(T)) : nullptr;
        const bool is_pinned = p != nullptr;
        if (!p) p = malloc(n * sizeof(T));
        if (!p) throw std::bad_alloc();
        std::lock_guard<std::mutex> lk(mu());
        pinned()[p] = is_pinned;
        return (T*)p;
    }
    void deallocate(T* p, size_t) {
        bool is_pinned = false;
        {
            std::lock_guard<std::mutex> lk(mu());
            auto it = pinned().find(p);
            if (it != pinned().end()) { is_pinned = it->second; pinned().erase(it); }
        }
        if (is_pinned) tsar_host_free(p); else free(p);
    }
    template <class U> bool operator==(const PinnedAllocator<U>&) const { return true; }
    template <class U> bool operator!=(const PinnedAllocator<U>&) const { return false; }
};
typedef std::vector<float, PinnedAllocator<float>> PinnedFloats;

typedef std::chrono::steady_clock Clock;
static double seconds_since(Clock::time_point t0) { return std::chrono::duration<double>(Clock::now() - t0).count(); }

static std::string stem8(const std::string& name) { return name.substr(0, 8); }   // main.cpp:1460
static std::string pnm_name(const std::string& name, const char* want) {
    const size_t dot = name.find_last_of('.');
    const std::string ext = dot == std::string::npos ? "" : name.substr(dot);
    return (ext == want) ? name : name.substr(0, dot) + want;
}
// A view's image: the binary PGM (PPM with -color_processing) of that name where it exists, else the JPEG of the same stem beside
// it — what the reference's scene folders hold (scripts/courtyard.sh:7,16) — decoded like the reference's imread (host/tsar_jpeg.h).
static bool file_exists(const std::string& p) { struct stat st; return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode); }
static bool is_jpeg_name(const std::string& p) {
    const size_t dot = p.find_last_of('.');
    if (dot == std::string::npos) return false;
    std::string e = p.substr(dot);
    for (char& c : e) c = (char)tolower((unsigned char)c);
    return e == ".jpg" || e == ".jpeg";
}
static std::string resolve_view_image(const std::string& path) {
    if (file_exists(path)) return path;
    const size_t dot = path.find_last_of('.');
    const std::string stem = dot == std::string::npos ? path : path.substr(0, dot);
    for (const char* ext : {".jpg", ".JPG", ".jpeg", ".JPEG"})
        if (file_exists(stem + ext)) return stem + ext;
    return path;
}
static bool read_view_image(const std::string& path, bool blue, std::vector<uint8_t>& px, int& w, int& h, std::string* why = nullptr) {
    const std::string p = resolve_view_image(path);
    if (is_jpeg_name(p)) return tsar_jpeg::read(p, blue ? tsar_jpeg::BLUE : tsar_jpeg::LUMA, px, w, h, why);
    const bool ok = blue ? read_ppm_channel(p, 2, px, w, h) : read_pgm_u8(p, px, w, h);
    if (!ok && why) *why = std::string("not a readable binary ") + (blue ? "PPM" : "PGM") + " and no JPEG of that name beside it";
    return ok;
}
static bool view_image_size(const std::string& path, int& w, int& h) {
    const std::string p = resolve_view_image(path);
    return is_jpeg_name(p) ? tsar_jpeg::size(p, w, h) : pnm_size(p, w, h);
}
static void mkdirs(const std::string& path) {
    std::string cur;
    for (size_t i = 0; i < path.size(); i++) {
        cur += path[i];
        if (path[i] == '/' || i + 1 == path.size()) mkdir(cur.c_str(), 0777);
    }
}

static void usage() {
    printf("usage: tsar_gipuma <ref image> <source images...> -images_folder DIR/ -mslp_folder DIR/ [-krt_file F] [-output_folder DIR]\n"
           "                   [--iterations=N] [--blocksize=N] [--cost_comb=all|best_n|angle|good] [--n_best=N] [--cam_scale=S]\n"
           "                   [--depth_min=D --depth_max=D] [--mode=patchmatch|load|tsar] [--all --gpus=N --workers=W] [--seed=S] [--strict] [--fix-quirks] [--texture-filter-8bit] [-color_processing] [--display_outputs] [--timing]\n"
           "                   [--multi_scale=L [--coarse_iterations=N] [--textureless_merge]]\n"
           "       tsar_gipuma --all [--gpus=N] [--force] [--fuse [--num_consistent=N --reproj_error=PX --depth_diff=REL --angle=DEG --used_list=0|1]]\n"
           "                   [--geom_consistency [--geom_iterations=N] [--geom_weight=W] [--geom_clip=PX] [--geom_multi_scale=L [--geom_coarse_iterations=N]]\n"
           "                    [--geom_cross_view[=K] [--geom_cross_view_depth_diff=REL]]\n"
           "                    [--geom_plane_prior=STEM [--geom_prior_weight_depth=W] [--geom_prior_weight_normal=W] [--geom_prior_depth_clip=REL]\n"
           "                     [--geom_prior_angle_clip=DEG]]\n"
           "                    [--geom_build_prior[=CELL] [--geom_build_prior_levels=N] [the four --geom_prior_* settings]]]\n"
           "                   [--consistency_filter[=K] [--filter_reproj_error=PX] [--filter_depth_diff=REL]]\n"
           "                   -images_folder DIR/ -mslp_folder DIR/ [options]\n"
           "       tsar_gipuma --check-mask=MASK.png | --encode-mask=DEPTH.dmb:MASK.png | --decode-image=IN[:OUT.pgm]     (no GPU)\n");
}

// the text after "--name=" when `a` is that option, else null
static const char* value_of(const char* a, const char* name) {
    const size_t n = strlen(name);
    return strncmp(a, name, n) == 0 && a[n] == '=' ? a + n + 1 : nullptr;
}
// a whole decimal integer in lo..hi into `out`; false, and `out` as it was, for anything else (empty text included)
static bool checked_int(const char* v, long lo, long hi, int& out) {
    char* end = nullptr;
    const long k = strtol(v, &end, 10);
    if (!*v || *end || k < lo || k > hi) return false;
    out = (int)k;
    return true;
}
static int parse_args(int argc, char** argv, Options& o) {   // main.cpp:708-946: same spellings, unknown options only warn
    for (int i = 1; i < argc; i++) {
        const char* a = argv[i];
        const char* v = nullptr;                              // the value of the option `opt` matched last
        auto opt = [&](const char* name) { return (v = value_of(a, name)) != nullptr; };
        auto is = [&](const char* name) { return strcmp(a, name) == 0; };
        if (a[0] != '-') o.images.push_back(a);
        else if (opt("--iterations")) o.iterations = atoi(v);
        else if (opt("--blocksize")) {
            const int k = atoi(v);
            if (k < 1 || k % 2 != 1) { printf("Command-line parameter error: The block size (--blocksize=<...>) must be a positive odd number\n"); return -1; }
            o.blocksize = k;
        } else if (opt("--n_best")) o.n_best = atoi(v);
        else if (opt("--cost_comb")) {
            if (!strcmp(v, "all")) o.cost_comb = TSAR_COMB_ALL;
            else if (!strcmp(v, "best_n")) o.cost_comb = TSAR_COMB_BEST_N;
            else if (!strcmp(v, "angle")) o.cost_comb = TSAR_COMB_ANGLE;      // main.cpp:787-790; the kernels treat both as "all" (gipuma.cu:496-499)
            else if (!strcmp(v, "good")) o.cost_comb = TSAR_COMB_GOOD;
            else { printf("Command-line parameter error: Unknown cost combination method\n\n"); usage(); return -1; }
        } else if (opt("--cam_scale")) o.cam_scale = (float)atof(v);
        else if (opt("--depth_min")) o.depth_min = (float)atof(v);
        else if (opt("--depth_max")) o.depth_max = (float)atof(v);
        else if (opt("--gpus")) o.gpus = atoi(v);
        else if (opt("--workers")) o.workers = atoi(v);
        else if (opt("--seed")) o.seed = strtoull(v, nullptr, 10);
        else if (opt("--mode")) o.mode = v;
        else if (opt("--multi_scale") || opt("--geom_multi_scale")) {
            if (!checked_int(v, 0, 8, value_of(a, "--multi_scale") ? o.multi_scale : o.geom_multi_scale)) { printf("Command-line parameter error: %s must be an integer in 0..8\n", a); return -1; }
        }
        else if (opt("--coarse_iterations") || opt("--geom_coarse_iterations")) {
            const bool geom = !value_of(a, "--coarse_iterations");
            if (!checked_int(v, 0, 1000000, geom ? o.geom_coarse_iterations : o.coarse_iterations)) { printf("Command-line parameter error: %s must be a non-negative integer\n", a); return -1; }
            (geom ? o.geom_coarse_iterations_set : o.coarse_iterations_set) = true;
        }
        else if (is("--textureless_merge")) o.textureless_merge = true;
        else if (opt("--check-mask")) {              // diagnostics, no GPU: decode a weak.png the way --mode=tsar does
            std::vector<float> scale;
            int mw = 0, mh = 0;
            if (!read_reliable_mask(v, scale, mw, mh)) { printf("cannot decode %s\n", v); return -1; }
            size_t ones = 0, wsum = 0;
            for (size_t k = 0; k < scale.size(); k++)
                if (scale[k] == 1.0f) { ones++; wsum += k % 9973; }
            printf("mask %d x %d reliable %zu checksum %zu\n", mw, mh, ones, wsum);
            return 1;
        }
        else if (opt("--encode-mask")) {             // diagnostics, no GPU: the mask of a filtered depth map (kept = depth > 0) the way --consistency_filter writes TSAR_consistent.png
            std::string in = v, out;
            const size_t colon = in.rfind(':');
            if (colon != std::string::npos) { out = in.substr(colon + 1); in = in.substr(0, colon); }
            std::vector<float> depth;
            int dh = 0, dw = 0, dnb = 0;
            if (out.empty() || !read_dmb(in, depth, dh, dw, dnb) || dnb != 1) { printf("cannot read %s as a depth map (--encode-mask=DEPTH.dmb:MASK.png)\n", in.c_str()); return -1; }
            size_t ones = 0;
            for (float& d : depth) { d = d > 0.0f ? 1.0f : 0.0f; ones += d == 1.0f; }
            if (!write_mask_png(out, depth.data(), dw, dh)) { printf("cannot write %s\n", out.c_str()); return -1; }
            printf("mask %d x %d reliable %zu -> %s\n", dw, dh, ones, out.c_str());
            return 1;
        }
        else if (opt("--decode-image")) {            // no GPU: decode an image the way a run would, --decode-image=IN[:OUT.pgm] [-color_processing first]
            std::string in = v, out;
            const size_t colon = in.rfind(':');
            if (colon != std::string::npos) { out = in.substr(colon + 1); in = in.substr(0, colon); }
            std::vector<uint8_t> px;
            int iw = 0, ih = 0;
            std::string why;
            if (!read_view_image(in, o.color, px, iw, ih, &why)) { printf("cannot decode %s: %s\n", in.c_str(), why.c_str()); return -1; }
            uint64_t sum = 0, mix = 1469598103934665603ull;
            for (uint8_t b : px) { sum += b; mix = (mix ^ b) * 1099511628211ull; }
            printf("image %d x %d sum %llu fnv1a %016llx\n", iw, ih, (unsigned long long)sum, (unsigned long long)mix);
            if (!out.empty()) {
                FILE* f = fopen(out.c_str(), "wb");
                if (!f || fprintf(f, "P5\n%d %d\n255\n", iw, ih) < 0 || fwrite(px.data(), 1, px.size(), f) != px.size()) { printf("cannot write %s\n", out.c_str()); if (f) fclose(f); return -1; }
                fclose(f);
            }
            return 1;
        }
        else if (is("--all")) o.all = true;
        else if (is("--geom_consistency")) o.geom = true;
        else if (opt("--geom_iterations")) o.geom_iterations = atoi(v);
        else if (opt("--geom_weight")) o.geom_weight = (float)atof(v);
        else if (opt("--geom_clip")) o.geom_clip = (float)atof(v);
        else if (is("--geom_cross_view")) { o.geom_cross_view = true; o.cross.min_views = 2; }
        else if (opt("--geom_cross_view")) {
            if (!checked_int(v, 1, 63, o.cross.min_views)) { printf("Command-line parameter error: --geom_cross_view=K must be an integer in 1..63\n"); return -1; }
            o.geom_cross_view = true;
        }
        else if (opt("--geom_cross_view_depth_diff")) { o.cross.depth_diff = (float)atof(v); o.geom_cross_view_option_set = true; }
        else if (opt("--geom_plane_prior")) { o.geom_prior = true; o.geom_prior_stem = v; }
        else if (opt("--geom_prior_weight_depth")) { o.prior.weight_depth = (float)atof(v); o.geom_prior_option_set = true; }
        else if (opt("--geom_prior_weight_normal")) { o.prior.weight_normal = (float)atof(v); o.geom_prior_option_set = true; }
        else if (opt("--geom_prior_depth_clip")) { o.prior.depth_clip = (float)atof(v); o.geom_prior_option_set = true; }
        else if (opt("--geom_prior_angle_clip")) { o.geom_prior_angle = atof(v); o.geom_prior_option_set = true; }
        else if (is("--geom_build_prior")) o.geom_build = true;
        else if (opt("--geom_build_prior")) {
            if (!checked_int(v, 2, 256, o.geom_build_cell)) { printf("Command-line parameter error: --geom_build_prior=CELL must be an integer in 2..256\n"); return -1; }
            o.geom_build = true;
        }
        else if (opt("--geom_build_prior_levels")) {
            if (!checked_int(v, 0, TSAR_PLANE_PRIOR_MAX_LEVELS, o.geom_build_levels)) { printf("Command-line parameter error: --geom_build_prior_levels=N must be an integer in 0..16\n"); return -1; }
            o.geom_build_levels_set = true;
        }
        else if (is("--consistency_filter")) o.filter = true;
        else if (opt("--consistency_filter")) {
            if (!checked_int(v, 1, 31, o.check.min_consistent)) { printf("Command-line parameter error: --consistency_filter=K must be an integer in 1..31\n"); return -1; }
            o.filter = true;
        }
        else if (opt("--filter_reproj_error")) { o.check.reproj_error = (float)atof(v); o.filter_option_set = true; }
        else if (opt("--filter_depth_diff")) { o.check.depth_diff = (float)atof(v); o.filter_option_set = true; }
        else if (is("--fuse")) o.fuse = true;
        else if (is("--force")) o.force = true;                                // --all: recompute views whose outputs are already there
        else if (opt("--num_consistent")) o.fusion.num_consistent = atoi(v);
        else if (opt("--reproj_error")) o.fusion.reproj_error = (float)atof(v);
        else if (opt("--depth_diff")) o.fusion.depth_diff = (float)atof(v);
        else if (opt("--angle")) o.fusion.angle_deg = (float)atof(v);
        else if (opt("--used_list")) o.fusion.used_list = atoi(v);
        else if (is("--strict")) o.strict = true;
        else if (is("--fix-quirks")) o.fix_quirks = true;
        else if (is("--texture-filter-8bit")) o.tex8 = true;              // bilinear weights with 8 fractional bits, like the CUDA texture unit
        else if (is("-images_folder") && i + 1 < argc) o.images_folder = argv[++i];
        else if (is("-mslp_folder") && i + 1 < argc) o.mslp_folder = argv[++i];
        else if (is("-krt_file") && i + 1 < argc) o.krt_file = argv[++i];
        else if (is("-output_folder") && i + 1 < argc) o.output_folder = argv[++i];
        else if (is("-color_processing")) o.color = true;              // main.cpp:727,909
        else if (is("--timing")) o.timing = true;                             // wall time of each host-side step of a view, on stdout
        else if (is("--display_outputs")) o.display_outputs = true;           // TSAR_normals.png + TSAR_model.ply (main.cpp:1800-1838)
        else if (is("-no_display") || opt("--cost_gamma") || opt("--min_angle") || opt("--max_angle") || opt("--cost_tau_color") ||
                 opt("--cost_tau_gradient") || opt("--cost_alpha") || opt("--max_views") || opt("--num_img_processed")) {
            // accepted for script compatibility; these feed cost functions / view selection the GPU path does not use
        } else if (is("-h") || is("--help")) { usage(); return 1; }
        else printf("Command-line parameter warning: unknown option %s\n", a);
    }
    return 0;
}

// Decoded images shared by all views of a run (--all visits every image as a reference once and as a source ~N times).
struct ImageCache {
    struct Entry { std::vector<uint8_t> gray; int w = 0, h = 0; bool ok = false; std::string why; };      // the 8-bit decode as it is: widened to float on the device (tsar_set_views_u8)
    std::mutex mu;
    std::map<std::string, std::shared_ptr<Entry>> items;
    std::shared_ptr<Entry> get(const std::string& path) {
        {
            std::lock_guard<std::mutex> lk(mu);
            auto it = items.find(path);
            if (it != items.end()) return it->second;
        }
        auto e = std::make_shared<Entry>();                       // decode outside the lock; a rare double decode is harmless
        const bool ppm = path.size() > 4 && path.compare(path.size() - 4, 4, ".ppm") == 0;
        e->ok = read_view_image(path, ppm, e->gray, e->w, e->h, &e->why);   // the PGM / PPM of that name, else the JPEG beside it (colour: blue, see tsar_io.h)
        std::lock_guard<std::mutex> lk(mu);
        auto ins = items.emplace(path, e);
        return ins.first->second;
    }
};
static ImageCache g_images;

// --all: every GPU keeps every image of the scene it has used resident (44 x 97.5 MB = 4.3 GB at ETH3D size, of
// 288 GB), uploaded once; a view then hands device pointers to tsar_set_views instead of pushing its 1 + N images over PCIe
// again (a scene's images are each the reference once and a source ~N times).
struct DeviceImageCache {
    std::mutex mu;
    std::map<std::pair<int, std::string>, uint8_t*> items;      // (device, path) -> device copy (bytes)
    const uint8_t* get(int device, const std::string& path, const ImageCache::Entry& host) {
        std::lock_guard<std::mutex> lk(mu);                       // uploads are rare (once per image and device): serialised
        auto it = items.find({device, path});
        if (it != items.end()) return it->second;
        const size_t bytes = (size_t)host.w * host.h;
        uint8_t* d = (uint8_t*)tsar_device_alloc(device, bytes);
        if (!d) return nullptr;
        if (tsar_device_write(device, d, host.gray.data(), bytes) != TSAR_OK) { tsar_device_free(device, d); return nullptr; }
        items[{device, path}] = d;
        return d;
    }
    void release() {
        std::lock_guard<std::mutex> lk(mu);
        for (auto& kv : items) tsar_device_free(kv.first.first, kv.second);
        items.clear();
    }
};
static DeviceImageCache g_device_images;

// --fuse: what a matched view leaves on its GPU for the gather (device memory, owned by the run)
struct DeviceResult {
    int device = -1, w = 0, h = 0;
    float *depth = nullptr, *normal = nullptr;
};
static void release(DeviceResult& r) {
    if (r.depth) tsar_device_free(r.device, r.depth);
    if (r.normal) tsar_device_free(r.device, r.normal);
    r = DeviceResult{};
}

// What the refinement modes read per view besides the reference image: the external depth / normal maps and (--mode=tsar)
// weak.png.  Loaded by helper threads; in --all runs a worker keeps a ring of these, page-locked, and starts loading the next views'
// while view k is on the GPU (inflating a full-size weak.png alone takes longer than the view's kernels).
struct ExternalInputs {
    bool pinned = false;                       // --all: buffers reused by every view of the worker, worth page-locking
    PinnedFloats pdepth, pnormal;
    std::vector<float> vdepth, vnormal, scale;
    int dh = 0, dw = 0, dnb = 0, nh = 0, nw = 0, nnb = 0, mw = 0, mh = 0;
    bool depth_ok = false, normal_ok = false, mask_ok = false, started = false;
    std::string dir;
    std::future<void> maps, mask;
    const float* depth() const { return pinned ? pdepth.data() : vdepth.data(); }
    const float* normal() const { return pinned ? pnormal.data() : vnormal.data(); }
    void start(const std::string& view_dir, bool want_mask, const std::string& ref_image_path);
};
void ExternalInputs::start(const std::string& view_dir, bool want_mask, const std::string& ref_image_path) {
    dir = view_dir;
    started = true;
    depth_ok = normal_ok = mask_ok = false;
    maps = std::async(std::launch::async, [this, ref_image_path]() {
        auto read_maps = [this](auto& depth, auto& normal) {
            depth_ok = read_dmb(dir + "depths_geom.dmb", depth, dh, dw, dnb);
            normal_ok = read_dmb(dir + "normals.dmb", normal, nh, nw, nnb);
        };
        if (pinned) read_maps(pdepth, pnormal); else read_maps(vdepth, vnormal);
        if (!ref_image_path.empty()) g_images.get(ref_image_path);      // a prefetch: decoded into the cache for the view's own start
    });
    if (want_mask) mask = std::async(std::launch::async, [this]() { mask_ok = read_reliable_mask(dir + "weak.png", scale, mw, mh); });
}

// one view's result maps on the host and where they go; a worker's sets are allocated once and reused for every view it processes
// (page-locking 390 MB per view would cost more than the copy it speeds up)
struct HostResult {
    PinnedFloats depth, normal;
    std::string out_dir;        // where the view's .dmb files go
    int w = 0, h = 0;
};

// Fault injection for the re-queue path (tests): TSAR_GIPUMA_INJECT_FAILURE=<view id>[:<times>] makes the first <times> (default 1)
// attempts at that view fail after its context exists, the way a device-side error would (the context is dropped).
static int g_inject_view = -1;
static std::atomic<int> g_inject_left{0};
static void read_injection() {
    const char* e = getenv("TSAR_GIPUMA_INJECT_FAILURE");
    if (!e || !*e) return;
    g_inject_view = atoi(e);
    const char* c = strchr(e, ':');
    g_inject_left = c ? atoi(c + 1) : 1;
}

static std::string id8(int id) { char b[32]; snprintf(b, sizeof b, "%08d", id); return b; }
static std::string view_dir_of(const Options& o, int ref) { return o.mslp_folder + "APD/" + id8(ref) + "/"; }
static std::string image_path(const Options& o, const std::string& name) { return o.images_folder + pnm_name(name, o.color ? ".ppm" : ".pgm"); }
static std::string view_image_of(const Options& o, int ref) { return image_path(o, id8(ref) + ".pgm"); }
static std::string cam_path(const Options& o, const std::string& name) { return o.mslp_folder + "cams/" + stem8(name) + "_cam.txt"; }
// --all: the image names of a reference view and its pair.txt sources, as the per-view command line gives them
static std::vector<std::string> names_of(int ref, const std::vector<int>& srcs) {
    std::vector<std::string> names = {id8(ref) + ".pgm"};
    for (int s : srcs) names.push_back(id8(s) + ".pgm");
    return names;
}

// ---- settings records: what each phase leaves in APD/<id>/ and when --all takes it as done ------------------------------------
// A phase's two output files, with the channel count of each that is a .dmb map (0: not a map, only its presence counts), and the
// record of the settings they were made with.  For a matching phase the two are its depth and normal maps.
struct PhaseFiles {
    const char* out[2];
    int channels[2];
    const char* record;
    const char* depth() const { return out[0]; }
    const char* normal() const { return out[1]; }
};
static const PhaseFiles PHASE1_FILES = {{"TSAR_disp.dmb", "TSAR_normals.dmb"}, {1, 3}, "TSAR_multiscale.txt"};
static const PhaseFiles GEOM_FILES = {{"TSAR_geom_disp.dmb", "TSAR_geom_normals.dmb"}, {1, 3}, "TSAR_geom.txt"};
static const PhaseFiles FILTER_FILES = {{"TSAR_filtered_disp.dmb", "TSAR_consistent.png"}, {1, 0}, "TSAR_filter.txt"};
// what a multi-scale view records beside its maps (empty for a single-scale run, which leaves no record)
static std::string ms_record_of(const Options& o) {
    if (o.multi_scale == 0) return "";
    char b[128];
    snprintf(b, sizeof b, "multi_scale=%d coarse_iterations=%d textureless_merge=%d\n", o.multi_scale,
             o.coarse_iterations_set ? o.coarse_iterations : o.iterations, o.textureless_merge ? 1 : 0);
    return b;
}
static int geom_coarse_iterations_of(const Options& o) { return o.geom_coarse_iterations_set ? o.geom_coarse_iterations : o.geom_iterations; }
static std::string prior_file_of(const Options& o, int ref, const char* what) { return view_dir_of(o, ref) + o.geom_prior_stem + what; }
static std::string geom_record_of(const Options& o, const std::vector<int>&) {
    char b[640];
    snprintf(b, sizeof b, "geom_iterations=%d geom_weight=%.9g geom_clip=%.9g blocksize=%d n_best=%d cost_comb=%d seed=%llu strict=%d fix_quirks=%d texture_filter_8bit=%d cam_scale=%.9g depth_min=%.9g depth_max=%.9g\n",
             o.geom_iterations, (double)o.geom_weight, (double)o.geom_clip, o.blocksize, o.n_best, o.cost_comb, (unsigned long long)o.seed, o.strict ? 1 : 0,
             o.fix_quirks ? 1 : 0, o.tex8 ? 1 : 0, (double)o.cam_scale, (double)o.depth_min, (double)o.depth_max);
    std::string rec = b;
    if (o.geom_cross_view) {          // (a record without the switch is byte for byte what it was before the switch existed)
        snprintf(b, sizeof b, "geom_cross_view=%d geom_cross_view_depth_diff=%.9g\n", o.cross.min_views, (double)o.cross.depth_diff);
        rec += b;
    }
    if (o.geom_prior) {
        snprintf(b, sizeof b, "geom_plane_prior=%s geom_prior_weight_depth=%.9g geom_prior_weight_normal=%.9g geom_prior_depth_clip=%.9g geom_prior_angle_clip=%.9g\n",
                 o.geom_prior_stem.c_str(), (double)o.prior.weight_depth, (double)o.prior.weight_normal, (double)o.prior.depth_clip, o.geom_prior_angle);
        rec += b;
    }
    if (o.geom_build) {
        snprintf(b, sizeof b, "geom_build_prior=%d geom_build_prior_levels=%d geom_build_min_consistent=%d geom_build_reproj_error=%.9g geom_build_depth_diff=%.9g "
                 "geom_prior_weight_depth=%.9g geom_prior_weight_normal=%.9g geom_prior_depth_clip=%.9g geom_prior_angle_clip=%.9g\n",
                 o.build.cell, o.build.max_levels, o.build_check.min_consistent, (double)o.build_check.reproj_error, (double)o.build_check.depth_diff,
                 (double)o.prior.weight_depth, (double)o.prior.weight_normal, (double)o.prior.depth_clip, o.geom_prior_angle);
        rec += b;
    }
    if (o.geom_multi_scale > 0) {     // (an L = 0 record is the single-scale one, byte for byte)
        snprintf(b, sizeof b, "geom_multi_scale=%d geom_coarse_iterations=%d\n", o.geom_multi_scale, geom_coarse_iterations_of(o));
        rec += b;
    }
    return rec;
}
// the filter phase: the maps it checks are those of the matching phase that ran last
static const PhaseFiles& filter_input_files(const Options& o) { return o.geom ? GEOM_FILES : PHASE1_FILES; }
static std::string filter_record_of(const Options& o, const std::vector<int>& srcs) {
    char b[256];
    snprintf(b, sizeof b, "min_consistent=%d reproj_error=%.9g depth_diff=%.9g cam_scale=%.9g checked=%s sources=", o.check.min_consistent,
             (double)o.check.reproj_error, (double)o.check.depth_diff, (double)o.cam_scale, filter_input_files(o).depth());
    std::string rec = b;
    for (size_t i = 0; i < srcs.size(); i++) rec += (i ? "," : "") + id8(srcs[i]);
    return rec + "\n";
}
static std::string read_text_file(const std::string& path) {          // (no file reads as empty)
    std::stringstream txt;
    txt << std::ifstream(path).rdbuf();
    return txt.str();
}
// a phase's maps complete for the size of the view's reference image, and a record that reads exactly `record` (no file reads as
// empty): the done marker of a phase-1 view, whose record is this run's multi-scale settings
static bool outputs_recorded(const Options& o, int ref, const PhaseFiles& f, const std::string& record) {
    int w = 0, h = 0;
    if (!view_image_size(view_image_of(o, ref), w, h)) return false;
    const std::string d = view_dir_of(o, ref);
    for (int i = 0; i < 2; i++)
        if (f.channels[i] && !dmb_complete(d + f.out[i], h, w, f.channels[i])) return false;
    return read_text_file(d + f.record) == record;
}
// Outputs under their record: the record goes first and comes back last, so outputs that are being replaced never carry the record
// of other settings.  `write_outputs` writes the files; an empty record: none is written.
static bool write_under_record(const std::string& dir, const PhaseFiles& f, const std::string& record, const std::function<bool()>& write_outputs) {
    unlink((dir + f.record).c_str());
    bool ok = write_outputs();
    if (ok && !record.empty()) {
        FILE* fp = fopen((dir + f.record).c_str(), "w");
        ok = fp && fputs(record.c_str(), fp) >= 0;
        if (fp && fclose(fp) != 0) ok = false;
    }
    return ok;
}
// a matching phase's two maps, side by side (a write is a copy into the page cache)
static bool write_maps(const HostResult& r, const PhaseFiles& f, const std::string& record) {
    return write_under_record(r.out_dir, f, record, [&r, &f]() {
        auto normals = std::async(std::launch::async, [&r, &f]() { return write_dmb(r.out_dir + f.normal(), r.normal.data(), r.h, r.w, 3); });
        const bool depth_ok = write_dmb(r.out_dir + f.depth(), r.depth.data(), r.h, r.w, 1);
        return normals.get() && depth_ok;
    });
}
static bool mtime_of(const std::string& path, struct timespec& t) {
    struct stat st;
    if (stat(path.c_str(), &st) != 0) return false;
    t = st.st_mtim;
    return true;
}
static bool newer(const struct timespec& a, const struct timespec& b) { return a.tv_sec != b.tv_sec ? a.tv_sec > b.tv_sec : a.tv_nsec > b.tv_nsec; }

// The GPU state of one pool thread of --all (or of a one-view process), kept across its views: its context and, coarse to fine, the
// contexts of the coarser levels (device planes are allocated once); two page-locked result sets its views alternate between (the
// .dmb files of view k are written by a helper thread while the kernels of view k+1 run: file output is ~0.1 s of a 0.5 s view at
// ETH3D size); and phase 1's ring of external inputs read ahead.
struct Worker {
    const int device;
    const char* const phase;           // null: phase 1; "geom" / "filter": the later phases, whose messages say so
    const bool resident;               // --all: images stay resident on the device across views (a one-view process would only hold every image twice)
    tsar_ctx* ctx = nullptr;
    std::vector<tsar_ctx*> coarse;     // the coarser levels, finest first (level(1) = coarse[0])
    HostResult result[2];
    std::future<void> writing[2];      // after `result`: a pending write is joined before its set is released
    std::vector<ExternalInputs> ring;
    Worker(int device, const char* phase, bool resident) : device(device), phase(phase), resident(resident) {}
    ~Worker() { drop(); }
    tsar_ctx* level(int k) const { return k ? coarse[k - 1] : ctx; }     // 0: full resolution
    int create_failed(int rc) const {
        if (phase) fprintf(stderr, "tsar_create(device %d) failed\n", device);
        else fprintf(stderr, "tsar_create(device %d) failed: %d\n", device, rc);
        return rc;
    }
    int ensure(int L) {                // levels 1..L, created on first use
        while ((int)coarse.size() < L) {
            tsar_ctx* c = nullptr;
            const int rc = tsar_create(device, &c);
            if (rc != TSAR_OK) return create_failed(rc);
            coarse.push_back(c);
        }
        return TSAR_OK;
    }
    void drop() {                      // after a failed view: the next one starts from fresh contexts
        for (tsar_ctx* c : coarse) tsar_destroy(c);
        coarse.clear();
        tsar_destroy(ctx);
        ctx = nullptr;
    }
    int fail(int ref, const char* what, tsar_ctx* c = nullptr) const {   // a library call of view `ref` failed on c (default: ctx)
        const char* err = tsar_last_error(c ? c : ctx);
        if (phase) fprintf(stderr, "view %08d (%s): %s: %s\n", ref, phase, what, err);
        else fprintf(stderr, "%s: %s\n", what, err);
        return -1;
    }
};

// The pyramid ladder over a worker's chain of contexts, for phase 1's --multi_scale and phase 2's --geom_multi_scale: they differ in the
// call made per level, named in the failure message.  Down: level by level from the full resolution, each of `calls` as fn(level k,
// level k - 1).  0, or non-zero after the message.
struct LevelCall { int (*fn)(tsar_ctx* to, const tsar_ctx* from); const char* name; };
static int descend(const Worker& wk, int ref, int L, std::initializer_list<LevelCall> calls) {
    for (int k = 1; k <= L; k++)
        for (const LevelCall& c : calls)
            if (c.fn(wk.level(k), wk.level(k - 1)) != TSAR_OK) return wk.fail(ref, c.name, wk.level(k));
    return 0;
}
// up: coarse_iters iterations at the coarsest level, then per finer level up.fn(level k, level k + 1) and iters iterations
static int climb(const Worker& wk, int ref, int L, int coarse_iters, int iters, LevelCall up) {
    if (tsar_pm_iterate(wk.level(L), coarse_iters) != TSAR_OK) return wk.fail(ref, "tsar_pm_iterate (coarsest level)", wk.level(L));
    for (int k = L - 1; k >= 0; k--) {
        if (up.fn(wk.level(k), wk.level(k + 1)) != TSAR_OK) return wk.fail(ref, up.name, wk.level(k));
        if (tsar_pm_iterate(wk.level(k), iters) != TSAR_OK) return wk.fail(ref, "tsar_pm_iterate", wk.level(k));
    }
    return 0;
}

// A view's images and cameras as tsar_set_views_u8 takes them (the reference first), and the depth range it is matched in
struct ViewSet {
    std::vector<std::shared_ptr<ImageCache::Entry>> gray;
    std::vector<const uint8_t*> px;    // the resident device copies where the worker keeps them, else the host bytes
    int mem = TSAR_MEM_HOST;
    std::vector<tsar_camera> cams;
    int w = 0, h = 0;
    float dmin = 0.f, dmax = 0.f;
    double ms_create = 0.0, ms_decode = 0.0;   // --timing: the two concurrent legs of the start-up, each on its own clock
};
// Everything a view needs before its first kernel, side by side: the worker's context if it has none yet (~0.2 s in a fresh process)
// and the decode of the named images (~45 ms each at ETH3D size, kept in g_images).  Then their sizes are checked, their cameras read
// and the depth range taken from the reference camera (fileIoUtils.h:150-153) unless the command line gave it.  0, or non-zero after
// a message.
static int load_views(const Options& o, Worker& wk, const std::vector<std::string>& names, ViewSet& v) {
    const auto t0 = Clock::now();
    std::future<int> creating;
    if (!wk.ctx) creating = std::async(std::launch::async, [&wk, &v]() {
        const auto c0 = Clock::now();
        const int rc = tsar_create(wk.device, &wk.ctx);
        v.ms_create = 1e3 * seconds_since(c0);
        return rc;
    });
    std::vector<std::future<std::shared_ptr<ImageCache::Entry>>> decoding;
    for (const std::string& name : names)
        decoding.push_back(std::async(std::launch::async, [&o, &name]() { return g_images.get(image_path(o, name)); }));
    for (auto& d : decoding) v.gray.push_back(d.get());
    v.ms_decode = 1e3 * seconds_since(t0);
    const int create_rc = creating.valid() ? creating.get() : TSAR_OK;
    if (create_rc != TSAR_OK) return wk.create_failed(create_rc);
    std::vector<const uint8_t*> host, dev;
    v.dmin = o.depth_min;
    v.dmax = o.depth_max;
    for (size_t i = 0; i < names.size(); i++) {
        const ImageCache::Entry& e = *v.gray[i];
        const std::string ip = image_path(o, names[i]);
        if (!e.ok) { fprintf(stderr, "cannot read image %s: %s\n", ip.c_str(), e.why.c_str()); return -1; }
        if (i == 0) { v.w = e.w; v.h = e.h; }
        if (e.w != v.w || e.h != v.h) { fprintf(stderr, "image %s has a different size\n", ip.c_str()); return -1; }
        host.push_back(e.gray.data());
        if (wk.resident)               // uploaded once per GPU (falls back to the host bytes)
            if (const uint8_t* d = g_device_images.get(wk.device, ip, e)) dev.push_back(d);
        CamFile cf;
        const std::string cp = cam_path(o, names[i]);
        if (!read_cam(cp, cf)) { fprintf(stderr, "cannot read camera %s\n", cp.c_str()); return -1; }
        v.cams.push_back(cf.cam);
        if (i == 0) {
            if (v.dmin <= 0) v.dmin = cf.depth_min;
            if (v.dmax <= 0) v.dmax = cf.depth_max;
        }
    }
    const bool on_device = dev.size() == names.size();
    v.px = on_device ? dev : host;
    v.mem = on_device ? TSAR_MEM_DEVICE : TSAR_MEM_HOST;
    return 0;
}

// --display_outputs: what the reference always writes beside the maps; here on request (a full-size view's PLY is 0.66 GB)
static bool write_display_outputs(const HostResult& r, const std::vector<uint8_t>& ref_image, const tsar_camera& cam) {
    const size_t np = (size_t)r.w * r.h;
    std::vector<uint16_t> vis(3 * np);
    for (size_t k = 0; k < 3 * np; k++) {
        const float v = r.normal[k] * 32767.f + 32767.f;               // convertTo(CV_16U, 32767, 32767): saturate + round
        vis[k] = (uint16_t)(v <= 0.f ? 0 : v >= 65535.f ? 65535 : (int)lrintf(v));
    }
    if (!write_png_rgb16(r.out_dir + "TSAR_normals.png", vis.data(), r.w, r.h)) return false;
    const std::vector<float> ref_gray(ref_image.begin(), ref_image.end());
    return write_view_ply(r.out_dir + "TSAR_model.ply", r.depth.data(), r.normal.data(), ref_gray.data(), r.w, r.h, cam);
}

static tsar_params params_of(const Options& o, int ref_id, float dmin, float dmax) {
    tsar_params p;
    tsar_default_params(&p);
    p.box_hsize = p.box_vsize = o.blocksize;
    p.n_best = o.n_best; p.cost_comb = o.cost_comb; p.cam_scale = o.cam_scale;
    p.depth_min = dmin; p.depth_max = dmax;
    p.seed = o.seed + (uint64_t)ref_id;
    p.flags = (o.strict ? TSAR_FLAG_STRICT_DIV : 0) | (o.fix_quirks ? (TSAR_FLAG_FIX_DOWN_FAR_SEED | TSAR_FLAG_FIX_RIGHT_FAR_CMP) : 0) |
              (o.tex8 ? TSAR_FLAG_TEX_FILTER_8BIT : 0);
    return p;
}

// Phase 1 of one reference view on the worker's GPU: names[0] is the reference, the rest the candidate sources in argv order.  The
// maps land in hr and, unless the caller defers that (--all writes them while the next view is matched), in their files.
static int run_view(const Options& o, Worker& wk, const std::vector<std::string>& names, const std::vector<int>& subset_slots, int ref_id, double* seconds,
                    HostResult& hr, DeviceResult* keep = nullptr, bool defer_write = false, ExternalInputs* preloaded = nullptr) {
    const auto t0 = Clock::now();
    auto t_last = t0;
    std::string steps;                                            // --timing: "step ms | step ms | ..."
    auto stamp = [&](const char* what) {
        if (!o.timing) return;
        char buf[96];
        snprintf(buf, sizeof buf, "%s%s %.1f", steps.empty() ? "" : " | ", what, 1e3 * seconds_since(t_last));
        steps += buf;
        t_last = Clock::now();
    };
    // The refinement modes never read a source image (load_planes, weak-texture detection, region RANSAC and fill work on the
    // reference view and the plane maps): only the reference image is decoded and handed to the library there.
    const bool tsar_mode = o.mode == "tsar", external = o.mode == "load" || tsar_mode;
    const int n = external ? 1 : (int)names.size();
    const std::string out_dir = o.mslp_folder + "APD/" + stem8(names[0]) + "/";   // main.cpp:1462, 1813-1830
    // the external maps and weak.png (inflating a full-size PNG takes ~0.3 s) load beside the context and the images
    ExternalInputs own_inputs;
    ExternalInputs& ext = (preloaded && preloaded->started && preloaded->dir == out_dir) ? *preloaded : own_inputs;   // --all: started a view ago
    if (external && !ext.started) ext.start(out_dir, tsar_mode, "");
    struct Consumed { ExternalInputs& e; ~Consumed() { if (e.maps.valid()) e.maps.get(); if (e.mask.valid()) e.mask.get(); e.started = false; } } consumed{ext};
    ViewSet v;
    if (const int rc = load_views(o, wk, std::vector<std::string>(names.begin(), names.begin() + n), v)) return rc;
    // (the map / mask readers are joined where their data is needed — set_views and load_planes run while weak.png is still
    // inflating — or by `consumed` on an early return)
    tsar_ctx* const ctx = wk.ctx;
    const int w = v.w, h = v.h;
    auto fail = [&](const char* what, tsar_ctx* c = nullptr) { return wk.fail(ref_id, what, c); };
    const tsar_params p = params_of(o, ref_id, v.dmin, v.dmax);
    if (tsar_set_params(ctx, &p) != TSAR_OK) return fail("tsar_set_params");
    if (ref_id == g_inject_view && g_inject_left.fetch_sub(1) > 0) {
        fprintf(stderr, "view %08d on gpu %d: injected failure (TSAR_GIPUMA_INJECT_FAILURE)\n", ref_id, wk.device);
        return -1;
    }
    if (o.timing) { tsar_enable_kernel_timing(ctx, 1); tsar_reset_kernel_timing(ctx); }
    stamp(external ? "context + reference image (external maps and weak.png still loading)" : "context + images + cameras (concurrent)");
    if (o.timing) {
        char buf[96];
        snprintf(buf, sizeof buf, " [tsar_create %.1f beside decode of %d images %.1f]", v.ms_create, n, v.ms_decode);
        steps += buf;
    }
    if (tsar_set_views_u8(ctx, n, w, h, v.px.data(), v.mem, v.cams.data()) != TSAR_OK) return fail("tsar_set_views_u8");
    if (!subset_slots.empty() && !external) {
        std::vector<int32_t> s(subset_slots.begin(), subset_slots.end());
        if (tsar_set_view_subset(ctx, (int)s.size(), s.data()) != TSAR_OK) return fail("tsar_set_view_subset");
    }
    stamp("set_views");
    // (One view per process: releasing the decoded images — 1.07 GB of host memory at ETH3D size — here, on a helper thread beside the
    // kernels, instead of leaving them to the exit path was measured and removed: the caller waits ~40 ms per GB the process still
    // holds when main() leaves, but the munmap contends with the runtime's own mappings while pm_init's code object loads, 65 -> 200 ms
    // for that step, and the invocation got slower, 1239 -> 1323 ms median: profiles/r05/cli_single_view_breakdown.txt.)
    mkdirs(out_dir);
    const size_t np = (size_t)w * h;
    // sizing (and, in --all, page-locking once per worker) of the result buffers happens beside the kernels
    std::future<void> sizing;
    if (hr.depth.size() != np) sizing = std::async(std::launch::async, [&hr, np]() { hr.depth.resize(np); hr.normal.resize(3 * np); });
    struct JoinSizing { std::future<void>& f; ~JoinSizing() { if (f.valid()) f.get(); } } join_sizing{sizing};   // on every return path
    if (external) {
        if (ext.maps.valid()) ext.maps.get();
        if (!ext.depth_ok || ext.dh != h || ext.dw != w || ext.dnb != 1) { fprintf(stderr, "cannot read %sdepths_geom.dmb\n", out_dir.c_str()); return -1; }
        if (!ext.normal_ok || ext.nh != h || ext.nw != w || ext.nnb != 3) { fprintf(stderr, "cannot read %snormals.dmb\n", out_dir.c_str()); return -1; }
        if (tsar_load_planes(ctx, ext.depth(), ext.normal(), TSAR_MEM_HOST) != TSAR_OK) return fail("tsar_load_planes");
        stamp("load_planes");
    } else if (o.multi_scale > 0) {
        // coarse to fine (api.run_multiscale): the pyramid below ctx, init + coarse iterations at the coarsest level, upsample +
        // iterations at each finer one
        const int L = o.multi_scale;
        if (wk.ensure(L) != TSAR_OK) return -1;
        if (descend(wk, ref_id, L, {{tsar_pyramid_views, "tsar_pyramid_views"}})) return -1;
        stamp("pyramid_views");
        if (tsar_pm_init(wk.level(L)) != TSAR_OK) return fail("tsar_pm_init (coarsest level)", wk.level(L));
        if (climb(wk, ref_id, L, o.coarse_iterations_set ? o.coarse_iterations : o.iterations, o.iterations, {tsar_upsample_planes, "tsar_upsample_planes"})) return -1;
        stamp("coarse-to-fine pm_init + pm_iterate");
    } else {
        if (tsar_pm_init(ctx) != TSAR_OK) return fail("tsar_pm_init");
        if (o.timing) { tsar_synchronize(ctx); stamp("pm_init (first launch of its code object)"); }
        if (tsar_pm_iterate(ctx, o.iterations) != TSAR_OK) return fail("tsar_pm_iterate");
        stamp(o.timing ? "pm_iterate" : "pm_init + pm_iterate");
    }
    if (tsar_mode) {
        // the reference's live path, runGipuma main.cpp:1493-1783: external planes (above: firstcuda) -> reliability mask
        // from weak.png -> weak-texture regions of the reference image (texture(), main.cpp:214-596) -> sliccuda
        // (gipuma_getview) -> per-region plane RANSAC (:1520-1730) -> fakecuda -> fillcuda
        if (ext.mask.valid()) ext.mask.get();
        stamp("weak.png (rest of its inflate)");
        if (!ext.mask_ok || ext.mw != w || ext.mh != h) { fprintf(stderr, "cannot read %sweak.png (8-bit PNG of the image size)\n", out_dir.c_str()); return -1; }
        if (tsar_set_reliable_mask(ctx, ext.scale.data(), TSAR_MEM_HOST) != TSAR_OK) return fail("tsar_set_reliable_mask");
        stamp("set_reliable_mask");
        int n_regions = 0;
        if (tsar_detect_weak_texture(ctx, nullptr, TSAR_MEM_HOST, &n_regions, nullptr, nullptr, 0) != TSAR_OK) return fail("tsar_detect_weak_texture");
        stamp("detect_weak_texture");
        if (tsar_getview(ctx) != TSAR_OK) return fail("tsar_getview");
        std::vector<float> planes((size_t)4 * (n_regions > 0 ? n_regions : 1)), ratio((size_t)(n_regions > 0 ? n_regions : 1));
        if (tsar_ransac_regions(ctx, planes.data(), ratio.data()) != TSAR_OK) return fail("tsar_ransac_regions");
        stamp("getview + ransac_regions");
        if (tsar_fake_depth(ctx, nullptr, TSAR_MEM_HOST) != TSAR_OK) return fail("tsar_fake_depth");
        if (tsar_fill_textureless(ctx) != TSAR_OK) return fail("tsar_fill_textureless");
        stamp("fake_depth + fill_textureless");
        printf("view %08d: %d regions labelled, textureless ones refitted and filled\n", ref_id, n_regions);
    } else if (o.textureless_merge) {
        // TSAR's multi-scale merge (gipuma_compute_disp_final): lines->text = the region text of each pixel's weak-texture label
        std::vector<int32_t> labels(np);
        std::vector<float> region_text(np), text(np);
        int n_regions = 0;
        if (tsar_detect_weak_texture(ctx, labels.data(), TSAR_MEM_HOST, &n_regions, region_text.data(), nullptr, (int)np) != TSAR_OK) return fail("tsar_detect_weak_texture");
        for (size_t p = 0; p < np; p++) text[p] = region_text[labels[p]];
        if (tsar_compute_disp_final_upsampled(ctx, text.data(), TSAR_MEM_HOST) != TSAR_OK) return fail("tsar_compute_disp_final_upsampled");
        stamp("detect_weak_texture + compute_disp_final_upsampled");
    } else if (tsar_compute_disp(ctx) != TSAR_OK) return fail("tsar_compute_disp");
    if (sizing.valid()) sizing.get();
    if (tsar_get_result(ctx, hr.depth.data(), hr.normal.data(), nullptr, nullptr, TSAR_MEM_HOST) != TSAR_OK) return fail("tsar_get_result");
    stamp("get_result");
    if (keep) {   // the same maps stay on this GPU for the gather to the fusing device
        keep->device = wk.device; keep->w = w; keep->h = h;
        keep->depth = (float*)tsar_device_alloc(wk.device, np * 4);
        keep->normal = (float*)tsar_device_alloc(wk.device, np * 12);
        if (!keep->depth || !keep->normal) return fail("tsar_device_alloc");
        if (tsar_get_result(ctx, keep->depth, keep->normal, nullptr, nullptr, TSAR_MEM_DEVICE) != TSAR_OK) return fail("tsar_get_result (device)");
    }
    hr.out_dir = out_dir; hr.w = w; hr.h = h;
    if (!defer_write && !write_maps(hr, PHASE1_FILES, ms_record_of(o))) return -1;
    if (!defer_write) stamp("write .dmb");
    if (o.timing) {
        printf("view %08d steps (ms): %s\n", ref_id, steps.c_str());
        tsar_kernel_timing kt[64];
        int nk = 0;
        if (tsar_get_kernel_timing(ctx, kt, 64, &nk) == TSAR_OK) {
            printf("view %08d kernels (launches x mean ms):", ref_id);
            for (int k = 0; k < nk && k < 64; k++) printf(" %s %d x %.3f |", kt[k].name, kt[k].launches, kt[k].launches ? kt[k].total_ms / kt[k].launches : 0.0);
            printf("\n");
        }
    }
    if (o.display_outputs && !write_display_outputs(hr, v.gray[0]->gray, v.cams[0])) return -1;
    const double sec = seconds_since(t0);
    if (seconds) *seconds = sec;
    FILE* rf = fopen((out_dir + "TSAR_results.txt").c_str(), "a");   // main.cpp:1854-1860
    if (rf) { fprintf(rf, "Total runtime: %g sec ( %g min)\n", sec, sec / 60.0); fclose(rf); }
    return 0;
}

// --timing, one view per process: milliseconds from exec() to now, from the process's start time in /proc (10 ms resolution)
static double ms_since_exec() {
    FILE* f = fopen("/proc/self/stat", "r");
    if (!f) return -1.0;
    char buf[2048];
    const size_t n = fread(buf, 1, sizeof buf - 1, f);
    fclose(f);
    buf[n] = 0;
    const char* p = strrchr(buf, ')');                 // the command name may contain blanks
    if (!p) return -1.0;
    unsigned long long start_ticks = 0;
    int field = 2;
    for (p++; *p && field < 22; p++)
        if (*p == ' ') { field++; if (field == 22) start_ticks = strtoull(p + 1, nullptr, 10); }
    double up = 0.0;
    f = fopen("/proc/uptime", "r");
    if (!f || fscanf(f, "%lf", &up) != 1) { if (f) fclose(f); return -1.0; }
    fclose(f);
    return (up - (double)start_ticks / (double)sysconf(_SC_CLK_TCK)) * 1e3;
}

// ---- the phases of --all after phase 1 (--geom_consistency, --consistency_filter): one view at a time on one worker per GPU, from map
// files to map files ---------------------------------------------------------------------------------------------------------------
struct LaterPhase {
    const char* name;                                                             // in its messages: "geom", "filter"
    const PhaseFiles& files;                                                      // what it writes; the resume line names the two outputs
    std::string (*record_of)(const Options&, const std::vector<int>& srcs);       // its record for a view
    const PhaseFiles& (*reads)(const Options&);                                   // the phase whose maps are its inputs: the sources' depth maps, the view's own depth map
    bool reads_normal;                                                            // ... and the view's own normal map
    std::vector<std::string> (*optional_inputs)(const Options&, int ref);         // files a view may lack (it then runs without them); may be null
    int (*view)(const Options&, Worker&, const LaterPhase&, int ref, const std::vector<int>& srcs, double* seconds);
};
static const PhaseFiles& phase1_files(const Options&) { return PHASE1_FILES; }
static std::vector<std::string> prior_files_of(const Options& o, int ref) {
    if (!o.geom_prior) return {};
    return {prior_file_of(o, ref, "_disp.dmb"), prior_file_of(o, ref, "_normals.dmb")};
}
// the map files a view of the phase reads, its own first
static std::vector<std::string> inputs_of(const Options& o, const LaterPhase& ph, int ref, const std::vector<int>& srcs) {
    const PhaseFiles& in = ph.reads(o);
    std::vector<std::string> inputs = {view_dir_of(o, ref) + in.depth()};
    if (ph.reads_normal) inputs.push_back(view_dir_of(o, ref) + in.normal());
    for (int s : srcs) inputs.push_back(view_dir_of(o, s) + in.depth());
    return inputs;
}
// resume of a later phase: its outputs complete, under the record of this run's settings, and no input newer than the older of the two
// outputs (an optional input that is not there is no input)
static bool outputs_current(const Options& o, const LaterPhase& ph, int ref, const std::vector<int>& srcs) {
    if (!outputs_recorded(o, ref, ph.files, ph.record_of(o, srcs))) return false;
    const std::string d = view_dir_of(o, ref);
    struct timespec t1, t2, ti;
    if (!mtime_of(d + ph.files.out[0], t1) || !mtime_of(d + ph.files.out[1], t2)) return false;
    const struct timespec out = newer(t1, t2) ? t2 : t1;
    for (const std::string& in : inputs_of(o, ph, ref, srcs))
        if (!mtime_of(in, ti) || newer(ti, out)) return false;
    if (ph.optional_inputs)
        for (const std::string& in : ph.optional_inputs(o, ref))
            if (mtime_of(in, ti) && newer(ti, out)) return false;
    return true;
}

static bool read_map(const std::string& path, int h, int w, int nb, std::vector<float>& out) {   // a .dmb map of exactly h x w x nb
    int hh = 0, ww = 0, nn = 0;
    return read_dmb(path, out, hh, ww, nn) && hh == h && ww == w && nn == nb;
}
// What a view of a later phase starts from: its images and cameras on the worker's context (parameters and views set), its own map(s)
// of the phase it reads and, per view slot, its pair.txt sources' depth maps of that phase (slot 0: none), each of the image size
struct LaterView : ViewSet {
    std::vector<float> own_depth, own_normal;
    std::vector<std::vector<float>> src_depth;
    std::vector<const float*> maps;    // as tsar_set_geom_depths takes them
};
static int load_later_view(const Options& o, Worker& wk, const LaterPhase& ph, int ref, const std::vector<int>& srcs, LaterView& lv) {
    ViewSet& v = lv;
    if (const int rc = load_views(o, wk, names_of(ref, srcs), v)) return rc;
    const int n = (int)v.cams.size();
    const std::vector<std::string> inputs = inputs_of(o, ph, ref, srcs);
    size_t next = 0;
    auto read_next = [&](int nb, std::vector<float>& out) {          // the inputs in their order
        const std::string& path = inputs[next++];
        if (read_map(path, v.h, v.w, nb, out)) return true;
        fprintf(stderr, "cannot read %s\n", path.c_str());
        return false;
    };
    if (!read_next(1, lv.own_depth) || (ph.reads_normal && !read_next(3, lv.own_normal))) return -1;
    lv.src_depth.resize(n);
    lv.maps.assign(n, nullptr);
    for (int i = 1; i < n; i++) {
        if (!read_next(1, lv.src_depth[i])) return -1;
        lv.maps[i] = lv.src_depth[i].data();
    }
    const tsar_params p = params_of(o, ref, v.dmin, v.dmax);
    if (tsar_set_params(wk.ctx, &p) != TSAR_OK) return wk.fail(ref, "tsar_set_params");
    if (tsar_set_views_u8(wk.ctx, n, v.w, v.h, v.px.data(), v.mem, v.cams.data()) != TSAR_OK) return wk.fail(ref, "tsar_set_views_u8");
    return 0;
}

// Phase 2 of one view (--geom_consistency): it starts from its own phase-1 maps (TSAR_disp.dmb + TSAR_normals.dmb), installs its
// pair.txt sources' TSAR_disp.dmb as the geometric-consistency term, rescores, runs --geom_iterations iterations at full resolution
// and writes TSAR_geom_disp.dmb + TSAR_geom_normals.dmb (the layout of the phase-1 maps) under TSAR_geom.txt, the settings they were
// made with.  --geom_multi_scale=L >= 1 runs the pass coarse to fine instead (api.run_geom_pass_multiscale's chain).
static int run_geom_view(const Options& o, Worker& wk, const LaterPhase& ph, int ref, const std::vector<int>& srcs, double* seconds) {
    const auto t0 = Clock::now();
    LaterView lv;
    if (const int rc = load_later_view(o, wk, ph, ref, srcs, lv)) return rc;
    const int n = (int)lv.maps.size(), w = lv.w, h = lv.h;
    tsar_ctx* const ctx = wk.ctx;
    auto fail = [&](const char* what) { return wk.fail(ref, what); };
    // coarse to fine: every level's views first, while no term is installed (the coarse contexts still hold the previous view's)
    const int L = o.geom_multi_scale;
    if (wk.ensure(L) != TSAR_OK) return -1;
    if (descend(wk, ref, L, {{[](tsar_ctx* c, const tsar_ctx*) { return tsar_clear_geom(c); }, "tsar_clear_geom"}, {tsar_pyramid_views, "tsar_pyramid_views"}})) return -1;
    if (tsar_load_planes(ctx, lv.own_depth.data(), lv.own_normal.data(), TSAR_MEM_HOST) != TSAR_OK) return fail("tsar_load_planes");
    if (tsar_set_geom_depths(ctx, n, lv.maps.data(), TSAR_MEM_HOST, o.geom_weight, o.geom_clip) != TSAR_OK) return fail("tsar_set_geom_depths");
    if (o.geom_prior) {
        // the view's plane prior, on the full-resolution context only; a view without the two files runs without one
        const std::vector<std::string> files = prior_files_of(o, ref);
        std::vector<float> prior_d, prior_n;
        if (!read_map(files[0], h, w, 1, prior_d) || !read_map(files[1], h, w, 3, prior_n)) printf("view %08d (geom): no plane prior (%s / %s not readable at %d x %d): runs without one\n", ref, files[0].c_str(), files[1].c_str(), w, h);
        else if (tsar_set_plane_prior(ctx, prior_d.data(), prior_n.data(), TSAR_MEM_HOST, &o.prior) != TSAR_OK) return fail("tsar_set_plane_prior");
    }
    if (o.geom_build) {
        // the view's plane prior built from its own depth where its sources confirm it (api.run_geom_pass's build_prior), in device memory:
        // one buffer holds the stored cost, then the prior's depth; one the own depth, filtered in place; one the prior's normals
        const size_t np = (size_t)w * h;
        float* score = (float*)tsar_device_alloc(wk.device, np * sizeof(float));
        float* kept = (float*)tsar_device_alloc(wk.device, np * sizeof(float));
        float* built = (float*)tsar_device_alloc(wk.device, 4 * np * sizeof(float));
        const char* what = "tsar_device_alloc";
        int rc = score && kept && built ? TSAR_OK : TSAR_ERR_NOMEM;
        auto step = [&](const char* name, int status) { if (rc == TSAR_OK) { rc = status; what = name; } };
        if (rc == TSAR_OK) {
            step("tsar_pm_rescore", tsar_pm_rescore(ctx));
            if (rc == TSAR_OK) step("tsar_get_plane", tsar_get_plane(ctx, nullptr, score, nullptr, nullptr, TSAR_MEM_DEVICE));
            if (rc == TSAR_OK) step("tsar_device_write", tsar_device_write(wk.device, kept, lv.own_depth.data(), np * sizeof(float)));
            if (rc == TSAR_OK) step("tsar_geom_check", tsar_geom_check(ctx, kept, &o.build_check, nullptr, kept, TSAR_MEM_DEVICE));
            if (rc == TSAR_OK) step("tsar_build_plane_prior", tsar_build_plane_prior(ctx, kept, score, TSAR_MEM_DEVICE, &o.build, built, built + np, nullptr));
            if (rc == TSAR_OK) step("tsar_set_plane_prior", tsar_set_plane_prior(ctx, built, built + np, TSAR_MEM_DEVICE, &o.prior));
            if (rc == TSAR_OK) step("tsar_pm_rescore", tsar_pm_rescore(ctx));
        }
        if (score) tsar_device_free(wk.device, score);
        if (kept) tsar_device_free(wk.device, kept);
        if (built) tsar_device_free(wk.device, built);
        if (rc != TSAR_OK) return fail(what);
    }
    if (o.geom_cross_view) {
        // the sources' maps rendered into this view, kept where K of them agree, and offered to the matcher; the rendered map stays on the
        // device.  The merge rescores first: at L = 0 it stands in for tsar_pm_rescore, at L >= 1 the chain is carried down from its planes
        float* rendered = (float*)tsar_device_alloc(wk.device, (size_t)w * h * sizeof(float));
        if (!rendered) return fail("tsar_device_alloc");
        int rc = tsar_geom_reproject(ctx, &o.cross, rendered, nullptr, TSAR_MEM_DEVICE);
        const char* what = "tsar_geom_reproject";
        if (rc == TSAR_OK) { rc = tsar_pm_merge_depths(ctx, rendered, TSAR_MEM_DEVICE, nullptr); what = "tsar_pm_merge_depths"; }
        tsar_device_free(wk.device, rendered);
        if (rc != TSAR_OK) return fail(what);
    }
    if (L == 0) {
        if (!o.geom_cross_view && !o.geom_build /* (which ends with the rescore) */ && tsar_pm_rescore(ctx) != TSAR_OK) return fail("tsar_pm_rescore");
        if (tsar_pm_iterate(ctx, o.geom_iterations) != TSAR_OK) return fail("tsar_pm_iterate");
    } else {
        if (descend(wk, ref, L, {{tsar_geom_pyramid, "tsar_geom_pyramid"}, {tsar_pyramid_planes, "tsar_pyramid_planes"}})) return -1;
        if (climb(wk, ref, L, geom_coarse_iterations_of(o), o.geom_iterations, {tsar_upsample_merge, "tsar_upsample_merge"})) return -1;
    }
    if (tsar_compute_disp(ctx) != TSAR_OK) return fail("tsar_compute_disp");
    HostResult& hr = wk.result[0];
    hr.out_dir = view_dir_of(o, ref); hr.w = w; hr.h = h;
    hr.depth.resize((size_t)w * h);
    hr.normal.resize((size_t)3 * w * h);
    if (tsar_get_result(ctx, hr.depth.data(), hr.normal.data(), nullptr, nullptr, TSAR_MEM_HOST) != TSAR_OK) return fail("tsar_get_result");
    if (tsar_clear_geom(ctx) != TSAR_OK) return fail("tsar_clear_geom");
    if (tsar_clear_plane_prior(ctx) != TSAR_OK) return fail("tsar_clear_plane_prior");
    const bool ok = write_maps(hr, ph.files, ph.record_of(o, srcs));
    if (seconds) *seconds = seconds_since(t0);
    return ok ? 0 : -1;
}

// The filter phase of one view (--consistency_filter): its depth map of the matching phase that ran last is checked against its
// pair.txt sources' maps of that phase (tsar_geom_check; the maps are installed as a term of weight 0, which only the check reads), and
// TSAR_filtered_disp.dmb + TSAR_consistent.png are written under TSAR_filter.txt, the settings and maps they were made with.
static int run_filter_view(const Options& o, Worker& wk, const LaterPhase& ph, int ref, const std::vector<int>& srcs, double* seconds) {
    const auto t0 = Clock::now();
    LaterView lv;
    if (const int rc = load_later_view(o, wk, ph, ref, srcs, lv)) return rc;
    const int n = (int)lv.maps.size(), w = lv.w, h = lv.h;
    tsar_ctx* const ctx = wk.ctx;
    auto fail = [&](const char* what) { return wk.fail(ref, what); };
    if (tsar_set_geom_depths(ctx, n, lv.maps.data(), TSAR_MEM_HOST, 0.0f, 3.0f) != TSAR_OK) return fail("tsar_set_geom_depths");
    std::vector<float> filtered((size_t)w * h), mask((size_t)w * h);
    if (tsar_geom_check(ctx, lv.own_depth.data(), &o.check, nullptr, filtered.data(), TSAR_MEM_HOST) != TSAR_OK) return fail("tsar_geom_check");
    if (tsar_get_reliable_mask(ctx, mask.data(), TSAR_MEM_HOST) != TSAR_OK) return fail("tsar_get_reliable_mask");
    if (tsar_clear_geom(ctx) != TSAR_OK) return fail("tsar_clear_geom");
    const std::string d = view_dir_of(o, ref);
    const bool ok = write_under_record(d, ph.files, ph.record_of(o, srcs), [&]() {
        return write_dmb(d + ph.files.out[0], filtered.data(), h, w, 1) && write_mask_png(d + ph.files.out[1], mask.data(), w, h);
    });
    size_t kept = 0;
    for (float m : mask) kept += m == 1.0f;
    if (ok) printf("view %08d (filter): %zu of %zu pixels of %s kept\n", ref, kept, mask.size(), ph.reads(o).depth());
    if (seconds) *seconds = seconds_since(t0);
    return ok ? 0 : -1;
}

// One phase of --all over every view of pair.txt, dealt round-robin to nthr threads (every view of a scene costs the same); thread t
// drives GPU t % ngpu with a worker of its own and calls view(worker, k, turn, &seconds) for each view k it is dealt that is not
// skipped (turn: the thread's count of views dealt so far).  A worker drops its contexts after a failed view.  A view that failed
// is then tried once more on the NEXT gpu's turn (the same one when there is only one) with a worker of its own, created fresh and
// destroyed with the view (turn -1) — never the contexts the failure left behind.  Returns each view's status; a skipped view's is
// what skipped(worker, k) returns (0 without it).
typedef std::function<int(Worker&, size_t k, int turn, double* seconds)> ViewFn;
static std::vector<int> run_pool(const Options& o, const char* phase, const std::vector<int>& refs, const std::vector<char>& skip, int nthr,
                                 const ViewFn& view, const std::function<int(Worker&, size_t k)>& skipped = nullptr) {
    const int ngpu = std::max(1, o.gpus);
    std::vector<int> rc(refs.size(), 0), gpu_of(refs.size(), 0);
    const std::string label = phase ? std::string(" (") + phase + ")" : "";
    std::vector<std::thread> th;
    for (int t = 0; t < nthr; t++)
        th.emplace_back([&, t]() {
            Worker wk(t % ngpu, phase, true);
            int turn = 0;
            for (size_t k = t; k < refs.size(); k += nthr, turn++) {
                gpu_of[k] = wk.device;
                if (skip[k]) {
                    printf("view %08d: %s%soutputs present, skipped\n", refs[k], phase ? phase : "", phase ? " " : "");
                    if (skipped) rc[k] = skipped(wk, k);
                    continue;
                }
                double sec = 0;
                rc[k] = view(wk, k, turn, &sec);
                if (rc[k] != 0) wk.drop();
                printf("view %08d on gpu %d%s: %s (%.2f s)\n", refs[k], wk.device, label.c_str(), rc[k] == 0 ? "ok" : "FAILED", sec);
            }
        });
    for (auto& t : th) t.join();
    for (size_t k = 0; k < refs.size(); k++) {
        if (skip[k] || rc[k] == 0) continue;
        const int g2 = (gpu_of[k] + 1) % ngpu;
        if (!phase) printf("view %08d FAILED on gpu %d: retrying once on gpu %d with a fresh context\n", refs[k], gpu_of[k], g2);
        double sec = 0;
        {
            Worker fresh(g2, phase, true);
            rc[k] = view(fresh, k, -1, &sec);
        }
        printf("view %08d on gpu %d (%s%sretry): %s (%.2f s)\n", refs[k], g2, phase ? phase : "", phase ? ", " : "", rc[k] == 0 ? "ok" : "FAILED", sec);
    }
    return rc;
}

// --fuse: a view's maps read back from its files onto device g (a resumed view's phase-1 maps, or every view's geom maps)
static bool load_kept(const Options& o, int ref, int g, const PhaseFiles& f, DeviceResult& r) {
    std::vector<float> d, nr;
    int h = 0, w = 0, nb = 0, h2 = 0, w2 = 0, nb2 = 0;
    const std::string dir = view_dir_of(o, ref);
    if (!read_dmb(dir + f.depth(), d, h, w, nb) || !read_dmb(dir + f.normal(), nr, h2, w2, nb2) || h != h2 || w != w2 || nb != 1 || nb2 != 3) return false;
    r.device = g; r.w = w; r.h = h;
    r.depth = (float*)tsar_device_alloc(g, d.size() * 4);
    r.normal = (float*)tsar_device_alloc(g, nr.size() * 4);
    return r.depth && r.normal && tsar_device_write(g, r.depth, d.data(), d.size() * 4) == TSAR_OK && tsar_device_write(g, r.normal, nr.data(), nr.size() * 4) == TSAR_OK;
}

// --all phase 1 over every view, dealt to ngpu x --workers threads; a worker's views alternate between its two result sets, whose
// files a helper thread writes while the next view is matched.  With --fuse each view's maps stay on its GPU in kept[k].  False when
// a view's outputs are missing.
static bool run_phase1(const Options& o, const std::vector<int>& refs, const std::map<int, std::vector<int>>& pairs, std::vector<DeviceResult>& kept) {
    const int nthr = std::max(1, o.gpus) * std::max(1, o.workers);
    // resume: the views whose output files are complete are not matched again (decided up front, so that nothing is read ahead for them)
    const std::string record = ms_record_of(o);
    std::vector<char> skip(refs.size(), 0);
    size_t n_skip = 0;
    if (!o.force)
        for (size_t k = 0; k < refs.size(); k++) n_skip += (skip[k] = outputs_recorded(o, refs[k], PHASE1_FILES, record) ? 1 : 0);
    if (n_skip) printf("resuming: %zu of %zu views already have complete TSAR_disp.dmb / TSAR_normals.dmb and are skipped (--force recomputes them)\n", n_skip, refs.size());
    const bool tsar_mode = o.mode == "tsar", external = o.mode == "load" || tsar_mode;
    // refinement modes: a ring of (page-locked) input buffers per worker; the maps, weak.png and reference image of its next seven
    // views are read while view k is on the GPU (one weak.png inflates in ~0.3 s, a view's kernels take ~0.1 s).  (About sixteen
    // sets in flight per process: eight with one worker, two per worker on an 8-GPU node — each set page-locks 0.39 GB at ETH3D
    // size, and the inflates run on as many host threads.)
    const size_t RING = std::max<size_t>(2, std::min<size_t>(8, 16 / (size_t)nthr));
    std::atomic<int> write_failures{0};
    auto view = [&](Worker& wk, size_t k, int turn, double* sec) {
        const int ref = refs[k];
        DeviceResult* keep = o.fuse ? &kept[k] : nullptr;
        if (keep) release(*keep);                 // what a failed attempt left there
        if (turn < 0) return run_view(o, wk, names_of(ref, pairs.at(ref)), {}, ref, sec, wk.result[0], keep);   // a retry: written at once
        HostResult& hr = wk.result[turn & 1];
        std::future<void>& writing = wk.writing[turn & 1];
        if (writing.valid()) writing.get();       // the set's previous files are on disk
        ExternalInputs* in = nullptr;
        if (external) {
            if (wk.ring.empty()) {
                wk.ring.resize(RING);
                for (ExternalInputs& e : wk.ring) e.pinned = true;
            }
            in = &wk.ring[turn % RING];
            if (!in->started) in->start(view_dir_of(o, ref), tsar_mode, "");
            for (size_t j = 1; j < RING; j++) {
                ExternalInputs& ahead = wk.ring[(turn + j) % RING];
                const size_t kk = k + j * nthr;
                if (kk < refs.size() && !skip[kk] && !ahead.started) ahead.start(view_dir_of(o, refs[kk]), tsar_mode, view_image_of(o, refs[kk]));
            }
        }
        const int rc = run_view(o, wk, names_of(ref, pairs.at(ref)), {}, ref, sec, hr, keep, /*defer_write*/ true, in);
        if (rc == 0) writing = std::async(std::launch::async, [&hr, &record, &write_failures]() { if (!write_maps(hr, PHASE1_FILES, record)) write_failures++; });
        return rc;
    };
    // --fuse needs a skipped view's maps on a device all the same: read back from its files
    auto skipped = [&](Worker& wk, size_t k) {
        if (!o.fuse || load_kept(o, refs[k], wk.device, PHASE1_FILES, kept[k])) return 0;
        fprintf(stderr, "view %08d: cannot read its output files back for --fuse\n", refs[k]);
        return -1;
    };
    const std::vector<int> rc = run_pool(o, nullptr, refs, skip, nthr, view, skipped);
    int missing = 0;
    for (size_t k = 0; k < refs.size(); k++)
        if (rc[k] != 0 || !outputs_recorded(o, refs[k], PHASE1_FILES, record)) { fprintf(stderr, "view %08d: outputs missing or incomplete\n", refs[k]); missing++; }
    return missing == 0 && write_failures == 0;       // (a file of an otherwise matched view that could not be written)
}

static const LaterPhase GEOM_PHASE = {"geom", GEOM_FILES, geom_record_of, phase1_files, true, prior_files_of, run_geom_view};
static const LaterPhase FILTER_PHASE = {"filter", FILTER_FILES, filter_record_of, filter_input_files, false, nullptr, run_filter_view};
// A later phase of --all over every view, one worker per GPU.  False when a view has no current outputs of the phase.
static bool run_later_phase(const Options& o, const LaterPhase& ph, const std::vector<int>& refs, const std::map<int, std::vector<int>>& pairs) {
    std::vector<char> skip(refs.size(), 0);
    size_t n_skip = 0;
    if (!o.force)
        for (size_t k = 0; k < refs.size(); k++) n_skip += (skip[k] = outputs_current(o, ph, refs[k], pairs.at(refs[k])) ? 1 : 0);
    if (n_skip) printf("%s: resuming: %zu of %zu views have current %s / %s and are skipped (--force recomputes them)\n", ph.name, n_skip, refs.size(), ph.files.out[0], ph.files.out[1]);
    const std::vector<int> rc = run_pool(o, ph.name, refs, skip, std::max(1, o.gpus),
                                         [&](Worker& wk, size_t k, int, double* sec) { return ph.view(o, wk, ph, refs[k], pairs.at(refs[k]), sec); });
    int missing = 0;
    for (size_t k = 0; k < refs.size(); k++)
        if (rc[k] != 0) { fprintf(stderr, "view %08d: %s outputs missing\n", refs[k], ph.name); missing++; }
    return missing == 0;
}

// --fuse: every view's maps gathered to GPU 0 (peer copies over xGMI; views matched on GPU 0 are already there), fused there, and the
// cloud written to APD/APD_TSAR.ply
static int fuse_views(const Options& o, const std::vector<int>& refs, const std::map<int, std::vector<int>>& pairs, std::vector<DeviceResult>& kept) {
    const auto t0 = Clock::now();
    if (refs.empty() || kept.empty()) { fprintf(stderr, "--fuse: no view was matched\n"); return 1; }
    const int n = (int)refs.size(), fw = kept[0].w, fh = kept[0].h;
    const size_t np = (size_t)fw * fh;
    std::map<int, int> slot;
    for (int k = 0; k < n; k++) slot[refs[k]] = k;
    std::vector<const float*> pd(n), pn(n), pg(n);
    std::vector<tsar_camera> cams(n);
    std::vector<void*> owned;                       // device-0 buffers to release
    auto release_owned = [&]() { for (void* q : owned) tsar_device_free(0, q); };
    size_t moved = 0;
    for (int k = 0; k < n; k++) {
        if (kept[k].w != fw || kept[k].h != fh) { fprintf(stderr, "--fuse: views differ in size\n"); release_owned(); return 1; }
        float *d = kept[k].depth, *nr = kept[k].normal;
        if (kept[k].device != 0) {
            float* d0 = (float*)tsar_device_alloc(0, np * 4);
            float* n0 = (float*)tsar_device_alloc(0, np * 12);
            if (d0) owned.push_back(d0);            // released on every error path below
            if (n0) owned.push_back(n0);
            if (!d0 || !n0 || tsar_peer_copy(0, d0, kept[k].device, d, np * 4) != TSAR_OK || tsar_peer_copy(0, n0, kept[k].device, nr, np * 12) != TSAR_OK) {
                fprintf(stderr, "--fuse: gather of view %08d from gpu %d failed\n", refs[k], kept[k].device);
                release_owned();
                return 1;
            }
            tsar_device_free(kept[k].device, d);
            tsar_device_free(kept[k].device, nr);
            d = d0; nr = n0;
            moved += np * 16;
        } else {
            owned.push_back(d); owned.push_back(nr);
        }
        auto img = g_images.get(view_image_of(o, refs[k]));
        float* g0 = (float*)tsar_device_alloc(0, np * 4);
        if (g0) owned.push_back(g0);
        const std::vector<float> img_f(img->gray.begin(), img->gray.end());      // the fuser colours its points from float images
        if (!img->ok || img_f.size() != np || !g0 || tsar_device_write(0, g0, img_f.data(), np * 4) != TSAR_OK) { fprintf(stderr, "--fuse: image of view %08d\n", refs[k]); release_owned(); return 1; }
        pd[k] = d; pn[k] = nr; pg[k] = g0;
        CamFile cf;
        if (!read_cam(cam_path(o, id8(refs[k])), cf)) { fprintf(stderr, "--fuse: camera of view %08d\n", refs[k]); release_owned(); return 1; }
        cams[k] = cf.cam;
    }
    const double t_gather = seconds_since(t0);
    std::vector<int32_t> off(n + 1, 0), idx;
    for (int k = 0; k < n; k++) {
        for (int sv : pairs.at(refs[k]))
            if (slot.count(sv)) idx.push_back(slot[sv]);
        off[k + 1] = (int32_t)idx.size();
    }
    if (idx.empty()) idx.push_back(0);
    const int64_t cap = (int64_t)n * fw * fh;
    std::unique_ptr<float[]> pts(new float[(size_t)cap * 9]);   // not zero-filled: only the fused points' pages are ever touched
    int64_t cnt = 0;
    const int rc = tsar_fuse(0, n, fw, fh, cams.data(), pd.data(), pn.data(), pg.data(), TSAR_MEM_DEVICE, off.data(), idx.data(), &o.fusion, pts.get(), cap, &cnt);
    release_owned();
    if (rc != TSAR_OK) { fprintf(stderr, "tsar_fuse failed: %d\n", rc); return 1; }
    if (cnt > cap) cnt = cap;
    const std::string out = o.mslp_folder + "APD/APD_TSAR.ply";
    if (!write_cloud_ply(out, pts.get(), cnt)) { fprintf(stderr, "cannot write %s\n", out.c_str()); return 1; }
    const double t_all = seconds_since(t0);
    printf("fused %d views on gpu 0: %lld points -> %s (gather of %.1f MB from other gpus + uploads %.3f s, total %.3f s)\n", n, (long long)cnt, out.c_str(),
           moved / 1e6, t_gather, t_all);
    return 0;
}

// --all: phase 1, then phase 2 once every view has its phase-1 maps (it reads them from the files), then the filter phase over the
// maps of whichever ran last (while the images are still resident on the devices), then --fuse
static int run_all(const Options& o, const std::map<int, std::vector<int>>& pairs) {
    g_pin_results = true;
    std::vector<int> refs;
    for (auto& kv : pairs) refs.push_back(kv.first);
    std::vector<DeviceResult> kept(o.fuse ? refs.size() : 0);
    bool ok = run_phase1(o, refs, pairs, kept);
    if (ok && o.geom) ok = run_later_phase(o, GEOM_PHASE, refs, pairs);
    if (ok && o.filter) ok = run_later_phase(o, FILTER_PHASE, refs, pairs);
    g_device_images.release();
    if (!ok) return 1;
    if (o.geom && o.fuse)        // --fuse fuses the geom maps: they replace the phase-1 maps kept on each view's device
        for (size_t k = 0; k < refs.size(); k++) {
            const int g = kept[k].device >= 0 ? kept[k].device : (int)(k % (size_t)std::max(1, o.gpus));
            release(kept[k]);
            if (!load_kept(o, refs[k], g, GEOM_FILES, kept[k])) { fprintf(stderr, "view %08d: cannot read its geom maps for --fuse\n", refs[k]); return 1; }
        }
    return o.fuse ? fuse_views(o, refs, pairs, kept) : 0;
}

// the refusals decided from the command line alone: false after the message
static bool options_valid(const Options& o) {
    if (o.mslp_folder.empty() || o.images_folder.empty()) { usage(); return false; }
    if (o.multi_scale > 0 || o.coarse_iterations_set || o.textureless_merge) {
        if (o.mode != "patchmatch") { fprintf(stderr, "--multi_scale / --coarse_iterations / --textureless_merge work with --mode=patchmatch only\n"); return false; }
        if (o.multi_scale == 0) { fprintf(stderr, "--coarse_iterations / --textureless_merge need --multi_scale=L with L >= 1\n"); return false; }
    }
    if ((o.geom_multi_scale > 0 || o.geom_coarse_iterations_set) && !o.geom) {
        fprintf(stderr, "--geom_multi_scale / --geom_coarse_iterations work with --geom_consistency only\n");
        return false;
    }
    if (o.geom_coarse_iterations_set && o.geom_multi_scale == 0) { fprintf(stderr, "--geom_coarse_iterations needs --geom_multi_scale=L with L >= 1\n"); return false; }
    if (o.geom) {
        if (!o.all) { fprintf(stderr, "--geom_consistency needs --all (phase 2 reads every view's phase-1 maps)\n"); return false; }
        if (o.mode == "tsar") { fprintf(stderr, "--geom_consistency does not work with --mode=tsar\n"); return false; }
        if (o.geom_iterations < 0 || !(o.geom_weight >= 0.f) || !(o.geom_clip > 0.f)) { fprintf(stderr, "--geom_iterations must be >= 0, --geom_weight >= 0, --geom_clip > 0\n"); return false; }
    }
    if ((o.geom_cross_view || o.geom_cross_view_option_set) && !o.geom) {
        fprintf(stderr, "--geom_cross_view / --geom_cross_view_depth_diff work with --geom_consistency only\n");
        return false;
    }
    if (o.geom_cross_view_option_set && !o.geom_cross_view) { fprintf(stderr, "--geom_cross_view_depth_diff needs --geom_cross_view\n"); return false; }
    if (o.geom_cross_view && (!(o.cross.depth_diff > 0.f) || !(o.cross.depth_diff < INFINITY))) {
        fprintf(stderr, "--geom_cross_view_depth_diff must be finite and > 0\n");
        return false;
    }
    if ((o.geom_build || o.geom_build_levels_set) && !o.geom) {
        fprintf(stderr, "--geom_build_prior and --geom_build_prior_levels work with --geom_consistency only\n");
        return false;
    }
    if (o.geom_build_levels_set && !o.geom_build) { fprintf(stderr, "--geom_build_prior_levels needs --geom_build_prior\n"); return false; }
    if (o.geom_build && o.geom_prior) { fprintf(stderr, "--geom_build_prior and --geom_plane_prior=STEM are mutually exclusive\n"); return false; }
    if (o.geom_build && (!tsar_build_plane_prior || !tsar_default_plane_prior_build_params || !tsar_get_plane)) {
        fprintf(stderr, "--geom_build_prior: this libtsar_hip.so has no tsar_build_plane_prior\n");
        return false;
    }
    if ((o.geom_prior || o.geom_prior_option_set) && !o.geom) {
        fprintf(stderr, "--geom_plane_prior and its settings work with --geom_consistency only\n");
        return false;
    }
    if (o.geom_prior_option_set && !o.geom_prior && !o.geom_build) {
        fprintf(stderr, "--geom_prior_weight_depth / --geom_prior_weight_normal / --geom_prior_depth_clip / --geom_prior_angle_clip need --geom_plane_prior=STEM or --geom_build_prior\n");
        return false;
    }
    if (o.geom_prior) {
        const std::string& st = o.geom_prior_stem;
        if (st.empty() || st.find('/') != std::string::npos || st.find('\\') != std::string::npos) {
            fprintf(stderr, "--geom_plane_prior=STEM: STEM must be a non-empty file-name stem without a path separator\n");
            return false;
        }
        if (st == "TSAR" || st == "TSAR_geom") { fprintf(stderr, "--geom_plane_prior=STEM: TSAR and TSAR_geom name a phase's own outputs\n"); return false; }
    }
    if (o.geom_prior || o.geom_build) {
        const tsar_plane_prior_params& q = o.prior;
        if (!(q.weight_depth >= 0.f) || !(q.weight_depth < INFINITY) || !(q.weight_normal >= 0.f) || !(q.weight_normal < INFINITY) || !(q.depth_clip > 0.f) ||
            !(q.depth_clip < INFINITY) || !(o.geom_prior_angle > 0.0) || !(o.geom_prior_angle <= 180.0) || !(q.normal_clip > 0.f) || !(q.normal_clip <= 2.f)) {
            fprintf(stderr, "--geom_prior_weight_depth / --geom_prior_weight_normal must be finite and >= 0, --geom_prior_depth_clip finite and > 0, --geom_prior_angle_clip in (0, 180] degrees\n");
            return false;
        }
    }
    if (o.filter_option_set && !o.filter) { fprintf(stderr, "--filter_reproj_error / --filter_depth_diff work with --consistency_filter only\n"); return false; }
    if (o.filter) {
        if (!o.all) { fprintf(stderr, "--consistency_filter needs --all (the filter reads every view's depth map)\n"); return false; }
        if (o.mode != "patchmatch") { fprintf(stderr, "--consistency_filter does not work with --mode=tsar or --mode=load\n"); return false; }
        const tsar_geom_check_params& c = o.check;
        if (c.min_consistent < 1 || c.min_consistent > 31 || !(c.reproj_error > 0.f) || !(c.reproj_error <= 1048576.f) || !(c.depth_diff > 0.f) || !(c.depth_diff < INFINITY)) {
            fprintf(stderr, "--consistency_filter=K must be in 1..31, --filter_reproj_error in (0, 2^20] pixels, --filter_depth_diff finite and > 0\n");
            return false;
        }
    }
    return true;
}

int main(int argc, char** argv) {
    const double ms_exec_to_main = ms_since_exec();
    Options o;
    tsar_default_fusion_params(&o.fusion);
    tsar_default_geom_check_params(&o.check);
    tsar_default_geom_reproject_params(&o.cross);
    tsar_default_plane_prior_params(&o.prior);
    const int pr = parse_args(argc, argv, o);
    if (pr != 0) return pr < 0 ? 1 : 0;
    o.prior.normal_clip = (float)(1.0 - cos(o.geom_prior_angle * (M_PI / 180.0)));   // 1 - cos(angle), rounded once from float64
    if (!options_valid(o)) return 1;
    if (o.geom_build) {                                  // (the entries are there: options_valid looked)
        tsar_default_plane_prior_build_params(&o.build);
        tsar_default_geom_check_params(&o.build_check);
        if (o.geom_build_cell) o.build.cell = o.geom_build_cell;
        if (o.geom_build_levels_set) o.build.max_levels = o.geom_build_levels;
    }
    if (o.mslp_folder.back() != '/') o.mslp_folder += '/';
    if (o.images_folder.back() != '/') o.images_folder += '/';
    std::map<int, std::vector<int>> pairs;
    const bool have_pairs = read_pairs(o.mslp_folder + "pair.txt", pairs);
    read_injection();
    if (o.all) {
        if (!have_pairs) { fprintf(stderr, "--all needs %spair.txt\n", o.mslp_folder.c_str()); return 1; }
        return run_all(o, pairs);
    }
    if (o.images.size() < 2) { usage(); return 1; }
    // camera id from the reference image name, source slots from pair.txt (main.cpp:1347-1376)
    const int camera_id = atoi(o.images[0].substr(4, 8).c_str());
    std::vector<int> slots;
    if (have_pairs && pairs.count(camera_id))
        for (int s : pairs[camera_id]) slots.push_back(s > camera_id ? s : s + 1);
    for (int s : slots)
        if (s < 1 || s >= (int)o.images.size()) { fprintf(stderr, "pair.txt refers to view slot %d but only %zu images were given\n", s, o.images.size()); return 1; }
    double sec = 0;
    // one view per process (the reference's shell loop): the context and the buffers stay alive until the process ends, and the
    // process ends without tearing them down one by one — the files are on disk, the driver reclaims the rest (0.25 s of a 1.4 s
    // invocation at ETH3D size went into freeing 1.5 GB of host buffers, the context and the runtime's own shutdown)
    static Worker single(0, nullptr, false);
    const int rc = run_view(o, single, o.images, slots, camera_id, &sec, single.result[0]);
    printf("Total runtime including disk i/o: %gsec\n", sec);
    if (o.timing) printf("process (ms since exec, 10 ms resolution): main entered at %.0f, leaving at %.0f (what the caller waits for beyond that is the teardown of the process's GPU state by the driver)\n",
                         ms_exec_to_main, ms_since_exec());
    fflush(nullptr);
    _exit(rc == 0 ? 0 : 1);
}
