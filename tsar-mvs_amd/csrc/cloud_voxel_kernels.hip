// cloud_voxel_kernels.hip — a voxel grid over a point cloud (include/tsar.h tsar_cloud_voxels): per occupied voxel the number of its
// points, the index of the point nearest the cell's centre and, per tolerance, how many of its points have dist2 within it; per point the
// number of its voxel.  Every output is an integer count or a minimum of a bit-defined 64-bit code, so the result is the same bits in
// every run and equals the numpy restatement (tests/cloud_voxels_ref.py).
//
// Per call:  bounds of the candidates (cloud_grid.hip: the origin is their per-axis minimum; the extents come from there too)
//            -> a cell key per point, z-major (z, y, x packed with as many bits per axis as the extents need, which orders the keys like
//               z << 42 | y << 21 | x), non-candidates above all; radix-sorted with the indices (cloud_grid.hip's sort; stable: a voxel's points keep index order)
//            -> head flags over the sorted keys and an inclusive scan: the voxel number of every sorted position
//            -> the reduce kernel, one lane per sorted point: its code (d2f bits, index) and its tolerance flags, reduced over the wave's
//               runs of one voxel by the head mask; the first lane of each (wave, run) issues one 64-bit atomicMin and one 32-bit
//               atomicAdd per tolerance.  Head lanes store their sorted position; rank is a scatter through the sorted indices
//            -> the finish kernel: rep = the code's index, count = the difference of neighbouring starts.
// No floating-point atomic, no loop over a voxel's population, no LDS, no scratch.
#include <rocprim/device/device_scan.hpp>

#include "cloud_grid.h"

#define CV_MAX_EXTENT (1 << 21)           // cells per axis: refused from here on

struct CvGrid {
    double ox, oy, oz;                    // per-axis minimum of the candidates
    double v;                             // (double)V
    int ex, ey, ez;                       // cells per axis
    int bx, by;                           // bits of the x and y fields of the packed key (the z field lies above them)
    unsigned long long none;              // key of a non-candidate: one bit above the z field
};

__device__ __forceinline__ unsigned long long cv_clampu(double c, int hi) { return (unsigned long long)(c < 0.0 ? 0 : (c > (double)hi ? hi : (int)c)); }

__global__ __launch_bounds__(CD_BLOCK) void cv_keys_kernel(const float* __restrict__ pts, long long n, int stride, CvGrid g, unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float* p = pts + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    unsigned long long key = g.none;
    if (cd_candidate(x, y, z)) {
        // (the origin is the minimum and the extent comes from the maximum through the same monotone function: the clamps never bind)
        const unsigned long long cx = cv_clampu(cd_cell(x, g.ox, g.v), g.ex - 1), cy = cv_clampu(cd_cell(y, g.oy, g.v), g.ey - 1), cz = cv_clampu(cd_cell(z, g.oz, g.v), g.ez - 1);
        key = (cz << (g.bx + g.by)) | (cy << g.bx) | cx;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

// head[k] = 1 where sorted position k starts a voxel (the candidates are the first n_cand positions)
__global__ __launch_bounds__(CD_BLOCK) void cv_heads_kernel(const unsigned long long* __restrict__ keys, uint32_t n_cand, uint32_t* __restrict__ head) {
    const uint32_t k = blockIdx.x * CD_BLOCK + threadIdx.x;
    if (k >= n_cand) return;
    head[k] = (k == 0 || keys[k] != keys[k - 1]) ? 1u : 0u;
}

// One lane per sorted position k < n.  incl[k] - 1 is the voxel number of candidate position k.  Outputs are written for voxels below
// n_write only (the caller's cap); start has n_write + 1 entries, best n_write, within n_write * n_tol.
__global__ __launch_bounds__(CD_BLOCK) void cv_reduce_kernel(const float* __restrict__ pts, int stride, const unsigned long long* __restrict__ keys,
                                                             const uint32_t* __restrict__ vals, const uint32_t* __restrict__ incl, uint32_t n, uint32_t n_cand, CvGrid g,
                                                             const float* __restrict__ dist2, int n_tol, const float* __restrict__ tol2, uint32_t n_write,
                                                             int32_t* __restrict__ rank_out, unsigned long long* __restrict__ best, uint32_t* __restrict__ start,
                                                             int32_t* __restrict__ within) {
    const uint32_t k = blockIdx.x * CD_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool cand = k < n_cand;
    uint32_t i = 0, v = 0xffffffffu;
    bool head = false;
    if (k < n) {
        i = vals[k];
        if (cand) {
            v = incl[k] - 1u;
            head = k == 0 || incl[k - 1] != incl[k];
        }
        if (rank_out) rank_out[i] = cand ? (int32_t)v : -1;
    }
    if (!best && !start && !within) return;
    if (cand && start) {
        if (head && v <= n_write) start[v] = k;                              // (entry n_write: the start of the first voxel not written)
        if (k == n_cand - 1 && v + 1u <= n_write) start[v + 1u] = n_cand;    // the end of the last voxel
    }
    // the wave's runs: a run starts at lane 0, at a head, and at every lane that holds no candidate (a run of its own, never issued)
    const unsigned long long starts = __ballot(lane == 0 || head || !cand);
    const unsigned long long upto = (2ull << lane) - 1ull;                    // lanes 0 .. lane (lane 63: all)
    const int last = (starts & ~upto) ? __ffsll((long long)(starts & ~upto)) - 2 : 63;   // the last lane of this lane's run
    const bool first = (starts >> lane) & 1ull;
    const unsigned long long run = first ? (((2ull << last) - 1ull) & ~(upto >> 1)) : 0ull;   // lanes lane .. last
    if (best) {
        unsigned long long code = ~0ull;
        if (cand) {
            const float* p = pts + (size_t)i * stride;
            const unsigned long long key = keys[k];
            const double cx = (double)(key & ((1ull << g.bx) - 1ull)), cy = (double)((key >> g.bx) & ((1ull << g.by) - 1ull)), cz = (double)(key >> (g.bx + g.by));
            // centre = o + (cell + 0.5) * V: one product, then one sum (the library is built with -ffp-contract=off)
            const double dx = (double)p[0] - (g.ox + (cx + 0.5) * g.v), dy = (double)p[1] - (g.oy + (cy + 0.5) * g.v), dz = (double)p[2] - (g.oz + (cz + 0.5) * g.v);
            const float d2f = (float)((dx * dx + dy * dy) + dz * dz);
            code = ((unsigned long long)__float_as_uint(d2f) << 32) | i;
        }
        // segmented minimum: after the step of offset s a lane holds the minimum over lanes lane .. min(lane + 2 s - 1, last)
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned long long o = __shfl_down(code, s, 64);
            if (lane + s <= last) code = o < code ? o : code;
        }
        if (first && cand && v < n_write) atomicMin(&best[v], code);
    }
    if (within) {
        const float d2 = cand ? dist2[i] : INFINITY;
        for (int t = 0; t < n_tol; t++) {
            const unsigned long long m = __ballot(cand && d2 <= tol2[t]);    // NaN and +inf never pass
            const int c = __popcll(m & run);
            if (first && cand && c && v < n_write) atomicAdd(&within[(size_t)v * n_tol + t], c);
        }
    }
}

__global__ __launch_bounds__(CD_BLOCK) void cv_finish_kernel(const unsigned long long* __restrict__ best, const uint32_t* __restrict__ start, uint32_t n_write,
                                                             int32_t* __restrict__ rep_out, int32_t* __restrict__ count_out) {
    const uint32_t v = blockIdx.x * CD_BLOCK + threadIdx.x;
    if (v >= n_write) return;
    if (rep_out) rep_out[v] = (int32_t)(uint32_t)best[v];
    if (count_out) count_out[v] = (int32_t)(start[v + 1] - start[v]);
}

__global__ __launch_bounds__(CD_BLOCK) void cv_fill_kernel(int32_t* __restrict__ out, long long n, int32_t value) {
    const long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x;
    if (i < n) out[i] = value;
}

static inline int cv_bits(int extent) { int b = 0; while ((1ll << b) < (long long)extent) b++; return b; }   // bits that hold 0 .. extent - 1

// cloud and dist2 are device pointers (the frame's views); rank_out, rep_out, count_out and within_out are the caller's own pointers in
// `mem`: how much of the per-voxel arrays is written is known only mid-call, so their staging happens here.  tol2 and the two counts are
// host memory.  The arguments have been checked (tsar_api.hip); 0 <= n < 2^31.
int run_cloud_voxels(CallFrame& f, const float* cloud, long long n, int stride, double voxel, const float* dist2, int n_tol, const float* tol2, int32_t* rank_out,
                     long long cap, int32_t* rep_out, int32_t* count_out, int32_t* within_out, int64_t* n_voxels_out, int64_t* n_valid_out, int mem) {
    tsar_ctx* ctx = f.ctx;
    hipStream_t st = ctx->stream;
    CdCounters* dc = f.tmp<CdCounters>(1);           // (cloud_grid.h; this operator has no counter of its own on the device)
    int32_t* d_rank = f.out(rank_out, (size_t)n, mem);
    if (!f.ok()) return f.finish();
    CdBounds bounds;
    if (!cd_measure(f, cloud, n, stride, dc, bounds)) return f.finish();
    const long long n_cand = bounds.n_cand;
    if (n_cand == 0) {                               // no voxel: every rank is -1
        if (n > 0 && d_rank) {
            ScopedKernelTimer tm(ctx, "voxel_reduce");
            hipLaunchKernelGGL(cv_fill_kernel, dim3(cd_blocks(n)), dim3(CD_BLOCK), 0, st, d_rank, n, -1);
        }
        f.launched();
        if (n_voxels_out) *n_voxels_out = 0;
        if (n_valid_out) *n_valid_out = 0;
        return f.finish();
    }
    CdGrid cg;
    if (!cd_grid(f, bounds, voxel, CV_MAX_EXTENT, "tsar_cloud_voxels: the cloud spans 2^21 cells or more of edge voxel on an axis: voxel is too small for this cloud's extent", cg))
        return f.finish();
    CvGrid g;
    g.ox = cg.ox; g.oy = cg.oy; g.oz = cg.oz;
    g.v = voxel;
    g.ex = cg.ex; g.ey = cg.ey; g.ez = cg.ez;
    g.bx = cv_bits(g.ex); g.by = cv_bits(g.ey);
    const int key_bits = g.bx + g.by + cv_bits(g.ez);        // at most 63
    g.none = 1ull << key_bits;

    unsigned long long *k0 = f.tmp<unsigned long long>((size_t)n), *k1 = f.tmp<unsigned long long>((size_t)n);
    uint32_t *v0 = f.tmp<uint32_t>((size_t)n), *v1 = f.tmp<uint32_t>((size_t)n);
    if (!f.ok()) return f.finish();
    {
        ScopedKernelTimer tm(ctx, "voxel_keys");
        hipLaunchKernelGGL(cv_keys_kernel, dim3(cd_blocks(n)), dim3(CD_BLOCK), 0, st, cloud, n, stride, g, k0, v0);
    }
    f.launched();
    if (!cd_sort(f, "cloud_sort", k0, k1, v0, v1, n, key_bits + 1)) return f.finish();
    // the unsorted keys and indices are done with: the head flags and the scanned voxel numbers take their place
    uint32_t *d_head = v0, *d_incl = (uint32_t*)k0;
    {
        ScopedKernelTimer tm(ctx, "voxel_heads");
        hipLaunchKernelGGL(cv_heads_kernel, dim3(cd_blocks(n_cand)), dim3(CD_BLOCK), 0, st, k1, (uint32_t)n_cand, d_head);
    }
    f.launched();
    {
        size_t bytes = 0;
        if (!f.ok() || !f.hip(rocprim::inclusive_scan(nullptr, bytes, d_head, d_incl, (size_t)n_cand, rocprim::plus<uint32_t>(), st), "rocprim::inclusive_scan sizing")) return f.finish();
        void* tmp = f.tmp<char>(bytes ? bytes : 1);
        if (!f.ok()) return f.finish();
        ScopedKernelTimer tm(ctx, "voxel_scan");
        if (!f.hip(rocprim::inclusive_scan(tmp, bytes, d_head, d_incl, (size_t)n_cand, rocprim::plus<uint32_t>(), st), "rocprim::inclusive_scan")) return f.finish();
    }
    uint32_t last_voxel = 0;                                 // the last candidate's inclusive scan: the number of voxels
    f.copy(&last_voxel, d_incl + (n_cand - 1), sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (!f.sync()) return f.finish();
    const long long n_voxels = (long long)last_voxel;
    const long long n_write = n_voxels < cap ? n_voxels : cap;
    const bool per_voxel = n_write > 0 && (rep_out || count_out || within_out);
    const bool want_best = per_voxel && rep_out, want_start = per_voxel && count_out, want_within = per_voxel && within_out;
    // device views of the first n_write entries of the per-voxel outputs (host buffers: only those entries are copied back)
    auto view = [&](int32_t* dst, size_t count, bool want) -> int32_t* {
        if (!want || mem == TSAR_MEM_DEVICE) return want ? dst : nullptr;
        int32_t* d = f.tmp<int32_t>(count);
        if (d) f.back.push_back({dst, d, count * sizeof(int32_t)});
        return d;
    };
    int32_t* d_rep = view(rep_out, (size_t)n_write, want_best);
    int32_t* d_count = view(count_out, (size_t)n_write, want_start);
    int32_t* d_within = view(within_out, (size_t)n_write * (size_t)(n_tol > 0 ? n_tol : 1), want_within);
    unsigned long long* d_best = want_best ? f.tmp<unsigned long long>((size_t)n_write) : nullptr;
    uint32_t* d_start = want_start ? f.tmp<uint32_t>((size_t)n_write + 1) : nullptr;
    float* d_tol2 = want_within ? f.tmp<float>((size_t)n_tol) : nullptr;
    if (!f.ok()) return f.finish();
    if (d_best) f.hip(hipMemsetAsync(d_best, 0xff, 8 * (size_t)n_write, st), "hipMemsetAsync");     // ~0: above every code
    if (d_within) { f.zero(d_within, 4 * (size_t)n_write * n_tol); f.copy(d_tol2, tol2, 4 * (size_t)n_tol, hipMemcpyHostToDevice); }
    if (f.ok() && (d_rank || per_voxel)) {
        ScopedKernelTimer tm(ctx, "voxel_reduce");
        hipLaunchKernelGGL(cv_reduce_kernel, dim3(cd_blocks(n)), dim3(CD_BLOCK), 0, st, cloud, stride, k1, v1, d_incl, (uint32_t)n, (uint32_t)n_cand, g, dist2, n_tol, d_tol2,
                           (uint32_t)n_write, d_rank, d_best, d_start, d_within);
    }
    f.launched();
    if (f.ok() && (d_best || d_start)) {
        ScopedKernelTimer tm(ctx, "voxel_finish");
        hipLaunchKernelGGL(cv_finish_kernel, dim3(cd_blocks(n_write)), dim3(CD_BLOCK), 0, st, d_best, d_start, (uint32_t)n_write, d_rep, d_count);
    }
    f.launched();
    if (n_voxels_out) *n_voxels_out = (int64_t)n_voxels;
    if (n_valid_out) *n_valid_out = (int64_t)n_cand;
    return f.finish();
}
