// cloud_grid.hip — the steps every grid operator on a point cloud begins with (cloud_grid.h declares them): the bounds of the candidates,
// the grid over those bounds, the radix sort of (key, index) pairs, the sorted index of a cloud's cells with its 16-byte records, and the
// pair count and refusals of a search of a cloud among its own points.  rocPRIM's radix sort is instantiated here and nowhere else in
// the library.
#include <rocprim/device/device_radix_sort.hpp>

#include "cloud_grid.h"

// bounds[0..2] = codes of the per-axis minima, bounds[3..5] = of the maxima, *count = the candidates
__global__ __launch_bounds__(CD_BLOCK) void cd_bounds_kernel(const float* __restrict__ pts, long long n, int stride, uint32_t* __restrict__ bounds,
                                                             unsigned long long* __restrict__ count) {
    uint32_t lo[3] = {0xffffffffu, 0xffffffffu, 0xffffffffu}, hi[3] = {0u, 0u, 0u};
    unsigned long long cnt = 0;
    for (long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * CD_BLOCK) {
        const float* p = pts + (size_t)i * stride;
        const float x = p[0], y = p[1], z = p[2];
        if (!cd_candidate(x, y, z)) continue;
        const uint32_t c[3] = {cd_code(x), cd_code(y), cd_code(z)};
        for (int a = 0; a < 3; a++) { lo[a] = c[a] < lo[a] ? c[a] : lo[a]; hi[a] = c[a] > hi[a] ? c[a] : hi[a]; }
        cnt++;
    }
    for (int a = 0; a < 3; a++) { lo[a] = cd_wave_min(lo[a]); hi[a] = cd_wave_max(hi[a]); }
    cnt = cd_wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) {
        for (int a = 0; a < 3; a++) { atomicMin(&bounds[a], lo[a]); atomicMax(&bounds[3 + a], hi[a]); }
        atomicAdd(count, cnt);
    }
}

__global__ __launch_bounds__(CD_BLOCK) void cd_keys_kernel(const float* __restrict__ pts, long long n, int stride, CdGrid g, unsigned long long* __restrict__ keys,
                                                           uint32_t* __restrict__ vals) {
    const long long i = (long long)blockIdx.x * CD_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float* p = pts + (size_t)i * stride;
    const float x = p[0], y = p[1], z = p[2];
    unsigned long long key = CD_T_NONE;
    if (cd_candidate(x, y, z)) {
        // (the origin is the minimum and the extent comes from the maximum through the same monotone function: the clamps never bind)
        const unsigned long long cx = (unsigned)cd_clampi(cd_cell(x, g.ox, g.e), 0, g.ex - 1), cy = (unsigned)cd_clampi(cd_cell(y, g.oy, g.e), 0, g.ey - 1),
                                 cz = (unsigned)cd_clampi(cd_cell(z, g.oz, g.e), 0, g.ez - 1);
        key = (cz << 40) | (cy << 20) | cx;
    }
    keys[i] = key;
    vals[i] = (uint32_t)i;
}

__global__ __launch_bounds__(CD_BLOCK) void cd_gather_kernel(const float* __restrict__ pts, int stride, const uint32_t* __restrict__ vals, uint32_t n_cand,
                                                             CdRec* __restrict__ rec) {
    const uint32_t k = blockIdx.x * CD_BLOCK + threadIdx.x;
    if (k >= n_cand) return;
    const uint32_t j = vals[k];
    const float* p = pts + (size_t)j * stride;
    CdRec r;
    r.x = p[0]; r.y = p[1]; r.z = p[2]; r.j = j;
    rec[k] = r;
}

// *pairs += the number of candidates in the 27 cells around every candidate, itself included: what a search of the cloud among its own
// points looks at (cd_pairs_kernel of cloud_distance_kernels.hip counts for queries from another cloud)
__global__ __launch_bounds__(CD_BLOCK) void cd_self_pairs_kernel(const unsigned long long* __restrict__ keys, uint32_t n_cand, CdGrid g, unsigned long long* __restrict__ pairs) {
    const uint32_t t = blockIdx.x * CD_BLOCK + threadIdx.x;
    unsigned long long cnt = 0;
    if (t < n_cand) {
        const unsigned long long qkey = cd_self_query_key(keys[t]);
        for (int r = 0; r < 9; r++) {
            uint32_t b, e;
            if (cd_query_range(qkey, r, g, keys, n_cand, b, e)) cnt += e - b;
        }
    }
    cnt = cd_wave_sum(cnt);
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(pairs, cnt);
}

static inline float cd_decode(uint32_t c) { const uint32_t u = (c & 0x80000000u) ? (c & 0x7fffffffu) : ~c; float f; memcpy(&f, &u, 4); return f; }

bool cd_measure(CallFrame& f, const float* pts, long long n, int stride, CdCounters* dc, CdBounds& b) {
    CdCounters h = {};
    for (int a = 0; a < 3; a++) h.bounds[a] = 0xffffffffu;   // above every code; the maxima start at 0, below every code
    f.copy(dc, &h, sizeof h, hipMemcpyHostToDevice);
    if (n > 0 && f.ok()) {
        ScopedKernelTimer tm(f.ctx, "cloud_bounds");
        const unsigned blocks = cd_blocks(n) < 2048u ? cd_blocks(n) : 2048u;
        hipLaunchKernelGGL(cd_bounds_kernel, dim3(blocks), dim3(CD_BLOCK), 0, f.ctx->stream, pts, n, stride, dc->bounds, &dc->n_cand);
    }
    f.launched();
    f.copy(&h, dc, sizeof h, hipMemcpyDeviceToHost);
    if (!f.sync()) return false;
    for (int a = 0; a < 3; a++) { b.lo[a] = cd_decode(h.bounds[a]); b.hi[a] = cd_decode(h.bounds[3 + a]); }
    b.n_cand = (long long)h.n_cand;
    return true;
}

bool cd_grid(CallFrame& f, const CdBounds& b, double edge, int limit, const char* refusal, CdGrid& g) {
    g.ox = (double)b.lo[0]; g.oy = (double)b.lo[1]; g.oz = (double)b.lo[2];
    g.e = edge;
    int ext[3];
    for (int a = 0; a < 3; a++) {
        const double cells = floor(((double)b.hi[a] - (double)b.lo[a]) / edge) + 1.0;     // the cell of the maximum (cd_cell), plus one
        if (!(cells >= 1.0 && cells < (double)limit)) { f.fail(TSAR_ERR_INVALID, refusal); return false; }
        ext[a] = (int)cells;
    }
    g.ex = ext[0]; g.ey = ext[1]; g.ez = ext[2];
    return true;
}

bool cd_sort(CallFrame& f, const char* name, unsigned long long* keys_in, unsigned long long* keys_out, uint32_t* vals_in, uint32_t* vals_out, long long n, int end_bit) {
    size_t bytes = 0;
    if (!f.ok() || !f.hip(rocprim::radix_sort_pairs(nullptr, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, end_bit, f.ctx->stream), "rocprim::radix_sort_pairs sizing")) return false;
    void* tmp = f.tmp<char>(bytes);
    if (!f.ok()) return false;
    ScopedKernelTimer tm(f.ctx, name);
    return f.hip(rocprim::radix_sort_pairs(tmp, bytes, keys_in, keys_out, vals_in, vals_out, (size_t)n, 0, end_bit, f.ctx->stream), "rocprim::radix_sort_pairs");
}

bool cd_index(CallFrame& f, const float* pts, long long n, int stride, long long n_cand, const CdGrid& g, CdIndex& ix, const std::function<void()>& also_keys) {
    hipStream_t st = f.ctx->stream;
    unsigned long long* k0 = f.tmp<unsigned long long>((size_t)n);
    ix.keys = f.tmp<unsigned long long>((size_t)n);
    uint32_t* v0 = f.tmp<uint32_t>((size_t)n);
    ix.vals = f.tmp<uint32_t>((size_t)n);
    ix.rec = f.tmp<CdRec>((size_t)n_cand);
    if (!f.ok()) return false;
    {
        ScopedKernelTimer tm(f.ctx, "cloud_keys");
        hipLaunchKernelGGL(cd_keys_kernel, dim3(cd_blocks(n)), dim3(CD_BLOCK), 0, st, pts, n, stride, g, k0, v0);
        if (also_keys) also_keys();
    }
    f.launched();
    if (!cd_sort(f, "cloud_sort", k0, ix.keys, v0, ix.vals, n, 61)) return false;
    {
        ScopedKernelTimer tm(f.ctx, "cloud_gather");
        hipLaunchKernelGGL(cd_gather_kernel, dim3(cd_blocks(n_cand)), dim3(CD_BLOCK), 0, st, pts, stride, ix.vals, (uint32_t)n_cand, ix.rec);
    }
    return f.launched();
}

bool cd_self_search(CallFrame& f, const float* pts, long long n, int stride, double edge, long long max_pairs, int64_t* pairs_out, CdSelf& s) {
    s = {};
    s.dc = f.tmp<CdCounters>(1);
    if (!f.ok()) return false;
    CdBounds bounds;
    if (!cd_measure(f, pts, n, stride, s.dc, bounds)) return false;
    s.n_cand = bounds.n_cand;
    unsigned long long pairs = 0;
    if (s.n_cand > 0) {
        const std::string refusal = std::string(f.entry) + ": the cloud spans 2^20 cells or more of edge radius on an axis: radius is too small for this cloud's extent";
        if (!cd_grid(f, bounds, edge, CD_MAX_EXTENT, refusal.c_str(), s.g)) return false;
        if (!cd_index(f, pts, n, stride, s.n_cand, s.g, s.ix)) return false;
        {
            ScopedKernelTimer tm(f.ctx, "cloud_pairs");
            hipLaunchKernelGGL(cd_self_pairs_kernel, dim3(cd_blocks(s.n_cand)), dim3(CD_BLOCK), 0, f.ctx->stream, s.ix.keys, (uint32_t)s.n_cand, s.g, &s.dc->own[0]);
        }
        f.launched();
        f.copy(&pairs, &s.dc->own[0], sizeof pairs, hipMemcpyDeviceToHost);
        if (!f.sync()) return false;
    }
    if (pairs_out) *pairs_out = (int64_t)pairs;
    if (pairs > (unsigned long long)max_pairs) {
        char msg[256];
        snprintf(msg, sizeof msg, "%s: the call would look at %llu pairs, more than max_pairs = %lld: lower radius or raise max_pairs", f.entry, pairs, max_pairs);
        f.fail(TSAR_ERR_INVALID, msg);
        return false;
    }
    return true;
}
