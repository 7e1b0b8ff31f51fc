// wl_hist.h -- Histogram: PDFs, joint PDFs and the extremes of flow fields, counted on the device (waterlily_amd/hist.py;
// wl_histogram / wl_field_range in include/wlhip.h, which holds the definition).  The third consumer of render_value() of
// wl_render.h -- a stored element, a face pair's mean or a Metrics.jl metric, formed in registers -- and the first that
// produces integers: counts are exact in any order, so LDS and global INTEGER atomics keep the contract "a function of the
// field alone, bit for bit, decomposed or not".  No float atomics, no scratch volume, nothing allocated.
//
//   k_hist      : one wavefront walks x-rows of the box, 64 consecutive cells at a time (plain kinds: HIST_UNROLL such pieces
//                 are loaded before the first is counted).  The bin of every lane goes to a workgroup-private uint32 table in
//                 LDS; within the wavefront, lanes that follow each other with the same bin are counted by the first of them
//                 (hist_add below: one shuffle, one ballot), so a constant field costs one LDS atomic per 64 cells and a smooth
//                 one a handful.  At the end the workgroup adds its non-zero bins to the int64 table with 64-bit global atomics.
//                 At most HIST_WG workgroups: the flush is at most HIST_WG x (non-zero bins) atomics, and HIST_WG x 4
//                 wavefronts are the 32 per CU that keep the plain kinds' loads streaming.
//                 A workgroup counts fewer than 2^32 cells: the rows are dealt round-robin to the wavefronts, so with R rows of
//                 X cells a workgroup takes at most 4 * ceil(R / (4 * W)) * X of them, W = min(HIST_WG, ceil(R / 4)) workgroups;
//                 for that to reach 2^32 the box would need more than 2^41 cells, which no device memory holds.
//   k_field_range     : the same walk; every lane keeps the smallest and the largest order-preserving integer image of its
//                 values (range_key: integer comparison of the images IS the IEEE total order, so -0 < +0 and the result does
//                 not depend on the order of combination) and two counts; wavefront, then workgroup, then one row of four
//                 integers per workgroup in the caller's scratch.
//   k_field_range_fin : one workgroup combines the rows and writes the four doubles.  A kernel boundary, no "last block"
//                 protocol.
#pragma once
#include "wl_render.h"

namespace wl {

constexpr int HIST_MAXBINS = 8192;    // A * B: 32 KB of LDS as uint32
constexpr int HIST_MAXEDGES = 1024;   // interior bins of an axis given by edges (copied to LDS)
constexpr int HIST_WG = 2048;         // the launch cap of k_hist and k_field_range: 8 workgroups of 4 wavefronts per CU
constexpr int HIST_UNROLL = 4;        // row pieces a wavefront loads before it counts (plain kinds)
#ifndef WL_HIST_AGG
#define WL_HIST_AGG 1                 // 1: runs of equal bins are counted by their first lane; 0: one LDS atomic per lane
#endif                                // (tools/hist_bench.py measures both builds; DESIGN.md has the numbers)

enum { HIST_HOST = 0, HIST_DEVRANGE = 1, HIST_EDGES = 2 };
// one axis as the kernels carry it
struct HistAxisDev {
    RenderWhat w;
    int absval, n, how;
    double lo, hi;                    // HIST_HOST
    const double *range, *edges;      // HIST_DEVRANGE: two doubles; HIST_EDGES: n + 1 doubles
};
// the cells of one call: lo_d <= J_d < hi_d with LOCAL planes along z; rows = ny * nz x-rows of pieces 64-cell pieces each
struct HistBox {
    int lo[3], hi[3];
    int ny, rows, pieces;
    unsigned long long cells;
};
inline bool hist_box(const G &g, const int l[3], const int h[3], HistBox &B) {
    for (int d = 0; d < 3; ++d) { B.lo[d] = l[d]; B.hi[d] = h[d]; }
    if (g.D == 3) box_planes(g, l[2], h[2], &B.lo[2], &B.hi[2]);
    const long nx = B.hi[0] - B.lo[0], ny = B.hi[1] - B.lo[1], nz = B.hi[2] - B.lo[2];
    B.ny = (int)ny;
    B.rows = (int)(ny * nz);
    B.pieces = (int)((nx + 63) / 64);
    B.cells = (unsigned long long)(nx * ny * nz);
    return ny * nz <= 0x3fffffffL;                             // (row + the launch's wavefronts stays an int)
}
inline unsigned hist_workgroups(const HistBox &B) {
    const int need = (B.rows + 3) / 4;
    return (unsigned)(need < HIST_WG ? need : HIST_WG);
}

template <class T, int D, bool METRIC>
__device__ __forceinline__ double hist_value(const G &g, const T *__restrict__ f, const HistAxisDev &a, int i, int j, int k) {
    const double v = render_value<T, D, METRIC>(g, f, a.w, i, j, k);
    return a.absval ? fabs(v) : v;
}

// ------------------------------------------------------------------------------------------ the bin of a value
struct HistBins {
    double lo, hi, scale;
    int n;
    const double *e;                  // the edges in LDS, or nullptr: uniform
};
__device__ __forceinline__ HistBins hist_bins(const HistAxisDev &a, const double *e_lds) {
    HistBins b;
    b.n = a.n;
    b.e = a.how == HIST_EDGES ? e_lds : nullptr;
    b.lo = a.how == HIST_DEVRANGE ? a.range[0] : a.lo;
    b.hi = a.how == HIST_DEVRANGE ? a.range[1] : a.hi;
    b.scale = (double)a.n / (b.hi - b.lo);
    return b;
}
// v is not NaN.  0: underflow, 1..n: interior, n + 1: overflow (include/wlhip.h has the rule in words)
__device__ __forceinline__ int hist_bin(const HistBins &b, double v) {
    if (b.e) {
        if (v < b.e[0]) return 0;
        if (v > b.e[b.n]) return b.n + 1;
        int l = 1, r = b.n;           // the first k in 1..n-1 with e_k > v (n: none) = 1 + the number of e_1..e_{n-1} <= v
        while (l < r) {
            const int m = (l + r) >> 1;
            if (b.e[m] <= v) l = m + 1; else r = m;
        }
        return l;
    }
    if (v < b.lo) return 0;
    if (v > b.hi) return b.n + 1;
    if (!(b.hi > b.lo)) return (b.lo <= v && v <= b.hi) ? 1 : b.n + 1;
    const double t = (v - b.lo) * b.scale;
    return 1 + (t < (double)(b.n - 1) ? (int)t : b.n - 1);
}
// h[bin] += 1 for every lane with bin >= 0.  Called by whole wavefronts.
__device__ __forceinline__ void hist_add(uint32_t *h, int bin, int lane) {
#if WL_HIST_AGG
    const int prev = __shfl_up(bin, 1, 64);
    const bool head = lane == 0 || prev != bin;
    const unsigned long long heads = __ballot(head);
    if (head && bin >= 0) {
        const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);   // bit 0: is lane + 1 a head?
        atomicAdd(&h[bin], (uint32_t)(above ? __ffsll(above) : 64 - lane));         // the run's length
    }
#else
    if (bin >= 0) atomicAdd(&h[bin], 1u);
#endif
}

// BK: 0 no second axis, 1 a plain one, 2 a metric
template <class T, int D, bool MA, int BK>
__global__ __launch_bounds__(256) void k_hist(const G g, const HistBox B, const HistAxisDev a, const HistAxisDev b, const T *__restrict__ fa,
                                              const T *__restrict__ fb, unsigned long long *__restrict__ cnt) {
    extern __shared__ double hist_lds[];                       // uint32 h[nb + 1] (the last: NaN cells), then the edges of a and b
    constexpr int U = (MA || BK == 2) ? 1 : HIST_UNROLL;
    uint32_t *h = (uint32_t *)hist_lds;
    const int A = a.n + 2, nb = A * (BK ? b.n + 2 : 1);
    double *ea = hist_lds + (nb + 2) / 2, *eb = ea + (a.how == HIST_EDGES ? a.n + 1 : 0);
    const int tid = threadIdx.x, lane = tid & 63;
    for (int t = tid; t <= nb; t += 256) h[t] = 0;
    if (a.how == HIST_EDGES) for (int t = tid; t <= a.n; t += 256) ea[t] = a.edges[t];
    if (BK && b.how == HIST_EDGES) for (int t = tid; t <= b.n; t += 256) eb[t] = b.edges[t];
    const HistBins ba = hist_bins(a, ea), bb = BK ? hist_bins(b, eb) : ba;
    __syncthreads();
    uint32_t nnan = 0;                                         // (the same in every lane of the wavefront)
    const int nw = (int)gridDim.x * 4;
    for (int row = (int)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        const int j = B.lo[1] + row % B.ny, k = B.lo[2] + row / B.ny;
        for (int p0 = 0; p0 < B.pieces; p0 += U) {
            double va[U], vb[U];
            bool in[U];
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const int i = B.lo[0] + (p0 + q) * 64 + lane;
                in[q] = i < B.hi[0];                            // (a piece past the row's end: no lane is in)
                const int ic = in[q] ? i : B.hi[0] - 1;         // a lane that is out loads the row's last cell and drops it: no
                va[q] = hist_value<T, D, MA>(g, fa, a, ic, j, k);                     // branch between the U loads, which so
                vb[q] = BK ? hist_value<T, D, BK == 2>(g, fb, b, ic, j, k) : 0.0;     // are all in flight before the first use
            }
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const bool nan = in[q] && (va[q] != va[q] || vb[q] != vb[q]);
                nnan += (uint32_t)__popcll(__ballot(nan));
                int bin = -1;
                if (in[q] && !nan) bin = hist_bin(ba, va[q]) + (BK ? A * hist_bin(bb, vb[q]) : 0);
                hist_add(h, bin, lane);
            }
        }
    }
    if (lane == 0 && nnan) atomicAdd(&h[nb], nnan);
    __syncthreads();
    for (int t = tid; t < nb; t += 256)
        if (h[t]) atomicAdd(&cnt[2 + t], (unsigned long long)h[t]);
    if (tid == 0 && h[nb]) atomicAdd(&cnt[1], (unsigned long long)h[nb]);
    if (tid == 0 && blockIdx.x == 0) atomicAdd(&cnt[0], B.cells);   // every cell of the box is visited: the rows above cover it
}

inline HistAxisDev hist_axis(int D, const wl_hist_axis *a) {
    HistAxisDev d;
    d.w.kind = a->kind; d.w.ipar = a->ipar; d.w.mode = 0;
    d.w.mp = metric_par(D, a->par, a->par2);
    d.absval = a->absval ? 1 : 0;
    d.n = a->nbins;
    d.how = a->edges_dev ? HIST_EDGES : (a->range_dev ? HIST_DEVRANGE : HIST_HOST);
    d.lo = a->lo; d.hi = a->hi;
    d.range = a->range_dev; d.edges = a->edges_dev;
    return d;
}

// l / h: the box in GLOBAL indices, already validated (D == 2: l[2] = 0, h[2] = 1)
template <class T, int D>
int op_histogram(const G &g, const wl_hist_axis *a, const wl_hist_axis *b, const int l[3], const int h[3], int accumulate, int64_t *cnt) {
    const HistAxisDev da = hist_axis(D, a), db = b ? hist_axis(D, b) : da;
    const int nb = (da.n + 2) * (b ? db.n + 2 : 1);
    hipStream_t st = ctx().stream;
    if (!accumulate) WL_HIP(hipMemsetAsync(cnt, 0, sizeof(int64_t) * (size_t)(2 + nb), st));
    HistBox B;
    if (!hist_box(g, l, h, B)) return fail(WL_E_ARG, "wl_histogram: more than 2^30 - 1 rows in the box", __FILE__, __LINE__);
    if (B.cells == 0) return 0;                                // no cell of this rank's
    const size_t lds = sizeof(double) * (size_t)((nb + 2) / 2 + (da.how == HIST_EDGES ? da.n + 1 : 0) + (b && db.how == HIST_EDGES ? db.n + 1 : 0));
    const bool ma = da.w.kind >= WL_R_METRIC;
    const int bk = !b ? 0 : (db.w.kind >= WL_R_METRIC ? 2 : 1);
    const T *fa = (const T *)a->f, *fb = b ? (const T *)b->f : fa;
    unsigned long long *c = (unsigned long long *)cnt;
    const dim3 grid(hist_workgroups(B)), blk(256);
    Prof pr(WL_K_MISC, (int64_t)B.cells);
#define WL_HIST_GO(MA, BK) hipLaunchKernelGGL((k_hist<T, D, MA, BK>), grid, blk, lds, st, g, B, da, db, fa, fb, c)
    if (ma) { if (bk == 0) WL_HIST_GO(true, 0); else if (bk == 1) WL_HIST_GO(true, 1); else WL_HIST_GO(true, 2); }
    else { if (bk == 0) WL_HIST_GO(false, 0); else if (bk == 1) WL_HIST_GO(false, 1); else WL_HIST_GO(false, 2); }
#undef WL_HIST_GO
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ the extremes
// the order-preserving integer image of a double: a < b in the IEEE total order <=> range_key(a) < range_key(b) as unsigned
__host__ __device__ inline unsigned long long range_key(double v) {
    unsigned long long u;
    memcpy(&u, &v, 8);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__host__ __device__ inline double range_unkey(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &u, 8);
    return v;
}
// four integers: the smallest key, the largest key, non-NaN cells, NaN cells
struct RangeAcc {
    unsigned long long kmin, kmax, n, nnan;
};
__device__ __forceinline__ RangeAcc range_start() { return RangeAcc{~0ull, 0ull, 0ull, 0ull}; }
__device__ __forceinline__ void range_join(RangeAcc &x, const RangeAcc &y) {
    x.kmin = y.kmin < x.kmin ? y.kmin : x.kmin;
    x.kmax = y.kmax > x.kmax ? y.kmax : x.kmax;
    x.n += y.n;
    x.nnan += y.nnan;
}
// all 256 threads call it; thread 0 returns the workgroup's result
__device__ __forceinline__ RangeAcc range_block(RangeAcc x, unsigned long long (*lds)[4]) {
    const int tid = threadIdx.x, lane = tid & 63;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        RangeAcc y;
        y.kmin = __shfl_down(x.kmin, off, 64); y.kmax = __shfl_down(x.kmax, off, 64);
        y.n = __shfl_down(x.n, off, 64); y.nnan = __shfl_down(x.nnan, off, 64);
        range_join(x, y);
    }
    if (lane == 0) { lds[tid >> 6][0] = x.kmin; lds[tid >> 6][1] = x.kmax; lds[tid >> 6][2] = x.n; lds[tid >> 6][3] = x.nnan; }
    __syncthreads();
    if (tid == 0)
        for (int w = 1; w < 4; ++w) range_join(x, RangeAcc{lds[w][0], lds[w][1], lds[w][2], lds[w][3]});
    return x;
}
template <class T, int D, bool METRIC>
__global__ __launch_bounds__(256) void k_field_range(const G g, const HistBox B, const HistAxisDev a, const T *__restrict__ f,
                                               unsigned long long *__restrict__ part) {
    __shared__ unsigned long long lds[4][4];
    constexpr int U = METRIC ? 1 : HIST_UNROLL;
    const int tid = threadIdx.x, lane = tid & 63;
    RangeAcc x = range_start();
    const int nw = (int)gridDim.x * 4;
    for (int row = (int)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        const int j = B.lo[1] + row % B.ny, k = B.lo[2] + row / B.ny;
        for (int p0 = 0; p0 < B.pieces; p0 += U) {
            double v[U];
            bool in[U];
#pragma unroll
            for (int q = 0; q < U; ++q) {
                const int i = B.lo[0] + (p0 + q) * 64 + lane;
                in[q] = i < B.hi[0];
                v[q] = hist_value<T, D, METRIC>(g, f, a, in[q] ? i : B.hi[0] - 1, j, k);      // (k_hist's branch-free loads)
            }
#pragma unroll
            for (int q = 0; q < U; ++q) {
                if (!in[q]) continue;
                if (v[q] != v[q]) { x.nnan += 1; continue; }
                const unsigned long long key = range_key(v[q]);
                x.kmin = key < x.kmin ? key : x.kmin;
                x.kmax = key > x.kmax ? key : x.kmax;
                x.n += 1;
            }
        }
    }
    x = range_block(x, lds);
    if (tid == 0) {
        unsigned long long *o = part + 4 * (size_t)blockIdx.x;
        o[0] = x.kmin; o[1] = x.kmax; o[2] = x.n; o[3] = x.nnan;
    }
}
__global__ __launch_bounds__(256) void k_field_range_fin(const unsigned long long *__restrict__ part, int np, double *__restrict__ out) {
    __shared__ unsigned long long lds[4][4];
    RangeAcc x = range_start();
    for (int p = threadIdx.x; p < np; p += 256) range_join(x, RangeAcc{part[4 * p], part[4 * p + 1], part[4 * p + 2], part[4 * p + 3]});
    x = range_block(x, lds);
    if (threadIdx.x == 0) {
        out[0] = x.n ? range_unkey(x.kmin) : __builtin_nan("");
        out[1] = x.n ? range_unkey(x.kmax) : __builtin_nan("");
        out[2] = (double)x.n;
        out[3] = (double)x.nnan;
    }
}
constexpr int64_t RANGE_SCRATCH = (int64_t)HIST_WG * 4 * sizeof(unsigned long long);

template <class T, int D>
int op_field_range(const G &g, const wl_hist_axis *a, const int l[3], const int h[3], void *scratch, double *out) {
    const HistAxisDev da = hist_axis(D, a);
    HistBox B;
    if (!hist_box(g, l, h, B)) return fail(WL_E_ARG, "wl_field_range: more than 2^30 - 1 rows in the box", __FILE__, __LINE__);
    hipStream_t st = ctx().stream;
    const unsigned np = B.cells ? hist_workgroups(B) : 0u;
    unsigned long long *part = (unsigned long long *)scratch;
    if (np) {
        Prof pr(WL_K_MISC, (int64_t)B.cells);
        if (da.w.kind >= WL_R_METRIC) hipLaunchKernelGGL((k_field_range<T, D, true>), dim3(np), dim3(256), 0, st, g, B, da, (const T *)a->f, part);
        else hipLaunchKernelGGL((k_field_range<T, D, false>), dim3(np), dim3(256), 0, st, g, B, da, (const T *)a->f, part);
        WL_HIP(hipGetLastError());
    }
    Prof pr(WL_K_SCALAR, 0);
    hipLaunchKernelGGL(k_field_range_fin, dim3(1), dim3(256), 0, st, (const unsigned long long *)part, (int)np, out);
    return (int)hipGetLastError();
}

}  // namespace wl
