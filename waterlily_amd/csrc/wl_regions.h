// wl_regions.h -- Regions: the connected regions of a threshold set, labelled on the device (waterlily_amd/regions.py;
// wl_regions / wl_regions_scratch in include/wlhip.h, which holds the definition).  The fifth consumer of render_value() of
// wl_render.h and the first that is a graph problem on the grid: a cell is IN when its value is below (above) a level, two IN
// cells that share a face are joined, and every connected component gets a number, a row of integers and two extremes.
//
// Labelling is union-find over the dense indices q of the box by label equivalence (Komura 2015; Playne & Hawick 2018: PAPERS.md).
// The parent array IS the label volume: label[q] = -1 for a cell that is not IN, else the parent of q, and at all times
//     parent[q] <= q                                                                                              (INVARIANT)
// so every chain of parents strictly descends and ends in a ROOT (parent[q] == q), the smallest q a find can reach.  Ten
// launches (seven with cap == 0) and one memset, a fixed number; nothing allocated, nothing read back:
//   k_rg_init    : one wavefront per x-row, 64 cells at a time: the value, the set (a ballot), the NaN count.  Each IN cell is
//                  linked to the start of its run of IN cells by a bit scan of the ballot; a run that goes on over the 64-cell
//                  seam keeps the start the wavefront carries from the piece before.  No atomics but three counts per wavefront.
//   k_rg_union   : rows without an IN cell leave.  The first cell of every stretch in which a row and its -y (-z, wrap) partner
//                  row are both IN unites the two runs: atomicMin on the larger root.  The x wrap joins a row's two end cells.
//   k_rg_flatten : every parent is replaced by its root; the roots of each row are counted.
//   k_scan_rows  : (wl_measure.h) exclusive scan of the row counts -> the number of each row's first root, and R.
//   k_rg_number  : roots take their number r in ascending q, kept as -(r + 2) so that no pass mistakes it for a parent.
//   k_rg_relabel : every other IN cell takes the number of its root.
//   k_rg_tab_init, k_rg_table : rows r < min(R, cap) of the table.  The roots decode their number here (with any cap).  A
//                  64-cell piece that holds cells of one region is combined in the wavefront and merged into the share the
//                  wavefront keeps of that region; shares go to the table with integer atomics when the region changes and,
//                  the four wavefronts' together, at the end (a region that fills the box: a dozen atomics per workgroup -- the
//                  first form, one set per run, spent 250 ms at 512^3 on one row of the table).  A piece of several regions
//                  adds per run of equal labels.  The extremes are atomicMin / atomicMax on range_key images, kept in ext_dev.
//   k_rg_peak    : columns 11, 12: cells whose key equals the region's extreme take atomicMin on q.
//   k_rg_fin     : the keys in ext_dev become doubles.
// Integer atomics only: every output is a count, a sum, an extreme of integers or of an order-preserving integer image, so the
// result is a function of the field, c and the box alone on any launch shape.  No thread waits for another wavefront: no locks,
// no flags, no "last block"; kernel boundaries are the only global barriers.  Parents are read and written through atomics or
// relaxed agent-scope atomic loads / stores, so no stale parent stays in a register.
#pragma once
#include "wl_hist.h"
#include "wl_measure.h"

namespace wl {

constexpr int RG_WG = 8192;           // the launch cap of the row kernels: workgroups of 4 wavefronts, rows dealt round-robin
constexpr int RG_TAB_WG = 2048;       // ... of k_rg_table: 32 wavefronts per CU, and a workgroup ends with one flush per region it holds
constexpr int RG_COLS = 13;

// the cells of one call: lo_d <= J_d < hi_d; rows = ny * nz x-rows of `pieces` 64-cell pieces; q = row * nx + (i - lo_0)
struct RgBox {
    int lo[3];
    int nx, ny, nz, rows, pieces;
    int wrap;                         // periodic_mask
    long cells;
};
inline RgBox rg_box(const int l[3], const int h[3], int wrap) {
    RgBox B;
    for (int d = 0; d < 3; ++d) B.lo[d] = l[d];
    B.nx = h[0] - l[0]; B.ny = h[1] - l[1]; B.nz = h[2] - l[2];
    B.rows = B.ny * B.nz;
    B.pieces = (B.nx + 63) / 64;
    B.wrap = wrap;
    B.cells = (long)B.nx * B.ny * B.nz;
    return B;
}
// scratch (8-byte aligned): rowoff long[rows + 1] | rowin int[rows] | rowcnt int[rows]
inline int64_t rg_scratch_bytes(long rows) { return 8 * (rows + 1) + 8 * rows; }
struct RgScratch {
    int *rowin, *rowcnt;
    long *rowoff;
};
inline RgScratch rg_scratch(void *p, long rows) {
    RgScratch s;
    s.rowoff = (long *)p;
    s.rowin = (int *)(s.rowoff + rows + 1);
    s.rowcnt = s.rowin + rows;
    return s;
}
inline unsigned rg_workgroups(const RgBox &B) {
    const int need = (B.rows + 3) / 4;
    return (unsigned)(need < RG_WG ? need : RG_WG);
}
struct RgWhat {
    RenderWhat w;
    int absval, above;
    double c;
};

__device__ __forceinline__ int rg_load(const int *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void rg_store(int *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long rg_load(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x (x is IN).  Bound: by the INVARIANT p = parent[x] < x whenever x is not a root, so x strictly descends and the
// loop runs at most x + 1 times.  HALVE: a cell met on the way is pointed at its grandparent -- atomicMin only ever lowers a
// parent to an ancestor, which is in the same set and below it, so the INVARIANT and every other thread's find stay valid; a
// root is never touched (its grandparent is itself).
template <bool HALVE>
__device__ __forceinline__ int rg_find(int *parent, int x) {
    int p = rg_load(&parent[x]);
    while (p != x) {
        const int gp = rg_load(&parent[p]);
        if (HALVE && gp != p) atomicMin(&parent[x], gp);
        x = p;
        p = gp;
    }
    return x;
}
// The sets of a and b become one.  Bound: an iteration either ends the loop, or its atomicMin found that `a` was no root any
// more -- another thread lowered parent[a] to old < a since the find -- and goes on from old: a retry only follows another
// thread's successful atomic, `a` strictly descends (old < a), and every successful atomic lowers the sum of all parents, which
// is bounded below.  Nothing here waits for a value that has yet to be written.
__device__ __forceinline__ void rg_union(int *parent, int a, int b) {
    for (;;) {
        a = rg_find<true>(parent, a);
        b = rg_find<true>(parent, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }          // a: the larger root, which takes the smaller one as parent
        const int old = atomicMin(&parent[a], b);
        if (old == a) return;                                  // a was a root: linked
        a = old;                                               // old < a: somebody linked a first; unite old's set with b's
    }
}

template <class T, int D, bool METRIC>
__device__ __forceinline__ double rg_value(const G &g, const T *__restrict__ f, const RgWhat &a, int i, int j, int k) {
    const double v = render_value<T, D, METRIC>(g, f, a.w, i, j, k);
    return a.absval ? fabs(v) : v;
}

// ------------------------------------------------------------------------------------------ the set and the x-runs
template <class T, int D, bool METRIC>
__global__ __launch_bounds__(256) void k_rg_init(const G g, const RgBox B, const RgWhat a, const T *__restrict__ f, int *__restrict__ label,
                                                 int *__restrict__ rowin, unsigned long long *__restrict__ n) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long nin = 0, nnan = 0, nvis = 0;            // (the same in every lane of the wavefront)
    const int nw = (int)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        const int j = B.lo[1] + (int)(row % B.ny), k = B.lo[2] + (int)(row / B.ny);
        const long q0 = row * B.nx;
        int carry = -1;                                        // the start of the run that reaches the end of the piece before
        bool any = false;
        for (int p = 0; p < B.pieces; ++p) {
            const int x = p * 64 + lane;
            const bool ok = x < B.nx;
            const double v = rg_value<T, D, METRIC>(g, f, a, B.lo[0] + (ok ? x : B.nx - 1), j, k);
            const bool nan = ok && v != v;
            const bool in = ok && (a.above ? v > a.c : v < a.c);       // (false for NaN)
            const unsigned long long m = __ballot(in);
            nnan += (unsigned long long)__popcll(__ballot(nan));
            nin += (unsigned long long)__popcll(m);
            nvis += (unsigned long long)__popcll(__ballot(ok));
            if (ok) {
                int lab = -1;
                if (in) {
                    const unsigned long long out_below = ~m & ((1ull << lane) - 1ull);       // lanes below that are not IN
                    const int s = out_below ? 64 - __clzll((long long)out_below) : 0;        // the run's first lane
                    lab = (s == 0 && carry >= 0) ? carry : (int)(q0 + p * 64 + s);
                }
                label[q0 + x] = lab;
            }
            if (m >> 63) {                                     // the run of lane 63 goes on into the next piece
                const unsigned long long out = ~m;
                const int s = out ? 64 - __clzll((long long)out) : 0;
                carry = (s == 0 && carry >= 0) ? carry : (int)(q0 + p * 64 + s);
            } else carry = -1;
            any = any || m != 0ull;
        }
        if (lane == 0) rowin[row] = any ? 1 : 0;
    }
    if (lane == 0) {
        if (nin) atomicAdd(&n[1], nin);
        if (nnan) atomicAdd(&n[2], nnan);
        if (nvis) atomicAdd(&n[3], nvis);
    }
}

// ------------------------------------------------------------------------------------------ the joins across rows
// the cells of row `row` (first dense index q0) and of its partner row (first dense index r0): one union per stretch of lanes
// in which both are IN -- inside a stretch the cells of either row are already one x-run
__device__ __forceinline__ void rg_join_rows(int *label, const RgBox &B, long q0, long r0, int lane) {
    for (int p = 0; p < B.pieces; ++p) {
        const int x = p * 64 + lane;
        const bool ok = x < B.nx;
        const bool both = ok && rg_load(&label[q0 + x]) >= 0 && rg_load(&label[r0 + x]) >= 0;
        const unsigned long long m = __ballot(both);
        if (both && !((m << 1) >> lane & 1ull)) rg_union(label, (int)(q0 + x), (int)(r0 + x));
    }
}
__global__ __launch_bounds__(256) void k_rg_union(const RgBox B, int *label, const int *__restrict__ rowin) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int nw = (int)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        if (!rowin[row]) continue;
        const int j = (int)(row % B.ny), k = (int)(row / B.ny);
        const long q0 = row * B.nx;
        if (j > 0 && rowin[row - 1]) rg_join_rows(label, B, q0, q0 - B.nx, lane);
        if (k > 0 && rowin[row - B.ny]) rg_join_rows(label, B, q0, q0 - (long)B.ny * B.nx, lane);
        if ((B.wrap & 2) && j == 0 && B.ny > 1 && rowin[row + B.ny - 1]) rg_join_rows(label, B, q0, q0 + (long)(B.ny - 1) * B.nx, lane);
        if ((B.wrap & 4) && k == 0 && B.nz > 1 && rowin[row + (long)(B.nz - 1) * B.ny])
            rg_join_rows(label, B, q0, q0 + (long)(B.nz - 1) * B.ny * B.nx, lane);
        if ((B.wrap & 1) && lane == 0 && B.nx > 1 && rg_load(&label[q0]) >= 0 && rg_load(&label[q0 + B.nx - 1]) >= 0)
            rg_union(label, (int)q0, (int)(q0 + B.nx - 1));
    }
}
// every parent becomes its root (a store of the root of x into parent[x] keeps the INVARIANT and every concurrent find valid:
// the root is an ancestor of x); rowcnt: the roots of each row
__global__ __launch_bounds__(256) void k_rg_flatten(const RgBox B, int *label, const int *__restrict__ rowin, int *__restrict__ rowcnt) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int nw = (int)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        int roots = 0;
        if (rowin[row]) {
            const long q0 = row * B.nx;
            for (int p = 0; p < B.pieces; ++p) {
                const int x = p * 64 + lane;
                bool root = false;
                if (x < B.nx && rg_load(&label[q0 + x]) >= 0) {
                    const int q = (int)(q0 + x), r = rg_find<true>(label, q);       // (halving: the rows after this one find short chains)
                    root = r == q;
                    if (!root) rg_store(&label[q], r);
                }
                roots += __popcll(__ballot(root));
            }
        }
        if (lane == 0) rowcnt[row] = roots;
    }
}
// the roots take their numbers in ascending q: label[root] = -(r + 2)
__global__ __launch_bounds__(256) void k_rg_number(const RgBox B, int *label, const int *__restrict__ rowcnt, const long *__restrict__ rowoff,
                                                   unsigned long long *__restrict__ n) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (blockIdx.x == 0 && tid == 0) n[0] = (unsigned long long)rowoff[B.rows];
    const int nw = (int)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        if (!rowcnt[row]) continue;
        const long q0 = row * B.nx;
        long next = rowoff[row];
        for (int p = 0; p < B.pieces; ++p) {
            const int x = p * 64 + lane;
            const bool root = x < B.nx && label[q0 + x] == (int)(q0 + x);
            const unsigned long long m = __ballot(root);
            if (root) label[q0 + x] = -(int)(next + __popcll(m & ((1ull << lane) - 1ull))) - 2;
            next += __popcll(m);
        }
    }
}
// every IN cell that is no root reads its root's number (the roots keep -(r + 2) in this pass: nothing it reads changes)
__global__ __launch_bounds__(256) void k_rg_relabel(const RgBox B, int *label, const int *__restrict__ rowin) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int nw = (int)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        if (!rowin[row]) continue;
        const long q0 = row * B.nx;
        for (int p = 0; p < B.pieces; ++p) {
            const int x = p * 64 + lane;
            if (x >= B.nx) continue;
            const int l = rg_load(&label[q0 + x]);
            if (l >= 0) rg_store(&label[q0 + x], -rg_load(&label[l]) - 2);
        }
    }
}

// ------------------------------------------------------------------------------------------ the table
__global__ __launch_bounds__(256) void k_rg_tab_init(long cap, const unsigned long long *__restrict__ n, unsigned long long *__restrict__ tab,
                                                     unsigned long long *__restrict__ ext) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    const long R = (long)n[0];
    if (r >= cap || r >= R) return;
    unsigned long long *t = tab + RG_COLS * r;
    const unsigned long long big = 0x7fffffffffffffffull;
    t[0] = 0; t[1] = 0; t[2] = 0; t[3] = 0; t[4] = 0;
    t[5] = big; t[6] = 0; t[7] = big; t[8] = 0; t[9] = big; t[10] = 0;
    t[11] = big; t[12] = big;
    ext[2 * r] = ~0ull;
    ext[2 * r + 1] = 0ull;
}
// One region's share of a row of the table, the same in every lane of a wavefront: what k_rg_table keeps between two flushes.
struct RgAcc {
    int r;                                                     // -1: nothing kept
    unsigned long long n, si, sj, sk, ilo, ihi, jlo, jhi, klo, khi, kmin, kmax;
};
__device__ __forceinline__ unsigned long long rg_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ unsigned long long rg_wave_min(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ unsigned long long rg_wave_max(unsigned long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const unsigned long long o = __shfl_xor(v, off, 64); v = o > v ? o : v; }
    return v;
}
// t[c] = min / max(t[c], v): a relaxed load first, so that only a value that would change the extreme pays for an atomic
__device__ __forceinline__ void rg_min(unsigned long long *p, unsigned long long v) { if (v < rg_load(p)) atomicMin(p, v); }
__device__ __forceinline__ void rg_max(unsigned long long *p, unsigned long long v) { if (v > rg_load(p)) atomicMax(p, v); }
__device__ __forceinline__ void rg_flush(const RgAcc &A, unsigned long long *tab, unsigned long long *ext, int lane) {
    if (A.r < 0 || lane != 0) return;
    unsigned long long *t = tab + RG_COLS * (long)A.r;
    atomicAdd(&t[1], A.n); atomicAdd(&t[2], A.si); atomicAdd(&t[3], A.sj); atomicAdd(&t[4], A.sk);
    rg_min(&t[5], A.ilo); rg_max(&t[6], A.ihi); rg_min(&t[7], A.jlo); rg_max(&t[8], A.jhi); rg_min(&t[9], A.klo); rg_max(&t[10], A.khi);
    rg_min(&ext[2 * (long)A.r], A.kmin); rg_max(&ext[2 * (long)A.r + 1], A.kmax);
}
// Called by whole wavefronts.  The roots decode their number (with any cap); rows r < cap of the table.  A 64-cell piece whose
// IN cells all belong to ONE region -- nearly every piece of a large region -- is combined in the wavefront (a ballot, three
// butterfly reductions) and merged into the share the wavefront keeps of that region, which goes to the table with integer
// atomics when the region changes and at the end: a region that fills the box costs a dozen atomics per wavefront, not per run.
// A piece that holds cells of several regions takes the plain way: the first lane of every run of equal labels adds the run's
// integer columns, which follow from its first index and its length in closed form, and every lane offers its key.
template <class T, int D, bool METRIC>
__global__ __launch_bounds__(256) void k_rg_table(const G g, const RgBox B, const RgWhat a, const T *__restrict__ f, int *label,
                                                  const int *__restrict__ rowin, long cap, unsigned long long *tab, unsigned long long *ext) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int nw = (int)gridDim.x * 4;
    RgAcc A;
    A.r = -1;
    for (long row = (long)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        if (!rowin[row]) continue;
        const int j = B.lo[1] + (int)(row % B.ny), k = B.lo[2] + (int)(row / B.ny);
        const long q0 = row * B.nx;
        for (int p = 0; p < B.pieces; ++p) {
            const int x = p * 64 + lane;
            int r = -1;
            if (x < B.nx) {
                r = label[q0 + x];
                if (r <= -2) {                                 // a root
                    r = -r - 2;
                    label[q0 + x] = r;
                    if (r < cap) tab[RG_COLS * (long)r] = (unsigned long long)(q0 + x);
                }
            }
            const bool valid = r >= 0 && r < cap;
            const unsigned long long m = __ballot(valid);
            if (!m) continue;                                  // (the same in every lane)
            const unsigned long long i = (unsigned long long)(B.lo[0] + x);
            const unsigned long long key = valid ? range_key(rg_value<T, D, METRIC>(g, f, a, B.lo[0] + x, j, k)) : 0ull;
            const int first = __ffsll((long long)m) - 1;
            const int r0 = __shfl(r, first, 64);
            if (!__ballot(valid && r != r0)) {                 // one region in this piece
                const unsigned long long n = (unsigned long long)__popcll(m);
                const unsigned long long si = rg_wave_sum(valid ? i : 0ull);
                const unsigned long long kmin = rg_wave_min(valid ? key : ~0ull), kmax = rg_wave_max(valid ? key : 0ull);
                const unsigned long long ilo = (unsigned long long)(B.lo[0] + p * 64 + first);
                const unsigned long long ihi = (unsigned long long)(B.lo[0] + p * 64 + 63 - __clzll((long long)m));
                if (A.r != r0) {
                    rg_flush(A, tab, ext, lane);
                    A.r = r0; A.n = 0; A.si = 0; A.sj = 0; A.sk = 0;
                    A.ilo = ilo; A.ihi = ihi; A.jlo = A.jhi = (unsigned long long)j; A.klo = A.khi = (unsigned long long)k;
                    A.kmin = kmin; A.kmax = kmax;
                }
                A.n += n; A.si += si; A.sj += (unsigned long long)j * n; A.sk += (unsigned long long)k * n;
                A.ilo = ilo < A.ilo ? ilo : A.ilo; A.ihi = ihi > A.ihi ? ihi : A.ihi;
                A.jlo = (unsigned long long)j < A.jlo ? (unsigned long long)j : A.jlo; A.jhi = (unsigned long long)j > A.jhi ? (unsigned long long)j : A.jhi;
                A.klo = (unsigned long long)k < A.klo ? (unsigned long long)k : A.klo; A.khi = (unsigned long long)k > A.khi ? (unsigned long long)k : A.khi;
                A.kmin = kmin < A.kmin ? kmin : A.kmin; A.kmax = kmax > A.kmax ? kmax : A.kmax;
                continue;
            }
            const int prev = __shfl_up(r, 1, 64);
            const bool head = lane == 0 || prev != r;
            const unsigned long long heads = __ballot(head);
            if (!valid) continue;
            unsigned long long *t = tab + RG_COLS * (long)r;
            if (head) {
                const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
                const unsigned long long len = (unsigned long long)(above ? __ffsll((long long)above) : 64 - lane);      // the run's length
                const unsigned long long i1 = i + len - 1;
                atomicAdd(&t[1], len);
                atomicAdd(&t[2], (i + i1) * len / 2);          // i + (i + 1) + .. + i1
                atomicAdd(&t[3], (unsigned long long)j * len);
                atomicAdd(&t[4], (unsigned long long)k * len);
                rg_min(&t[5], i); rg_max(&t[6], i1);
                rg_min(&t[7], (unsigned long long)j); rg_max(&t[8], (unsigned long long)j);
                rg_min(&t[9], (unsigned long long)k); rg_max(&t[10], (unsigned long long)k);
            }
            rg_min(&ext[2 * (long)r], key);
            rg_max(&ext[2 * (long)r + 1], key);
        }
    }
    // the four wavefronts' last shares: those of one region (a region that fills the box: all four) go to the table as one
    __shared__ RgAcc last[4];
    if (lane == 0) last[tid >> 6] = A;
    __syncthreads();                                           // (every thread arrives: the loops above leave by `continue` alone)
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) {
            const RgAcc &Y = last[w];
            if (Y.r < 0) continue;
            if (Y.r != A.r) { rg_flush(A, tab, ext, 0); A = Y; continue; }
            A.n += Y.n; A.si += Y.si; A.sj += Y.sj; A.sk += Y.sk;
            A.ilo = Y.ilo < A.ilo ? Y.ilo : A.ilo; A.ihi = Y.ihi > A.ihi ? Y.ihi : A.ihi;
            A.jlo = Y.jlo < A.jlo ? Y.jlo : A.jlo; A.jhi = Y.jhi > A.jhi ? Y.jhi : A.jhi;
            A.klo = Y.klo < A.klo ? Y.klo : A.klo; A.khi = Y.khi > A.khi ? Y.khi : A.khi;
            A.kmin = Y.kmin < A.kmin ? Y.kmin : A.kmin; A.kmax = Y.kmax > A.kmax ? Y.kmax : A.kmax;
        }
        rg_flush(A, tab, ext, 0);
    }
}
// columns 11, 12: the smallest q at which the region's minimum (maximum) is attained
template <class T, int D, bool METRIC>
__global__ __launch_bounds__(256) void k_rg_peak(const G g, const RgBox B, const RgWhat a, const T *__restrict__ f, const int *__restrict__ label,
                                                 const int *__restrict__ rowin, long cap, unsigned long long *tab, const unsigned long long *__restrict__ ext) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int nw = (int)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        if (!rowin[row]) continue;
        const int j = B.lo[1] + (int)(row % B.ny), k = B.lo[2] + (int)(row / B.ny);
        const long q0 = row * B.nx;
        for (int p = 0; p < B.pieces; ++p) {
            const int x = p * 64 + lane;
            if (x >= B.nx) continue;
            const int r = label[q0 + x];
            if (r < 0 || r >= cap) continue;
            const unsigned long long key = range_key(rg_value<T, D, METRIC>(g, f, a, B.lo[0] + x, j, k));
            const unsigned long long q = (unsigned long long)(q0 + x);
            unsigned long long *t = tab + RG_COLS * (long)r;
            if (key == ext[2 * (long)r] && q < rg_load(&t[11])) atomicMin(&t[11], q);
            if (key == ext[2 * (long)r + 1] && q < rg_load(&t[12])) atomicMin(&t[12], q);
        }
    }
}
__global__ __launch_bounds__(256) void k_rg_fin(long cap, const unsigned long long *__restrict__ n, unsigned long long *ext) {
    const long r = (long)blockIdx.x * 256 + threadIdx.x;
    if (r >= cap || r >= (long)n[0]) return;
    double *e = (double *)ext;
    const unsigned long long k0 = ext[2 * r], k1 = ext[2 * r + 1];
    e[2 * r] = range_unkey(k0);
    e[2 * r + 1] = range_unkey(k1);
}

// l / h: the box, already validated (D == 2: l[2] = 0, h[2] = 1; one rank: global planes are local planes)
template <class T, int D>
int op_regions(const G &g, const wl_rg_value *v, int cmp, double c, int wrap, const int l[3], const int h[3], int32_t *label, int64_t cap,
               int64_t *tab_dev, double *ext_dev, int64_t *n_dev, void *scratch) {
    const RgBox B = rg_box(l, h, wrap);
    const RgScratch s = rg_scratch(scratch, B.rows);
    RgWhat a;
    a.w.kind = v->kind; a.w.ipar = v->ipar; a.w.mode = 0;
    a.w.mp = metric_par(D, v->par, v->par2);
    a.absval = v->absval ? 1 : 0;
    a.above = cmp == WL_RG_ABOVE ? 1 : 0;
    a.c = c;
    const bool metric = v->kind >= WL_R_METRIC;
    const T *f = (const T *)v->f;
    unsigned long long *n = (unsigned long long *)n_dev, *tab = (unsigned long long *)tab_dev, *ext = (unsigned long long *)ext_dev;
    hipStream_t st = ctx().stream;
    const dim3 grid(rg_workgroups(B)), blk(256);
    WL_HIP(hipMemsetAsync(n_dev, 0, 4 * sizeof(int64_t), st));
    {
        Prof pr(WL_K_MISC, (int64_t)B.cells);
        if (metric) hipLaunchKernelGGL((k_rg_init<T, D, true>), grid, blk, 0, st, g, B, a, f, label, s.rowin, n);
        else hipLaunchKernelGGL((k_rg_init<T, D, false>), grid, blk, 0, st, g, B, a, f, label, s.rowin, n);
        WL_HIP(hipGetLastError());
    }
    {
        Prof pr(WL_K_MISC, (int64_t)B.cells);
        hipLaunchKernelGGL(k_rg_union, grid, blk, 0, st, B, label, (const int *)s.rowin);
        WL_HIP(hipGetLastError());
    }
    {
        Prof pr(WL_K_MISC, (int64_t)B.cells);
        hipLaunchKernelGGL(k_rg_flatten, grid, blk, 0, st, B, label, (const int *)s.rowin, s.rowcnt);
        WL_HIP(hipGetLastError());
    }
    {
        Prof pr(WL_K_SCALAR, 0);
        hipLaunchKernelGGL(k_scan_rows, dim3(1), dim3(1024), 0, st, (const int *)s.rowcnt, s.rowoff, (long)B.rows);
        WL_HIP(hipGetLastError());
    }
    {
        Prof pr(WL_K_MISC, (int64_t)B.cells);
        hipLaunchKernelGGL(k_rg_number, grid, blk, 0, st, B, label, (const int *)s.rowcnt, (const long *)s.rowoff, n);
        WL_HIP(hipGetLastError());
    }
    {
        Prof pr(WL_K_MISC, (int64_t)B.cells);
        hipLaunchKernelGGL(k_rg_relabel, grid, blk, 0, st, B, label, (const int *)s.rowin);
        WL_HIP(hipGetLastError());
    }
    const dim3 tgrid((unsigned)((cap + 255) / 256));
    if (cap > 0) {
        Prof pr(WL_K_SCALAR, 0);
        hipLaunchKernelGGL(k_rg_tab_init, tgrid, blk, 0, st, (long)cap, (const unsigned long long *)n, tab, ext);
        WL_HIP(hipGetLastError());
    }
    {
        Prof pr(WL_K_MISC, (int64_t)B.cells);
        const dim3 tg(grid.x < (unsigned)RG_TAB_WG ? grid.x : (unsigned)RG_TAB_WG);
        if (metric) hipLaunchKernelGGL((k_rg_table<T, D, true>), tg, blk, 0, st, g, B, a, f, label, (const int *)s.rowin, (long)cap, tab, ext);
        else hipLaunchKernelGGL((k_rg_table<T, D, false>), tg, blk, 0, st, g, B, a, f, label, (const int *)s.rowin, (long)cap, tab, ext);
        WL_HIP(hipGetLastError());
    }
    if (cap > 0) {
        {
            Prof pr(WL_K_MISC, (int64_t)B.cells);
            if (metric) hipLaunchKernelGGL((k_rg_peak<T, D, true>), grid, blk, 0, st, g, B, a, f, (const int *)label, (const int *)s.rowin, (long)cap, tab, (const unsigned long long *)ext);
            else hipLaunchKernelGGL((k_rg_peak<T, D, false>), grid, blk, 0, st, g, B, a, f, (const int *)label, (const int *)s.rowin, (long)cap, tab, (const unsigned long long *)ext);
            WL_HIP(hipGetLastError());
        }
        Prof pr(WL_K_SCALAR, 0);
        hipLaunchKernelGGL(k_rg_fin, tgrid, blk, 0, st, (long)cap, (const unsigned long long *)n, ext);
        WL_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace wl
