// wl_twopoint.h -- TwoPoint: correlations, structure functions and spectra along one grid axis, summed on the device
// (waterlily_amd/twopoint.py; wl_twopoint / wl_twopoint_scratch in include/wlhip.h, which holds the definition).  The fourth
// consumer of render_value() of wl_render.h and the first read-out that relates the value at x to the value at x + r: a line
// of the box along `axis` is formed once, kept in LDS as doubles, and used nsep times.  No float atomics, nothing allocated.
//
//   k_twopoint     : a workgroup of 4 wavefronts takes ROUNDS of L consecutive lines (tp_lines: 16, 8 or 4 by the line's length,
//                    so that two staged values per cell fit 64 KB).  All 256 threads stage the round: along axis 0 a line is an
//                    x-row and is loaded as it lies; along axis 1 or 2 consecutive lines are neighbours in x, so a thread takes
//                    line (e mod L) at position (e div L) -- every row segment of L cells is one coalesced load -- and stores it
//                    transposed, line by line, with the odd pitch ld that spreads those stores over the banks.  Then wavefront w
//                    takes the lines w, w + 4, ... of the round.  Lane l owns the separations l, l + 64, ...: it walks i = 0, 1,
//                    ... up the line with a = A(i) read as an LDS broadcast and b = B(i + r) at unit stride across the lanes,
//                    nine accumulators in registers.  Between rounds (and between groups of 64 separations) the accumulators
//                    rest in the wavefront's own [9][nsep] block of the caller's scratch, which at the end IS its partial.
//                    Every wavefront of the launch writes its block, the ones that never get a line +0.  The round loop depends
//                    on blockIdx alone, so both __syncthreads() of a round are reached by all 256 threads.
//   k_twopoint_fin : one thread per (column, separation) adds the blocks in ascending wavefront order from +0, forms N(r) by
//                    arithmetic, and overwrites the table or adds the total to it once.  A kernel boundary, no "last block"
//                    protocol.
// The order of every sum -- i ascending within a line, a wavefront's lines ascending, wavefronts ascending -- is the contract
// (tests/twopoint_ref.py restates it with numpy and gets the same bits).
#pragma once
#include "wl_render.h"

namespace wl {

constexpr int TP_MAX_LINE = WL_TP_MAX_LINE;   // 4 lines x 2 values x 1024 doubles = 64 KB of LDS
constexpr int TP_WG = 512;                    // the launch cap of k_twopoint: 2 workgroups of 4 wavefronts per CU
constexpr int TP_COLS = 10;                   // N and the nine sums
constexpr int TP_LDS = 65536;

// lines staged per round, from the line's length alone (the same with and without a second value: b == NULL gives the bits
// of b = a)
inline int tp_lines(int n) { return n <= 255 ? 16 : (n <= 511 ? 8 : 4); }

// the lines of one call: the box lo_d <= J_d < hi_d with LOCAL planes along z, cut along `axis` into nlines lines of n cells.
// Line q: axis 0: j = lo_1 + q mod e0, k = lo_2 + q div e0 (e0 = the box's y extent); axis 1 / 2: i = lo_0 + q mod e0, the
// remaining direction lo + q div e0 (e0 = the box's x extent).
struct TpBox {
    int lo[3], hi[3];
    int axis, n, nsep, periodic, e0;
    int L, ld, rounds;
    long nlines;
};
inline TpBox tp_box(const G &g, const int l[3], const int h[3], int axis, int nsep, int periodic) {
    TpBox B;
    for (int d = 0; d < 3; ++d) { B.lo[d] = l[d]; B.hi[d] = h[d]; }
    if (g.D == 3) box_planes(g, l[2], h[2], &B.lo[2], &B.hi[2]);
    B.axis = axis; B.nsep = nsep; B.periodic = periodic ? 1 : 0;
    B.n = B.hi[axis] - B.lo[axis];
    const int a = axis == 0 ? 1 : 0, b = axis == 2 ? 1 : 2;    // the two other directions, the faster one first
    B.e0 = B.hi[a] - B.lo[a];
    B.nlines = (long)B.e0 * (long)(B.hi[b] - B.lo[b]);
    B.L = tp_lines(B.n);
    B.ld = B.n | 1;
    if ((long)B.L * 2 * B.ld * (long)sizeof(double) > TP_LDS) B.ld = B.n;      // (n == 1024 alone: no room for the pad)
    B.rounds = (int)((B.nlines + B.L - 1) / B.L);
    return B;
}
inline unsigned tp_workgroups(const TpBox &B) { return (unsigned)(B.rounds < TP_WG ? B.rounds : TP_WG); }
inline int64_t tp_scratch_bytes(const TpBox &B) {
    return (int64_t)tp_workgroups(B) * 4 * (TP_COLS - 1) * (int64_t)B.nsep * (int64_t)sizeof(double);
}

struct TpAcc {
    double s[TP_COLS - 1];
};
// one pair: the nine sums of include/wlhip.h, every operation on its own
__device__ __forceinline__ void tp_pair(TpAcc &x, double a, double b) {
    const double d = b - a, d2 = d * d;
    x.s[0] += a;
    x.s[1] += b;
    x.s[2] += a * a;
    x.s[3] += b * b;
    x.s[4] += a * b;
    x.s[5] += d2;
    x.s[6] += d2 * d;
    x.s[7] += d2 * d2;
    x.s[8] += fabs(d) * d2;
}

// BK: 0 B is A, 1 a plain second value, 2 a metric
template <class T, int D, bool MA, int BK>
__global__ __launch_bounds__(256) void k_twopoint(const G g, const TpBox B, const RenderWhat wa, const RenderWhat wb, const T *__restrict__ fa,
                                                  const T *__restrict__ fb, double *__restrict__ part) {
    extern __shared__ double tp_lds[];                         // A: L lines of pitch ld; then B's, if it is given
    double *sa = tp_lds, *sb = BK ? tp_lds + B.L * B.ld : tp_lds;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int n = B.n, nsep = B.nsep;
    double *mine = part + ((size_t)blockIdx.x * 4 + w) * (size_t)((TP_COLS - 1) * nsep);
    bool first = true;
    for (int round = (int)blockIdx.x; round < B.rounds; round += (int)gridDim.x, first = false) {
        const long line0 = (long)round * B.L;
        const long left = B.nlines - line0;
        const int have = left < B.L ? (int)left : B.L;         // the lines of this round (the last one may be short)
        __syncthreads();                                       // the walks of the round before are over
        for (int e = tid; e < B.L * n; e += 256) {
            const int m = B.axis == 0 ? e / n : e % B.L, pos = B.axis == 0 ? e % n : e / B.L;
            if (m >= have) continue;
            const long q = line0 + m;
            const int q0 = (int)(q % B.e0), q1 = (int)(q / B.e0);
            int i, j, k;
            if (B.axis == 0) { i = B.lo[0] + pos; j = B.lo[1] + q0; k = B.lo[2] + q1; }
            else if (B.axis == 1) { i = B.lo[0] + q0; j = B.lo[1] + pos; k = B.lo[2] + q1; }
            else { i = B.lo[0] + q0; j = B.lo[1] + q1; k = B.lo[2] + pos; }
            sa[m * B.ld + pos] = render_value<T, D, MA>(g, fa, wa, i, j, k);
            if (BK) sb[m * B.ld + pos] = render_value<T, D, BK == 2>(g, fb, wb, i, j, k);
        }
        __syncthreads();
        for (int r0 = 0; r0 < nsep; r0 += 64) {
            const int r = r0 + lane;
            const bool on = r < nsep;
            TpAcc x;
#pragma unroll
            for (int c = 0; c < TP_COLS - 1; ++c) x.s[c] = (first || !on) ? 0.0 : mine[c * nsep + r];
            for (int m = w; m < have; m += 4) {
                const double *la = sa + m * B.ld, *lb = sb + m * B.ld;
                if (B.periodic) {
                    int p = on ? r : 0;                        // (r < nsep <= n)
#pragma unroll 4
                    for (int i = 0; i < n; ++i) {
                        tp_pair(x, la[i], lb[p]);
                        p = p + 1 == n ? 0 : p + 1;
                    }
                } else {
                    const int cnt = on ? n - r : 0;            // the pairs of this lane: i + r < n
                    const int all = n - r0 - 63 > 0 ? n - r0 - 63 : 0;     // so many pairs has every r of the group, r0 + 63 too:
#pragma unroll 4
                    for (int i = 0; i < all; ++i) tp_pair(x, la[i], lb[i + r]);       // no lane is asked (one that is not `on`
                    for (int i = all; i < n - r0; ++i)                                 // reads inside the line and drops its sums)
                        if (i < cnt) tp_pair(x, la[i], lb[i + r]);
                }
            }
            if (on) {
#pragma unroll
                for (int c = 0; c < TP_COLS - 1; ++c) mine[c * nsep + r] = x.s[c];
            }
        }
    }
}

// out[r * 10 + c]: c == 0: N(r) = lines * (periodic ? n : n - r); c >= 1: the blocks' entries added in ascending wavefront order
__global__ __launch_bounds__(256) void k_twopoint_fin(const double *__restrict__ part, int nw, int nsep, double lines, int n, int periodic,
                                                      int accumulate, double *__restrict__ out) {
    const int t = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (t >= TP_COLS * nsep) return;
    const int c = t / nsep, r = t % nsep;
    double s = 0.0;
    if (c == 0) s = lines * (double)(periodic ? n : n - r);
    else
        for (int v = 0; v < nw; ++v) s += part[((size_t)v * (TP_COLS - 1) + (size_t)(c - 1)) * (size_t)nsep + r];
    double *o = out + (size_t)r * TP_COLS + c;
    *o = accumulate ? *o + s : s;
}

// l / h: the box in GLOBAL indices, already validated (D == 2: l[2] = 0, h[2] = 1)
template <class T, int D>
int op_twopoint(const G &g, const wl_tp_value *a, const wl_tp_value *b, int axis, int nsep, int periodic, const int l[3], const int h[3],
                int accumulate, void *scratch, double *out) {
    const TpBox B = tp_box(g, l, h, axis, nsep, periodic);
    RenderWhat wa, wb;
    wa.kind = a->kind; wa.ipar = a->ipar; wa.mode = 0; wa.mp = metric_par(D, a->par, a->par2);
    wb = wa;
    if (b) { wb.kind = b->kind; wb.ipar = b->ipar; wb.mp = metric_par(D, b->par, b->par2); }
    hipStream_t st = ctx().stream;
    const unsigned nwg = B.nlines > 0 ? tp_workgroups(B) : 0u;
    double *part = (double *)scratch;
    if (nwg) {
        const size_t lds = sizeof(double) * (size_t)B.L * (size_t)B.ld * (b ? 2 : 1);
        const bool ma = wa.kind >= WL_R_METRIC;
        const int bk = !b ? 0 : (wb.kind >= WL_R_METRIC ? 2 : 1);
        const T *fa = (const T *)a->f, *fb = b ? (const T *)b->f : fa;
        const dim3 grid(nwg), blk(256);
        Prof pr(WL_K_MISC, B.nlines * (int64_t)B.n);
#define WL_TP_GO(MA, BK) hipLaunchKernelGGL((k_twopoint<T, D, MA, BK>), grid, blk, lds, st, g, B, wa, wb, fa, fb, part)
        if (ma) { if (bk == 0) WL_TP_GO(true, 0); else if (bk == 1) WL_TP_GO(true, 1); else WL_TP_GO(true, 2); }
        else { if (bk == 0) WL_TP_GO(false, 0); else if (bk == 1) WL_TP_GO(false, 1); else WL_TP_GO(false, 2); }
#undef WL_TP_GO
        WL_HIP(hipGetLastError());
    }
    Prof pr(WL_K_SCALAR, 0);
    hipLaunchKernelGGL(k_twopoint_fin, dim3((unsigned)((TP_COLS * nsep + 255) / 256)), dim3(256), 0, st, (const double *)part, (int)nwg * 4, nsep,
                       (double)B.nlines, B.n, B.periodic, accumulate ? 1 : 0, out);
    return (int)hipGetLastError();
}

}  // namespace wl
