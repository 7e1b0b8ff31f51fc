// wl_integrals.h -- Integrals: the volume integrals of a velocity field in ONE sweep over u (waterlily_amd/integrals.py,
// wl_flow_integrals in include/wlhip.h).  Over the cells I of inside(p) (z-slabs: the owned interior planes), with
// d(i,j) = ∂(i,j,I,u) of src/Metrics.jl:28-30, one row of 6 + D doubles:
//     0 E      sum 0.125 sum_i (u[I,i] + u[I+d_i,i] - 2 U_i)^2          (ke, Metrics.jl:19-21)
//     1 Z      sum 0.5 |omega|^2      omega of Metrics.jl:60; D == 2: omega_3 = d(2,1) - d(1,2)
//     2 S      sum S_ij S_ij          S_ij = (d(i,j) + d(j,i)) / 2
//     3 div2   sum (sum_i d(i,i))^2
//     4 divmax max |sum_i d(i,i)|
//     5 umax   max_i |u[I,i]|
//     6.. P_i  sum (u[I,i] + u[I+d_i,i]) / 2
// Every operand is converted to double BEFORE the first operation and everything after is double, for Float32 and Float64
// flows alike (wl_metric rounds each cell to T because it fills a field of T; a sum over 10^8 cells must not inherit 10^8
// Float32 roundings).  Sums and maxima are reduced in a fixed order -- per thread along its column, wavefront, workgroup,
// then the partials of the workgroups by one final workgroup -- so the same field gives the same bits, run to run; no
// floating-point atomics.  A NaN in u surfaces as NaN in the sums that read it; the maxima use RED_MAX's comparison
// (w > v ? w : v, false for NaN) from 0, so they skip NaN operands exactly as wl_max does.
//
// Mapping: the marching tiling of wl_common.h with the axes fixed to (x, y, z) -- a workgroup owns a 64x4 tile of the
// (x, y) plane and marches along z.  The stencil of a cell is a "plus" of each component, not the 3x3x3 cube:
//     u_x at (i..i+1, j-1..j+1, k) and (i..i+1, j, k+-1);  u_y at (i-1..i+1, j..j+1, k) and (i, j..j+1, k+-1);
//     u_z at (i-1..i+1, j, k..k+1) and (i, j+-1, k..k+1)
// A thread keeps three planes of its column in registers in the flow's own type (converted to double only at use: a
// Float32 flow stays in 32-bit registers): per plane it loads its own cell of every component and the row neighbours
// (j-1, j+1: 8 coalesced loads, the rows shared by the tile's wavefronts come from the CU's L1), takes the i-1 / i+1 values
// from the neighbouring lanes by DPP shifts, and only the first / last lane of the tile loads its own.  Each plane is
// loaded once per thread and used as k+1, k and k-1 of three consecutive cells; a z chunk re-reads two planes.
#pragma once
#include "wl_common.h"

namespace wl {

__host__ __device__ constexpr bool ig_is_max(int q) { return q == 4 || q == 5; }

// block reduction of NV values per thread, value q by sum or (ig_is_max) by maximum; result valid in thread 0
template <int NV, int NW>
__device__ inline void ig_block_red(double (&v)[NV]) {
    __shared__ double sm[NV][NW];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        const double x = wave_red(v[q], ig_is_max(q) ? RED_MAX : RED_SUM);
        if (lane == 0) sm[q][w] = x;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) {
            double x = sm[q][0];
            for (int i = 1; i < NW; ++i) x = ig_is_max(q) ? (sm[q][i] > x ? sm[q][i] : x) : x + sm[q][i];
            v[q] = x;
        }
    }
}

// the marching tiling with a = x, b = y, c = z whatever the extents (mk_tiling moves the fast axis off an axis of extent 1;
// the lane shifts below need the lanes along x)
inline Tiling ig_tiling(const Range &R) {
    Tiling t;
    t.a = 0; t.b = 1; t.c = 2;
    t.na = R.hi[0] - R.lo[0] + 1; t.nb = R.hi[1] - R.lo[1] + 1; t.nc = R.hi[2] - R.lo[2] + 1;
    t.nta = (t.na + WL_BX - 1) / WL_BX;
    t.tpp = t.nta * ((t.nb + WL_BY - 1) / WL_BY);
    t.ptb = ((t.tpp + 7) / 8) * 8;
    if (t.ptb > WL_GRID) t.ptb = WL_GRID;
    int want = WL_GRID / t.ptb;
    if (want < 1) want = 1;
    if (want > t.nc) want = t.nc;
    t.clen = (t.nc + want - 1) / want;
    t.nchunk = (t.nc + t.clen - 1) / t.clen;
    t.nblk = t.ptb * t.nchunk;
    for (int d = 0; d < 3; ++d) t.lo[d] = R.lo[d];
    return t;
}

// one plane of a thread's column (i, j): the values of the "plus" above that lie in it
template <class T> struct IgPlane {
    T a0, a0x, a0m, a0mx, a0p, a0px;    // u_x at (i,j) (i+1,j) (i,j-1) (i+1,j-1) (i,j+1) (i+1,j+1)
    T a1, a1p, a1l, a1pl, a1r, a1pr;    // u_y at (i,j) (i,j+1) (i-1,j) (i-1,j+1) (i+1,j) (i+1,j+1)
    T a2, a2m, a2p, a2l, a2r;           // u_z at (i,j) (i,j-1) (i,j+1) (i-1,j) (i+1,j)
};
// o: offset of (i, j, k).  FULL = false: only what the planes k-1 / k+1 contribute to u_x and u_y (a0, a0x, a1, a1p).
// eL / eR: this lane is the first / last of its tile row -- its i-1 / i+1 neighbour is in no lane, it loads the value itself
// (issued first, so that the single-lane loads are in flight together with the coalesced ones).  Every lane of the
// wavefront must call this (DPP).
template <class T, int D, bool FULL>
__device__ __forceinline__ IgPlane<T> ig_load(const T *__restrict__ u, long sc, long s1, long o, bool eL, bool eR) {
    const T *u0 = u, *u1 = u + sc, *u2 = u + (D == 3 ? 2 : 1) * sc;   // (u2 is read when D == 3 only)
    IgPlane<T> P = {};
    T r0 = 0, r0m = 0, r0p = 0, r1 = 0, r1p = 0, r2 = 0, l1 = 0, l1p = 0, l2 = 0;
    if (eR) {
        r0 = u0[o + 1];
        if (FULL) { r0m = u0[o - s1 + 1]; r0p = u0[o + s1 + 1]; r1 = u1[o + 1]; r1p = u1[o + s1 + 1]; }
        if (FULL && D == 3) r2 = u2[o + 1];
    }
    if (FULL && eL) {
        l1 = u1[o - 1]; l1p = u1[o + s1 - 1];
        if (D == 3) l2 = u2[o - 1];
    }
    P.a0 = u0[o]; P.a1 = u1[o]; P.a1p = u1[o + s1];
    if (FULL) {
        P.a0m = u0[o - s1]; P.a0p = u0[o + s1];
        if (D == 3) { P.a2 = u2[o]; P.a2m = u2[o - s1]; P.a2p = u2[o + s1]; }
    }
    const T x0 = lane_dn1(P.a0);
    P.a0x = eR ? r0 : x0;
    if (FULL) {
        const T xm = lane_dn1(P.a0m), xp = lane_dn1(P.a0p);
        P.a0mx = eR ? r0m : xm; P.a0px = eR ? r0p : xp;
        const T yl = lane_up1(P.a1), ypl = lane_up1(P.a1p), yr = lane_dn1(P.a1), ypr = lane_dn1(P.a1p);
        P.a1l = eL ? l1 : yl; P.a1pl = eL ? l1p : ypl; P.a1r = eR ? r1 : yr; P.a1pr = eR ? r1p : ypr;
        if (D == 3) {
            const T zl = lane_up1(P.a2), zr = lane_dn1(P.a2);
            P.a2l = eL ? l2 : zl; P.a2r = eR ? r2 : zr;
        }
    }
    return P;
}

// the contributions of one cell: p / c / n = the planes k-1 / k / k+1 of its column (p, n unused when D == 2)
template <class T, int D>
__device__ __forceinline__ void ig_cell(const IgPlane<T> &p, const IgPlane<T> &c, const IgPlane<T> &n, double U0, double U1, double U2,
                                        double (&acc)[6 + D]) {
    const double c0 = (double)c.a0, c1 = (double)c.a1, c0x = (double)c.a0x, c1p = (double)c.a1p;
    const double c2 = (double)c.a2, n2 = (double)n.a2;
    // in-line derivatives, twice the cell-centred velocity
    const double d00 = c0x - c0, d11 = c1p - c1, d22 = D == 3 ? n2 - c2 : 0.0;
    const double m0 = c0 + c0x, m1 = c1 + c1p, m2 = D == 3 ? c2 + n2 : 0.0;
    // cross derivatives (Metrics.jl:29-30: the four operands left to right, then / 4)
    const double d01 = ((((double)c.a0p + (double)c.a0px) - (double)c.a0m) - (double)c.a0mx) * 0.25;
    const double d10 = ((((double)c.a1r + (double)c.a1pr) - (double)c.a1l) - (double)c.a1pl) * 0.25;
    const double w2 = d10 - d01, s01 = 0.5 * (d01 + d10);
    double zz = w2 * w2, ss = d00 * d00 + d11 * d11, so = s01 * s01;
    double dv = d00 + d11;
    const double e0 = m0 - 2.0 * U0, e1 = m1 - 2.0 * U1;
    double ee = e0 * e0 + e1 * e1;
    double um = fabs(c0);
    um = fabs(c1) > um ? fabs(c1) : um;
    if constexpr (D == 3) {
        const double d02 = ((((double)n.a0 + (double)n.a0x) - (double)p.a0) - (double)p.a0x) * 0.25;
        const double d12 = ((((double)n.a1 + (double)n.a1p) - (double)p.a1) - (double)p.a1p) * 0.25;
        const double d20 = ((((double)c.a2r + (double)n.a2r) - (double)c.a2l) - (double)n.a2l) * 0.25;
        const double d21 = ((((double)c.a2p + (double)n.a2p) - (double)c.a2m) - (double)n.a2m) * 0.25;
        const double w0 = d21 - d12, w1 = d02 - d20;
        const double s02 = 0.5 * (d02 + d20), s12 = 0.5 * (d12 + d21);
        zz = (w0 * w0 + w1 * w1) + zz;
        ss += d22 * d22;
        so += s02 * s02 + s12 * s12;
        dv += d22;
        const double e2 = m2 - 2.0 * U2;
        ee += e2 * e2;
        um = fabs(c2) > um ? fabs(c2) : um;
        acc[8] += 0.5 * m2;
    }
    acc[0] += 0.125 * ee;
    acc[1] += 0.5 * zz;
    acc[2] += ss + 2.0 * so;
    acc[3] += dv * dv;
    const double ad = fabs(dv);
    acc[4] = ad > acc[4] ? ad : acc[4];
    acc[5] = um > acc[5] ? um : acc[5];
    acc[6] += 0.5 * m0;
    acc[7] += 0.5 * m1;
}

// partials[q * gridDim.x + blockIdx.x] = the workgroup's value of column q
template <class T, int D>
__global__ __launch_bounds__(WL_BX *WL_BY) void k_integrals(G g, Tiling t, const T *__restrict__ u, double U0, double U1, double U2,
                                                            double *__restrict__ partials) {
    constexpr int NV = 6 + D;
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) acc[q] = 0.0;
    const int tx = threadIdx.x & (WL_BX - 1), ty = threadIdx.x / WL_BX;
    const int lb = logical_block(t.nblk);
    const int ch = lb / t.ptb, p0 = lb - ch * t.ptb;
    const int c0 = ch * t.clen, c1 = min(t.nc, c0 + t.clen);
    const long s1 = g.s[1], s2 = g.s[2], sc = g.sc;
    for (int pt = p0; pt < t.tpp && c0 < c1; pt += t.ptb) {
        const int ta = pt % t.nta, tb = pt / t.nta;
        const int ia = ta * WL_BX + tx, ib = tb * WL_BY + ty;
        if (ib >= t.nb) continue;                        // a wavefront is one row: uniform
        // lanes beyond the row's end repeat its last cell (every lane takes part in the shifts) and contribute nothing
        const bool active = ia < t.na;
        const bool eL = tx == 0, eR = tx == WL_BX - 1 || ia >= t.na - 1;
        const long col = (long)(t.lo[0] + min(ia, t.na - 1)) + s1 * (long)(t.lo[1] + ib);
        if constexpr (D == 2) {
            const IgPlane<T> c = ig_load<T, D, true>(u, sc, s1, col, eL, eR);
            if (active) ig_cell<T, D>(c, c, c, U0, U1, U2, acc);
        } else {
            const int k0 = t.lo[2] + c0, k1 = t.lo[2] + c1;  // planes k0 .. k1-1; k0-1 and k1 exist (checked by the host)
            IgPlane<T> p = ig_load<T, D, false>(u, sc, s1, col + s2 * (k0 - 1), eL, eR);
            IgPlane<T> c = ig_load<T, D, true>(u, sc, s1, col + s2 * k0, eL, eR);
            for (int k = k0; k < k1; ++k) {
                const IgPlane<T> n = ig_load<T, D, true>(u, sc, s1, col + s2 * (k + 1), eL, eR);
                if (active) ig_cell<T, D>(p, c, n, U0, U1, U2, acc);
                p = c;
                c = n;
            }
        }
    }
    ig_block_red<NV, WL_BY>(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) partials[(long)q * gridDim.x + blockIdx.x] = acc[q];
    }
}

// final stage: one workgroup reduces the np partials of every column in a fixed order and writes the row
template <int NV>
__global__ __launch_bounds__(WL_FIN_T) void k_integrals_fin(const double *__restrict__ partials, int np, double *__restrict__ row) {
    double acc[NV];
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        double a = 0.0;
        for (int i = threadIdx.x; i < np; i += WL_FIN_T) {
            const double w = partials[(long)q * np + i];
            a = ig_is_max(q) ? (w > a ? w : a) : a + w;
        }
        acc[q] = a;
    }
    ig_block_red<NV, WL_FIN_T / 64>(acc);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NV; ++q) row[q] = acc[q];
    }
}

// two launches, nothing allocated, nothing communicated: a z-slab rank writes the row of its own planes (all zeros when it
// owns no interior plane).  That those planes have a halo plane on each side is the caller's check (wl_flow_integrals).
template <class T, int D>
int op_integrals(const G &g, const T *u, const double *U, double *partials, double *row) {
    constexpr int NV = 6 + D;
    const Range R = r_inside(g);
    int np = 0;
    if (R.count() > 0) {
        const Tiling t = ig_tiling(R);
        np = t.nblk;
        if ((long)NV * np > 4L * WL_MAXB) return fail(WL_E_ARG, "wl_flow_integrals: grid too large for the reduction scratch", __FILE__, __LINE__);
        Prof p(WL_K_MISC, R.count());
        hipLaunchKernelGGL((k_integrals<T, D>), dim3(np), dim3(WL_BX * WL_BY), 0, ctx().stream, g, t, u, U[0], U[1], D == 3 ? U[2] : 0.0,
                           partials);
        WL_HIP(hipGetLastError());
    }
    Prof p(WL_K_SCALAR, 0);
    hipLaunchKernelGGL((k_integrals_fin<NV>), dim3(1), dim3(WL_FIN_T), 0, ctx().stream, (const double *)partials, np, row);
    return (int)hipGetLastError();
}

}  // namespace wl
