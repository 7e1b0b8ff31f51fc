// wl_budget.h -- Budget: the time-averaged turbulent kinetic energy budget (waterlily_amd/budget.py; include/wlhip.h:
// wl_budget_update, wl_budget_terms).
//
// k_budget_update keeps CENTRAL moments of the cell-centred fluctuation incrementally, one update per time step, over the
// cells of inside().  With Uf, Pm the running means BEFORE the update (a MeanFlow's fields), eps = dt / (t - t0) and
// keep = 1 - eps, per cell I in double arithmetic, every operand converted first, one rounding to A per store:
//     d[J,i] = u[J,i] - Uf[J,i]                 a_i = 0.5 (d[I,i] + d[I+d_i,i])          q = p[I] - Pm[I]
//     h_ij = d(i,j,I,d) of Metrics.jl:28-30:    h_ii = d[I+d_i,i] - d[I,i]
//            h_ij = (d[I+d_j,i] + d[I+d_j+d_i,i] - d[I-d_j,i] - d[I-d_j+d_i,i]) / 4      (left to right)
//     s = sum_i a_i a_i;  gg = sum_i sum_j h_ij h_ij (i outer, j inner);  every sum ascending, added to the first term
//     T3_j <- (keep T3_j + ((keep eps (1 - 2 eps)) s) a_j) - (eps keep) (2 sum_i a_i R_ij + a_j sum_i R_ii)     (R old)
//     R_q  <- keep (R_q + (eps a_ia) a_ib)      PU_j <- keep (PU_j + (eps q) a_j)        GG <- keep (GG + eps gg)
// first: every moment becomes 0 and nothing is read.  The means are NOT advanced here: the thread of a neighbouring cell
// reads Uf at the faces of this one, so wl_meanflow_update follows as a second launch.
//
// Mapping: that of k_meanflow (wl_stats.h) -- lane = V = 16/sizeof(A) cells of a row from i = 1 (4 beside Float32 accumulators,
// 2 beside Float64 ones, whose Float32 flow is then read in 8-B pairs), wavefront = row segment, workgroup = 4 rows, marching
// along z over the rows and planes of inside() -- but with ONE operand set per lane: the 13 accumulators, p and Pm of a plane
// are requested first and consumed after the stencil work of that plane.  k_meanflow's second set, in flight for plane k+1, does
// not fit beside the stencil's doubles (256 VGPRs and scratch when compiled so: profiles/budget_kernel_resources.txt); at 234-254
// VGPRs two waves per SIMD hide the latency instead.  The stencil reads of u and Uf (ten faces per component in 3-D) are row
// loads of the lane's own cells on the five (x component) or six (y, z) lines it touches plus one or two single elements
// beyond the row segment's ends; all but the first touch of a line are cache hits.  inside() starts at i = 1, so a row has no
// leading cell outside the vectors; the tail after the last whole vector (< V cells) is updated by extra workgroups of the
// same launch, one cell per thread, through the same code with W = 1.  No LDS, no atomics, no scratch.
//
// k_budget_terms turns the moments into the eight budget terms (summation orders: include/wlhip.h).
#pragma once
#include "wl_stats.h"

namespace wl {

// W consecutive values of type X with element alignment: one element, one 8-B vector (two floats beside two doubles) or 16-B
// vectors (W*sizeof(X) is 16 or 32)
typedef float wl_f2u __attribute__((ext_vector_type(2), aligned(4)));
template <class X, int W> struct BgRow {
    X v[W];
    __device__ __forceinline__ void load(const X *p) {
        if constexpr (W == 1) v[0] = p[0];
        else if constexpr (W * sizeof(X) == 8) {
            const wl_f2u q = *reinterpret_cast<const wl_f2u *>(p);
            __builtin_memcpy(v, &q, 8);
        } else {
            constexpr int VX = Vec16<X>::V;
#pragma unroll
            for (int q = 0; q < W / VX; ++q) {
                const VecA<X> x = VecA<X>::load(p + q * VX);
#pragma unroll
                for (int e = 0; e < VX; ++e) v[q * VX + e] = x.v[e];
            }
        }
    }
    __device__ __forceinline__ void store(X *p) const {
        if constexpr (W == 1) p[0] = v[0];
        else if constexpr (W * sizeof(X) == 8) {
            wl_f2u q;
            __builtin_memcpy(&q, v, 8);
            *reinterpret_cast<wl_f2u *>(p) = q;
        } else {
            constexpr int VX = Vec16<X>::V;
#pragma unroll
            for (int q = 0; q < W / VX; ++q) {
                VecA<X> x;
#pragma unroll
                for (int e = 0; e < VX; ++e) x.v[e] = v[q * VX + e];
                x.store(p + q * VX);
            }
        }
    }
};

struct BgArgs {
    long fsc, asc;       // component strides of the flow fields / of the accumulators
    double eps;
    int first;
};

// index of R_ij in ParaView's symmetric-tensor order (the inverse of mf_ia / mf_ib)
template <int D> __host__ __device__ constexpr int bg_sym(int i, int j) {
    if (i == j) return i;
    if (D == 2) return 2;
    const int lo = i < j ? i : j, hi = i < j ? j : i;
    return lo == 0 ? (hi == 1 ? 3 : 5) : 4;
}

template <class T, class A, int D> struct BgPtr {
    const T *u, *p;
    const A *Uf, *Pm;
    A *R, *PU, *GG, *T3;
};

// the accumulators (and p, Pm) of W cells
template <class T, class A, int D, int W> struct BgDat {
    static constexpr int NR = D * (D + 1) / 2;
    BgRow<T, W> p;
    BgRow<A, W> Pm, R[NR], PU[D], GG, T3[D];
};

template <class T, class A, int D, int W>
__device__ __forceinline__ BgDat<T, A, D, W> bg_load(const BgPtr<T, A, D> &f, long fo, long ao, const BgArgs &m) {
    BgDat<T, A, D, W> d;
    constexpr int NR = D * (D + 1) / 2;
    if (m.first) return d;
    d.p.load(f.p + fo);
    d.Pm.load(f.Pm + ao);
#pragma unroll
    for (int q = 0; q < NR; ++q) d.R[q].load(f.R + ao + q * m.asc);
#pragma unroll
    for (int c = 0; c < D; ++c) d.PU[c].load(f.PU + ao + c * m.asc);
    d.GG.load(f.GG + ao);
#pragma unroll
    for (int c = 0; c < D; ++c) d.T3[c].load(f.T3 + ao + c * m.asc);
    return d;
}

// d = u - Uf of component c on the line at flow offset fo / accumulator offset ao: the cells x = LO .. W-1+HI relative to the
// first of the W cells (LO in {0, -1}, HI in {0, 1}), out[x - LO]
template <class T, class A, int D, int W, int LO, int HI>
__device__ __forceinline__ void bg_line(const BgPtr<T, A, D> &f, const BgArgs &m, int c, long fo, long ao, double *out) {
    const T *u = f.u + c * m.fsc + fo;
    const A *U = f.Uf + c * m.asc + ao;
    BgRow<T, W> x;
    BgRow<A, W> y;
    x.load(u);
    y.load(U);
    if constexpr (LO < 0) out[0] = (double)u[-1] - (double)U[-1];
#pragma unroll
    for (int e = 0; e < W; ++e) out[e - LO] = (double)x.v[e] - (double)y.v[e];
    if constexpr (HI > 0) out[W - LO] = (double)u[W] - (double)U[W];
}

// the update of W cells of one row, the first at flow offset fo / accumulator offset ao
template <class T, class A, int D, int W>
__device__ __forceinline__ void bg_update(const G &g, const G &ga, const BgPtr<T, A, D> &f, long fo, long ao, const BgArgs &m,
                                          BgDat<T, A, D, W> &dat) {
    constexpr int NR = D * (D + 1) / 2;
    if (m.first) {
        BgRow<A, W> z;
#pragma unroll
        for (int e = 0; e < W; ++e) z.v[e] = (A)0;
#pragma unroll
        for (int q = 0; q < NR; ++q) z.store(f.R + ao + q * m.asc);
#pragma unroll
        for (int c = 0; c < D; ++c) z.store(f.PU + ao + c * m.asc);
        z.store(f.GG + ao);
#pragma unroll
        for (int c = 0; c < D; ++c) z.store(f.T3 + ao + c * m.asc);
        return;
    }
    const double eps = m.eps, keep = 1.0 - m.eps;
    double a[D][W], gg[W];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        if (c == 0) {
            // lines of the x component: the row itself and its neighbours in the other directions, x = 0 .. W
            double L[W + 1];
            bg_line<T, A, D, W, 0, 1>(f, m, 0, fo, ao, L);
#pragma unroll
            for (int e = 0; e < W; ++e) {
                a[0][e] = 0.5 * (L[e] + L[e + 1]);
                const double h = L[e + 1] - L[e];
                gg[e] = h * h;
            }
#pragma unroll
            for (int j = 1; j < D; ++j) {
                double P[W + 1], M[W + 1];
                bg_line<T, A, D, W, 0, 1>(f, m, 0, fo + g.s[j], ao + ga.s[j], P);
                bg_line<T, A, D, W, 0, 1>(f, m, 0, fo - g.s[j], ao - ga.s[j], M);
#pragma unroll
                for (int e = 0; e < W; ++e) {
                    const double h = (P[e] + P[e + 1] - M[e] - M[e + 1]) / 4.0;
                    gg[e] = gg[e] + h * h;
                }
            }
        } else {
            // component c != 0: the lines 0 and +d_c, x = -1 .. W, and their neighbours in the remaining direction
            double L0[W + 2], L1[W + 2];
            bg_line<T, A, D, W, -1, 1>(f, m, c, fo, ao, L0);
            bg_line<T, A, D, W, -1, 1>(f, m, c, fo + g.s[c], ao + ga.s[c], L1);
#pragma unroll
            for (int e = 0; e < W; ++e) a[c][e] = 0.5 * (L0[e + 1] + L1[e + 1]);
#pragma unroll
            for (int j = 0; j < D; ++j) {
                if (j == 0) {
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        const double h = (L0[e + 2] + L1[e + 2] - L0[e] - L1[e]) / 4.0;
                        gg[e] = gg[e] + h * h;
                    }
                } else if (j == c) {
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        const double h = L1[e + 1] - L0[e + 1];
                        gg[e] = gg[e] + h * h;
                    }
                } else {
                    double P0[W], P1[W], M0[W], M1[W];
                    bg_line<T, A, D, W, 0, 0>(f, m, c, fo + g.s[j], ao + ga.s[j], P0);
                    bg_line<T, A, D, W, 0, 0>(f, m, c, fo + g.s[j] + g.s[c], ao + ga.s[j] + ga.s[c], P1);
                    bg_line<T, A, D, W, 0, 0>(f, m, c, fo - g.s[j], ao - ga.s[j], M0);
                    bg_line<T, A, D, W, 0, 0>(f, m, c, fo - g.s[j] + g.s[c], ao - ga.s[j] + ga.s[c], M1);
#pragma unroll
                    for (int e = 0; e < W; ++e) {
                        const double h = (P0[e] + P1[e] - M0[e] - M1[e]) / 4.0;
                        gg[e] = gg[e] + h * h;
                    }
                }
            }
        }
    }
    const double c1 = keep * eps * (1.0 - 2.0 * eps), c2 = eps * keep;
#pragma unroll
    for (int e = 0; e < W; ++e) {
        double s = a[0][e] * a[0][e], tr = (double)dat.R[0].v[e];
#pragma unroll
        for (int i = 1; i < D; ++i) {
            s = s + a[i][e] * a[i][e];
            tr = tr + (double)dat.R[i].v[e];
        }
#pragma unroll
        for (int j = 0; j < D; ++j) {
            double sr = a[0][e] * (double)dat.R[bg_sym<D>(0, j)].v[e];
#pragma unroll
            for (int i = 1; i < D; ++i) sr = sr + a[i][e] * (double)dat.R[bg_sym<D>(i, j)].v[e];
            const double t3 = (double)dat.T3[j].v[e];
            dat.T3[j].v[e] = (A)((keep * t3 + c1 * s * a[j][e]) - c2 * (2.0 * sr + a[j][e] * tr));
        }
#pragma unroll
        for (int q = 0; q < NR; ++q)
            dat.R[q].v[e] = (A)(keep * ((double)dat.R[q].v[e] + eps * a[mf_ia<D>(q)][e] * a[mf_ib<D>(q)][e]));
        const double qp = (double)dat.p.v[e] - (double)dat.Pm.v[e];
#pragma unroll
        for (int j = 0; j < D; ++j) dat.PU[j].v[e] = (A)(keep * ((double)dat.PU[j].v[e] + eps * qp * a[j][e]));
        dat.GG.v[e] = (A)(keep * ((double)dat.GG.v[e] + eps * gg[e]));
    }
#pragma unroll
    for (int q = 0; q < NR; ++q) dat.R[q].store(f.R + ao + q * m.asc);
#pragma unroll
    for (int c = 0; c < D; ++c) dat.PU[c].store(f.PU + ao + c * m.asc);
    dat.GG.store(f.GG + ao);
#pragma unroll
    for (int c = 0; c < D; ++c) dat.T3[c].store(f.T3 + ao + c * m.asc);
}

// rows j = 1 .. n1-2 and planes klo .. khi (inside()); nv whole vectors per row from i = 1, nt = n0 - 2 - nv*V tail cells
template <class T, class A, int D>
__global__ __launch_bounds__(256) void k_budget_update(G g, G ga, BgPtr<T, A, D> f, BgArgs m, int klo, int khi, int nv, int ntx,
                                                       int tpp, int nblk, int clen) {
    constexpr int V = Vec16<A>::V;
    const int nrow = g.n[1] - 2;
    if ((int)blockIdx.x >= nblk) {
        // ---- the tail after the last whole vector: i = 1 + nv*V .. n0-2, one cell per thread
        const int nt = g.n[0] - 2 - nv * V;
        const long e = (long)(blockIdx.x - nblk) * blockDim.x + threadIdx.x;
        if (e >= (long)nrow * (khi - klo + 1) * nt) return;
        const long row = e / nt;
        const int i = 1 + nv * V + (int)(e - row * nt);
        const int j = 1 + (int)(row % nrow), k = klo + (int)(row / nrow);
        const long fo = g.at(i, j, k), ao = ga.at(i, j, k);
        BgDat<T, A, D, 1> d = bg_load<T, A, D, 1>(f, fo, ao, m);
        bg_update<T, A, D, 1>(g, ga, f, fo, ao, m, d);
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int lb, pslot;
    // (contiguous map, tpp = 0: every row of the budget update costs the same, body or not, so there is nothing to spread)
    tile_of(blockIdx.x, nblk, 0, 0, lb, pslot);
    (void)pslot;
    const int ch = lb / tpp, pt = lb - ch * tpp;
    const int q = (pt % ntx) * 64 + lane;                             // vector index within the row
    const int j = 1 + (pt / ntx) * S7_BY + wv;
    const int k0 = klo + ch * clen, k1 = min(khi + 1, k0 + clen);
    if (q >= nv || j > g.n[1] - 2 || k0 >= k1) return;
    const int i = 1 + q * V;
    const long fcol = (long)i + g.s[1] * (long)j, acol = (long)i + ga.s[1] * (long)j;
    const long fsz = g.s[2], asz = ga.s[2];
    for (int k = k0; k < k1; ++k) {
        const long fo = fcol + fsz * k, ao = acol + asz * k;
        BgDat<T, A, D, V> d = bg_load<T, A, D, V>(f, fo, ao, m);
        bg_update<T, A, D, V>(g, ga, f, fo, ao, m, d);
    }
}

template <class T, class A, int D>
int op_budget_update(const G &g, const G &ga, const T *u, const T *p, const A *Uf, const A *Pm, A *R, A *PU, A *GG, A *T3, double eps,
                     int first) {
    constexpr int V = Vec16<A>::V;
    const Range Ri = r_inside(g);
    if (Ri.count() <= 0) return 0;
    const int nown = Ri.hi[2] - Ri.lo[2] + 1;
    const int nv = (g.n[0] - 2) / V;                                  // whole vectors of a row (from i = 1)
    const int ntx = nv > 0 ? (nv + 63) / 64 : 0, nty = (g.n[1] - 2 + S7_BY - 1) / S7_BY;
    int tpp = 0, clen = 1, nchunk = 0;
    if (ntx > 0) {
        tpp = ((ntx * nty + 7) / 8) * 8;
        chunking(tpp, nown, 0, opt(WL_OPT_STREAM_GRID_K), &clen, &nchunk);
    }
    const long nblk = (long)tpp * nchunk;
    const long nsc = (long)(g.n[0] - 2 - nv * V) * (g.n[1] - 2) * nown;   // the tail of every row
    const long nb = nblk + (nsc + 255) / 256;
    if (nb > 0x7fffffffL) return fail(WL_E_ARG, "wl_budget_update: grid too large", __FILE__, __LINE__);
    const BgPtr<T, A, D> f{u, p, Uf, Pm, R, PU, GG, T3};
    const BgArgs m{g.sc, ga.sc, eps, first ? 1 : 0};
    Prof pr(WL_K_MISC, Ri.count());
    hipLaunchKernelGGL((k_budget_update<T, A, D>), dim3((unsigned)nb), dim3(256), 0, ctx().stream, g, ga, f, m, Ri.lo[2], Ri.hi[2], nv,
                       ntx, tpp, (int)nblk, clen);
    return (int)hipGetLastError();
}

// ---- the budget terms: one thread per cell of inside(); the cells of its rim (a neighbour outside inside()) get zeros
template <class A, int D>
int op_budget_terms(const G &g, const A *Uf, const A *R, const A *PU, const A *GG, const A *T3, double nu, A *out) {
    const G gg = g;
    return launch_range(WL_K_MISC, r_inside(g), [=] __device__(int i, int j, int k) {
        const long I = gg.at(i, j, k);
        const long sc = gg.sc;
        const int x[3] = {i, j, gg.kg(k)};
        bool rim = false;
#pragma unroll
        for (int d = 0; d < D; ++d) rim = rim || x[d] < 2 || x[d] > (d == 2 ? gg.nzg : gg.n[d]) - 3;
        if (rim) {
#pragma unroll
            for (int c = 0; c < 8; ++c) out[I + c * sc] = (A)0;
            return;
        }
        auto ke = [&](long J) {
            double s = (double)R[J];
#pragma unroll
            for (int d = 1; d < D; ++d) s = s + (double)R[J + d * sc];
            return 0.5 * s;
        };
        const double k0 = ke(I);
        double prod = 0, tt = 0, pt = 0, vd = 0, cv = 0;
#pragma unroll
        for (int a = 0; a < D; ++a) {
            const A *ua = Uf + a * sc;
#pragma unroll
            for (int b = 0; b < D; ++b) {
                const long sa = gg.s[a], sb = gg.s[b];
                const double G_ab = a == b ? (double)ua[I + sa] - (double)ua[I]
                                           : ((double)ua[I + sb] + (double)ua[I + sb + sa] - (double)ua[I - sb] - (double)ua[I - sb + sa]) / 4.0;
                const double t = (double)R[I + bg_sym<D>(a, b) * sc] * G_ab;
                prod = (a == 0 && b == 0) ? t : prod + t;
            }
        }
#pragma unroll
        for (int b = 0; b < D; ++b) {
            const long sb = gg.s[b];
            const double kp = ke(I + sb), km = ke(I - sb);
            const double t3 = ((double)T3[I + sb + b * sc] - (double)T3[I - sb + b * sc]) / 2.0;
            const double pu = ((double)PU[I + sb + b * sc] - (double)PU[I - sb + b * sc]) / 2.0;
            const double lap = (kp - 2.0 * k0) + km;
            const double Cb = 0.5 * ((double)Uf[I + b * sc] + (double)Uf[I + sb + b * sc]);
            const double adv = Cb * ((kp - km) / 2.0);
            tt = b == 0 ? t3 : tt + t3;
            pt = b == 0 ? pu : pt + pu;
            vd = b == 0 ? lap : vd + lap;
            cv = b == 0 ? adv : cv + adv;
        }
        const double t1 = -prod, t2 = nu * (double)GG[I], t3 = -0.5 * tt, t4 = -pt, t5 = nu * vd, t6 = -cv;
        out[I] = (A)k0;
        out[I + sc] = (A)t1;
        out[I + 2 * sc] = (A)t2;
        out[I + 3 * sc] = (A)t3;
        out[I + 4 * sc] = (A)t4;
        out[I + 5 * sc] = (A)t5;
        out[I + 6 * sc] = (A)t6;
        out[I + 7 * sc] = (A)(((((t1 - t2) + t3) + t4) + t5) + t6);
    });
}

}  // namespace wl
