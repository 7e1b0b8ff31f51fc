// wl_stats.h -- MeanFlow: running time averages of u and p and their (co)variances, updated after a time step
// (waterlily_amd/stats.py).  Per element of the LOCAL arrays (ghost cells and slab halo planes included, pitch padding
// excluded), with eps = dt / (t - t0) computed by the host in Float64:
//     d_c   = u_c - U_c                       U_c   <- U_c + eps d_c
//     UU_ij <- (1 - eps) (UU_ij + eps d_i d_j)          (West's weighted incremental covariance)
// and the same for P and pp with d_p = p - P.  Arithmetic in double, one rounding to the accumulator type per store;
// `first` (eps == 1 after creation / reset): U = u, P = p, UU = pp = 0 and no accumulator is read.
//
// Mapping: the 16-B-vectorised, software-pipelined row streaming of k_rowvec (wl_stencil7.h) -- lane = V = 16/sizeof(T)
// cells of a row starting at i = 1 (128-B aligned in the padded layout, element-aligned in the dense one), wavefront =
// row segment, workgroup = 4 rows, marching along z with the loads of plane k+1 in flight while plane k is updated --
// over EVERY row j = 0..n1-1 and plane k = 0..n2-1.  The cells outside the whole vectors (i = 0 and the tail after the
// last whole vector, < V cells) are updated by extra workgroups of the same launch, one cell per thread: those cells sit
// on cache lines of their own in either layout, so a scalar access costs no extra line.  Absent statistics (UU / pp
// null) are template parameters: they cost neither bytes nor registers.
#pragma once
#include "wl_stencil7.h"

namespace wl {

// N consecutive values of type A moved as 16-B vectors (N*sizeof(A) is 16 or 32 bytes)
template <class A, int N> struct MfVec {
    A v[N];
    static constexpr int VA = Vec16<A>::V;
    __device__ __forceinline__ void load(const A *p) {
#pragma unroll
        for (int q = 0; q < N / VA; ++q) {
            const VecA<A> x = VecA<A>::load(p + q * VA);
#pragma unroll
            for (int e = 0; e < VA; ++e) v[q * VA + e] = x.v[e];
        }
    }
    __device__ __forceinline__ void store(A *p) const {
#pragma unroll
        for (int q = 0; q < N / VA; ++q) {
            VecA<A> x;
#pragma unroll
            for (int e = 0; e < VA; ++e) x.v[e] = v[q * VA + e];
            x.store(p + q * VA);
        }
    }
};

struct MfArgs {
    long fsc, asc;       // component strides of the flow fields / of the accumulators
    double eps;
    int first;
};

// ParaView's symmetric-tensor order: 3-D xx, yy, zz, xy, yz, xz; 2-D xx, yy, xy
template <int D> __host__ __device__ constexpr int mf_ia(int q) { return q < D ? q : (D == 2 ? 0 : (q == 3 ? 0 : (q == 4 ? 1 : 0))); }
template <int D> __host__ __device__ constexpr int mf_ib(int q) { return q < D ? q : (D == 2 ? 1 : (q == 3 ? 1 : 2)); }

// the update of one element: nu velocity components at flow offset fo / accumulator offset ao
template <class T, class A, int D, bool UU, bool PP>
__device__ __forceinline__ void mf_scalar(const T *u, const T *p, A *Um, A *Pm, A *UUm, A *ppm, long fo, long ao, const MfArgs &m) {
    constexpr int NU = D * (D + 1) / 2;
    double d[D];
#pragma unroll
    for (int c = 0; c < D; ++c) {
        const double x = (double)u[fo + c * m.fsc];
        if (m.first) { Um[ao + c * m.asc] = (A)x; d[c] = 0.0; continue; }
        const double U = (double)Um[ao + c * m.asc];
        d[c] = x - U;
        Um[ao + c * m.asc] = (A)(U + m.eps * d[c]);
    }
    if (UU) {
#pragma unroll
        for (int q = 0; q < NU; ++q) {
            A *o = UUm + ao + q * m.asc;
            *o = m.first ? (A)0 : (A)((1.0 - m.eps) * ((double)*o + m.eps * d[mf_ia<D>(q)] * d[mf_ib<D>(q)]));
        }
    }
    const double x = (double)p[fo];
    if (m.first) {
        Pm[ao] = (A)x;
        if (PP) ppm[ao] = (A)0;
        return;
    }
    const double P = (double)Pm[ao];
    const double dp = x - P;
    Pm[ao] = (A)(P + m.eps * dp);
    if (PP) ppm[ao] = (A)((1.0 - m.eps) * ((double)ppm[ao] + m.eps * dp * dp));
}

template <class T, class A, int D, bool UU, bool PP>
__global__ __launch_bounds__(256) void k_meanflow(G g, G ga, const T *__restrict__ u, const T *__restrict__ p, A *__restrict__ Um,
                                                  A *__restrict__ Pm, A *__restrict__ UUm, A *__restrict__ ppm, MfArgs m, int nv,
                                                  int ntx, int tpp, int nblk, int clen) {
    constexpr int V = Vec16<T>::V;
    constexpr int NU = D * (D + 1) / 2;
    if ((int)blockIdx.x >= nblk) {
        // ---- the cells outside the whole vectors: i = 0 and i = 1 + nv*V .. n0-1, one per thread
        const int ns = g.n[0] - nv * V;                               // 1 + tail
        const long e = (long)(blockIdx.x - nblk) * blockDim.x + threadIdx.x;
        const long nrow = (long)g.n[1] * g.n[2];
        if (e >= nrow * ns) return;
        const long row = e / ns;
        const int w = (int)(e - row * ns);
        const int i = w == 0 ? 0 : nv * V + w;
        const int j = (int)(row % g.n[1]), k = (int)(row / g.n[1]);
        mf_scalar<T, A, D, UU, PP>(u, p, Um, Pm, UUm, ppm, g.at(i, j, k), ga.at(i, j, k), m);
        return;
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int lb, pslot;
    // (contiguous map, tpp = 0: every row of the mean-flow update costs the same, body or not, so there is nothing to spread)
    tile_of(blockIdx.x, nblk, 0, 0, lb, pslot);
    (void)pslot;
    const int ch = lb / tpp, pt = lb - ch * tpp;
    const int q = (pt % ntx) * 64 + lane;                             // vector index within the row
    const int j = (pt / ntx) * S7_BY + wv;
    const int k0 = ch * clen, k1 = min(g.n[2], k0 + clen);
    if (q >= nv || j >= g.n[1] || k0 >= k1) return;
    const int i = 1 + q * V;
    const long fcol = (long)i + g.s[1] * (long)j, acol = (long)i + ga.s[1] * (long)j;
    const long fsz = g.s[2], asz = ga.s[2];
    const bool first = m.first != 0;
    const double eps = m.eps, keep = 1.0 - m.eps;
    struct Dat {
        VecA<T> u[D], p;
        MfVec<A, V> U[D], P, S[UU ? NU : 1], pp;
    };
    auto ld = [&](int k) {
        Dat d;
        const long fo = fcol + fsz * k, ao = acol + asz * k;
#pragma unroll
        for (int c = 0; c < D; ++c) d.u[c] = VecA<T>::load(u + fo + c * m.fsc);
        d.p = VecA<T>::load(p + fo);
        if (!first) {
#pragma unroll
            for (int c = 0; c < D; ++c) d.U[c].load(Um + ao + c * m.asc);
            d.P.load(Pm + ao);
            if (UU) {
#pragma unroll
                for (int s = 0; s < NU; ++s) d.S[s].load(UUm + ao + s * m.asc);
            }
            if (PP) d.pp.load(ppm + ao);
        }
        return d;
    };
    auto st = [&](int k, Dat &d) {
        const long ao = acol + asz * k;
        if (first) {
#pragma unroll
            for (int c = 0; c < D; ++c) {
#pragma unroll
                for (int e = 0; e < V; ++e) d.U[c].v[e] = (A)d.u[c].v[e];
                d.U[c].store(Um + ao + c * m.asc);
            }
#pragma unroll
            for (int e = 0; e < V; ++e) d.P.v[e] = (A)d.p.v[e];
            d.P.store(Pm + ao);
            MfVec<A, V> z;
#pragma unroll
            for (int e = 0; e < V; ++e) z.v[e] = (A)0;
            if (UU) {
#pragma unroll
                for (int s = 0; s < NU; ++s) z.store(UUm + ao + s * m.asc);
            }
            if (PP) z.store(ppm + ao);
            return;
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
            double dl[D];
#pragma unroll
            for (int c = 0; c < D; ++c) {
                const double U = (double)d.U[c].v[e];
                dl[c] = (double)d.u[c].v[e] - U;
                d.U[c].v[e] = (A)(U + eps * dl[c]);
            }
            if (UU) {
#pragma unroll
                for (int s = 0; s < NU; ++s)
                    d.S[s].v[e] = (A)(keep * ((double)d.S[s].v[e] + eps * dl[mf_ia<D>(s)] * dl[mf_ib<D>(s)]));
            }
            const double P = (double)d.P.v[e];
            const double dp = (double)d.p.v[e] - P;
            d.P.v[e] = (A)(P + eps * dp);
            if (PP) d.pp.v[e] = (A)(keep * ((double)d.pp.v[e] + eps * dp * dp));
        }
#pragma unroll
        for (int c = 0; c < D; ++c) d.U[c].store(Um + ao + c * m.asc);
        d.P.store(Pm + ao);
        if (UU) {
#pragma unroll
            for (int s = 0; s < NU; ++s) d.S[s].store(UUm + ao + s * m.asc);
        }
        if (PP) d.pp.store(ppm + ao);
    };
    // two operand sets alternate (loop unrolled by two): a set is never copied while its loads are outstanding
    Dat dA = ld(k0), dB;
    for (int k = k0; k < k1; k += 2) {
        dB = ld(min(k + 1, k1 - 1));
        st(k, dA);
        if (k + 1 < k1) {
            dA = ld(min(k + 2, k1 - 1));
            st(k + 1, dB);
        }
    }
}

template <class T, class A, int D, bool UU, bool PP>
inline int launch_meanflow(const G &g, const G &ga, const T *u, const T *p, A *U, A *P, A *S, A *pp, const MfArgs &m) {
    constexpr int V = Vec16<T>::V;
    const int nv = (g.n[0] - 1) / V;                                  // whole vectors of a row (from i = 1)
    const int ntx = nv > 0 ? (nv + 63) / 64 : 0, nty = (g.n[1] + S7_BY - 1) / S7_BY;
    int tpp = 0, clen = 1, nchunk = 0;
    if (ntx > 0) {
        tpp = ((ntx * nty + 7) / 8) * 8;
        chunking(tpp, g.n[2], 0, opt(WL_OPT_STREAM_GRID_K), &clen, &nchunk);
    }
    const long nblk = (long)tpp * nchunk;
    const long nsc = (long)(g.n[0] - nv * V) * g.n[1] * g.n[2];       // i = 0 and the tail of every row
    const long nb = nblk + (nsc + 255) / 256;
    if (nb > 0x7fffffffL) return fail(WL_E_ARG, "wl_meanflow_update: grid too large", __FILE__, __LINE__);
    Prof pr(WL_K_MISC, g.cells());
    hipLaunchKernelGGL((k_meanflow<T, A, D, UU, PP>), dim3((unsigned)nb), dim3(256), 0, ctx().stream, g, ga, u, p, U, P, S, pp, m, nv,
                       ntx, tpp, (int)nblk, clen);
    return (int)hipGetLastError();
}

template <class T, class A, int D>
int op_meanflow(const G &g, const G &ga, const T *u, const T *p, A *U, A *P, A *S, A *pp, double eps, int first) {
    const MfArgs m{g.sc, ga.sc, eps, first ? 1 : 0};
    if (S && pp) return launch_meanflow<T, A, D, true, true>(g, ga, u, p, U, P, S, pp, m);
    if (S) return launch_meanflow<T, A, D, true, false>(g, ga, u, p, U, P, S, pp, m);
    if (pp) return launch_meanflow<T, A, D, false, true>(g, ga, u, p, U, P, S, pp, m);
    return launch_meanflow<T, A, D, false, false>(g, ga, u, p, U, P, S, pp, m);
}

}  // namespace wl
