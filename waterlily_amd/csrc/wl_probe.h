// wl_probe.h -- interp (src/util.jl:232-257) at lists of points, and a frozen-field Heun step of passive tracers
// (waterlily_amd/probes.py).
//
// interp, restated: a point x is given in the reference's 1-based INDEX coordinates of a cell-centred array (physical
// position + 1.5, loc at util.jl:160; global z on a z-slab).  With i = floor(x), y = x - i, the result is
//     s = 0;  for J in i:i+1 (CartesianIndices order, first index fastest):  s += a[J] * prod_d(J_d == i_d ? 1 - y_d : y_d)
// with the product taken in d order, every operation in double (the reference's `zero(T)` promotes to the points'
// Float64), whatever T is.  A staggered vector field samples component c at x + 0.5 e_c (one double addition).  A corner
// whose weight is exactly 0 is not read (x_d == n_d is in range); a point with a weighted corner outside the array (ghosts
// included) gives NaN -- the reference reads out of bounds there.
//
// z-slabs: every (point, component) entry is owned by ONE rank, the one whose owned global planes hold the entry's floor
// plane (after the shift); floor planes nobody owns (the z ghost planes of a ring) and planes outside the array go to the
// first / last rank.  The owner writes the value, every other rank 0, so a sum over the ranks is exact.  The owner's upper
// corner may sit in its first halo plane: u and p carry a current halo there when sim_step returns.
//
// Mapping: one thread per point (tracers: per particle), all its components and both Heun stages in registers.  Corner rows
// are scattered loads, one cache line per row for scattered points; points sorted by row (probes.sort_by_cell) put
// neighbouring lanes on the same lines (profiles/probes_512_f32.txt).
#pragma once
#include "wl_common.h"

namespace wl {

struct ProbeZ {          // z-slab ownership of the entries (dist == false: every entry is this rank's)
    bool dist, first, last;
    double glo, ghi;     // owned global planes, 0-based
};

inline ProbeZ mk_probe_z(const G &g) {
    ProbeZ z{g.dist, true, true, 0.0, 0.0};
    if (g.dist) {
        z.glo = (double)(g.kz0 + g.zlo);
        z.ghi = (double)(g.kz0 + g.zhi);
        z.first = g.kz0 + g.zlo <= 1;              // owns global plane 0 (1 on a ring, whose ghost planes nobody owns)
        z.last = g.kz0 + g.zhi >= g.nzg - 2;
    }
    return z;
}

// interp of one scalar component at 1-based index coordinate x (global z); NaN when a weighted corner lies outside
template <class T, int D>
__device__ __forceinline__ double probe_interp(const G &g, const T *__restrict__ a, const double (&x)[D]) {
    int i0[D];
    double y[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double f = floor(x[d]);
        const double ng = (double)(d == 2 ? g.nzg : g.n[d]);
        if (!(f >= 0.0 && f <= ng)) return __builtin_nan("");    // both corners outside (or x is NaN)
        i0[d] = (int)f - 1;                                     // 0-based lower corner
        y[d] = x[d] - f;
    }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < (1 << D); ++c) {
        double w = 1.0;
        long off = 0;
        bool in = true;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const int up = (c >> d) & 1;
            const double wd = up ? y[d] : 1.0 - y[d];
            w = d == 0 ? wd : w * wd;
            const int J = i0[d] + up;
            const int ng = d == 2 ? g.nzg : g.n[d];
            const int jl = d == 2 ? J - g.kz0 : J;                 // local plane (z-slab)
            in = in && J >= 0 && J < ng && jl >= 0 && jl < g.n[d];
            off += (long)jl * g.s[d];
        }
        if (w == 0.0) continue;
        if (!in) return __builtin_nan("");
        s = s + (double)a[off] * w;
    }
    return s;
}

// does this rank own the entry sampled at p (the point AFTER the stagger shift)?  See "z-slabs" above.
template <int D>
__device__ __forceinline__ bool probe_owned(const ProbeZ &z, const double (&p)[D]) {
    if (D != 3 || !z.dist) return true;
    const double fz = floor(p[D - 1]) - 1.0;                      // the entry's floor plane, 0-based global
    return (fz == fz) ? ((fz >= z.glo || z.first) && (fz <= z.ghi || z.last)) : z.first;
}

// out[q*ldo + c] = interp(x_q (+ 0.5 e_c), a_c), c < max(1, nc); nc = 0: scalar field
template <class T, int D>
__global__ void __launch_bounds__(256) k_interp(const G g, const ProbeZ z, const T *__restrict__ a, int nc,
                                                const double *__restrict__ xs, int64_t m, double *__restrict__ out, int64_t ldo) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    double x[D];
#pragma unroll
    for (int d = 0; d < D; ++d) x[d] = xs[q * D + d];
    const int ncomp = nc == 0 ? 1 : nc;
    for (int c = 0; c < ncomp; ++c) {
        double p[D];
#pragma unroll
        for (int d = 0; d < D; ++d) p[d] = (nc != 0 && d == c) ? x[d] + 0.5 : x[d];
        out[q * ldo + c] = probe_owned<D>(z, p) ? probe_interp<T, D>(g, a + (long)c * g.sc, p) : 0.0;
    }
}

// the staggered velocity at x: component c at x + 0.5 e_c
template <class T, int D>
__device__ __forceinline__ void probe_vel(const G &g, const T *__restrict__ u, const double (&x)[D], double (&v)[D]) {
#pragma unroll
    for (int c = 0; c < D; ++c) {
        double p[D];
#pragma unroll
        for (int d = 0; d < D; ++d) p[d] = d == c ? x[d] + 0.5 : x[d];
        v[c] = probe_interp<T, D>(g, u + (long)c * g.sc, p);
    }
}

// periodic direction of N interior cells: into [1.5, N + 1.5) (moves of less than one period per stage)
__device__ __forceinline__ double probe_wrap(double v, double N) {
    if (v < 1.5) v = v + N;
    if (v >= N + 1.5) v = v - N;
    return v;
}

// one Heun step on the frozen field: k1 = u(x), xs = x + dt k1, k2 = u(xs), x <- x + (dt/2)(k1 + k2).  Periodic directions
// wrap xs and x; a particle that leaves [1.5, N_d + 1.5] in another direction, or meets a NaN velocity, dies (all of its
// coordinates NaN); dead particles are skipped.
template <class T, int D>
__global__ void __launch_bounds__(256) k_tracer_advance(const G g, const T *__restrict__ u, double *__restrict__ xs, int64_t m,
                                                        double dt, int permask) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= m) return;
    double x[D];
    bool dead = false;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        x[d] = xs[q * D + d];
        dead = dead || x[d] != x[d];
    }
    if (dead) return;
    const double h = 0.5 * dt;
    double k1[D], k2[D], p[D];
    probe_vel<T, D>(g, u, x, k1);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        p[d] = x[d] + dt * k1[d];
        if ((permask >> d) & 1) p[d] = probe_wrap(p[d], (double)(g.n[d] - 2));
    }
    probe_vel<T, D>(g, u, p, k2);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const double N = (double)(g.n[d] - 2);
        double v = x[d] + h * (k1[d] + k2[d]);
        if ((permask >> d) & 1) v = probe_wrap(v, N);
        else dead = dead || !(v >= 1.5 && v <= N + 1.5);
        dead = dead || k1[d] != k1[d] || k2[d] != k2[d];
        p[d] = v;
    }
#pragma unroll
    for (int d = 0; d < D; ++d) xs[q * D + d] = dead ? __builtin_nan("") : p[d];
}

template <class T, int D>
int op_interp(const G &g, const T *a, int nc, const double *x, int64_t m, double *out, int64_t ldo) {
    if (m == 0) return 0;
    const int64_t nb = (m + 255) / 256;
    if (nb > 0x7fffffffL) return fail(WL_E_ARG, "wl_interp: too many points", __FILE__, __LINE__);
    Prof pr(WL_K_MISC, m);
    hipLaunchKernelGGL((k_interp<T, D>), dim3((unsigned)nb), dim3(256), 0, ctx().stream, g, mk_probe_z(g), a, nc, x, m, out, ldo);
    return (int)hipGetLastError();
}

template <class T, int D>
int op_tracer_advance(const G &g, const T *u, double *x, int64_t m, double dt, int permask) {
    if (m == 0) return 0;
    const int64_t nb = (m + 255) / 256;
    if (nb > 0x7fffffffL) return fail(WL_E_ARG, "wl_tracer_advance: too many particles", __FILE__, __LINE__);
    Prof pr(WL_K_MISC, m);
    hipLaunchKernelGGL((k_tracer_advance<T, D>), dim3((unsigned)nb), dim3(256), 0, ctx().stream, g, u, x, m, dt, permask);
    return (int)hipGetLastError();
}

}  // namespace wl
