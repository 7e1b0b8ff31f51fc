// wl_surface.h -- SurfaceLoads: pressure and viscous traction PER TRIANGLE of a mesh body, and their sums
// (waterlily_amd/surface.py; wl_surface_sample / wl_surface_totals in include/wlhip.h).
//
// The band integrals of Metrics.jl (pressure_force :94, viscous_force :108) sum p n kern(d) over cells and never name a
// triangle.  Here every triangle t of the mesh, at the pose of one instant, gets (all in double, for either T):
//     x_v = Ainv (xi_v - b)  (x_v = xi_v for the identity map),  x_c = (x_a + x_b + x_c) / 3,
//     S = 1/2 (x_b - x_a) x (x_c - x_a)  (= area * outward normal, grid units of x),  n = S / |S|,
//     V_b = -Ainv (dA x_c + db)          (mesh_measure's V at the centroid; 0 for the identity map),
// one sample point x_s = x_c + delta n, in index coordinates X = x_s + 1.5 (wl_interp's convention), and there
//     p_t    = interp(X, p)
//     G_ij   = u_i(X + e_j/2) - u_i(X - e_j/2)     (u_i as probe_vel takes it: component i at + e_i/2; the central difference
//                                                    of the interpolant over one cell)
//     tau_i  = -nu sum_j (G_ij + G_ji) n_j          (the integrand of viscous_force, Metrics.jl:116-119)
// so that p_t S is the triangle's pressure load and tau |S| its viscous load, with the signs of the project's pressure_force /
// viscous_force (not negated).  19 interpolations per triangle, all through probe_interp (wl_probe.h): the out-of-range rule
// (NaN, in that triangle's entries only) and the z-slab ownership of every single entry are wl_interp's.  p_t and tau are
// linear in the entries, so each rank writes a partial row and the sum over the ranks is the value; the geometry is the same
// on every rank.  The optional running mean m <- m + w (v - m) of the four sampled values (first: m = v, m not read) is linear
// too.
//
// Mapping: one thread per triangle, 64-thread workgroups.  The twelve doubles of a record that are read (240-byte stride) are
// uncoalesced, 96 of the 19 * 8 * sizeof(T) + 96 + 104 bytes a triangle moves; the 152 corner loads are scattered over up to
// 76 cache lines and dominate.  At 10^3 .. 10^5 triangles the launch is latency-bound, not bandwidth-bound: one wavefront
// per workgroup spreads 1 280 triangles over 20 CUs instead of 5, and staging records through LDS would save none of the
// dependent corner loads (profiles/surface_512_f32.txt).
//
// Totals: 12 sums over the triangles -- Fp = sum p_t S, Fv = sum tau |S|, Mp = sum (x_c - x0) x p_t S,
// Mv = sum (x_c - x0) x tau |S| -- per thread in ascending triangle order with a fixed stride, wavefront, workgroup, then one
// final workgroup: a fixed order, no floating-point atomics, the same rows give the same bits; a NaN row makes the sums NaN.
#pragma once
#include "wl_mesh.h"
#include "wl_probe.h"

namespace wl {

constexpr int SURF_BLOCK = 64;       // sample: one wavefront per workgroup
constexpr int SURF_RED_T = 256;      // totals: threads per workgroup
constexpr int SURF_RED_MAXB = 256;   // totals: workgroups at most (12 * 256 partials of the reduction scratch)

// one interp entry under wl_interp's ownership rule: the owner's value, 0 on every other rank
template <class T>
__device__ __forceinline__ double surf_entry(const G &g, const ProbeZ &z, const T *__restrict__ a, const double (&x)[3]) {
    return probe_owned<3>(z, x) ? probe_interp<T, 3>(g, a, x) : 0.0;
}

template <class T>
__global__ void __launch_bounds__(SURF_BLOCK) k_surface_sample(const G g, const ProbeZ z, const double *__restrict__ tri, int64_t nt,
                                                               const PoseDev P, const T *__restrict__ p, const T *__restrict__ u,
                                                               double delta, double nu, double *__restrict__ rows,
                                                               double *__restrict__ geom, double *__restrict__ mean, double w,
                                                               int first) {
    const int64_t t = (int64_t)blockIdx.x * SURF_BLOCK + threadIdx.x;
    if (t >= nt) return;
    const double *r = tri + t * MESH_TRI_STRIDE;
    double xv[3][3];
#pragma unroll
    for (int v = 0; v < 3; ++v) {
        const double q[3] = {r[3 * v], r[3 * v + 1], r[3 * v + 2]};
        if (P.ident) { xv[v][0] = q[0]; xv[v][1] = q[1]; xv[v][2] = q[2]; }
        else {
            const double e[3] = {q[0] - P.b[0], q[1] - P.b[1], q[2] - P.b[2]};
#pragma unroll
            for (int a = 0; a < 3; ++a) xv[v][a] = (P.Ainv[3 * a] * e[0] + P.Ainv[3 * a + 1] * e[1]) + P.Ainv[3 * a + 2] * e[2];
        }
    }
    double xc[3], e1[3], e2[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        xc[a] = ((xv[0][a] + xv[1][a]) + xv[2][a]) / 3.0;
        e1[a] = xv[1][a] - xv[0][a];
        e2[a] = xv[2][a] - xv[0][a];
    }
    const double S[3] = {0.5 * (e1[1] * e2[2] - e1[2] * e2[1]), 0.5 * (e1[2] * e2[0] - e1[0] * e2[2]), 0.5 * (e1[0] * e2[1] - e1[1] * e2[0])};
    const double area = sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]);
    const double n[3] = {S[0] / area, S[1] / area, S[2] / area};
    double Vb[3] = {0.0, 0.0, 0.0};
    if (!P.ident) {
        double dot[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) dot[a] = ((P.dA[3 * a] * xc[0] + P.dA[3 * a + 1] * xc[1]) + P.dA[3 * a + 2] * xc[2]) + P.db[a];
#pragma unroll
        for (int a = 0; a < 3; ++a) Vb[a] = -((P.Ainv[3 * a] * dot[0] + P.Ainv[3 * a + 1] * dot[1]) + P.Ainv[3 * a + 2] * dot[2]);
    }
    if (geom) {
        double *o = geom + t * 9;
#pragma unroll
        for (int a = 0; a < 3; ++a) { o[a] = xc[a]; o[3 + a] = S[a]; o[6 + a] = Vb[a]; }
    }
    double X[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) X[a] = (xc[a] + delta * n[a]) + 1.5;
    double v[4];
    v[0] = surf_entry<T>(g, z, p, X);
    double Gm[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            double hi[3] = {X[0], X[1], X[2]}, lo[3] = {X[0], X[1], X[2]};
            hi[j] = X[j] + 0.5;
            lo[j] = X[j] - 0.5;
            hi[i] = hi[i] + 0.5;                                    // probe_vel's stagger shift of component i
            lo[i] = lo[i] + 0.5;
            const T *ui = u + (long)i * g.sc;
            Gm[i][j] = surf_entry<T>(g, z, ui, hi) - surf_entry<T>(g, z, ui, lo);
        }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i)
        v[1 + i] = -nu * (((Gm[i][0] + Gm[0][i]) * n[0] + (Gm[i][1] + Gm[1][i]) * n[1]) + (Gm[i][2] + Gm[2][i]) * n[2]);
    double *o = rows + t * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) o[q] = v[q];
    if (mean) {
        double *m = mean + t * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (first) m[q] = v[q];
            else { const double m0 = m[q]; m[q] = m0 + w * (v[q] - m0); }
        }
    }
}

// partials[q * gridDim.x + blockIdx.x] = the workgroup's sum of column q over its triangles (ascending, stride = all threads)
__global__ void __launch_bounds__(SURF_RED_T) k_surface_totals(const double *__restrict__ rows, const double *__restrict__ geom, int64_t nt,
                                                               double x0, double y0, double z0, double *__restrict__ partials) {
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.0;
    const int64_t stride = (int64_t)gridDim.x * SURF_RED_T;
    for (int64_t t = (int64_t)blockIdx.x * SURF_RED_T + threadIdx.x; t < nt; t += stride) {
        const double *v = rows + t * 4, *gm = geom + t * 9;
        const double S[3] = {gm[3], gm[4], gm[5]};
        const double area = sqrt((S[0] * S[0] + S[1] * S[1]) + S[2] * S[2]);
        const double d[3] = {gm[0] - x0, gm[1] - y0, gm[2] - z0};
        const double fp[3] = {v[0] * S[0], v[0] * S[1], v[0] * S[2]};
        const double fv[3] = {v[1] * area, v[2] * area, v[3] * area};
#pragma unroll
        for (int a = 0; a < 3; ++a) { acc[a] += fp[a]; acc[3 + a] += fv[a]; }
        acc[6] += d[1] * fp[2] - d[2] * fp[1];
        acc[7] += d[2] * fp[0] - d[0] * fp[2];
        acc[8] += d[0] * fp[1] - d[1] * fp[0];
        acc[9] += d[1] * fv[2] - d[2] * fv[1];
        acc[10] += d[2] * fv[0] - d[0] * fv[2];
        acc[11] += d[0] * fv[1] - d[1] * fv[0];
    }
    block_red<12, SURF_RED_T / 64>(acc, RED_SUM);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 12; ++q) partials[(long)q * gridDim.x + blockIdx.x] = acc[q];
    }
}
// one workgroup adds the np partials of every column in ascending order of the workgroups
__global__ void __launch_bounds__(SURF_RED_T) k_surface_totals_fin(const double *__restrict__ partials, int np, double *__restrict__ out) {
    double acc[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = threadIdx.x < np ? partials[(long)q * np + threadIdx.x] : 0.0;
    block_red<12, SURF_RED_T / 64>(acc, RED_SUM);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < 12; ++q) out[q] = acc[q];
    }
}

template <class T>
int op_surface_sample(const G &g, const MeshDev &M, int64_t nt, const PoseDev &P, const T *p, const T *u, double delta, double nu,
                      double *rows, double *geom, double *mean, double w, int first) {
    const int64_t nb = (nt + SURF_BLOCK - 1) / SURF_BLOCK;
    Prof pr(WL_K_MISC, nt);
    hipLaunchKernelGGL((k_surface_sample<T>), dim3((unsigned)nb), dim3(SURF_BLOCK), 0, ctx().stream, g, mk_probe_z(g), M.tri, nt, P, p, u,
                       delta, nu, rows, geom, mean, w, first);
    return (int)hipGetLastError();
}

inline int op_surface_totals(const double *rows, const double *geom, int64_t nt, const double x0[3], double *partials, double *out) {
    int64_t nb = (nt + SURF_RED_T - 1) / SURF_RED_T;
    if (nb > SURF_RED_MAXB) nb = SURF_RED_MAXB;
    static_assert(SURF_RED_MAXB <= SURF_RED_T && 12 * SURF_RED_MAXB <= 4 * WL_MAXB, "partials of the surface totals do not fit");
    {
        Prof pr(WL_K_PFORCE, nt);
        hipLaunchKernelGGL(k_surface_totals, dim3((unsigned)nb), dim3(SURF_RED_T), 0, ctx().stream, rows, geom, nt, x0[0], x0[1], x0[2], partials);
        WL_HIP(hipGetLastError());
    }
    Prof pr(WL_K_SCALAR, 0);
    hipLaunchKernelGGL(k_surface_totals_fin, dim3(1), dim3(SURF_RED_T), 0, ctx().stream, (const double *)partials, (int)nb, out);
    return (int)hipGetLastError();
}

}  // namespace wl
