// wl_mesh.h -- measure!(flow, body; t, eps) (src/Body.jl:31-53) for a body given as a CLOSED TRIANGLE MESH (3-D only).
//
// The mesh lives in xi = A(t) x + b(t) with A a similarity (A A^T = s^2 I, checked by the caller), so the distance in x is
// the distance in xi divided by s and its gradient is A^T grad_xi / s: no renormalisation.  Contract of mesh_sdf, in grid
// units of x and Float64 like the parametric families of wl_measure.h:
//   exact zone: where the true unsigned distance is < R/s (R = the mesh's exact radius, in xi units) the value is the
//               Euclidean distance to the closest point c of the surface, signed by sign((xi - c) . n_pseudo) with the
//               angle-weighted pseudonormal of the feature c lies on (face, edge, vertex: Baerentzen & Aanaes 2005), and
//               the normal is (xi - c)/d mapped back by A^T/s (the pseudonormal itself where |d| < 1e-9);
//   far zone  : elsewhere only the sign is right and |value| >= R/s -- all that measure! reads there (Body.jl:35,44).
//
// No per-point global search: a uniform grid of bins (edge h = R/2) over the bounding box dilated by R + h.  Per bin
//   * the ascending list (CSR) of the triangles within R + h*sqrt(3)/2 of the bin's CENTRE, i.e. every triangle that is
//     within R of any point of the bin;
//   * a sign byte: 0 where a triangle comes within h*sqrt(3)/2 of the centre ("crossed": every point of such a bin is
//     within h*sqrt(3) < R of the surface, so its list minimum is exact); otherwise the surface does not enter the bin,
//     the sign is one constant on it, and it is that of its face-connected component of uncrossed bins, found by ONE exact
//     brute-force query per component (so an outside pocket enclosed by crossed bins is still outside).
// A point whose list minimum is < R has its exact answer; one whose minimum is >= R lies in an uncrossed bin and takes the
// bin's sign; a point outside the dilated box is outside the body.
//
// Kernels keep the one-wavefront-per-x-row shape of k_measure_rows / k_measure_fill (the ballot / popcount band list
// depends on it).  With h = R/2 ~ 2 cells the 64 lanes of a row segment span ~32 bins, so a per-wave LDS stage of "the
// bin's triangles" has nothing to share; each lane walks its own bin's list, neighbouring lanes read the same 240-byte
// triangle records and hit in L1/L2.  Lanes whose bin list is empty (everything farther than R + h*sqrt(3) from the
// surface) do two loads and no arithmetic.
#pragma once
#include "wl_measure.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

namespace wl {

// per triangle: a, b, c (9 doubles), then 7 unit pseudonormals indexed by feature:
// 0 face, 1 edge ab, 2 edge bc, 3 edge ca, 4 vertex a, 5 vertex b, 6 vertex c
constexpr int MESH_TRI_STRIDE = 30;

struct MeshDev {
    const double *tri;
    const int *bin_start;
    const int *bin_tri;
    const signed char *bin_sign;
    double lo[3], h, inv_h, R;
    int nb[3];
};
struct PoseDev {
    double A[9], b[3], dA[9], db[3], Ainv[9];
    double s;        // A A^T = s^2 I
    int ident;
};

// closest point of triangle t to p (Ericson, Real-Time Collision Detection 5.1.5): returns the feature it lies on
__host__ __device__ inline int mesh_closest(const double *t, const double (&p)[3], double (&q)[3]) {
    double ab[3], ac[3], ap[3], bp[3], cp[3];
    for (int i = 0; i < 3; ++i) { ab[i] = t[3 + i] - t[i]; ac[i] = t[6 + i] - t[i]; ap[i] = p[i] - t[i]; }
    const double d1 = ab[0] * ap[0] + ab[1] * ap[1] + ab[2] * ap[2], d2 = ac[0] * ap[0] + ac[1] * ap[1] + ac[2] * ap[2];
    if (d1 <= 0 && d2 <= 0) { for (int i = 0; i < 3; ++i) q[i] = t[i]; return 4; }
    for (int i = 0; i < 3; ++i) bp[i] = p[i] - t[3 + i];
    const double d3 = ab[0] * bp[0] + ab[1] * bp[1] + ab[2] * bp[2], d4 = ac[0] * bp[0] + ac[1] * bp[1] + ac[2] * bp[2];
    if (d3 >= 0 && d4 <= d3) { for (int i = 0; i < 3; ++i) q[i] = t[3 + i]; return 5; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0 && d1 >= 0 && d3 <= 0) {
        const double v = d1 / (d1 - d3);
        for (int i = 0; i < 3; ++i) q[i] = t[i] + v * ab[i];
        return 1;
    }
    for (int i = 0; i < 3; ++i) cp[i] = p[i] - t[6 + i];
    const double d5 = ab[0] * cp[0] + ab[1] * cp[1] + ab[2] * cp[2], d6 = ac[0] * cp[0] + ac[1] * cp[1] + ac[2] * cp[2];
    if (d6 >= 0 && d5 <= d6) { for (int i = 0; i < 3; ++i) q[i] = t[6 + i]; return 6; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0 && d2 >= 0 && d6 <= 0) {
        const double w = d2 / (d2 - d6);
        for (int i = 0; i < 3; ++i) q[i] = t[i] + w * ac[i];
        return 3;
    }
    const double va = d3 * d6 - d5 * d4;
    if (va <= 0 && (d4 - d3) >= 0 && (d5 - d6) >= 0) {
        const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6));
        for (int i = 0; i < 3; ++i) q[i] = t[3 + i] + w * (t[6 + i] - t[3 + i]);
        return 2;
    }
    const double den = 1.0 / (va + vb + vc), v = vb * den, w = vc * den;
    for (int i = 0; i < 3; ++i) q[i] = t[i] + ab[i] * v + ac[i] * w;
    return 0;
}
__host__ __device__ inline void mesh_map(const PoseDev &P, const double (&x)[3], double (&xi)[3]) {
    if (P.ident) { xi[0] = x[0]; xi[1] = x[1]; xi[2] = x[2]; return; }
    for (int a = 0; a < 3; ++a) {
        double s = P.b[a];
        for (int c = 0; c < 3; ++c) s += P.A[3 * a + c] * x[c];
        xi[a] = s;
    }
}
// signed distance at x (grid units of x); n (if wanted): its gradient, filled in the exact zone only (else left alone)
__host__ __device__ inline double mesh_sdf(const MeshDev &M, const PoseDev &P, const double (&x)[3], double *n) {
    double xi[3];
    mesh_map(P, x, xi);
    int bi[3];
    for (int a = 0; a < 3; ++a) {
        const double f = floor((xi[a] - M.lo[a]) * M.inv_h);
        if (!(f >= 0 && f < (double)M.nb[a])) return M.R / P.s;          // outside the dilated box (or NaN): outside
        bi[a] = (int)f;
    }
    const long bin = (long)bi[0] + (long)M.nb[0] * ((long)bi[1] + (long)M.nb[1] * bi[2]);
    const int lo = M.bin_start[bin], hi = M.bin_start[bin + 1];
    double best = 1e300, bq[3] = {0, 0, 0};
    int bt = -1, bf = 0;
    for (int e = lo; e < hi; ++e) {
        const int ti = M.bin_tri[e];
        double q[3];
        const int f = mesh_closest(M.tri + (long)ti * MESH_TRI_STRIDE, xi, q);
        const double r0 = xi[0] - q[0], r1 = xi[1] - q[1], r2 = xi[2] - q[2];
        const double dd = r0 * r0 + r1 * r1 + r2 * r2;
        if (dd < best) { best = dd; bt = ti; bf = f; bq[0] = q[0]; bq[1] = q[1]; bq[2] = q[2]; }   // ties: the lowest index
    }
    double sgn;
    const double *pn = nullptr;
    double r[3] = {xi[0] - bq[0], xi[1] - bq[1], xi[2] - bq[2]};
    const bool exact = bt >= 0 && best < M.R * M.R;
    if (exact || (bt >= 0 && M.bin_sign[bin] == 0)) {
        pn = M.tri + (long)bt * MESH_TRI_STRIDE + 9 + 3 * bf;
        sgn = (r[0] * pn[0] + r[1] * pn[1] + r[2] * pn[2]) < 0 ? -1.0 : 1.0;
    } else {
        sgn = M.bin_sign[bin] < 0 ? -1.0 : 1.0;
    }
    if (!exact) {
        const double m = bt >= 0 ? sqrt(best) : M.R;
        return sgn * (m > M.R ? m : M.R) / P.s;
    }
    const double dxi = sgn * sqrt(best), d = dxi / P.s;
    if (n) {
        double nx[3];
        if (fabs(d) < 1e-9) { nx[0] = pn[0]; nx[1] = pn[1]; nx[2] = pn[2]; }
        else { nx[0] = r[0] / dxi; nx[1] = r[1] / dxi; nx[2] = r[2] / dxi; }
        if (P.ident) { n[0] = nx[0]; n[1] = nx[1]; n[2] = nx[2]; }
        else
            for (int c = 0; c < 3; ++c) n[c] = (P.A[c] * nx[0] + P.A[3 + c] * nx[1] + P.A[6 + c] * nx[2]) / P.s;   // A^T n / s
    }
    return d;
}
// measure(body, x, t; fastd2) (src/AutoBody.jl:115-131) with the mesh as the sdf: n = V = 0 where d^2 > fastd2
__host__ __device__ inline void mesh_measure(const MeshDev &M, const PoseDev &P, const double (&x)[3], double fastd2, double &d,
                                             double (&n)[3], double (&V)[3]) {
    for (int a = 0; a < 3; ++a) { n[a] = 0; V[a] = 0; }
    double g[3] = {0, 0, 0};
    d = mesh_sdf(M, P, x, g);
    if (d * d > fastd2) return;
    for (int a = 0; a < 3; ++a) n[a] = g[a];
    if (!P.ident) {
        double dot[3];
        for (int a = 0; a < 3; ++a) {
            double s = P.db[a];
            for (int c = 0; c < 3; ++c) s += P.dA[3 * a + c] * x[c];
            dot[a] = s;
        }
        for (int a = 0; a < 3; ++a) {
            double s = 0;
            for (int c = 0; c < 3; ++c) s += P.Ainv[3 * a + c] * dot[c];
            V[a] = -s;
        }
    }
}

// ---- kernels: the mesh twins of k_measure_rows / k_measure_fill / k_body_nds (same launch shape, same outputs) ----
template <class T>
__global__ __launch_bounds__(256) void k_mesh_rows(G g, MeshDev M, PoseDev P, T *sigma, T d2, int *rowcount, unsigned char *touched) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long nrows = (long)g.n[1] * g.n[2];
    if (row >= nrows) return;
    const int j = (int)(row % g.n[1]), k = (int)(row / g.n[1]);
    const int kg = k + g.kz0;
    int cnt = 0;
    bool any = false;
    const bool inside_row = j >= 1 && j <= g.n[1] - 2 && kg >= 1 && kg <= g.nzg - 2;
    if (inside_row) {
        for (int i = 1 + lane; i <= g.n[0] - 2; i += 64) {
            double x[3];
            cell_loc<3>(g, i, j, k, x);
            const T d = (T)mesh_sdf(M, P, x, nullptr);
            sigma[g.at(i, j, k)] = d;
            const bool band = d * d < d2;
            cnt += band ? 1 : 0;
            any = any || band || d < (T)0;
        }
    }
    const unsigned long long bm = __ballot(any);
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_down(cnt, o, 64);
    if (lane == 0) { rowcount[row] = cnt; touched[row] = bm ? 1 : 0; }
}
template <class T>
__global__ __launch_bounds__(256) void k_mesh_fill(G g, MeshDev M, PoseDev P, const T *sigma, T d2, double fast2, double eps, T *mu0, T *mu1,
                                                   T *V, const unsigned char *touched, const unsigned char *prev, bool full,
                                                   const long *rowoff, long *cand) {
    constexpr int D = 3;
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const long nrows = (long)g.n[1] * g.n[2];
    if (row >= nrows) return;
    const int j = (int)(row % g.n[1]), k = (int)(row / g.n[1]);
    const int kg = k + g.kz0;
    const bool inside_row = j >= 1 && j <= g.n[1] - 2 && kg >= 1 && kg <= g.nzg - 2;
    if (!inside_row) return;
    if (!full && !touched[row] && !prev[row]) return;
    long pos = rowoff[row];
    for (int i0 = 1; i0 <= g.n[0] - 2; i0 += 64) {
        const int i = i0 + lane;
        const bool ok = i <= g.n[0] - 2;
        const long I = g.at(ok ? i : 1, j, k);
        const T d = ok ? sigma[I] : (T)1e30;
        const bool band = ok && d * d < d2;
        const unsigned long long bm = __ballot(band);
        if (band) {
            const int rank = __popcll(bm & ((1ull << lane) - 1ull));
            cand[pos + rank] = (long)i + (long)g.n[0] * ((long)j + (long)g.n[1] * k);
        }
        pos += __popcll(bm);
        if (!ok) continue;
        if (band) {
            for (int c = 0; c < D; ++c) {
                double x[D], dc, n[D], Vc[D];
                cell_loc<D>(g, i, j, k, x);
                x[c] -= 0.5;
                mesh_measure(M, P, x, fast2, dc, n, Vc);
                const double q = wl_clamp1(dc / eps);
                V[I + (long)c * g.sc] = (T)Vc[c];
                mu0[I + (long)c * g.sc] = (T)wl_kern0(q);
                const double k1 = eps * wl_kern1(q);
#pragma unroll
                for (int jd = 0; jd < D; ++jd) mu1[I + (long)(c + D * jd) * g.sc] = (T)(k1 * n[jd]);
            }
        } else {
            const T m = d < (T)0 ? (T)0 : (T)1;
#pragma unroll
            for (int c = 0; c < D; ++c) {
                V[I + (long)c * g.sc] = (T)0;
                mu0[I + (long)c * g.sc] = m;
#pragma unroll
                for (int jd = 0; jd < D; ++jd) mu1[I + (long)(c + D * jd) * g.sc] = (T)0;
            }
        }
    }
}
__global__ __launch_bounds__(256) static void k_mesh_nds(G g, MeshDev M, PoseDev P, const long *cand, long n, double *out) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b >= n) return;
    const long lin = cand[b];
    const int i = (int)(lin % g.n[0]), j = (int)((lin / g.n[0]) % g.n[1]), k = (int)(lin / ((long)g.n[0] * g.n[1]));
    double x[3], d, nn[3], V[3];
    cell_loc<3>(g, i, j, k, x);
    mesh_measure(M, P, x, 1.0, d, nn, V);
    const double w = wl_kern(wl_clamp1(d));
    for (int c = 0; c < 3; ++c) out[b * 3 + c] = nn[c] * w;
}

}  // namespace wl

// ---- the handle: validated triangles, pseudonormals and bins on the host; device copies made at the first measure! ----
struct wl_mesh {
    int64_t nt = 0, nv = 0;
    std::vector<double> tri;
    std::vector<int> bin_start, bin_tri;
    std::vector<signed char> bin_sign;
    double lo[3] = {0, 0, 0}, h = 0, R = 0;
    int nb[3] = {0, 0, 0};
    int64_t max_per_bin = 0, crossed = 0, nonempty = 0;
    // device copies (created once, by the first call that needs them)
    mutable wl::Buf<double, wl::DevMem> d_tri;
    mutable wl::Buf<int, wl::DevMem> d_start, d_list;
    mutable wl::Buf<signed char, wl::DevMem> d_sign;
    size_t device_bytes() const {
        return tri.size() * sizeof(double) + (bin_start.size() + std::max<size_t>(bin_tri.size(), 1)) * sizeof(int) + bin_sign.size();
    }
    wl::MeshDev view(bool device) const {
        wl::MeshDev M;
        M.tri = device ? d_tri.get() : tri.data();
        M.bin_start = device ? d_start.get() : bin_start.data();
        M.bin_tri = device ? d_list.get() : bin_tri.data();
        M.bin_sign = device ? d_sign.get() : bin_sign.data();
        for (int a = 0; a < 3; ++a) { M.lo[a] = lo[a]; M.nb[a] = nb[a]; }
        M.h = h; M.inv_h = 1.0 / h; M.R = R;
        return M;
    }
};

namespace wl {

// build the host side of a mesh handle; returns nullptr on success, else what is wrong with the input
inline const char *mesh_build(wl_mesh &m, const double *vert, int64_t nv, const int32_t *tr, int64_t nt, double R) {
    for (int64_t q = 0; q < 3 * nv; ++q)
        if (!std::isfinite(vert[q])) return "wl_mesh_create: a vertex coordinate is not finite";
    for (int64_t q = 0; q < 3 * nt; ++q)
        if (tr[q] < 0 || tr[q] >= nv) return "wl_mesh_create: a triangle index is out of range";
    m.nt = nt; m.nv = nv; m.R = R;
    m.tri.assign((size_t)nt * MESH_TRI_STRIDE, 0.0);
    // face normals and corner angles
    std::vector<double> vn((size_t)nv * 3, 0.0);
    for (int64_t t = 0; t < nt; ++t) {
        double *o = &m.tri[(size_t)t * MESH_TRI_STRIDE];
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) o[3 * c + a] = vert[3 * (int64_t)tr[3 * t + c] + a];
        const double e1[3] = {o[3] - o[0], o[4] - o[1], o[5] - o[2]}, e2[3] = {o[6] - o[0], o[7] - o[1], o[8] - o[2]};
        double nf[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double l = std::sqrt(nf[0] * nf[0] + nf[1] * nf[1] + nf[2] * nf[2]);
        if (!(l > 0)) return "wl_mesh_create: degenerate (zero-area) triangle";
        for (int a = 0; a < 3; ++a) { nf[a] /= l; o[9 + a] = nf[a]; }
        for (int c = 0; c < 3; ++c) {   // angle at corner c, weight of the face normal in the vertex pseudonormal
            const double *p0 = o + 3 * c, *p1 = o + 3 * ((c + 1) % 3), *p2 = o + 3 * ((c + 2) % 3);
            const double u[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]}, v[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
            const double cr[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
            const double ang = std::atan2(std::sqrt(cr[0] * cr[0] + cr[1] * cr[1] + cr[2] * cr[2]), u[0] * v[0] + u[1] * v[1] + u[2] * v[2]);
            for (int a = 0; a < 3; ++a) vn[3 * (size_t)tr[3 * t + c] + a] += ang * nf[a];
        }
    }
    // edges: every undirected edge must belong to exactly two triangles, traversed once in each direction
    struct Edge { int32_t a, b; int32_t t, e, fwd; };
    std::vector<Edge> ed((size_t)nt * 3);
    for (int64_t t = 0; t < nt; ++t)
        for (int e = 0; e < 3; ++e) {
            const int32_t p = tr[3 * t + e], q = tr[3 * t + (e + 1) % 3];
            if (p == q) return "wl_mesh_create: degenerate (zero-area) triangle";
            ed[(size_t)t * 3 + e] = {std::min(p, q), std::max(p, q), (int32_t)t, e, p < q ? 1 : 0};
        }
    std::sort(ed.begin(), ed.end(), [](const Edge &x, const Edge &y) { return x.a != y.a ? x.a < y.a : (x.b != y.b ? x.b < y.b : x.t < y.t); });
    for (size_t q = 0; q < ed.size(); q += 2) {
        if (q + 1 >= ed.size() || ed[q].a != ed[q + 1].a || ed[q].b != ed[q + 1].b) return "wl_mesh_create: the mesh is not closed (an edge is not shared by exactly two triangles)";
        if (q + 2 < ed.size() && ed[q + 2].a == ed[q].a && ed[q + 2].b == ed[q].b) return "wl_mesh_create: the mesh is not closed (an edge is not shared by exactly two triangles)";
        if (ed[q].fwd == ed[q + 1].fwd) return "wl_mesh_create: inconsistently oriented triangles (a shared edge is traversed twice in the same direction)";
        const double *n0 = &m.tri[(size_t)ed[q].t * MESH_TRI_STRIDE + 9], *n1 = &m.tri[(size_t)ed[q + 1].t * MESH_TRI_STRIDE + 9];
        double s[3] = {n0[0] + n1[0], n0[1] + n1[1], n0[2] + n1[2]};
        const double l = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
        if (!(l > 1e-12)) return "wl_mesh_create: two triangles are folded flat onto each other along an edge";
        for (int a = 0; a < 3; ++a) {
            m.tri[(size_t)ed[q].t * MESH_TRI_STRIDE + 12 + 3 * ed[q].e + a] = s[a] / l;
            m.tri[(size_t)ed[q + 1].t * MESH_TRI_STRIDE + 12 + 3 * ed[q + 1].e + a] = s[a] / l;
        }
    }
    for (int64_t t = 0; t < nt; ++t)
        for (int c = 0; c < 3; ++c) {
            const double *s = &vn[3 * (size_t)tr[3 * t + c]];
            const double l = std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]);
            if (!(l > 1e-12)) return "wl_mesh_create: a vertex has no pseudonormal (its faces cancel)";
            for (int a = 0; a < 3; ++a) m.tri[(size_t)t * MESH_TRI_STRIDE + 21 + 3 * c + a] = s[a] / l;
        }
    // bins
    double bmin[3] = {1e300, 1e300, 1e300}, bmax[3] = {-1e300, -1e300, -1e300};
    for (int64_t t = 0; t < nt; ++t)
        for (int c = 0; c < 3; ++c)
            for (int a = 0; a < 3; ++a) {
                const double v = m.tri[(size_t)t * MESH_TRI_STRIDE + 3 * c + a];
                bmin[a] = std::min(bmin[a], v); bmax[a] = std::max(bmax[a], v);
            }
    const double h = R / 2;   // R > h*sqrt(3)
    m.h = h;
    double nbins = 1;
    for (int a = 0; a < 3; ++a) {
        m.lo[a] = bmin[a] - R - h;
        m.nb[a] = (int)std::ceil((bmax[a] + R + h - m.lo[a]) / h) + 1;
        nbins *= m.nb[a];
    }
    if (nbins > (double)(1 << 27)) return "wl_mesh_create: the mesh spans more than 2^27 bins of edge exact_radius/2";
    const size_t NB = (size_t)nbins;
    const double half = h * std::sqrt(3.0) / 2, slack = 1e-9 * (R + h);
    const double rad = R + half + slack, cross = half + slack;
    std::vector<int> count(NB + 1, 0);
    m.bin_sign.assign(NB, 1);
    std::vector<int64_t> pairs;   // bin * nt + tri, generated with tri ascending
    pairs.reserve((size_t)nt * 64);
    for (int64_t t = 0; t < nt; ++t) {
        const double *o = &m.tri[(size_t)t * MESH_TRI_STRIDE];
        int blo[3], bhi[3];
        for (int a = 0; a < 3; ++a) {
            const double tl = std::min(o[a], std::min(o[3 + a], o[6 + a])) - rad, th = std::max(o[a], std::max(o[3 + a], o[6 + a])) + rad;
            blo[a] = std::max(0, (int)std::floor((tl - m.lo[a]) / h));
            bhi[a] = std::min(m.nb[a] - 1, (int)std::floor((th - m.lo[a]) / h));
        }
        for (int kz = blo[2]; kz <= bhi[2]; ++kz)
            for (int jy = blo[1]; jy <= bhi[1]; ++jy)
                for (int ix = blo[0]; ix <= bhi[0]; ++ix) {
                    const double c[3] = {m.lo[0] + (ix + 0.5) * h, m.lo[1] + (jy + 0.5) * h, m.lo[2] + (kz + 0.5) * h};
                    double q[3];
                    mesh_closest(o, c, q);
                    const double dd = (c[0] - q[0]) * (c[0] - q[0]) + (c[1] - q[1]) * (c[1] - q[1]) + (c[2] - q[2]) * (c[2] - q[2]);
                    if (dd > rad * rad) continue;
                    const size_t bin = (size_t)ix + (size_t)m.nb[0] * ((size_t)jy + (size_t)m.nb[1] * kz);
                    pairs.push_back((int64_t)bin * nt + t);
                    count[bin + 1] += 1;
                    if (dd <= cross * cross) m.bin_sign[bin] = 0;
                }
    }
    if (pairs.size() > (size_t)0x7fffffff) return "wl_mesh_create: more than 2^31 bin entries";
    for (size_t b = 0; b < NB; ++b) {
        m.max_per_bin = std::max<int64_t>(m.max_per_bin, count[b + 1]);
        m.nonempty += count[b + 1] > 0;
        m.crossed += m.bin_sign[b] == 0;
        count[b + 1] += count[b];
    }
    m.bin_start = count;
    m.bin_tri.assign(pairs.size(), 0);
    {
        std::vector<int> fill(m.bin_start.begin(), m.bin_start.end() - 1);
        for (const int64_t pr : pairs) m.bin_tri[(size_t)fill[(size_t)(pr / nt)]++] = (int)(pr % nt);   // stable: tri ascending per bin
    }
    // sign of every face-connected component of uncrossed bins: one brute-force query at its first bin's centre
    std::vector<unsigned char> seen(NB, 0);
    std::vector<size_t> stack;
    for (size_t b0 = 0; b0 < NB; ++b0) {
        if (seen[b0] || m.bin_sign[b0] == 0) continue;
        const int ix0 = (int)(b0 % m.nb[0]), jy0 = (int)((b0 / m.nb[0]) % m.nb[1]), kz0 = (int)(b0 / ((size_t)m.nb[0] * m.nb[1]));
        const double c[3] = {m.lo[0] + (ix0 + 0.5) * h, m.lo[1] + (jy0 + 0.5) * h, m.lo[2] + (kz0 + 0.5) * h};
        double best = 1e300, br[3] = {0, 0, 0};
        const double *bn = nullptr;
        for (int64_t t = 0; t < nt; ++t) {
            const double *o = &m.tri[(size_t)t * MESH_TRI_STRIDE];
            double q[3];
            const int f = mesh_closest(o, c, q);
            const double r[3] = {c[0] - q[0], c[1] - q[1], c[2] - q[2]}, dd = r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
            if (dd < best) { best = dd; bn = o + 9 + 3 * f; br[0] = r[0]; br[1] = r[1]; br[2] = r[2]; }
        }
        const signed char sg = (br[0] * bn[0] + br[1] * bn[1] + br[2] * bn[2]) < 0 ? -1 : 1;
        stack.assign(1, b0);
        seen[b0] = 1;
        while (!stack.empty()) {
            const size_t b = stack.back();
            stack.pop_back();
            m.bin_sign[b] = sg;
            const int ix = (int)(b % m.nb[0]), jy = (int)((b / m.nb[0]) % m.nb[1]), kz = (int)(b / ((size_t)m.nb[0] * m.nb[1]));
            const int nbr[6][3] = {{ix - 1, jy, kz}, {ix + 1, jy, kz}, {ix, jy - 1, kz}, {ix, jy + 1, kz}, {ix, jy, kz - 1}, {ix, jy, kz + 1}};
            for (const auto &w : nbr) {
                if (w[0] < 0 || w[1] < 0 || w[2] < 0 || w[0] >= m.nb[0] || w[1] >= m.nb[1] || w[2] >= m.nb[2]) continue;
                const size_t q = (size_t)w[0] + (size_t)m.nb[0] * ((size_t)w[1] + (size_t)m.nb[1] * w[2]);
                if (seen[q] || m.bin_sign[q] == 0) continue;
                seen[q] = 1;
                stack.push_back(q);
            }
        }
    }
    return nullptr;
}

}  // namespace wl
