// wl_forces.h -- Forces: the load of the fluid on a body in ONE sweep over its band cells (waterlily_amd/forces.py;
// wl_body_loads / wl_body_loads_mesh / wl_band_loads in include/wlhip.h).  nds = n * kern(clamp(d,-1,1)) of Metrics.jl:84-87
// is evaluated in registers: no nds array, no compaction, and the active leaf and the body velocity V are at hand.
//
// Per counted cell I (T = the flow's type; everything else Float64):
//     fp[c] = Float64(T(p[I] * nds[c]))                                            wl_pforce's term (Metrics.jl:96-99)
//     fv[c] = Float64(T(sum_j Float64(T(-nu * (d(c,j) + d(j,c)))) * nds[j]))       wl_vforce's term (Metrics.jl:107-119)
//     r     = loc(0,I) - x0                                                        (global z on a slab)
// and one row of FORCES_NV = 16 doubles per leaf, every column a plain sum over the leaf's cells:
//     0-2  Fp = fp          3-5  Fv = fv          6-8  Mp = r x fp      9-11  Mv = r x fv
//     12   Wp = fp . V      13   Wv = fv . V      14   ncells           15    A = |nds|
// D == 2: the z slots of Fp, Fv and the x, y slots of Mp, Mv are 0 and the scalar moment r_x f_y - r_y f_x is in slot z
// (wl_pmoment writes it into both of its two slots instead, like the reference's broadcast).
//
// Counted: a cell whose nds has a non-zero component -- w = kern(clamp(d)) != 0 with a defined normal, the cells the
// compaction `(nds != 0).any(1)` of the composed path keeps.  Any other cell is left BEFORE p or u is read.  On a z-slab a
// candidate counts only if its plane is owned and globally interior.
//
// Leaves: row q < nleaf sums the cells whose ACTIVE leaf (body_sdf's `act` at the cell centre) is q.  For a union of disjoint
// bodies that is the load on each body; across `-` and `∩` it only says which leaf's surface the cell's normal came from.
// Row nleaf = row 0 + row 1 + ... in that order, formed by the final stage.
//
// Order: a workgroup makes one masked pass over the list per leaf (16 accumulators per thread, whatever nleaf), a thread
// walks its cells grid-strided in ascending list order; wavefront, workgroup (block_red), then ONE final workgroup sums the
// workgroups' partials in ascending order.  No floating-point atomics: same inputs, same bits.  Two launches, no allocation
// (the partials live in the library's reduction scratch), no synchronisation.
#pragma once
#include "wl_measure.h"
#include "wl_mesh.h"

// du_i/dx_j at the centre of cell I (Metrics.jl:28-31), defined in wl_api.hip beside k_vforce, which shares it
template <class T> __device__ inline T dudx(const wl::G &g, const T *u, long I, int i, int j);

namespace wl {

constexpr int FORCES_NV = 16;
constexpr int FORCES_CAP = 512;   // workgroups of 256: (WL_BODY_MAXLEAF * FORCES_NV) * FORCES_CAP partials fit the 4 * WL_MAXB scratch
static_assert((long)WL_BODY_MAXLEAF * FORCES_NV * FORCES_CAP <= 4L * WL_MAXB, "forces partials exceed the reduction scratch");

// candidate (local dense column-major index) -> (i, j, k); false when a z-slab does not count the plane
template <int D> __device__ __forceinline__ bool forces_cand(const G &g, long lin, int (&ijk)[3]) {
    ijk[0] = (int)(lin % g.n[0]);
    ijk[1] = (int)((lin / g.n[0]) % g.n[1]);
    ijk[2] = (int)(lin / ((long)g.n[0] * g.n[1]));
    // not a cell with its whole stencil in the local array (wl_measure_fill lists none): not counted
    if (lin < 0 || ijk[0] < 1 || ijk[0] > g.n[0] - 2 || ijk[1] < 1 || ijk[1] > g.n[1] - 2) return false;
    if (D == 3 ? (ijk[2] < 1 || ijk[2] > g.n[2] - 2) : ijk[2] != 0) return false;
    if (D == 3) {
        const int k = ijk[2], kg = k + g.kz0;
        if (k < g.zlo || k > g.zhi || kg < 1 || kg > g.nzg - 2) return false;
    }
    return true;
}

// The three sources of (cell, nds, V, leaf).  cell(g, b, q, ...) -> list entry b is counted AND belongs to leaf q.
template <int D> struct LoadsBody {
    BodyDev B;
    const long *cand;
    static constexpr bool has_V = true;
    __device__ __forceinline__ bool cell(const G &g, long b, int q, long &I, int (&ijk)[3], double (&nds)[D], double (&V)[D]) const {
        if (!forces_cand<D>(g, cand[b], ijk)) return false;
        double x[D], d, nn[D];
        int act;
        cell_loc<D>(g, ijk[0], ijk[1], ijk[2], x);
        body_measure<D>(B, x, 1.0, d, nn, V, act);
        if (act != q) return false;
        const double w = wl_kern(wl_clamp1(d));
        bool any = false;
#pragma unroll
        for (int c = 0; c < D; ++c) { nds[c] = nn[c] * w; any = any || nds[c] != 0; }
        I = g.at(ijk[0], ijk[1], ijk[2]);
        return any;
    }
};
struct LoadsMesh {
    MeshDev M;
    PoseDev P;
    const long *cand;
    static constexpr bool has_V = true;
    __device__ __forceinline__ bool cell(const G &g, long b, int q, long &I, int (&ijk)[3], double (&nds)[3], double (&V)[3]) const {
        if (!forces_cand<3>(g, cand[b], ijk)) return false;
        double x[3], d, nn[3];
        cell_loc<3>(g, ijk[0], ijk[1], ijk[2], x);
        mesh_measure(M, P, x, 1.0, d, nn, V);
        const double w = wl_kern(wl_clamp1(d));
        bool any = false;
        for (int c = 0; c < 3; ++c) { nds[c] = nn[c] * w; any = any || nds[c] != 0; }
        I = g.at(ijk[0], ijk[1], ijk[2]);
        return any;
    }
};
template <int D> struct LoadsBand {   // idx: element offsets (wl_pforce's), nds[b*D + c]
    const int64_t *idx;
    const double *ndsv;
    static constexpr bool has_V = false;
    __device__ __forceinline__ bool cell(const G &g, long b, int q, long &I, int (&ijk)[3], double (&nds)[D], double (&V)[D]) const {
        bool any = false;
#pragma unroll
        for (int c = 0; c < D; ++c) { nds[c] = ndsv[b * D + c]; V[c] = 0; any = any || nds[c] != 0; }
        if (!any) return false;
        I = idx[b];
        const long k = D > 2 ? I / g.s[2] : 0, rem = D > 2 ? I - k * g.s[2] : I;
        const long j = rem / g.s[1];
        ijk[0] = (int)(rem - j * g.s[1]); ijk[1] = (int)j; ijk[2] = (int)k;
        if (I < 0 || ijk[0] < 1 || ijk[0] > g.n[0] - 2 || j < 1 || j > g.n[1] - 2) return false;   // not a cell of inside(p): its
        if (D == 3 && (k < 1 || k > g.n[2] - 2)) return false;                                      // stencil would leave the array
        return true;
    }
};

// the 16 contributions of one counted cell
template <class T, int D>
__device__ __forceinline__ void forces_cell(const G &g, const T *__restrict__ p, const T *__restrict__ u, T nu, long I, const int (&ijk)[3],
                                            double x0, double y0, double z0, const double (&nds)[D], const double (&V)[D],
                                            double (&acc)[FORCES_NV]) {
    const double pv = (double)p[I];
    double fp[D], fv[D];
#pragma unroll
    for (int c = 0; c < D; ++c) fp[c] = (double)(T)(pv * nds[c]);
#pragma unroll
    for (int i = 0; i < D; ++i) {
        double s = 0;
#pragma unroll
        for (int j = 0; j < D; ++j) {
            const T m = -nu * (T)(::dudx<T>(g, u, I, i, j) + ::dudx<T>(g, u, I, j, i));   // (-nu * grad2u)[i,j] in T
            s += (double)m * nds[j];
        }
        fv[i] = (double)(T)s;
    }
    const double rx = (double)ijk[0] - 0.5 - x0, ry = (double)ijk[1] - 0.5 - y0;
    double wp = 0, wv = 0, a2 = 0;
#pragma unroll
    for (int c = 0; c < D; ++c) {
        acc[c] += fp[c];
        acc[3 + c] += fv[c];
        wp += fp[c] * V[c];
        wv += fv[c] * V[c];
        a2 += nds[c] * nds[c];
    }
    if constexpr (D == 3) {
        const double rz = (double)(ijk[2] + g.kz0) - 0.5 - z0;
        acc[6] += ry * fp[2] - rz * fp[1];
        acc[7] += rz * fp[0] - rx * fp[2];
        acc[8] += rx * fp[1] - ry * fp[0];
        acc[9] += ry * fv[2] - rz * fv[1];
        acc[10] += rz * fv[0] - rx * fv[2];
        acc[11] += rx * fv[1] - ry * fv[0];
    } else {
        acc[8] += rx * fp[1] - ry * fp[0];
        acc[11] += rx * fv[1] - ry * fv[0];
    }
    acc[12] += wp;
    acc[13] += wv;
    acc[14] += 1.0;
    acc[15] += sqrt(a2);
}

// partials[(q * FORCES_NV + c) * gridDim.x + blockIdx.x] = the workgroup's sum of column c over the cells of leaf q
template <class T, int D, class SRC>
__global__ __launch_bounds__(256) void k_loads(G g, SRC src, const T *__restrict__ p, const T *__restrict__ u, T nu, long n, double x0,
                                               double y0, double z0, int nleaf, double *__restrict__ partials) {
    for (int q = 0; q < nleaf; ++q) {
        double acc[FORCES_NV];
#pragma unroll
        for (int c = 0; c < FORCES_NV; ++c) acc[c] = 0.0;
        for (long b = (long)blockIdx.x * 256 + threadIdx.x; b < n; b += (long)gridDim.x * 256) {
            long I = 0;
            int ijk[3];
            double nds[D], V[D];
            if (!src.cell(g, b, q, I, ijk, nds, V)) continue;
            forces_cell<T, D>(g, p, u, nu, I, ijk, x0, y0, z0, nds, V, acc);
        }
        block_red<FORCES_NV>(acc, RED_SUM);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < FORCES_NV; ++c) partials[((long)q * FORCES_NV + c) * gridDim.x + blockIdx.x] = acc[c];
        }
    }
}

// final stage: one workgroup sums the np partials of every (leaf, column) in ascending order, writes the nleaf leaf rows and
// the total row = row 0 + row 1 + ...; has_V false: Wp, Wv of every row are NaN (the source carries no body velocity)
__global__ __launch_bounds__(WL_FIN_T) static void k_loads_fin(const double *__restrict__ partials, int np, int nleaf, bool has_V,
                                                               double *__restrict__ rows) {
    double tot[FORCES_NV] = {};
    for (int q = 0; q < nleaf; ++q) {
        double acc[FORCES_NV];
#pragma unroll
        for (int c = 0; c < FORCES_NV; ++c) {
            double a = 0.0;
            for (int i = threadIdx.x; i < np; i += WL_FIN_T) a += partials[((long)q * FORCES_NV + c) * np + i];
            acc[c] = a;
        }
        block_red<FORCES_NV, WL_FIN_T / 64>(acc, RED_SUM);
        if (threadIdx.x == 0) {
            if (!has_V) acc[12] = acc[13] = __builtin_nan("");
#pragma unroll
            for (int c = 0; c < FORCES_NV; ++c) {
                rows[(long)q * FORCES_NV + c] = acc[c];
                tot[c] = q == 0 ? acc[c] : tot[c] + acc[c];
            }
        }
    }
    if (threadIdx.x == 0) {
#pragma unroll
        for (int c = 0; c < FORCES_NV; ++c) rows[(long)nleaf * FORCES_NV + c] = tot[c];
    }
}

template <class T, int D, class SRC>
int op_loads(const G &g, const SRC &src, const T *p, const T *u, double nu, long n, const double *x0, int nleaf, double *partials, double *rows) {
    int nb = (int)((n + 255) / 256);
    if (nb > FORCES_CAP) nb = FORCES_CAP;
    if (nb > 0) {
        Prof pr(WL_K_PFORCE, n);
        hipLaunchKernelGGL((k_loads<T, D, SRC>), dim3(nb), dim3(256), 0, ctx().stream, g, src, p, u, (T)nu, n, x0[0], x0[1], D == 3 ? x0[2] : 0.0,
                           nleaf, partials);
        WL_HIP(hipGetLastError());
    }
    Prof pr(WL_K_SCALAR, 0);
    hipLaunchKernelGGL(k_loads_fin, dim3(1), dim3(WL_FIN_T), 0, ctx().stream, (const double *)partials, nb, nleaf, SRC::has_V, rows);
    return (int)hipGetLastError();
}

}  // namespace wl
