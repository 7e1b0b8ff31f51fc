// wl_render.h -- Render: slice and projection images of the flow, made on the device (waterlily_amd/render.py;
// wl_render_project / wl_render_shade in include/wlhip.h, which holds the definition).
//
// wl_render_project reduces a box of cells along one grid axis to an image of doubles.  The per-cell value -- a stored element, a
// face pair's mean, or one of the Metrics.jl field metrics -- is formed in registers from the flow arrays: no volume is written
// and none is read twice by a second pass.  The metric is metric_cell() below, the one function wl_metric's kernel calls too,
// so the image of a metric is the image of the field wl_metric would have stored, bit for bit.
//
// Two kernels, one launch per call, no atomics, nothing allocated:
//   k_render_march (axis 1 or 2): one thread per pixel, 64 lanes along x (every load of a wavefront is one coalesced row
//                                 segment), 4 image rows per workgroup; the thread walks the reduced axis in ascending order
//                                 with ONE accumulator.  The metric kinds re-read the three planes around the one they are on;
//                                 those reads are left to L2 / the Infinity Cache (no register window: tools/render_bench.py
//                                 measures what that costs).
//   k_render_row   (axis 0)     : one wavefront per x-row of the box; lane l takes the cells lo_0 + l, lo_0 + l + 64, ... in
//                                 ascending order, then the 64 partials are combined by the tree s_l (+)= s_{l+off},
//                                 off = 32, 16, ..., 1, over the lanes l < off.
// The order is part of the contract (tests/render_ref.py restates it with numpy loops and gets the same bits).
//
// wl_render_shade maps the image to RGBA8 through a 256-entry table: one thread per OUTPUT pixel, one 32-bit store each.
#pragma once
#include "wl_common.h"

namespace wl {

// ------------------------------------------------------------------------------------------ Metrics.jl, one cell
// One Jacobi rotation of a symmetric 3x3 matrix in the (p,q) plane (Golub & Van Loan 8.5): zeroes apq; dp, dq are the two
// diagonal entries, arp and arq the entries that couple the third index to p and to q.  A theta whose square overflows gives
// t = 0: apq is then far below an ulp of dq - dp and is dropped.
__host__ __device__ inline void jacobi_rot(double &dp, double &dq, double &apq, double &arp, double &arq) {
    if (apq == 0.0) return;
    const double th = (dq - dp) / (2.0 * apq);
    const double t = copysign(1.0, th) / (fabs(th) + sqrt(th * th + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c, x = arp;
    dp -= t * apq;
    dq += t * apq;
    apq = 0.0;
    arp = c * x - s * arq;
    arq = s * x + c * arq;
}
// middle eigenvalue of a symmetric 3x3 matrix -- lambda2 = eigvals(Hermitian(S^2+O^2))[2].  Cyclic Jacobi sweeps: every
// rotation is orthogonal to rounding, so the error stays a few eps * ||A|| however close two eigenvalues lie (solid
// rotation, plane shear, any axisymmetric region); the trigonometric closed form takes acos(r) at r = +-1 there and keeps
// only half the digits.  A diagonal matrix takes no rotation: its sorted diagonal comes back exactly.  Cyclic Jacobi
// converges quadratically: after 4 to 5 sweeps a 3x3 matrix is diagonal to working precision and further rotations change
// nothing.  The loop leaves early only when every off-diagonal entry is exactly zero (a diagonal input, or underflow), so a
// generic matrix runs all 8 sweeps: 24 rotations of 2 sqrt and 2 divisions each, per cell, in a post-processing kernel.
__host__ __device__ inline double sym3_mid_eig(double a00, double a01, double a02, double a11, double a12, double a22) {
    for (int sweep = 0; sweep < 8 && (a01 != 0.0 || a02 != 0.0 || a12 != 0.0); ++sweep) {
        jacobi_rot(a00, a11, a01, a02, a12);
        jacobi_rot(a00, a22, a02, a01, a12);
        jacobi_rot(a11, a22, a12, a01, a02);
    }
    double x = a00, y = a11, z = a22, t;
    if (x > y) { t = x; x = y; y = t; }
    if (y > z) { t = y; y = z; z = t; }
    if (x > y) { t = x; x = y; y = t; }
    return y;
}
// parameters of a metric as the kernels carry them: par (U of ke, z of omega_theta) and par2 (the centre of omega_theta)
struct MetricPar {
    double p[3], q[3];
};
inline MetricPar metric_par(int D, const double *par, const double *par2) {
    MetricPar m{{0, 0, 0}, {0, 0, 0}};
    if (par) for (int d = 0; d < D; ++d) m.p[d] = par[d];
    if (par2) for (int d = 0; d < D; ++d) m.q[d] = par2[d];
    return m;
}
// what `@inside out[I] = metric(I,u)` stores in cell I = (i, j, k) (k local), src/Metrics.jl:14-77: the value in T
template <class T, int D>
__device__ __forceinline__ T metric_cell(const G &gg, const T *__restrict__ u, int kind, int ipar, const MetricPar &mp, int i, int j, int k) {
    const long I = gg.at(i, j, k);
    const long S[3] = {gg.s[0], gg.s[1], gg.s[2]};
    const long SC = gg.sc;
    const double p0 = mp.p[0], p1 = mp.p[1], p2 = mp.p[2], q0 = mp.q[0], q1 = mp.q[1], q2 = mp.q[2];
    auto U = [&](int c, long off) -> T { return u[I + off + (long)c * SC]; };
    auto dudx = [&](int a, int b) -> T {   // Metrics.jl:28-31
        if (a == b) return U(a, S[a]) - U(a, 0);
        return (U(a, S[b]) + U(a, S[b] + S[a]) - U(a, -S[b]) - U(a, -S[b] + S[a])) / (T)4;
    };
    T res = 0;
    if (kind == WL_M_KE) {   // Metrics.jl:20-22
        const double UU[3] = {p0, p1, p2};
        double s = 0;   // (Float64 accumulation: exact for the reference's Float64 U, >= its precision for U=0)
        for (int c = 0; c < D; ++c) { const double v = (double)(T)(U(c, 0) + U(c, S[c])) - 2.0 * UU[c]; s += v * v; }
        res = (T)(0.125 * s);
    } else if (kind == WL_M_CURL) {   // Metrics.jl:54: permute((j,k)->d(j,CI(I,k),u), i), backward differences
        const int a = (ipar + 1) % 3, b = (ipar + 2) % 3;
        res = (U(b, 0) - U(b, -S[a])) - (U(a, 0) - U(a, -S[b]));
    } else if (D == 3) {
        T w[3];
        for (int c = 0; c < 3; ++c) { const int a = (c + 1) % 3, b = (c + 2) % 3; w[c] = dudx(b, a) - dudx(a, b); }   // Metrics.jl:60
        if (kind == WL_M_OMAG) {
            res = (T)sqrt((double)(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]));
        } else if (kind == WL_M_OTHETA) {   // Metrics.jl:72-76
            const double x[3] = {(double)i - 0.5 - q0, (double)j - 0.5 - q1, (double)(k + gg.kz0) - 0.5 - q2};
            const double th[3] = {p1 * x[2] - p2 * x[1], p2 * x[0] - p0 * x[2], p0 * x[1] - p1 * x[0]};
            const double n = sqrt(th[0] * th[0] + th[1] * th[1] + th[2] * th[2]);
            res = n <= 2.220446049250313e-16 * n ? (T)0 : (T)((th[0] * (double)w[0] + th[1] * (double)w[1] + th[2] * (double)w[2]) / n);
        } else {   // lambda2, Metrics.jl:41-45
            double J[3][3], M[3][3];
            for (int a = 0; a < 3; ++a) for (int b = 0; b < 3; ++b) J[a][b] = (double)dudx(a, b);
            for (int a = 0; a < 3; ++a)
                for (int b = a; b < 3; ++b) {
                    double m = 0;
                    for (int c = 0; c < 3; ++c) {
                        const double sa = 0.5 * (J[a][c] + J[c][a]), sb = 0.5 * (J[c][b] + J[b][c]);
                        const double oa = 0.5 * (J[a][c] - J[c][a]), ob = 0.5 * (J[c][b] - J[b][c]);
                        m += sa * sb + oa * ob;
                    }
                    M[a][b] = m;
                }
            res = (T)sym3_mid_eig(M[0][0], M[0][1], M[0][2], M[1][1], M[1][2], M[2][2]);
        }
    }
    return res;
}

// ------------------------------------------------------------------------------------------ projection
// the cells of one call: lo_d <= J_d < hi_d with LOCAL planes along z (the box clipped to the planes this rank owns); row0: the
// image row of the first visited plane when z is an image axis (the image keeps the box's global rows); cnt: the extent of the
// box along the reduced axis in the undecomposed array (MEAN divides by it on every rank: slab partials add up)
struct RenderBox {
    int lo[3], hi[3];
    int row0;
    double cnt;
};
struct RenderWhat {
    int kind, ipar, mode;
    MetricPar mp;
};

// the value of cell (i, j, k) as a double; METRIC selects the instantiation that carries the metric's registers
template <class T, int D, bool METRIC>
__device__ __forceinline__ double render_value(const G &g, const T *__restrict__ f, const RenderWhat &w, int i, int j, int k) {
    if (METRIC) return (double)metric_cell<T, D>(g, f, w.kind - WL_R_METRIC, w.ipar, w.mp, i, j, k);
    const long I = g.at(i, j, k);
    if (w.kind == WL_R_SCALAR) return (double)f[I];
    const T *fc = f + (long)w.ipar * g.sc;
    if (w.kind == WL_R_UCOMP) return (double)fc[I];
    return ((double)fc[I] + (double)fc[I + g.s[w.ipar]]) / 2.0;   // WL_R_CENTRE
}
// acc (+)= v, acc the EARLIER operand.  MAX / MIN / ABSMAX keep NaN as "nothing yet" and skip a NaN v (every comparison with
// it is false); strict comparisons: the first of two equal candidates stays.  SUM / MEAN add.
__device__ __forceinline__ double render_acc(int mode, double acc, double v) {
    if (mode == WL_R_MAX) return (v > acc || acc != acc) ? v : acc;
    if (mode == WL_R_MIN) return (v < acc || acc != acc) ? v : acc;
    if (mode == WL_R_ABSMAX) return (fabs(v) > fabs(acc) || acc != acc) ? v : acc;
    return acc + v;
}
__device__ __forceinline__ double render_init(int mode) { return mode >= WL_R_SUM ? 0.0 : __builtin_nan(""); }

// axis AX (1 or 2) reduced: pixel (a, b) = (x, the other axis)
template <class T, int D, int AX, bool METRIC>
__global__ __launch_bounds__(256) void k_render_march(const G g, const RenderBox B, const RenderWhat w, const T *__restrict__ f,
                                                     double *__restrict__ img, long ld) {
    constexpr int BA = AX == 1 ? 2 : 1;                        // the image's slow axis
    const int i = B.lo[0] + (int)blockIdx.x * 64 + (int)(threadIdx.x & 63);
    const int b = B.lo[BA] + (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (i >= B.hi[0] || b >= B.hi[BA]) return;
    double acc = render_init(w.mode);
    for (int c = B.lo[AX]; c < B.hi[AX]; ++c) {
        const int j = AX == 1 ? c : b, k = AX == 1 ? b : c;
        acc = render_acc(w.mode, acc, render_value<T, D, METRIC>(g, f, w, i, j, k));
    }
    if (w.mode == WL_R_MEAN) acc = acc / B.cnt;
    const long row = (AX == 1 ? B.row0 : 0) + (long)(b - B.lo[BA]);
    img[row * ld + (long)(i - B.lo[0])] = acc;
}
// axis 0 reduced: pixel (a, b) = (y, z), one wavefront per x-row
template <class T, bool METRIC>
__global__ __launch_bounds__(256) void k_render_row(const G g, const RenderBox B, const RenderWhat w, const T *__restrict__ f,
                                                   double *__restrict__ img, long ld) {
    const int lane = threadIdx.x & 63;
    const int nj = B.hi[1] - B.lo[1];
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (long)nj * (B.hi[2] - B.lo[2])) return;       // (whole wavefronts leave: the shuffles below see all 64 lanes)
    const int j = B.lo[1] + (int)(row % nj), k = B.lo[2] + (int)(row / nj);
    double acc = render_init(w.mode);
    for (int i = B.lo[0] + lane; i < B.hi[0]; i += 64) acc = render_acc(w.mode, acc, render_value<T, 3, METRIC>(g, f, w, i, j, k));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double up = __shfl_down(acc, off, 64);
        acc = render_acc(w.mode, acc, up);                     // (lanes >= off compute values nobody reads)
    }
    if (lane == 0) {
        if (w.mode == WL_R_MEAN) acc = acc / B.cnt;
        img[((long)B.row0 + (k - B.lo[2])) * ld + (j - B.lo[1])] = acc;
    }
}

// The LOCAL planes klo <= k < khi this rank visits of a box's GLOBAL planes lo2 <= z < hi2: the box, the planes it owns (the
// first rank of a ring takes the bottom ghost plane, which nobody owns), and the local array -- wl_isosurface's rule.  No plane:
// khi == klo.
inline void box_planes(const G &g, int lo2, int hi2, int *klo, int *khi) {
    int own_lo = g.kz0 + g.zlo, own_hi = g.kz0 + g.zhi;
    if (g.dist && g.zring && own_lo == 1) own_lo = 0;
    const int zlo = lo2 > own_lo ? lo2 : own_lo, zhi = hi2 < own_hi + 1 ? hi2 : own_hi + 1;
    *klo = zlo - g.kz0;
    *khi = zhi - g.kz0;
    if (*klo < 0) *klo = 0;
    if (*khi > g.n[2] - 1) *khi = g.n[2] - 1;
    if (*khi < *klo) *khi = *klo;
}

// lo / hi: the box in GLOBAL indices, already validated against the undecomposed extents (D == 2: lo[2] = 0, hi[2] = 1)
template <class T, int D>
int op_render_project(const G &g, const T *f, int kind, int ipar, const double *par, const double *par2, int axis, int mode,
                      const int lo[3], const int hi[3], double *img, int64_t ld) {
    RenderBox B;
    for (int d = 0; d < 3; ++d) { B.lo[d] = lo[d]; B.hi[d] = hi[d]; }
    B.row0 = 0;
    B.cnt = (double)(hi[axis] - lo[axis]);
    if (D == 3) {
        box_planes(g, lo[2], hi[2], &B.lo[2], &B.hi[2]);
        B.row0 = B.lo[2] + g.kz0 - lo[2];
    }
    RenderWhat w;
    w.kind = kind; w.ipar = ipar; w.mode = mode;
    w.mp = metric_par(D, par, par2);
    const bool metric = kind >= WL_R_METRIC;
    const int a = axis == 0 ? 1 : 0, b = axis == 2 ? 1 : 2;   // the image axes
    const long na = B.hi[a] - B.lo[a], nb = B.hi[b] - B.lo[b];
    if (na <= 0 || nb <= 0) return 0;                          // no pixel of this rank's
    Prof pr(WL_K_MISC, na * nb * (long)(B.hi[axis] - B.lo[axis]));
    hipStream_t st = ctx().stream;
    if constexpr (D == 3) {
        if (axis == 0) {
            const dim3 grid((unsigned)((na * nb + 3) / 4));
            if (metric) hipLaunchKernelGGL((k_render_row<T, true>), grid, dim3(256), 0, st, g, B, w, f, img, (long)ld);
            else hipLaunchKernelGGL((k_render_row<T, false>), grid, dim3(256), 0, st, g, B, w, f, img, (long)ld);
            return (int)hipGetLastError();
        }
        if (axis == 1) {
            const dim3 grid((unsigned)((na + 63) / 64), (unsigned)((nb + 3) / 4));
            if (metric) hipLaunchKernelGGL((k_render_march<T, 3, 1, true>), grid, dim3(256), 0, st, g, B, w, f, img, (long)ld);
            else hipLaunchKernelGGL((k_render_march<T, 3, 1, false>), grid, dim3(256), 0, st, g, B, w, f, img, (long)ld);
            return (int)hipGetLastError();
        }
    }
    const dim3 grid((unsigned)((na + 63) / 64), (unsigned)((nb + 3) / 4));
    if (metric) hipLaunchKernelGGL((k_render_march<T, D, 2, true>), grid, dim3(256), 0, st, g, B, w, f, img, (long)ld);
    else hipLaunchKernelGGL((k_render_march<T, D, 2, false>), grid, dim3(256), 0, st, g, B, w, f, img, (long)ld);
    return (int)hipGetLastError();
}

// ------------------------------------------------------------------------------------------ shading
struct ShadeArgs {
    long ld, ldm;
    int nx, ny, levels, zoom, flip_y, masked;
    double vmin, vmax, mask_lt;
    uint32_t mask_rgba, nan_rgba;                              // byte 0 = R (the little-endian word the store writes)
};
// the entry of the 256-entry colour table a value v (not NaN) takes: the one statement of wl_render_shade's rule (wl_scene_shade
// calls it too)
__device__ __forceinline__ int shade_index(double v, double vmin, double vmax, int levels) {
    const double t = (v - vmin) / (vmax - vmin);
    double x;
    if (levels == 0) {
        x = floor(t * 256.0);
        x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
    } else {
        const double n = (double)levels;
        double bnd = floor(t * n);
        bnd = bnd < 0.0 ? 0.0 : (bnd > n - 1.0 ? n - 1.0 : bnd);
        x = floor((bnd + 0.5) * 256.0 / n);
    }
    return (int)x;
}
__global__ __launch_bounds__(256) void k_render_shade(const ShadeArgs A, const double *__restrict__ img, const double *__restrict__ mask,
                                                     const uint8_t *__restrict__ lut, uint32_t *__restrict__ rgba) {
    const long W = (long)A.nx * A.zoom, H = (long)A.ny * A.zoom;
    const long ox = (long)blockIdx.x * 64 + (threadIdx.x & 63), oy = (long)blockIdx.y * 4 + (threadIdx.x >> 6);
    if (ox >= W || oy >= H) return;
    const long px = ox / A.zoom, pr = oy / A.zoom, py = A.flip_y ? A.ny - 1 - pr : pr;
    uint32_t out;
    const double v = img[py * A.ld + px];
    if (A.masked && mask[py * A.ldm + px] < A.mask_lt) out = A.mask_rgba;
    else if (v != v) out = A.nan_rgba;
    else {
        const uint8_t *e = lut + 4 * shade_index(v, A.vmin, A.vmax, A.levels);
        out = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16) | ((uint32_t)e[3] << 24);
    }
    rgba[oy * W + ox] = out;
}
inline int op_render_shade(const ShadeArgs &A, const double *img, const double *mask, const uint8_t *lut, uint8_t *rgba) {
    if (A.nx == 0 || A.ny == 0) return 0;
    const long W = (long)A.nx * A.zoom, H = (long)A.ny * A.zoom;
    Prof pr(WL_K_MISC, W * H);
    hipLaunchKernelGGL(k_render_shade, dim3((unsigned)((W + 63) / 64), (unsigned)((H + 3) / 4)), dim3(256), 0, ctx().stream, A, img, mask, lut,
                       (uint32_t *)rgba);
    return (int)hipGetLastError();
}

}  // namespace wl
