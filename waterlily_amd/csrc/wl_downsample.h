// wl_downsample.h -- Downsample: box-filtered, cropped volumes of the flow, made on the device (waterlily_amd/downsample.py;
// wl_downsample / wl_downsample_extent in include/wlhip.h, which holds the definition).  The 3-D counterpart of
// wl_render_project: a box of fine cells is cut into blocks of f^D cells and every block becomes one coarse cell.  The per-cell
// value is render_value() of wl_render.h -- a stored element, a face pair's mean or a Metrics.jl metric, formed in registers --
// so a downsampled metric costs one read of u and a store of 1/f^D of a field: no scratch volume, no second pass.
//
// One kernel, one launch per call, no atomics, no LDS, nothing allocated:
//   k_downsample: one wavefront takes 64 consecutive fine x of one block row of the box (64/f coarse cells; f divides 64, so a
//                 row that is no multiple of 64 leaves WHOLE coarse cells to the next wavefront); four coarse y rows per
//                 256-thread workgroup, the coarse z plane in blockIdx.z.  Every load of a wavefront is one coalesced row
//                 segment.  Lane l walks its column over the f x f rows of the block (z outer, y inner, ascending) with ONE
//                 accumulator; then the f lanes of a coarse cell are combined by the tree s_l (+)= s_{l+off}, off = f/2, ..., 1,
//                 the lower lane the earlier operand; the block's first lane scales (MEAN) and stores.
//                 WL_R_FACE visits only the block's low face of component c: c == 0: the block's first lane alone (the others
//                 keep the start value through the tree), c == 1: the block's first y row, c == 2: its first z plane.
//                 WL_R_SAMPLE: the block's first lane reads the block's first cell; no walk, no tree.
// The order is part of the contract (tests/downsample_ref.py restates it with numpy loops and gets the same bits).
#pragma once
#include "wl_render.h"

namespace wl {

// the blocks of one call: the block (I, J, K) of THIS RANK starts at the fine cell lo + f * (I, J, K) (lo[2] a LOCAL plane) and
// goes to out[((K * nc[1] + J) * nc[0] + I) * ntuple + c]
struct DownBox {
    int lo[3], nc[3];
    int f, fz;           // block edge; along z (1 when D == 2)
    int face;            // WL_R_FACE: the component whose low face is averaged; else -1
    int ntuple, c, out64;
    double scale;        // MEAN: the exact power of two 1 / (cells or faces of a block); else 1
};

// acc (+)= v with render_acc's rules; SAMPLE keeps the earlier operand
__device__ __forceinline__ double down_acc(int mode, double acc, double v) { return mode == WL_R_SAMPLE ? acc : render_acc(mode, acc, v); }

template <class T, int D, bool METRIC>
__global__ __launch_bounds__(256) void k_downsample(const G g, const DownBox B, const RenderWhat w, const T *__restrict__ f,
                                                   void *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int J = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (J >= B.nc[1]) return;                                  // (whole wavefronts leave: the shuffles below see all 64 lanes)
    const int K = (int)blockIdx.z;
    const int x = (int)blockIdx.x * 64 + lane;                 // fine x counted from the box's low corner
    const int a = x & (B.f - 1);                               // ... and inside its block
    const bool live = x < B.nc[0] * B.f;
    double acc = render_init(w.mode);
    if (live) {
        const int i = B.lo[0] + x, j0 = B.lo[1] + J * B.f, k0 = B.lo[2] + K * B.fz;
        if (w.mode == WL_R_SAMPLE) {
            if (a == 0) acc = render_value<T, D, METRIC>(g, f, w, i, j0, k0);
        } else if (B.face != 0 || a == 0) {
            const int ny = B.face == 1 ? 1 : B.f, nz = B.face == 2 ? 1 : B.fz;
            for (int kk = 0; kk < nz; ++kk)
                for (int jj = 0; jj < ny; ++jj) acc = render_acc(w.mode, acc, render_value<T, D, METRIC>(g, f, w, i, j0 + jj, k0 + kk));
        }
    }
    if (w.mode != WL_R_SAMPLE)
        for (int off = B.f >> 1; off > 0; off >>= 1) {
            const double up = __shfl_down(acc, off, 64);
            acc = render_acc(w.mode, acc, up);                 // (lanes a >= off compute values nobody reads)
        }
    if (live && a == 0) {
        if (w.mode == WL_R_MEAN) acc = acc * B.scale;
        const long o = (((long)K * B.nc[1] + J) * B.nc[0] + x / B.f) * B.ntuple + B.c;
        if (B.out64) ((double *)out)[o] = acc;
        else ((float *)out)[o] = (float)acc;
    }
}

// The coarse extents nc and the first coarse plane k0 of this rank for the box l..h (GLOBAL, validated, extents multiples of f),
// and klo: the LOCAL plane its first block starts on.  A rank emits the blocks that lie wholly within the planes it owns (the
// first rank of a ring also takes the bottom ghost plane, wl_isosurface's rule).  false: a boundary of the owned planes cuts a
// block.
inline bool down_extent(const G &g, int f, const int l[3], const int h[3], int nc[3], int *k0, int *klo) {
    nc[0] = (h[0] - l[0]) / f;
    nc[1] = (h[1] - l[1]) / f;
    nc[2] = 1;
    *k0 = 0;
    *klo = 0;
    if (g.D != 3) return true;
    int own_lo = g.kz0 + g.zlo;
    const int own_end = g.kz0 + g.zhi + 1;
    if (g.dist && g.zring && own_lo == 1) own_lo = 0;
    if (l[2] < own_lo && own_lo < h[2] && (own_lo - l[2]) % f != 0) return false;
    if (l[2] < own_end && own_end < h[2] && (own_end - l[2]) % f != 0) return false;
    int zs = l[2] > own_lo ? l[2] : own_lo, ze = h[2] < own_end ? h[2] : own_end;
    if (zs > h[2]) zs = h[2];
    if (ze < zs) ze = zs;
    nc[2] = (ze - zs) / f;
    *k0 = (zs - l[2]) / f;
    *klo = zs - g.kz0;
    return true;
}

template <class T, int D>
int op_downsample(const G &g, const T *f, int kind, int ipar, const double *par, const double *par2, int mode, int factor, const int lo[3],
                  const int nc[3], int out64, void *out, int ntuple, int c) {
    if (nc[0] <= 0 || nc[1] <= 0 || nc[2] <= 0) return 0;     // no block of this rank's
    DownBox B;
    for (int d = 0; d < 3; ++d) { B.lo[d] = lo[d]; B.nc[d] = nc[d]; }
    B.f = factor;
    B.fz = D == 3 ? factor : 1;
    B.face = kind == WL_R_FACE ? ipar : -1;
    B.ntuple = ntuple; B.c = c; B.out64 = out64;
    double n = 1.0;
    for (int d = 0; d < (kind == WL_R_FACE ? D - 1 : D); ++d) n *= (double)factor;
    B.scale = mode == WL_R_MEAN ? 1.0 / n : 1.0;
    RenderWhat w;
    w.kind = kind == WL_R_FACE ? WL_R_UCOMP : kind; w.ipar = ipar; w.mode = mode;
    w.mp = metric_par(D, par, par2);
    Prof pr(WL_K_MISC, (long)nc[0] * nc[1] * nc[2] * (mode == WL_R_SAMPLE ? 1L : (long)n));
    const dim3 grid((unsigned)(((long)nc[0] * factor + 63) / 64), (unsigned)((nc[1] + 3) / 4), (unsigned)nc[2]);
    if (kind >= WL_R_METRIC) hipLaunchKernelGGL((k_downsample<T, D, true>), grid, dim3(256), 0, ctx().stream, g, B, w, f, out);
    else hipLaunchKernelGGL((k_downsample<T, D, false>), grid, dim3(256), 0, ctx().stream, g, B, w, f, out);
    return (int)hipGetLastError();
}

}  // namespace wl
