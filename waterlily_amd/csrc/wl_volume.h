// wl_volume.h -- Volume: a scalar field ray-marched through Scene's camera and composited, front to back, over what Scene
// drew (waterlily_amd/volume.py; wl_scene_volume and wl_scene_average in include/wlhip.h, which holds the definition).
//
// One ray per pixel, in IEEE doubles one operation at a time (the library is built without contraction): the ray's end
// points come from the inverse camera, the samples lie at s_k = (k + 0.5) ds in NDC depth -- linear in eye depth along every
// ray, so the samples of all rays lie on common planes parallel to the picture plane -- and each sample is probe_interp
// (wl_probe.h) of the field, shade_index (wl_render.h) of the value, one opacity and one colour from two 256-entry tables.
// The depth buffer stops a ray at the surface its pixel shows.  No sqrt, no transcendental: tests/volume_ref.py restates the
// march with numpy scalars and gets acc and rgba bit for bit.
//
// Kernels (no LDS, no float atomics, nothing allocated):
//   k_scene_volume  : one wavefront per 8 x 8 tile of pixels (as k_scene_wave tiles a box), four tiles per workgroup.  The
//                     lanes start at the tile's smallest first k and step through the same k, so their eight corner rows fall
//                     in neighbouring rows of the field.  A tile whose rays all miss the box writes `base` and leaves after
//                     the setup.  A sample whose opacity is exactly 0 changes neither C nor T and skips the colour fetch.
//   k_scene_average : k_scene_resolve's block average without the key test (the volume pass has put the background in).
#pragma once
#include "wl_common.h"
#include "wl_probe.h"
#include "wl_scene.h"

namespace wl {

struct VolumeArgs {
    double mi[16];                                             // row-major inverse of the draw's M
    double ds, vmin, vmax, t_min;
    double blo[3], bhi[3];                                     // the cell centres of the box, in the frame x = J - 0.5
    int W, H, levels;
    uint32_t bg;                                               // byte 0 = R
};

// the world point of NDC depth z on the ray whose homogeneous point is h0 + z g
__device__ __forceinline__ void volume_point(const double (&h0)[4], const double (&g)[4], double z, double (&P)[3]) {
    const double w = h0[3] + z * g[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) P[d] = (h0[d] + z * g[d]) / w;
}
__device__ __forceinline__ bool volume_finite(const double (&P)[3]) {
    const double big = 1.79769313486231570815e308;
    return fabs(P[0]) <= big && fabs(P[1]) <= big && fabs(P[2]) <= big;   // (false for NaN and for +-inf)
}
__device__ __forceinline__ uint32_t volume_byte(double x) {
    x = floor(x + 0.5);
    x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);
    return (uint32_t)(x == x ? (int)x : 0);
}

// probe_interp's value (wl_probe.h: the same double operations in the same order, so the same bits) of a 3-D field that is not
// decomposed, with the eight corner loads in flight together.  probe_interp tests a corner's weight and bounds BEFORE it loads
// it, so a sample waits for eight trips to the cache one after the other, and a ray is a chain of such samples.  Here every
// corner is loaded from an index clamped into the array -- always a valid address -- and the tests select afterwards: a corner
// of weight 0 adds nothing, a weighted corner outside the array makes the value NaN.
template <class T>
__device__ __forceinline__ double volume_interp(const G &g, const T *__restrict__ a, const double (&x)[3]) {
    int i0[3];
    double y[3];
    bool bad = false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        const double f = floor(x[d]);
        const bool ok = f >= 0.0 && f <= (double)g.n[d];           // (false when x is NaN)
        bad = bad || !ok;
        i0[d] = (int)(ok ? f : 0.0) - 1;                           // 0-based lower corner
        y[d] = x[d] - f;
    }
    double v[8], w[8];
    bool in[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        long off = 0;
        in[c] = true;
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            const int up = (c >> d) & 1;
            const double wd = up ? y[d] : 1.0 - y[d];
            w[c] = d == 0 ? wd : w[c] * wd;
            const int J = i0[d] + up;
            in[c] = in[c] && J >= 0 && J < g.n[d];
            off += (long)(J < 0 ? 0 : (J < g.n[d] ? J : g.n[d] - 1)) * g.s[d];
        }
        v[c] = (double)a[off];
    }
    double s = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const bool use = !(w[c] == 0.0);
        bad = bad || (use && !in[c]);
        s = use ? s + v[c] * w[c] : s;
    }
    return bad ? __builtin_nan("") : s;
}

template <class T>
__global__ __launch_bounds__(256) void k_scene_volume(const G g, const VolumeArgs A, const T *__restrict__ f, const uint8_t *__restrict__ lut,
                                                     const double *__restrict__ opac, const unsigned long long *__restrict__ key,
                                                     uint32_t *__restrict__ rgba, double *__restrict__ acc) {
    const int lane = threadIdx.x & 63;
    const int tw = (A.W + 7) >> 3, th = (A.H + 7) >> 3;
    const long tile = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (tile >= (long)tw * th) return;                         // (the whole wavefront)
    const int i = (int)(tile % tw) * 8 + (lane & 7), j = (int)(tile / tw) * 8 + (lane >> 3);
    const bool pixel = i < A.W && j < A.H;
    const long p = (long)j * A.W + i;

    // the ray
    const double xn = (((double)i + 0.5) / (double)A.W) * 2.0 - 1.0;
    const double yn = 1.0 - (((double)j + 0.5) / (double)A.H) * 2.0;
    double h0[4], gz[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        h0[r] = (A.mi[4 * r] * xn + A.mi[4 * r + 1] * yn) + A.mi[4 * r + 3];
        gz[r] = A.mi[4 * r + 2];
    }
    double P0[3], P1[3], D[3];
    volume_point(h0, gz, 0.0, P0);
    volume_point(h0, gz, 1.0, P1);
    bool empty = !pixel || !volume_finite(P0) || !volume_finite(P1);
    double s_in = 0.0, s_out = 1.0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        D[d] = P1[d] - P0[d];
        if (D[d] == 0.0) {
            empty = empty || !(A.blo[d] <= P0[d] && P0[d] <= A.bhi[d]);
        } else {
            const double ta = (A.blo[d] - P0[d]) / D[d], tb = (A.bhi[d] - P0[d]) / D[d];
            const double tn = ta < tb ? ta : tb, tx = ta > tb ? ta : tb;
            s_in = s_in > tn ? s_in : tn;
            s_out = s_out < tx ? s_out : tx;
        }
    }

    // the surface in front of which the ray stops, and what lies behind the cloud
    const unsigned long long kq = pixel ? key[p] : SCENE_NOTHING;
    const uint32_t base = kq == SCENE_NOTHING ? A.bg : rgba[p];
    double s_stop = __builtin_inf();
    if (kq != SCENE_NOTHING) {
        const double z = (double)(unsigned)(kq >> 32) / 4294967296.0;
        double Ps[3];
        volume_point(h0, gz, z, Ps);
        s_stop = (((Ps[0] - P0[0]) * D[0] + (Ps[1] - P0[1]) * D[1]) + (Ps[2] - P0[2]) * D[2]) / ((D[0] * D[0] + D[1] * D[1]) + D[2] * D[2]);
    }

    // the first k of the tile: no lane's first taken sample lies before it (one k of slack covers the rounding of the quotient)
    const bool miss = empty || !(s_in <= s_out);
    int k0 = 0x7fffffff;
    if (!miss) {
        double kf = floor(s_in / A.ds - 0.5) - 1.0;
        kf = kf > 0.0 ? (kf < 2097152.0 ? kf : 2097152.0) : 0.0;
        k0 = (int)kf;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int o = __shfl_xor(k0, m, 64);
        k0 = o < k0 ? o : k0;
    }

    double C0 = 0.0, C1 = 0.0, C2 = 0.0, Tr = 1.0;
    if (!miss) {
        for (int k = k0;; ++k) {
            const double s = ((double)k + 0.5) * A.ds;
            if (!(s <= s_out && s < s_stop)) break;
            if (!(s >= s_in)) continue;
            const double x[3] = {(P0[0] + s * D[0]) + 1.5, (P0[1] + s * D[1]) + 1.5, (P0[2] + s * D[2]) + 1.5};
            const double v = volume_interp<T>(g, f, x);
            if (v != v) continue;
            const int idx = shade_index(v, A.vmin, A.vmax, A.levels);
            const double a = opac[idx];
            if (a == 0.0) continue;                            // (w = 0 and 1 - a = 1: C and T keep every bit)
            const uint8_t *e = lut + 4 * idx;
            const double w = Tr * a;
            C0 = C0 + w * (double)e[0];
            C1 = C1 + w * (double)e[1];
            C2 = C2 + w * (double)e[2];
            Tr = Tr * (1.0 - a);
            if (Tr < A.t_min) break;
        }
    }
    if (!pixel) return;
    const uint32_t out = volume_byte(C0 + Tr * (double)(base & 0xFFu)) | (volume_byte(C1 + Tr * (double)((base >> 8) & 0xFFu)) << 8) |
                         (volume_byte(C2 + Tr * (double)((base >> 16) & 0xFFu)) << 16) |
                         (volume_byte((1.0 - Tr) * 255.0 + Tr * (double)(base >> 24)) << 24);
    rgba[p] = out;
    if (acc) {
        acc[4 * p] = C0;
        acc[4 * p + 1] = C1;
        acc[4 * p + 2] = C2;
        acc[4 * p + 3] = Tr;
    }
}

__global__ __launch_bounds__(256) void k_scene_average(const uint32_t *__restrict__ rgba, int W, int H, int ssaa, uint32_t *__restrict__ out) {
    const int ow = W / ssaa, oh = H / ssaa;
    const int i = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), j = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (i >= ow || j >= oh) return;
    out[(long)j * ow + i] = scene_block_average<false>(rgba, nullptr, W, ssaa, 0u, i, j);
}

// ------------------------------------------------------------------------------------------ launches
template <class T>
int op_scene_volume(const G &g, const VolumeArgs &A, const T *f, const uint8_t *lut, const double *opac, const unsigned long long *key,
                    uint8_t *rgba, double *acc) {
    const long tiles = (long)((A.W + 7) / 8) * ((A.H + 7) / 8);
    Prof pr(WL_K_MISC, (long)A.W * A.H);
    hipLaunchKernelGGL((k_scene_volume<T>), dim3((unsigned)((tiles + 3) / 4)), dim3(256), 0, ctx().stream, g, A, f, lut, opac, key,
                       (uint32_t *)rgba, acc);
    return (int)hipGetLastError();
}
inline int op_scene_average(const uint8_t *rgba, int W, int H, int ssaa, uint8_t *out) {
    const int ow = W / ssaa, oh = H / ssaa;
    Prof pr(WL_K_MISC, (long)W * H);
    hipLaunchKernelGGL(k_scene_average, dim3((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4)), dim3(256), 0, ctx().stream,
                       (const uint32_t *)rgba, W, H, ssaa, (uint32_t *)out);
    return (int)hipGetLastError();
}

}  // namespace wl
