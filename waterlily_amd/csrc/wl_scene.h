// wl_scene.h -- Scene: depth-buffered pictures of triangles (isosurfaces, posed bodies), made on the device
// (waterlily_amd/scene.py; wl_scene_* in include/wlhip.h, which holds the definition).
//
// A small rasteriser.  The vertex stage is IEEE double, one operation at a time; from the snapped sub-pixel integers on,
// coverage and depth order are integer problems: a 64-bit key (depth << 32 | triangle id) per pixel and atomicMin.  The picture
// is a function of the triangles and the camera alone -- bit for bit on any launch shape, in any triangle order, on either path.
//
// Kernels (no LDS, no float atomics, nothing allocated):
//   k_scene_clear   : keys = all ones ("nothing")
//   k_scene_lane    : one lane per triangle.  A triangle whose clamped bounding box holds <= large_px pixels is rasterised by
//                     its lane (the isosurface case: a few pixels each); the others are appended to a list in caller scratch
//                     with one integer atomic per wavefront (ballot + popcount).
//   k_scene_wave    : one wavefront per listed triangle (grid-stride over the list), its 64 lanes tiling the bounding box 8x8
//                     pixels at a time (body triangles, close-ups).
//   k_scene_shade   : one thread per pixel: the winner's barycentrics from the same integers, the perspective-correct value
//                     through wl_render_shade's colour rule (shade_index, wl_render.h), flat two-sided lighting.
//   k_scene_resolve : background where the key is "nothing", then ssaa x ssaa integer box average.
// tests/scene_ref.py restates every rule with numpy float64 scalars and Python integers.
#pragma once
#include "wl_common.h"
#include "wl_render.h"

namespace wl {

struct SceneCam {
    double m[16];                                              // row-major: clip = M (x, y, z, 1)
};
constexpr unsigned long long SCENE_NOTHING = ~0ull;

// One triangle after the vertex stage and the orientation swap: sub-pixel integers, depths, clip w, the clamped bounding box.
struct SceneTri {
    long long X0, Y0, X1, Y1, X2, Y2, A2;
    double z0, z1, z2, w0, w1, w2;
    int ilo, ihi, jlo, jhi;                                    // pixels whose centre can be covered (both ends included)
    bool swapped;                                              // vertices 1 and 2 were exchanged (A2 was negative)
};

// vertex stage of one vertex: false when the triangle must be dropped.  X, Y: 8 sub-pixel bits; z = c2 / c3; w = c3.
__device__ __forceinline__ bool scene_vertex(const SceneCam &C, const double *__restrict__ p, int W, int H, long long &X, long long &Y,
                                             double &z, double &w) {
    const double x = p[0], y = p[1], zz = p[2];
    const double *m = C.m;
    const double c0 = ((m[0] * x + m[1] * y) + m[2] * zz) + m[3];
    const double c1 = ((m[4] * x + m[5] * y) + m[6] * zz) + m[7];
    const double c2 = ((m[8] * x + m[9] * y) + m[10] * zz) + m[11];
    const double c3 = ((m[12] * x + m[13] * y) + m[14] * zz) + m[15];
    const double big = 1.79769313486231570815e308;
    bool ok = fabs(x) <= big && fabs(y) <= big && fabs(zz) <= big && fabs(c0) <= big && fabs(c1) <= big && fabs(c2) <= big &&
              fabs(c3) <= big;                                 // (false for NaN and for +-inf)
    ok = ok && c3 > 0.0;
    const double d = ok ? c3 : 1.0;
    z = c2 / d;
    ok = ok && z >= 0.0 && z <= 1.0;
    const double sx = ((c0 / d) * 0.5 + 0.5) * (double)W;
    const double sy = (0.5 - (c1 / d) * 0.5) * (double)H;
    ok = ok && fabs(sx) < 524288.0 && fabs(sy) < 524288.0;     // 2^19 (false for NaN)
    X = ok ? (long long)floor(sx * 256.0 + 0.5) : 0;
    Y = ok ? (long long)floor(sy * 256.0 + 0.5) : 0;
    w = c3;
    return ok;
}
__device__ __forceinline__ long long scene_edge(long long Xa, long long Ya, long long Xb, long long Yb, long long Px, long long Py) {
    return (Xb - Xa) * (Py - Ya) - (Yb - Ya) * (Px - Xa);
}
// -1 for an edge a -> b on which a pixel centre is NOT accepted, 0 for a top or left edge (y grows downwards, A2 > 0):
// left: Yb < Ya; top: Yb == Ya and Xb > Xa
__device__ __forceinline__ long long scene_bias(long long Xa, long long Ya, long long Xb, long long Yb) {
    return (Yb < Ya || (Yb == Ya && Xb > Xa)) ? 0 : -1;
}
// false: the triangle draws nothing (dropped, zero area, or no pixel centre inside the viewport in its bounding box)
__device__ __forceinline__ bool scene_setup(const SceneCam &C, const double *__restrict__ tri, int W, int H, SceneTri &T) {
    bool ok = scene_vertex(C, tri, W, H, T.X0, T.Y0, T.z0, T.w0);
    ok = scene_vertex(C, tri + 3, W, H, T.X1, T.Y1, T.z1, T.w1) && ok;
    ok = scene_vertex(C, tri + 6, W, H, T.X2, T.Y2, T.z2, T.w2) && ok;
    if (!ok) return false;
    long long A2 = scene_edge(T.X0, T.Y0, T.X1, T.Y1, T.X2, T.Y2);
    if (A2 == 0) return false;
    T.swapped = A2 < 0;
    if (T.swapped) {
        long long t = T.X1; T.X1 = T.X2; T.X2 = t;
        t = T.Y1; T.Y1 = T.Y2; T.Y2 = t;
        double d = T.z1; T.z1 = T.z2; T.z2 = d;
        d = T.w1; T.w1 = T.w2; T.w2 = d;
        A2 = -A2;
    }
    T.A2 = A2;
    auto mn = [](long long a, long long b) { return a < b ? a : b; };
    auto mx = [](long long a, long long b) { return a > b ? a : b; };
    long long il = (mn(T.X0, mn(T.X1, T.X2)) + 127) >> 8, ih = (mx(T.X0, mx(T.X1, T.X2)) - 128) >> 8;   // centres 256 i + 128
    long long jl = (mn(T.Y0, mn(T.Y1, T.Y2)) + 127) >> 8, jh = (mx(T.Y0, mx(T.Y1, T.Y2)) - 128) >> 8;
    il = mx(il, 0); ih = mn(ih, (long long)W - 1);
    jl = mx(jl, 0); jh = mn(jh, (long long)H - 1);
    T.ilo = (int)il; T.ihi = (int)ih; T.jlo = (int)jl; T.jhi = (int)jh;
    return il <= ih && jl <= jh;
}
// the three edge values at pixel (i, j), E_k opposite vertex k; true when the pixel is covered
__device__ __forceinline__ bool scene_cover(const SceneTri &T, int i, int j, long long &E0, long long &E1, long long &E2) {
    const long long Px = 256ll * i + 128, Py = 256ll * j + 128;
    E0 = scene_edge(T.X1, T.Y1, T.X2, T.Y2, Px, Py);
    E1 = scene_edge(T.X2, T.Y2, T.X0, T.Y0, Px, Py);
    E2 = scene_edge(T.X0, T.Y0, T.X1, T.Y1, Px, Py);
    return E0 + scene_bias(T.X1, T.Y1, T.X2, T.Y2) >= 0 && E1 + scene_bias(T.X2, T.Y2, T.X0, T.Y0) >= 0 &&
           E2 + scene_bias(T.X0, T.Y0, T.X1, T.Y1) >= 0;
}
__device__ __forceinline__ void scene_bary(const SceneTri &T, long long E0, long long E1, long long E2, double &b0, double &b1, double &b2) {
    const double a = (double)T.A2;
    b0 = (double)E0 / a;
    b1 = (double)E1 / a;
    b2 = (double)E2 / a;
}
// test pixel (i, j) and, when covered, lower its key
__device__ __forceinline__ void scene_fragment(const SceneTri &T, int i, int j, int W, unsigned id, unsigned long long *__restrict__ key) {
    long long E0, E1, E2;
    if (!scene_cover(T, i, j, E0, E1, E2)) return;
    double b0, b1, b2;
    scene_bary(T, E0, E1, E2, b0, b1, b2);
    const double d = (b0 * T.z0 + b1 * T.z1) + b2 * T.z2;
    double q = floor(d * 4294967296.0);
    q = q < 0.0 ? 0.0 : (q > 4294967295.0 ? 4294967295.0 : q);
    const unsigned long long k = ((unsigned long long)(unsigned)q << 32) | (unsigned long long)id;
    unsigned long long *p = key + ((long)j * W + i);
    if (k < __atomic_load_n(p, __ATOMIC_RELAXED)) atomicMin(p, k);   // (keys only fall: a fragment that loses to what is there loses for good)
}

__global__ __launch_bounds__(256) void k_scene_clear(unsigned long long *__restrict__ key, long n) {
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p < n) key[p] = SCENE_NOTHING;
}

// scratch: word 0 = the length of the list, words 4.. = the listed triangle numbers (any order)
__global__ __launch_bounds__(256) void k_scene_lane(const SceneCam C, const double *__restrict__ tri, long nt, unsigned base, int W, int H,
                                                   long large_px, unsigned long long *__restrict__ key, unsigned *__restrict__ scratch) {
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    SceneTri T;
    const bool draws = t < nt && scene_setup(C, tri + 9 * t, W, H, T);
    const bool large = draws && (long)(T.ihi - T.ilo + 1) * (long)(T.jhi - T.jlo + 1) > large_px;
    const unsigned long long m = __ballot(large);
    if (m) {                                                   // one atomic per wavefront
        const int leader = __ffsll((long long)m) - 1;
        unsigned at = 0;
        if (lane == leader) at = atomicAdd(scratch, (unsigned)__popcll(m));
        at = __shfl(at, leader, 64);
        if (large) scratch[4 + at + (unsigned)__popcll(m & ((1ull << lane) - 1ull))] = (unsigned)t;
    }
    if (!draws || large) return;
    for (int j = T.jlo; j <= T.jhi; ++j)
        for (int i = T.ilo; i <= T.ihi; ++i) scene_fragment(T, i, j, W, base + (unsigned)t, key);
}
__global__ __launch_bounds__(256) void k_scene_wave(const SceneCam C, const double *__restrict__ tri, unsigned base, int W, int H,
                                                   unsigned long long *__restrict__ key, const unsigned *__restrict__ scratch) {
    const int lane = threadIdx.x & 63;
    const unsigned count = scratch[0];
    const unsigned nwave = gridDim.x * 4u;
    for (unsigned e = blockIdx.x * 4u + (threadIdx.x >> 6); e < count; e += nwave) {
        const unsigned t = scratch[4 + e];
        SceneTri T;
        if (!scene_setup(C, tri + 9 * (long)t, W, H, T)) continue;   // (never: the lane kernel listed it)
        for (int tj = T.jlo; tj <= T.jhi; tj += 8)
            for (int ti = T.ilo; ti <= T.ihi; ti += 8) {
                const int i = ti + (lane & 7), j = tj + (lane >> 3);
                if (i <= T.ihi && j <= T.jhi) scene_fragment(T, i, j, W, base + t, key);
            }
    }
}

struct SceneShade {
    int W, H, levels, has_val;
    unsigned base;
    long nt;
    double vmin, vmax, ambient, light[3];
    uint32_t solid, nan_rgba;                                  // byte 0 = R
};
__global__ __launch_bounds__(256) void k_scene_shade(const SceneCam C, const SceneShade A, const unsigned long long *__restrict__ key,
                                                    const double *__restrict__ tri, const double *__restrict__ val,
                                                    const uint8_t *__restrict__ lut, uint32_t *__restrict__ rgba) {
    const int i = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), j = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (i >= A.W || j >= A.H) return;
    const long p = (long)j * A.W + i;
    const unsigned long long k = key[p];
    const unsigned id = (unsigned)(k & 0xFFFFFFFFull);
    if (k == SCENE_NOTHING || id < A.base || (long)(id - A.base) >= A.nt) return;
    const long t = (long)(id - A.base);
    const double *P = tri + 9 * t;
    SceneTri T;
    if (!scene_setup(C, P, A.W, A.H, T)) return;               // (never: this triangle wrote the key)
    uint32_t col = A.solid;
    if (A.has_val) {
        long long E0, E1, E2;
        scene_cover(T, i, j, E0, E1, E2);
        double b0, b1, b2;
        scene_bary(T, E0, E1, E2, b0, b1, b2);
        const double v0 = val[3 * t], v1 = val[3 * t + (T.swapped ? 2 : 1)], v2 = val[3 * t + (T.swapped ? 1 : 2)];
        const double q0 = b0 / T.w0, q1 = b1 / T.w1, q2 = b2 / T.w2;
        const double v = ((q0 * v0 + q1 * v1) + q2 * v2) / ((q0 + q1) + q2);
        if (v != v) {
            rgba[p] = A.nan_rgba;
            return;
        }
        const uint8_t *e = lut + 4 * shade_index(v, A.vmin, A.vmax, A.levels);
        col = (uint32_t)e[0] | ((uint32_t)e[1] << 8) | ((uint32_t)e[2] << 16);
    }
    // flat, two-sided: the normal of the world-space triangle as stored
    const double ax = P[3] - P[0], ay = P[4] - P[1], az = P[5] - P[2];
    const double bx = P[6] - P[0], by = P[7] - P[1], bz = P[8] - P[2];
    const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const double len = sqrt((nx * nx + ny * ny) + nz * nz);
    double s = A.ambient;
    if (len > 0.0) s = A.ambient + (1.0 - A.ambient) * fabs(((nx * A.light[0] + ny * A.light[1]) + nz * A.light[2]) / len);
    uint32_t out = 0xFF000000u;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double x = floor((double)((col >> (8 * c)) & 0xFFu) * s + 0.5);
        x = x < 0.0 ? 0.0 : (x > 255.0 ? 255.0 : x);           // (false for NaN too: a NaN s leaves x NaN -> 0 below)
        out |= (uint32_t)(x == x ? (int)x : 0) << (8 * c);
    }
    rgba[p] = out;
}
// the ssaa x ssaa block average of output pixel (i, j): per channel (sum + n/2) / n in integers.  KEYED: a pixel whose key is
// "nothing" counts as bg (wl_scene_resolve); otherwise every pixel counts as it is (wl_scene_average, wl_volume.h)
template <bool KEYED>
__device__ __forceinline__ uint32_t scene_block_average(const uint32_t *__restrict__ rgba, const unsigned long long *__restrict__ key, int W,
                                                        int ssaa, uint32_t bg, int i, int j) {
    unsigned s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    for (int b = 0; b < ssaa; ++b)
        for (int a = 0; a < ssaa; ++a) {
            const long p = (long)(j * ssaa + b) * W + (i * ssaa + a);
            const uint32_t c = (KEYED && key[p] == SCENE_NOTHING) ? bg : rgba[p];
            s0 += c & 0xFFu; s1 += (c >> 8) & 0xFFu; s2 += (c >> 16) & 0xFFu; s3 += c >> 24;
        }
    const unsigned n = (unsigned)(ssaa * ssaa), h = n / 2;
    return ((s0 + h) / n) | (((s1 + h) / n) << 8) | (((s2 + h) / n) << 16) | (((s3 + h) / n) << 24);
}
__global__ __launch_bounds__(256) void k_scene_resolve(const uint32_t *__restrict__ rgba, const unsigned long long *__restrict__ key, int W,
                                                      int H, int ssaa, uint32_t bg, uint32_t *__restrict__ out) {
    const int ow = W / ssaa, oh = H / ssaa;
    const int i = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), j = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (i >= ow || j >= oh) return;
    out[(long)j * ow + i] = scene_block_average<true>(rgba, key, W, ssaa, bg, i, j);
}

// ------------------------------------------------------------------------------------------ launches
inline int op_scene_clear(unsigned long long *key, int W, int H) {
    const long n = (long)W * H;
    Prof pr(WL_K_MISC, n);
    hipLaunchKernelGGL(k_scene_clear, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx().stream, key, n);
    return (int)hipGetLastError();
}
inline int64_t scene_scratch_bytes(int64_t nt) { return 16 + 4 * nt; }
inline int op_scene_draw(unsigned long long *key, int W, int H, const SceneCam &C, const double *tri, int64_t nt, unsigned base,
                         int64_t large_px, unsigned *scratch) {
    if (nt == 0) return 0;
    hipStream_t st = ctx().stream;
    WL_HIP(hipMemsetAsync(scratch, 0, 16, st));
    Prof pr(WL_K_MISC, nt);
    hipLaunchKernelGGL(k_scene_lane, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, C, tri, (long)nt, base, W, H, (long)large_px, key,
                       scratch);
    WL_HIP(hipGetLastError());
    if (large_px >= (int64_t)W * H) return 0;                  // nothing can have been listed
    const int64_t nb = (nt + 3) / 4;
    hipLaunchKernelGGL(k_scene_wave, dim3((unsigned)(nb < 4096 ? nb : 4096)), dim3(256), 0, st, C, tri, base, W, H, key, (const unsigned *)scratch);
    return (int)hipGetLastError();
}
inline int op_scene_shade(const SceneCam &C, const SceneShade &A, const unsigned long long *key, const double *tri, const double *val,
                          const uint8_t *lut, uint8_t *rgba) {
    if (A.nt == 0) return 0;
    Prof pr(WL_K_MISC, (long)A.W * A.H);
    hipLaunchKernelGGL(k_scene_shade, dim3((unsigned)((A.W + 63) / 64), (unsigned)((A.H + 3) / 4)), dim3(256), 0, ctx().stream, C, A, key, tri,
                       val, lut, (uint32_t *)rgba);
    return (int)hipGetLastError();
}
inline int op_scene_resolve(const uint8_t *rgba, const unsigned long long *key, int W, int H, int ssaa, uint32_t bg, uint8_t *out) {
    const int ow = W / ssaa, oh = H / ssaa;
    Prof pr(WL_K_MISC, (long)W * H);
    hipLaunchKernelGGL(k_scene_resolve, dim3((unsigned)((ow + 63) / 64), (unsigned)((oh + 3) / 4)), dim3(256), 0, ctx().stream,
                       (const uint32_t *)rgba, key, W, H, ssaa, bg, (uint32_t *)out);
    return (int)hipGetLastError();
}

}  // namespace wl
