// wl_region_sums.h -- value-weighted sums per region (circulation, enstrophy, weighted moments) as EXACT integers
// (waterlily_amd/regions.py: sums; wl_region_sums in include/wlhip.h, which holds the definition).  A term -- the value
// render_value() forms, optionally squared, optionally times a cell index -- is cut to a fixed-point integer of up to 127 bits
// against the column's scale E_c, n = trunc(term * 2^(126 - E_c)), and its four 32-bit digits are added, signed, to four int64
// limbs of the cell's region.  Integer addition is exact in any order: limbs, counts and the double the finish pass rounds them
// to (once, to nearest-even) are a function of the field, the labels and the box alone on any launch shape.  No order contract,
// no sort, no scan over a region; nothing allocated, nothing read back, no floating-point atomics.  Launches (a fixed number):
//   k_rs_init   : rows r < min(R, cap) of acc_dev and the ncol entries of over_dev are zeroed.
//   k_rs_scale  : WL_RS_FIND only.  The largest finite |term| of every column over the cells with a label >= 0, as atomicMax
//                 on its range_key image, kept in over_dev during the call: lane-private maxima, one butterfly per wavefront at
//                 the end, the four wavefronts through LDS, one atomic per column and workgroup.
//   k_rs_sum    : the walk of k_rg_table: one wavefront per x-row, pieces of 64 cells.  A piece whose cells belong to ONE region
//                 adds its digits to LANE-PRIVATE limbs (no cross-lane traffic, no atomics); the limbs are reduced over the
//                 wavefront and go to acc_dev when the region changes and, the four wavefronts' together through LDS, at the end:
//                 a region that fills the box costs a few atomics per workgroup.  A piece with several regions takes a
//                 segmented scan over its runs of equal labels; the last lane of a run adds the run's digits.  Zero digits are
//                 never added.  Columns that name the same value share it: the outer loop is over the DISTINCT values.
//   k_rs_finish : N = sum_k limb_k * 2^(32 k) by carry propagation, normalised, rounded once with round and sticky bit.
// With FIND the first workgroup of k_rs_sum writes scale_dev from the keys and k_rs_finish clears over_dev.
#pragma once
#include "wl_regions.h"

namespace wl {

constexpr int RS_MAXC = WL_RS_MAX_COLS;
constexpr int RS_WG = 2048;            // the launch cap of the row kernels (RG_TAB_WG: a workgroup ends with one flush)
constexpr int RS_ROW_WG = 1024;        // ... of the kernels over the rows of acc_dev (grid-stride)

struct RsVal {
    const void *f;
    RenderWhat w;
    int absval, metric;
};
// the columns of one call: v[0 .. nval) the distinct values, val[c] the value column c reads
struct RsCols {
    int ncol, nval, given;
    int val[RS_MAXC], power[RS_MAXC], moment[RS_MAXC];
    RsVal v[RS_MAXC];
};

// E_c of a caller (WL_RS_GIVEN), held to the range in which the scaling is exact and the result normal
__host__ __device__ inline int rs_clamp(int E) { return E < WL_RS_EMIN ? WL_RS_EMIN : (E > 1023 ? 1023 : E); }
// E_c of the largest finite |term| (0: there was none): max(ilogb(M), WL_RS_EMIN); a zero or subnormal M is below the clamp
__host__ __device__ inline int rs_scale_of_key(unsigned long long key) {
    if (!key) return WL_RS_EMIN;
    const int be = (int)((key >> 52) & 0x7ffull);              // (the key of M >= 0 is its bits with the top bit set)
    return be == 0 ? WL_RS_EMIN : rs_clamp(be - 1023);
}

template <class T, int D, bool ANYM>
__device__ __forceinline__ double rs_value(const G &g, const RsVal &V, int i, int j, int k) {
    double x;
    if (ANYM && V.metric) x = render_value<T, D, true>(g, (const T *)V.f, V.w, i, j, k);
    else x = render_value<T, D, false>(g, (const T *)V.f, V.w, i, j, k);
    return V.absval ? fabs(x) : x;
}
// w = v or v * v; term = w or w * (double)J_d: every operation an IEEE double operation of its own (-ffp-contract=off)
__device__ __forceinline__ double rs_term(double v, int power, int moment, int i, int j, int k) {
    const double w = power == 2 ? v * v : v;
    if (moment < 0) return w;
    return w * (double)(moment == 0 ? i : (moment == 1 ? j : k));
}
// The signed digits of n = trunc(term * 2^(126 - E)).  nf: term is not finite; over: |term| >= 2^(E + 1) (neither is added).
// A finite non-zero term is m * 2^(be - 1075) with the 53-bit m, so n = m * 2^s, s = be - 949 - E: s <= 74 once the term is
// not `over`, and m * 2^s < 2^127.  s < 0 cuts the low -s bits toward zero; a subnormal term lies below every unit (E >= -894).
__host__ __device__ inline void rs_digits(double term, int E, long long (&d)[4], bool &nf, bool &over) {
    unsigned long long u;
    memcpy(&u, &term, 8);
    const int be = (int)((u >> 52) & 0x7ffull);
    d[0] = d[1] = d[2] = d[3] = 0;
    nf = be == 0x7ff;
    over = !nf && be != 0 && be - 1023 > E;
    if (nf || over || be == 0) return;
    const unsigned long long m = (u & 0xfffffffffffffull) | (1ull << 52);
    const int s = be - 949 - E;
    if (s <= -53) return;
    unsigned long long lo, hi;
    if (s < 0) { lo = m >> (-s); hi = 0; }
    else if (s == 0) { lo = m; hi = 0; }
    else if (s < 64) { lo = m << s; hi = m >> (64 - s); }
    else { lo = 0; hi = m << (s - 64); }
    d[0] = (long long)(lo & 0xffffffffull); d[1] = (long long)(lo >> 32);
    d[2] = (long long)(hi & 0xffffffffull); d[3] = (long long)(hi >> 32);
    if (u >> 63) { d[0] = -d[0]; d[1] = -d[1]; d[2] = -d[2]; d[3] = -d[3]; }
}

__device__ __forceinline__ long long rs_wave_sum(long long v) { return (long long)rg_wave_sum((unsigned long long)v); }
__device__ __forceinline__ void rs_add(long long *p, long long v) {
    if (v) atomicAdd((unsigned long long *)p, (unsigned long long)v);
}

// ------------------------------------------------------------------------------------------ the rows, the maxima
__global__ __launch_bounds__(256) void k_rs_init(long cap, int ncol, const unsigned long long *__restrict__ n, long long *__restrict__ acc,
                                                 long long *__restrict__ over) {
    const long R = (long)n[0];
    const long m = (R < cap ? R : cap) * ncol * 5;
    const long t0 = (long)blockIdx.x * 256 + threadIdx.x;
    for (long x = t0; x < m; x += (long)gridDim.x * 256) acc[x] = 0;
    if (t0 < ncol) over[t0] = 0;                               // FIND: "no finite term yet"; GIVEN: the count
}

template <class T, int D, bool ANYM>
__global__ __launch_bounds__(256) void k_rs_scale(const G g, const RgBox B, const RsCols C, const int *__restrict__ label, unsigned long long *kmax) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned long long mx[RS_MAXC];
#pragma unroll
    for (int c = 0; c < RS_MAXC; ++c) mx[c] = 0ull;
    const int nw = (int)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        const int j = B.lo[1] + (int)(row % B.ny), k = B.lo[2] + (int)(row / B.ny);
        const long q0 = row * B.nx;
        for (int p = 0; p < B.pieces; ++p) {
            const int x = p * 64 + lane, i = B.lo[0] + x;
            const bool in = x < B.nx && label[q0 + x] >= 0;
            if (!__ballot(in)) continue;
            for (int u = 0; u < C.nval; ++u) {
                const double v = in ? rs_value<T, D, ANYM>(g, C.v[u], i, j, k) : 0.0;
#pragma unroll
                for (int c = 0; c < RS_MAXC; ++c) {
                    if (c >= C.ncol || C.val[c] != u) continue;
                    const double a = fabs(rs_term(v, C.power[c], C.moment[c], i, j, k));
                    const unsigned long long key = range_key(a);
                    if (in && a <= 1.7976931348623157e308 && key > mx[c]) mx[c] = key;      // (false for NaN and inf)
                }
            }
        }
    }
    __shared__ unsigned long long part[4][RS_MAXC];
#pragma unroll
    for (int c = 0; c < RS_MAXC; ++c) {
        const unsigned long long w = rg_wave_max(mx[c]);
        if (lane == 0) part[tid >> 6][c] = w;
    }
    __syncthreads();
    if (tid < C.ncol) {
        unsigned long long w = part[0][tid];
        for (int q = 1; q < 4; ++q) w = part[q][tid] > w ? part[q][tid] : w;
        if (w) rg_max(&kmax[tid], w);
    }
}

// ------------------------------------------------------------------------------------------ the sums
// What a wavefront keeps of one region between two flushes: lane-private limbs, one set per column (k = 4: non-finite terms).
struct RsAcc {
    int r;                                                     // -1: nothing kept (the same in every lane)
    long long s[RS_MAXC][5];
};
__device__ __forceinline__ void rs_zero(RsAcc &A) {
#pragma unroll
    for (int c = 0; c < RS_MAXC; ++c)
#pragma unroll
        for (int k = 0; k < 5; ++k) A.s[c][k] = 0;
}
// called by whole wavefronts: the lanes' limbs become one set, which lane 0 adds to the region's row
__device__ __forceinline__ void rs_flush(const RsAcc &A, int ncol, long long *acc, int lane) {
    if (A.r < 0) return;
#pragma unroll
    for (int c = 0; c < RS_MAXC; ++c) {
        if (c >= ncol) continue;
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const long long t = rs_wave_sum(A.s[c][k]);
            if (lane == 0) rs_add(&acc[((long)A.r * ncol + c) * 5 + k], t);
        }
    }
}
// inclusive sum over the lanes start .. lane of a run (start: the run's first lane)
__device__ __forceinline__ long long rs_run_sum(long long v, int lane, int start) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const long long o = (long long)__shfl_up((unsigned long long)v, off, 64);
        if (lane - off >= start) v += o;
    }
    return v;
}

template <class T, int D, bool ANYM>
__global__ __launch_bounds__(256) void k_rs_sum(const G g, const RgBox B, const RsCols C, const int *__restrict__ label, long cap, int *scale,
                                                unsigned long long *over, long long *acc) {
    const int tid = threadIdx.x, lane = tid & 63;
    int E[RS_MAXC];
#pragma unroll
    for (int c = 0; c < RS_MAXC; ++c) E[c] = c < C.ncol ? (C.given ? rs_clamp(scale[c]) : rs_scale_of_key(over[c])) : 0;
    if (!C.given && blockIdx.x == 0 && tid < C.ncol) scale[tid] = rs_scale_of_key(over[tid]);      // (nobody reads scale_dev in this pass)
    RsAcc A;
    A.r = -1;
    rs_zero(A);
    unsigned nover[RS_MAXC];
#pragma unroll
    for (int c = 0; c < RS_MAXC; ++c) nover[c] = 0u;
    const int nw = (int)gridDim.x * 4;
    for (long row = (long)blockIdx.x * 4 + (tid >> 6); row < B.rows; row += nw) {
        const int j = B.lo[1] + (int)(row % B.ny), k = B.lo[2] + (int)(row / B.ny);
        const long q0 = row * B.nx;
        for (int p = 0; p < B.pieces; ++p) {
            const int x = p * 64 + lane, i = B.lo[0] + x;
            const int r = x < B.nx ? label[q0 + x] : -1;
            const bool in = r >= 0, valid = in && r < cap;
            if (!__ballot(in)) continue;                       // (the same in every lane)
            const unsigned long long m = __ballot(valid);
            const int rr = valid ? r : -1;
            const int r0 = m ? __shfl(rr, __ffsll((long long)m) - 1, 64) : -1;
            const bool one = !__ballot(valid && rr != r0);     // one region in this piece (or none below cap: only `over` counts)
            int start = 0;
            bool tail = false;
            if (one) {
                if (m && A.r != r0) {
                    rs_flush(A, C.ncol, acc, lane);
                    A.r = r0;
                    rs_zero(A);
                }
            } else {                                           // the runs of equal labels
                const int prev = __shfl_up(rr, 1, 64);
                const unsigned long long heads = __ballot(lane == 0 || prev != rr);
                start = 63 - __clzll((long long)(heads & ((2ull << lane) - 1ull)));
                tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
            }
            for (int u = 0; u < C.nval; ++u) {
                const double v = in ? rs_value<T, D, ANYM>(g, C.v[u], i, j, k) : 0.0;
#pragma unroll
                for (int c = 0; c < RS_MAXC; ++c) {
                    if (c >= C.ncol || C.val[c] != u) continue;
                    long long d[5];
                    bool nf, ov;
                    {
                        long long dd[4];
                        rs_digits(rs_term(v, C.power[c], C.moment[c], i, j, k), E[c], dd, nf, ov);
                        d[0] = dd[0]; d[1] = dd[1]; d[2] = dd[2]; d[3] = dd[3];
                    }
                    nover[c] += (in && ov) ? 1u : 0u;
                    if (!valid) { d[0] = d[1] = d[2] = d[3] = 0; nf = false; }
                    d[4] = nf ? 1 : 0;
                    if (one) {
#pragma unroll
                        for (int q = 0; q < 5; ++q) A.s[c][q] += d[q];
                    } else {
#pragma unroll
                        for (int q = 0; q < 5; ++q) {
                            const long long t = rs_run_sum(d[q], lane, start);
                            if (valid && tail) rs_add(&acc[((long)r * C.ncol + c) * 5 + q], t);
                        }
                    }
                }
            }
        }
    }
    // the four wavefronts' last shares: those of one region (a region that fills the box: all four) go to acc_dev as one
    __shared__ long long last[4][RS_MAXC][5];
    __shared__ int lastr[4];
#pragma unroll
    for (int c = 0; c < RS_MAXC; ++c) {
        if (c >= C.ncol) continue;
#pragma unroll
        for (int q = 0; q < 5; ++q) {
            const long long t = rs_wave_sum(A.s[c][q]);
            if (lane == 0) last[tid >> 6][c][q] = t;
        }
    }
    if (lane == 0) lastr[tid >> 6] = A.r;
    __syncthreads();                                           // (every thread arrives: the loops above leave by `continue` alone)
    if (tid < C.ncol * 5) {
        const int c = tid / 5, q = tid % 5;
        int cr = lastr[0];
        long long cs = cr >= 0 ? last[0][c][q] : 0;
        for (int w = 1; w < 4; ++w) {
            const int wr = lastr[w];
            if (wr < 0) continue;
            if (wr != cr) {
                if (cr >= 0) rs_add(&acc[((long)cr * C.ncol + c) * 5 + q], cs);
                cr = wr;
                cs = last[w][c][q];
            } else cs += last[w][c][q];
        }
        if (cr >= 0) rs_add(&acc[((long)cr * C.ncol + c) * 5 + q], cs);
    }
    if (C.given) {
#pragma unroll
        for (int c = 0; c < RS_MAXC; ++c) {
            if (c >= C.ncol) continue;
            unsigned t = nover[c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, 64);
            if (lane == 0 && t) atomicAdd(&over[c], (unsigned long long)t);
        }
    }
}

// ------------------------------------------------------------------------------------------ the doubles
// N = sum_k l[k] * 2^(32 k) times 2^(E - 126), rounded once to nearest-even.  The carries run through a signed 64-bit register:
// a box has fewer than 2^31 cells and a digit is below 2^32, so |l[k]| <= (2^31 - 1)(2^32 - 1) < 2^63 - 2^32, and a carry is in
// [-2^31, 2^31), so |carry + l[k]| < 2^63 and no step overflows (limbs added over several boxes must keep that bound); the magnitude of the 160-bit result is shifted until its top bit is
// bit 191 of three words: 53 bits of significand, the round bit, and a sticky bit of everything below.
__host__ __device__ inline double rs_round(const long long *l, int E) {
    const unsigned long long M32 = 0xffffffffull;
    long long a = l[0];
    const unsigned long long w0 = (unsigned long long)a & M32;
    a = (a >> 32) + l[1];
    const unsigned long long w1 = (unsigned long long)a & M32;
    a = (a >> 32) + l[2];
    const unsigned long long w2 = (unsigned long long)a & M32;
    a = (a >> 32) + l[3];
    const unsigned long long w3 = (unsigned long long)a & M32;
    a >>= 32;
    const bool neg = a < 0;
    unsigned long long x0 = w0 | (w1 << 32), x1 = w2 | (w3 << 32), x2 = (unsigned long long)a;
    if (neg) {                                                 // two's complement of the 192 bits
        x0 = ~x0 + 1ull;
        const bool c0 = x0 == 0ull;
        x1 = ~x1 + (c0 ? 1ull : 0ull);
        x2 = ~x2 + ((c0 && x1 == 0ull) ? 1ull : 0ull);
    }
    if (!(x0 | x1 | x2)) return 0.0;
    const int h = x2 ? 191 - __builtin_clzll(x2) : (x1 ? 127 - __builtin_clzll(x1) : 63 - __builtin_clzll(x0));
    int L = 191 - h;
    if (L >= 128) { x2 = x0; x1 = 0; x0 = 0; L -= 128; }
    else if (L >= 64) { x2 = x1; x1 = x0; x0 = 0; L -= 64; }
    if (L) {
        x2 = (x2 << L) | (x1 >> (64 - L));
        x1 = (x1 << L) | (x0 >> (64 - L));
        x0 <<= L;
    }
    unsigned long long mant = x2 >> 11;
    const bool round = (x2 >> 10) & 1ull, sticky = ((x2 & 0x3ffull) | x1 | x0) != 0ull;
    if (round && (sticky || (mant & 1ull))) ++mant;
    int e = h + E - 126;                                       // >= -1020: never subnormal
    if (mant >> 53) { mant >>= 1; ++e; }
    unsigned long long bits = neg ? 0x8000000000000000ull : 0ull;
    if (e > 1023) bits |= 0x7ff0000000000000ull;
    else bits |= ((unsigned long long)(e + 1023) << 52) | (mant & 0xfffffffffffffull);
    double out;
    memcpy(&out, &bits, 8);
    return out;
}
__global__ __launch_bounds__(256) void k_rs_finish(long cap, int ncol, int given, const unsigned long long *__restrict__ n, const int *__restrict__ scale,
                                                   const long long *__restrict__ acc, double *__restrict__ sum, long long *over) {
    const long R = (long)n[0];
    const long m = (R < cap ? R : cap) * ncol;
    const long t0 = (long)blockIdx.x * 256 + threadIdx.x;
    for (long x = t0; x < m; x += (long)gridDim.x * 256) {
        const long long *l = acc + 5 * x;
        sum[x] = l[4] ? __builtin_nan("") : rs_round(l, rs_clamp(scale[x % ncol]));
    }
    if (!given && t0 < ncol) over[t0] = 0;                     // the keys of k_rs_scale leave: FIND counts nothing
}

inline bool rs_same_value(const wl_rg_value &a, const wl_rg_value &b, int D) {
    if (a.f != b.f || a.kind != b.kind || a.ipar != b.ipar || (a.absval != 0) != (b.absval != 0)) return false;
    for (int d = 0; d < D; ++d)
        if (a.par[d] != b.par[d] || a.par2[d] != b.par2[d]) return false;
    return true;
}

// l / h: the box, already validated (D == 2: l[2] = 0, h[2] = 1; one rank: global planes are local planes)
template <class T, int D>
int op_region_sums(const G &g, const int l[3], const int h[3], const int32_t *label, const int64_t *n_dev, int64_t cap, int ncol,
                   const wl_rs_col *cols, int mode, int32_t *scale, int64_t *acc_dev, double *sum, int64_t *over_dev) {
    const RgBox B = rg_box(l, h, 0);
    RsCols Cc;
    memset(&Cc, 0, sizeof Cc);
    Cc.ncol = ncol;
    Cc.given = mode == WL_RS_GIVEN ? 1 : 0;
    int first[RS_MAXC];                                        // the column that introduced each distinct value
    bool anym = false;
    for (int c = 0; c < ncol; ++c) {
        int u = 0;
        while (u < Cc.nval && !rs_same_value(cols[first[u]].v, cols[c].v, D)) ++u;
        if (u == Cc.nval) {
            const wl_rg_value &v = cols[c].v;
            RsVal &V = Cc.v[Cc.nval++];
            first[u] = c;
            V.f = v.f;
            V.w.kind = v.kind; V.w.ipar = v.ipar; V.w.mode = 0;
            V.w.mp = metric_par(D, v.par, v.par2);
            V.absval = v.absval ? 1 : 0;
            V.metric = v.kind >= WL_R_METRIC ? 1 : 0;
            anym = anym || V.metric;
        }
        Cc.val[c] = u;
        Cc.power[c] = cols[c].power;
        Cc.moment[c] = cols[c].moment;
    }
    const unsigned long long *n = (const unsigned long long *)n_dev;
    unsigned long long *over = (unsigned long long *)over_dev;
    long long *acc = (long long *)acc_dev;
    hipStream_t st = ctx().stream;
    const unsigned rwg = rg_workgroups(B);
    const dim3 grid(rwg < (unsigned)RS_WG ? rwg : (unsigned)RS_WG), blk(256);
    const int64_t need = (cap * ncol * 5 + 255) / 256;
    const dim3 tgrid((unsigned)(need < RS_ROW_WG ? need : RS_ROW_WG));
    {
        Prof pr(WL_K_SCALAR, 0);
        hipLaunchKernelGGL(k_rs_init, tgrid, blk, 0, st, (long)cap, ncol, n, acc, (long long *)over_dev);
        WL_HIP(hipGetLastError());
    }
    if (!Cc.given) {
        Prof pr(WL_K_MISC, (int64_t)B.cells);
        if (anym) hipLaunchKernelGGL((k_rs_scale<T, D, true>), grid, blk, 0, st, g, B, Cc, (const int *)label, over);
        else hipLaunchKernelGGL((k_rs_scale<T, D, false>), grid, blk, 0, st, g, B, Cc, (const int *)label, over);
        WL_HIP(hipGetLastError());
    }
    {
        Prof pr(WL_K_MISC, (int64_t)B.cells);
        if (anym) hipLaunchKernelGGL((k_rs_sum<T, D, true>), grid, blk, 0, st, g, B, Cc, (const int *)label, (long)cap, (int *)scale, over, acc);
        else hipLaunchKernelGGL((k_rs_sum<T, D, false>), grid, blk, 0, st, g, B, Cc, (const int *)label, (long)cap, (int *)scale, over, acc);
        WL_HIP(hipGetLastError());
    }
    {
        Prof pr(WL_K_SCALAR, 0);
        hipLaunchKernelGGL(k_rs_finish, tgrid, blk, 0, st, (long)cap, ncol, Cc.given, n, (const int *)scale, (const long long *)acc, sum, (long long *)over_dev);
        WL_HIP(hipGetLastError());
    }
    return 0;
}

}  // namespace wl
