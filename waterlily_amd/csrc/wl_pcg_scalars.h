// wl_pcg_scalars.h -- pcg!'s scalar logic (src/Poisson.jl:127,131-132,135,137-139), stated ONCE: the in-kernel form
// (gate_open, wl_stencil7.h) and every one-workgroup finalize epilogue of op_pcg (wl_pcg.h) call these functions, and
// tests/pcg_host.cpp drives them on the host.  Nothing of HIP is included here.
//
// The scalars are doubles that hold values already rounded to the solver's element type T (f32 != 0: Float32): pcg_rnd
// and pcg_div are (double)(float)x and (double)((float)a / (float)b) then -- the operations of `(T)rho / (T)v` in T
// arithmetic -- and the identity / a plain division for Float64.
#pragma once
#if defined(__HIPCC__)
#define WL_HD __host__ __device__ __forceinline__
#else
#define WL_HD inline
#endif

namespace wl {

struct PcgS {
    double rho, alpha, beta;   // each holding a value already rounded to T
    double r2;                 // L2(p) = r.r
    int active;                // pcg still running
    int xpend;                 // pcg stopped at :138 with x += alpha*eps still owed (deferred-x form, see op_pcg)
    int nupd;                  // number of (x,r) updates pcg performed
    int r2_valid;              // the last pcg! update already produced r.r (solver! can skip the separate L2 pass)
};

WL_HD double pcg_rnd(double x, int f32) { return f32 ? (double)(float)x : x; }
WL_HD double pcg_div(double a, double b, int f32) { return f32 ? (double)((float)a / (float)b) : a / b; }
// v = r.z (:126-127).  alpha, beta and r2 are zeroed with the rest: nothing reads them before they are set again --
// alpha by pcg_after_mult and beta by pcg_after_update while `active` (the only state in which a kernel uses them; xpend,
// the other way into the direction kernel, is raised only after both), r2 by pcg_after_last or op_L2 before any reader.
WL_HD void pcg_after_init(PcgS &s, double v, double eps10, int f32) {
    const double rho = pcg_rnd(v, f32);
    s.rho = rho; s.alpha = 0.0; s.beta = 0.0; s.r2 = 0.0;
    s.nupd = 0; s.r2_valid = 0; s.xpend = 0;
    s.active = !((rho < 0 ? -rho : rho) < eps10);
}
// v = z.eps (:131-132)
WL_HD void pcg_after_mult(PcgS &s, double v, int f32) {
    s.xpend = 0;   // any owed x update was applied by the direction kernel before this mult
    if (!s.active) return;
    const double alpha = pcg_div(s.rho, pcg_rnd(v, f32), f32);
    const double aa = alpha < 0 ? -alpha : alpha;
    s.alpha = alpha;
    if (aa < 1e-2 || aa > 1e2) s.active = 0;   // :132
}
// v = r.z' after a non-final update (:137-139); xnow: that update already applied x += alpha*eps
WL_HD void pcg_after_update(PcgS &s, double v, double eps10, int f32, bool xnow) {
    if (!s.active) return;
    s.nupd += 1;
    const double rho2 = pcg_rnd(v, f32);
    if ((rho2 < 0 ? -rho2 : rho2) < eps10) { s.active = 0; s.xpend = !xnow; return; }   // :138
    s.beta = pcg_div(rho2, s.rho, f32);
    s.rho = rho2;
}
// after the last update (:135); v = r.r when the caller wants L2(p) from this call (want_r2)
WL_HD void pcg_after_last(PcgS &s, double v, int f32, bool want_r2) {
    if (!s.active) return;
    s.nupd += 1;
    if (want_r2) { s.r2 = pcg_rnd(v, f32); s.r2_valid = 1; }
    s.active = 0;
}

}  // namespace wl
