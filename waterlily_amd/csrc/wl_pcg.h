// wl_pcg.h -- pcg! and L2 (src/Poisson.jl:123-143,146), the tail of wl_ops.h.
//
// pcg! with device-resident rho/alpha/beta and the four early exits turned into a device flag: once `active` drops, the
// remaining (already enqueued) kernels are no-ops, so no host sync.
// Fusions: [mult + z.eps], [x,r update + z=r*iD + r.z], [direction]; identical per-cell arithmetic.
// want_r2: the caller (solver!) needs L2(p) = r.r right after this call; it is accumulated by the last update kernel.
// Deferred x (WL_OPT_PCG_DEFER_X, default on): in iterations 1..it-1 the update x += alpha*eps (:133) moves from the
// update kernel into the direction kernel that follows it (which streams eps anyway): one array pass less per
// iteration (10T instead of 11T for update+direction).  Same per-cell expression, alpha unchanged in between; the :138
// exit leaves PcgS::xpend so that the direction kernel still applies the owed x update and nothing else.
// (A variant that folded the direction update into the next mult kernel -- eps_new evaluated on the fly at the 7 stencil
// points, one array pass less on paper -- was measured slower and removed: see DESIGN.md "measured dead ends".)
//
// One place per thing: the scalar logic (Poisson.jl:127,131-132,135,137-139) in wl_pcg_scalars.h, called by gate_open and by
// PcgDots' finalizes; what a stage does to a cell in the pcg_*_cells functions, called by the vector kernels (N = V lanes) and
// the scalar ones (N = 1); WHICH KERNELS run and HOW A DOT PRODUCT IS FINISHED in PcgPlan, decided once per call; the kernels of
// a stage and their fall-back in op_pcg_init / _mult / _update / _direction; the iteration in op_pcg.
#pragma once
#include "wl_ops.h"

namespace wl {

// ---- how a dot product is finished and pcg!'s scalar logic applied: one of three forms
//   FINALIZE   a one-workgroup launch after every reducing kernel sums its partials and updates st->pcg in place; the kernels
//              gate on st->pcg.active (every level when the layout rules out the vector kernels, and the levels above 2^25 cells);
//   IN_KERNEL  no such launches: the NEXT kernel sums the producer's <= 1024 partials itself in every workgroup and applies the
//              scalar logic (Gate kind 1..3), the state hops between the two st->slots; one finalize at the end publishes it
//              to st->pcg (single rank, levels of <= 2^25 cells: -2.8 % per step at 256^3 and below);
//   SLAB       z-slab levels: the producer's partials are reduced and summed over the ranks (mailbox or ncclAllReduce) into ONE
//              value, which the consuming kernel's gate treats like a single partial.
enum class PcgForm { FINALIZE, IN_KERNEL, SLAB };
template <class T> struct PcgDots {
    PcgForm form;
    State *st;
    double *partials;
    bool dist, xdef, want_r2;
    double eps10;
    int f32, zcap;
    double *P0, *PA, *PB;   // partials of rho (init) / z.eps (mult) / r.z' or r.r (update); one buffer in the FINALIZE form
    int cur = 0;            // the slot of st->slots holding the current state (IN_KERNEL, SLAB)
    PcgDots(PcgForm f, State *st_, double *partials_, bool dist_, bool xdef_, bool want_r2_, T eps10_, int zcap_)
        : form(f), st(st_), partials(partials_), dist(dist_), xdef(xdef_), want_r2(want_r2_), eps10((double)eps10_), f32(sizeof(T) == 4), zcap(zcap_) {
        const bool own = f != PcgForm::FINALIZE;
        P0 = partials; PA = own ? partials + WL_MAXB : partials; PB = own ? partials + 2 * WL_MAXB : partials;
    }
    Gate base() const { Gate g; g.eps10 = eps10; g.f32 = f32; g.zcap = zcap; return g; }
    // SLAB: the producer's partials become the one value summed over the ranks
    int ready(const double *&part, int &n) const {
        if (form != PcgForm::SLAB) return 0;
        Prof pr(WL_K_SCALAR, 0);
        WL_TRY((reduce_allreduce<1>(part, n, (int)RED_SUM, 0.0, st->red)));
        part = st->red;
        n = 1;
        return 0;
    }
    // ---- after the init kernel (rho = r.z, :126-127)
    int after_init(int np) const {
        if (form != PcgForm::FINALIZE) return 0;
        State *s = st;
        const double e10 = eps10;
        const int f = f32;
        return launch_finalize<1>(dist, partials, np, RED_SUM, 0.0, st->red, [=] __device__(const double *v) {
            pcg_after_init(s->pcg, v[0], e10, f);
        });
    }
    // ---- the gate of mult number n (it finishes rho when n == 1), then what follows the kernel (alpha, :131-132)
    int gate_mult(int n, int np0, Gate &g) {
        g = base();
        if (form == PcgForm::FINALIZE) { g.active = &st->pcg.active; return 0; }
        if (n == 1) {
            const double *gp = P0; int gn = np0;
            WL_TRY(ready(gp, gn));
            g.kind = 1; g.part = gp; g.np = gn; g.out = &st->slots[0]; cur = 0;
        } else { g.kind = 4; g.in = &st->slots[cur]; }
        return 0;
    }
    int after_mult(int np) const {
        if (form != PcgForm::FINALIZE) return 0;
        State *s = st;
        const int f = f32;
        return launch_finalize<1>(dist, partials, np, RED_SUM, 0.0, st->red, [=] __device__(const double *v) {
            pcg_after_mult(s->pcg, v[0], f);
        });
    }
    // ---- the update kernel's gate (it finishes z.eps), then what follows it (the new rho and beta, :137-139; :135 and r.r after the last)
    int gate_update(int npA, Gate &g) {
        g = base();
        if (form == PcgForm::FINALIZE) { g.active = &st->pcg.active; g.s0 = &st->pcg.alpha; return 0; }
        const double *gp = PA; int gn = npA;
        WL_TRY(ready(gp, gn));
        g.kind = 2; g.part = gp; g.np = gn; g.in = &st->slots[cur]; g.out = &st->slots[cur ^ 1];
        return 0;
    }
    void launched_update() { if (form != PcgForm::FINALIZE) cur ^= 1; }
    int after_update(int np, bool last, bool xnow) const {
        State *s = st;
        const bool wr2 = want_r2;
        const double e10 = eps10;
        const int f = f32;
        if (form == PcgForm::FINALIZE)
            return launch_finalize<1>(dist, partials, np, RED_SUM, 0.0, st->red, [=] __device__(const double *v) {
                if (last) pcg_after_last(s->pcg, v[0], f, wr2);
                else pcg_after_update(s->pcg, v[0], e10, f, xnow);
            });
        if (!last) return 0;
        const int cs = cur;   // the one finalize of the call: finishes r.r (:135) and publishes the state for the host / L2
        return launch_finalize<1>(dist, PB, np, RED_SUM, 0.0, st->red, [=] __device__(const double *v) {
            PcgS sl = s->slots[cs];
            pcg_after_last(sl, v[0], f, wr2);
            s->pcg = sl;
        });
    }
    // ---- the direction kernel's gate (it finishes r.z')
    int gate_direction(int npB, Gate &g) {
        g = base();
        if (form == PcgForm::FINALIZE) {
            g.active = &st->pcg.active; g.also = xdef ? &st->pcg.xpend : nullptr; g.s0 = &st->pcg.alpha; g.s1 = &st->pcg.beta;
            return 0;
        }
        const double *gp = PB; int gn = npB;
        WL_TRY(ready(gp, gn));
        g.kind = 3; g.part = gp; g.np = gn; g.in = &st->slots[cur]; g.out = &st->slots[cur ^ 1]; g.also_x = 1;
        return 0;
    }
    void launched_direction() { if (form != PcgForm::FINALIZE) cur ^= 1; }
};

// WL_OPT_PCG_RECOMPUTE_AEPS on a level of `cells` interior cells: 1 (default) = levels of 2^22 .. 2^26 cells, 3 = every level
// below 2^26, 2 = every level, 0 = never
inline bool pcg_recompute_aeps(long cells) {
    const int v = opt(WL_OPT_PCG_RECOMPUTE_AEPS);
    return v == 2 || (v == 3 && cells < (1L << 26)) || (v == 1 && cells < (1L << 26) && cells >= (1L << 22));
}
// WL_OPT_PCG_DOTS_IN_KERNEL: 1 (default) = on levels of at most 2^25 cells, 2 = on every level, 0 = never; a z-slab run
// (distr: the sums cross the ranks between the kernels either way) takes any non-zero value
inline bool pcg_dots_in_kernel(long cells, bool distr) {
    const int v = opt(WL_OPT_PCG_DOTS_IN_KERNEL);
    return distr ? v != 0 : (v == 2 || (v == 1 && cells <= (1L << 25)));
}

// ---- what one call of pcg! launches, decided once
struct PcgPlan {
    Range R;        // the interior cells
    bool vec;       // streaming pcg kernels in 16-B vector form where the layout allows (WL_OPT_PCG_VEC = 0: scalar range kernels)
    bool xdef;      // x += alpha*eps in the direction kernel (WL_OPT_PCG_DEFER_X)
    bool zrec;      // z' = r*iD is not stored
    bool zst;       // z = A*eps is not stored either
    bool distr;     // the level is a z-slab of a multi-rank run
    PcgForm form;
    int zcap;       // IN_KERNEL: the kernels cut z into at most this many chunks (Gate::zcap)
    bool own() const { return form != PcgForm::FINALIZE; }   // the vector kernels must take the launch: the gates live in them
};
template <class T, int D> PcgPlan pcg_plan(const LevelT<T> &p) {
    constexpr int V = Vec16<T>::V;
    PcgPlan pl;
    pl.R = r_inside(p.g);
    pl.vec = false;
    if constexpr (D == 3) pl.vec = pcg_vec_ok<T>(p.g);
    pl.xdef = opt(WL_OPT_PCG_DEFER_X) != 0;
    // z' = r*iD (:136) is not stored (WL_OPT_PCG_RECOMPUTE_PRECOND, default on): the direction kernel recomputes it from r
    // and iD (iD is a row constant away from the body), one array write + one read less per iteration; z keeps A*eps.
    pl.zrec = opt(WL_OPT_PCG_RECOMPUTE_PRECOND) != 0;
    // z = A*eps is not stored either (pcg_recompute_aeps; 3-D vector kernels): the update kernel is a second 7-point kernel
    // over eps that forms the same A*eps again (same expression, same operands => same bits) and applies
    // r -= alpha*(A*eps) in its epilogue.  Per iteration one array write (mult) and one array read (update) are replaced
    // by a second read of eps (with its halo rows and planes).  Measured: 512^3 mult 0.303 -> 0.224 ms but update
    // 0.344 -> 0.449 ms (the 7-point form of the update runs at 4.1 TB/s): no gain; 256^3 as the finest level: -2.5 % per
    // step; levels of 128^3 cells and below are latency-bound and lose 5-10 % of a pcg! call to the heavier update kernel
    // (tools/midlevels.py PCG_RECOMPUTE_AEPS=3,0: 194 / 175, 110 / 101, 77 / 72 us).
    pl.zst = false;
    if constexpr (D == 3) pl.zst = pcg_recompute_aeps(pl.R.count()) && pl.vec && pl.zrec;
    // how the dot products are finished (PcgDots above).  The in-kernel sums want few partials: the kernels of such a
    // call cut z into at most `zcap` chunks (Gate::zcap); levels above 2^25 cells keep the finalize launches
    // (pcg_dots_in_kernel): there the cap costs the streaming kernels more than the launches it saves (512^3: +0.8 %).
    const int tpp_v = D == 3 ? (((p.g.n[0] - 2 + 64 * V - 1) / (64 * V)) * ((p.g.n[1] - 2 + 3) / 4) + 7) / 8 * 8 : 0;
    pl.distr = p.g.dist && ctx().comm && ctx().comm->size > 1;
    const bool gates = pl.vec && pl.xdef && pl.zrec && pl.R.count() > 0 && tpp_v > 0 && pcg_dots_in_kernel(pl.R.count(), pl.distr) &&
                       (pl.distr || tpp_v <= WL_PCG_PARTIALS);
    pl.form = !gates ? PcgForm::FINALIZE : (pl.distr ? PcgForm::SLAB : PcgForm::IN_KERNEL);
    pl.zcap = pl.form == PcgForm::IN_KERNEL ? std::max(WL_PCG_PARTIALS / std::max(tpp_v, 1), 1) : 0;
    return pl;
}

// What a vector launch returned (0 = launched, > 0 = an error, < 0 = the level does not fit the launch), as what the stage does
// next: PCG_RAN, PCG_SCALAR (fall back to the scalar range kernel), or an error code to return -- the launch's own, or
// WL_E_STATE for a rejection where the gates live in the vector kernels (`must`: no scalar kernel could stand in).
enum { PCG_RAN = 0, PCG_SCALAR = -1 };
inline int pcg_vec_launched(int rv, bool must, const char *what) {
    if (rv < 0 && must) return fail(WL_E_STATE, what, __FILE__, __LINE__);
    return rv < 0 ? PCG_SCALAR : rv;
}

// ---- what the stages do to N cells (N = V lanes of a 16-B vector, or 1): each expression of pcg! once, for the vector
// kernels and the scalar ones alike.  They are separate steps, not one function per stage, because a kernel STORES between
// them: x before r is formed, x and r before iD is requested -- a load may not pass a store it might alias, and with the
// operands of a later step requested before the stores of an earlier one the update kernels hold them in registers for
// one wave of occupancy less (rowvec Float32 6 -> 5, 7-point Float32 4 -> 3: hipcc -Rpass-analysis=kernel-resource-usage).
// :125-126 and :136-137  z = r*iD ; r.z
template <class T, int N> __device__ __forceinline__ void pcg_precond_cells(const T (&r)[N], const T (&id)[N], T (&z)[N], double &acc) {
_Pragma("unroll")
    for (int v = 0; v < N; ++v) { z[v] = r[v] * id[v]; acc += (double)r[v] * (double)z[v]; }
}
// :133  x += alpha eps  (update kernel, or deferred to the direction kernel)
template <class T, int N> __device__ __forceinline__ void pcg_x_cells(T alpha, T (&x)[N], const T (&e)[N]) {
_Pragma("unroll")
    for (int v = 0; v < N; ++v) x[v] += alpha * e[v];
}
// :133  r -= alpha z
template <class T, int N> __device__ __forceinline__ void pcg_r_cells(T alpha, T (&r)[N], const T (&z)[N]) {
_Pragma("unroll")
    for (int v = 0; v < N; ++v) r[v] = r[v] - alpha * z[v];
}
// :146  r.r  (after the last update, when the caller wants L2(p) from this call)
template <class T, int N> __device__ __forceinline__ void pcg_r2_cells(const T (&r)[N], double &acc) {
_Pragma("unroll")
    for (int v = 0; v < N; ++v) acc += (double)r[v] * (double)r[v];
}
// :140  eps = beta eps + z'.  zr = z', or r when z' is recomputed as r*iD (zrec: :136); id is read only then
template <class T, int N> __device__ __forceinline__ void pcg_direction_cells(T beta, T (&e)[N], const T (&zr)[N], const T (&id)[N], bool zrec) {
_Pragma("unroll")
    for (int v = 0; v < N; ++v) e[v] = beta * e[v] + (zrec ? zr[v] * id[v] : zr[v]);
}

// ---- :125-127  eps = z = r*iD ; rho = r.z.  pre_np >= 0: both are already there (op_prolong_increment_fused).  *np0 = partials of rho
template <class T, int D>
int op_pcg_init(const LevelT<T> &p, const PcgPlan &pl, PcgDots<T> &dots, int pre_np, int *np0) {
    using VA = VecA<T>;
    const LevelT<T> q = p;
    const int n0 = p.g.n[0];
    const bool zrec = pl.zrec;
    int rv = PCG_SCALAR;
    if (pre_np >= 0) { rv = PCG_RAN; *np0 = pre_np; }
    else if (pl.vec) {
        rv = launch_rowvec<T, 1, true>(WL_K_PCG_INIT, p.g,
            [=] __device__(long o, int, int, const Pre &) { return VA::load(q.r + o); },
            [=] __device__(long o, int i, int, int, const VA &rr, const auto &rk, double *acc, const Pre &) {
                const VA id = row_iD<T>(rk, q.iD, o, i, n0);
                VA zv;
                pcg_precond_cells<T, VA::V>(rr.v, id.v, zv.v, acc[0]);
                if (!zrec) zv.store(q.z + o);
                zv.store(q.eps + o);
            }, p.rowc, dots.P0, np0, dots.base());
    }
    rv = pcg_vec_launched(rv, pl.own(), "pcg: vector init kernel rejected");
    if (rv > 0) return rv;
    if (rv == PCG_SCALAR)
        WL_TRY((launch_range_red<1>(WL_K_PCG_INIT, pl.R, [=] __device__(int i, int j, int k, double(&acc)[1]) {
            const long I = q.g.at(i, j, k);
            const T r[1] = {q.r[I]}, id[1] = {q.iD[I]};
            T z[1];
            pcg_precond_cells<T, 1>(r, id, z, acc[0]);
            if (!zrec) q.z[I] = z[0];
            q.eps[I] = z[0];
        }, dots.partials, RED_SUM, 0.0, np0)));
    return dots.after_init(*np0);
}

// ---- :129-132  perBC!(eps) ; z = A eps ; z.eps ; alpha.  n: the iteration; np0: partials of rho; *npA = partials of z.eps
template <class T, int D>
int op_pcg_mult(const LevelT<T> &p, const PcgPlan &pl, PcgDots<T> &dots, int n, int np0, int permask, bool ghost_z, int *npA) {
    using VA = VecA<T>;
    const LevelT<T> q = p;
    State *st = dots.st;
    const bool zst = pl.zst;
    WL_TRY((op_bc_per<T, D>(p.g, p.eps, permask, false)));  // (x/y copies; the z-slab halo exchange follows)
    bool exchanged = false;
    int rv = PCG_SCALAR;
    if constexpr (D == 3) {
        if (stencil7_ok<T>(p.g)) {
            exchanged = true;
            Gate gate;
            WL_TRY(dots.gate_mult(n, np0, gate));
            rv = launch_stencil7_halo<T, 1>(WL_K_PCG_MULT, p.g, p.eps, SrcArray<T>{p.eps}, p.L, p.rowc, (const T *)nullptr, (const T *)nullptr,
                [=] __device__(long o, int, int, int, const VA &ae, const VA &ec, const VA &, const VA &, const auto &, double *acc, const Pre &) {
                if (!zst) ae.store(q.z + o);
_Pragma("unroll")
                for (int v = 0; v < VA::V; ++v) acc[0] += (double)ae.v[v] * (double)ec.v[v];
            }, dots.PA, npA, gate);
            rv = pcg_vec_launched(rv, pl.own(), "pcg: vector mult kernel rejected");
            if (rv > 0) return rv;
        }
    }
    if (!exchanged) WL_TRY((halo_exchange<T>(p.g, p.eps, 1, 1)));
    if (rv == PCG_SCALAR)
        WL_TRY((launch_range_red<1>(WL_K_PCG_MULT, pl.R, [=] __device__(int i, int j, int k, double(&acc)[1]) {
            if (!st->pcg.active) return;
            const long I = q.g.at(i, j, k);
            const T v = mult1r<T, D>(q.g, q.L, q.eps, I);
            q.z[I] = v;
            acc[0] += (double)v * (double)q.eps[I];
        }, dots.partials, RED_SUM, 0.0, npA)));
    if (ghost_z && permask != 0) {
        // z⋅ϵ is a whole-array dot (Poisson.jl:131).  ϵ's ghost cells are zero except in the planes perBC! fills (:129), and
        // there z may be non-zero: on level 1 z is flow.σ, whose top ghost cells keep conv_diff!'s flux scratch.  Surface sum
        // over the periodic planes, appended to the partials of the interior sum.
        int planes = 0, nps = 0;
        for (int j = 0; j < D; ++j) if ((permask >> j) & 1) planes |= 3 << (2 * j);
        const G gg = p.g;
        WL_TRY((launch_shell_red(WL_K_PCG_MULT, p.g, planes, [=] __device__(int i, int j, int k, double(&acc)[1]) {
            const long I = gg.at(i, j, k);
            acc[0] += (double)q.z[I] * (double)q.eps[I];
        }, (rv == PCG_RAN ? dots.PA : dots.partials) + *npA, RED_SUM, 0.0, &nps, pl.own() ? 32 : 256)));
        *npA += nps;
    }
    return dots.after_mult(*npA);
}

// ---- :133-139  x += alpha eps (now or deferred) ; r -= alpha z ; z' = r*iD ; r.z' ; beta  (last iteration: :135, r.r).
// npA: partials of z.eps; *npB = partials of r.z' (r.r)
template <class T, int D>
int op_pcg_update(const LevelT<T> &p, const PcgPlan &pl, PcgDots<T> &dots, int npA, bool last, int *npB) {
    using VA = VecA<T>;
    const LevelT<T> q = p;
    State *st = dots.st;
    const int n0 = p.g.n[0];
    const bool zrec = pl.zrec, want_r2 = dots.want_r2;
    const bool xnow = last || !pl.xdef;   // x += alpha*eps in this kernel (else in the direction kernel)
    int rv = PCG_SCALAR;
    Gate gate;
    WL_TRY(dots.gate_update(npA, gate));
    if constexpr (D == 3) {
        if (pl.zst) {   // 7-point kernel over eps: Ae == the z the mult kernel would have stored; a = r, b = x (when x is due)
            const T *xin = xnow ? (const T *)q.x : (const T *)nullptr;
            rv = launch_stencil7<T, 1>(WL_K_PCG_UPDATE, p.g, SrcArray<T>{p.eps}, p.L, p.rowc, (const T *)q.r, xin,
                [=] __device__(long o, int i, int, int, const VA &ae, const VA &ec, const VA &r0, const VA &x0, const auto &rk, double *acc, const Pre &pre) {
                    const T alpha = (T)pre.s0;
                    VA rr = r0;
                    if (xnow) { VA xv = x0; pcg_x_cells<T, VA::V>(alpha, xv.v, ec.v); xv.store(q.x + o); }
                    pcg_r_cells<T, VA::V>(alpha, rr.v, ae.v);
                    rr.store(q.r + o);
                    if (!last) { const VA id = row_iD<T>(rk, q.iD, o, i, n0); VA zn; pcg_precond_cells<T, VA::V>(rr.v, id.v, zn.v, acc[0]); }
                    else if (want_r2) pcg_r2_cells<T, VA::V>(rr.v, acc[0]);
                }, dots.PB, npB, gate);
            rv = pcg_vec_launched(rv, true, "pcg: 7-point update kernel rejected");
            if (rv > 0) return rv;
        }
    }
    if (pl.vec && rv == PCG_SCALAR) {
        struct UD { VA r, z, x, e; };
        rv = launch_rowvec<T, 1, true>(WL_K_PCG_UPDATE, p.g,
            [=] __device__(long o, int, int, const Pre &) {
                UD d;
                d.r = VA::load(q.r + o);
                d.z = VA::load(q.z + o);
                if (xnow) { d.x = VA::load(q.x + o); d.e = VA::load(q.eps + o); }
                return d;
            },
            [=] __device__(long o, int i, int, int, const UD &d, const auto &rk, double *acc, const Pre &pre) {
                const T alpha = (T)pre.s0;
                VA rr = d.r;
                if (xnow) { VA xv = d.x; pcg_x_cells<T, VA::V>(alpha, xv.v, d.e.v); xv.store(q.x + o); }
                pcg_r_cells<T, VA::V>(alpha, rr.v, d.z.v);
                rr.store(q.r + o);
                if (!last) {
                    const VA id = row_iD<T>(rk, q.iD, o, i, n0);
                    VA zn;
                    pcg_precond_cells<T, VA::V>(rr.v, id.v, zn.v, acc[0]);
                    if (!zrec) zn.store(q.z + o);   // (else) the direction kernel recomputes r*iD: z' is never stored
                } else if (want_r2) pcg_r2_cells<T, VA::V>(rr.v, acc[0]);
            }, p.rowc, dots.PB, npB, gate);
        rv = pcg_vec_launched(rv, pl.own(), "pcg: vector update kernel rejected");
        if (rv > 0) return rv;
    }
    if (rv == PCG_RAN) dots.launched_update();
    else
        WL_TRY((launch_range_red<1>(WL_K_PCG_UPDATE, pl.R, [=] __device__(int i, int j, int k, double(&acc)[1]) {
            if (!st->pcg.active) return;
            const long I = q.g.at(i, j, k);
            const T alpha = (T)st->pcg.alpha;
            if (xnow) { T x[1] = {q.x[I]}; const T e[1] = {q.eps[I]}; pcg_x_cells<T, 1>(alpha, x, e); q.x[I] = x[0]; }
            T r[1] = {q.r[I]};
            const T z[1] = {q.z[I]};
            pcg_r_cells<T, 1>(alpha, r, z);
            q.r[I] = r[0];
            if (!last) {
                const T id[1] = {q.iD[I]};
                T zn[1];
                pcg_precond_cells<T, 1>(r, id, zn, acc[0]);
                if (!zrec) q.z[I] = zn[0];
            } else if (want_r2) pcg_r2_cells<T, 1>(r, acc[0]);
        }, dots.partials, RED_SUM, 0.0, npB)));
    return dots.after_update(*npB, last, xnow);
}

// ---- :140  eps = beta eps + z'  (+ the deferred x += alpha eps).  npB: partials of r.z'
// gate: the kernel runs when pcg is active, or (deferred x) when only the x update of the :138 exit is owed
template <class T, int D>
int op_pcg_direction(const LevelT<T> &p, const PcgPlan &pl, PcgDots<T> &dots, int npB) {
    using VA = VecA<T>;
    const LevelT<T> q = p;
    State *st = dots.st;
    const int n0 = p.g.n[0];
    const bool xdef = pl.xdef, zrec = pl.zrec;
    int rv = PCG_SCALAR;
    Gate gate;
    WL_TRY(dots.gate_direction(npB, gate));
    if (pl.vec) {
        struct DD { VA e, x, z; };
        rv = launch_rowvec<T, 0, true>(WL_K_PCG_DIR, p.g,
            [=] __device__(long o, int, int, const Pre &pre) {
                DD d;
                d.e = VA::load(q.eps + o);
                if (xdef) d.x = VA::load(q.x + o);
                if (pre.act) d.z = VA::load((zrec ? q.r : q.z) + o);
                return d;
            },
            [=] __device__(long o, int i, int, int, const DD &d, const auto &rk, double *, const Pre &pre) {
                VA ev = d.e, id;
                if (pre.act && zrec) id = row_iD<T>(rk, q.iD, o, i, n0);   // z' = r*iD (:136) recomputed
                if (xdef) { VA xv = d.x; pcg_x_cells<T, VA::V>((T)pre.s0, xv.v, ev.v); xv.store(q.x + o); }   // :133, deferred
                if (!pre.act) return;
                pcg_direction_cells<T, VA::V>((T)pre.s1, ev.v, d.z.v, id.v, zrec);
                ev.store(q.eps + o);
            }, p.rowc, nullptr, nullptr, gate);
        rv = pcg_vec_launched(rv, pl.own(), "pcg: vector direction kernel rejected");
        if (rv > 0) return rv;
    }
    if (rv == PCG_RAN) { dots.launched_direction(); return 0; }
    return launch_range(WL_K_PCG_DIR, pl.R, [=] __device__(int i, int j, int k) {
        const int act = st->pcg.active;
        if (!act && !(xdef && st->pcg.xpend)) return;
        const long I = q.g.at(i, j, k);
        T e[1] = {q.eps[I]};
        if (xdef) { T x[1] = {q.x[I]}; pcg_x_cells<T, 1>((T)st->pcg.alpha, x, e); q.x[I] = x[0]; }
        if (!act) return;
        const T zr[1] = {zrec ? q.r[I] : q.z[I]}, id[1] = {zrec ? q.iD[I] : (T)0};
        pcg_direction_cells<T, 1>((T)st->pcg.beta, e, zr, id, zrec);
        q.eps[I] = e[0];
    });
}

// pcg!  src/Poisson.jl:123-143
template <class T, int D>
int op_pcg(const LevelT<T> &p, int it, int permask, double *partials, State *st, bool want_r2 = false,
           int pre_np = -1,     // pre_np >= 0: eps = r*iD and the partials of rho are already there (op_prolong_increment_fused)
           bool ghost_z = false) {   // z's ghost cells may hold non-zero values (level 1: z is flow.sigma, see op_sigma_ghosts)
    const PcgPlan pl = pcg_plan<T, D>(p);
    PcgDots<T> dots(pl.form, st, partials, p.g.dist, pl.xdef, want_r2, (T)10 * Lim<T>::eps, pl.zcap);
    int np0 = 0, npA = 0, npB = 0;   // partials of rho, of z.eps, of r.z' (r.r)
    WL_TRY((op_pcg_init<T, D>(p, pl, dots, pre_np, &np0)));                             // :125-127
    for (int n = 1; n <= it; ++n) {
        const bool last = (n == it);
        WL_TRY((op_pcg_mult<T, D>(p, pl, dots, n, np0, permask, ghost_z, &npA)));       // :129-132
        WL_TRY((op_pcg_update<T, D>(p, pl, dots, npA, last, &npB)));                    // :133-139
        if (last) break;                                                                // :135
        WL_TRY((op_pcg_direction<T, D>(p, pl, dots, npB)));                             // :140
    }
    return 0;
}

// L2(p) = r.r  src/Poisson.jl:146 -> st->pcg.r2.  after_pcg: skip the work when the pcg! call just before already
// produced it (r2_valid, see op_pcg want_r2); the kernels are still enqueued (no host decision) but return at once.
template <class T, int D>
int op_L2(const LevelT<T> &p, double *partials, State *st, bool after_pcg = false) {
    const LevelT<T> q = p;
    int np = 0;
    int rcv = -1;
    if constexpr (D == 3) {
        if (pcg_vec_ok<T>(p.g)) {   // 16-B streaming form; when the pcg! before it already produced r.r the
            using VA = VecA<T>;                      // gate closes and every workgroup leaves at once
            Gate gate;
            if (after_pcg) { gate.active = &st->pcg.r2_valid; gate.inv = 1; }
            rcv = launch_rowvec<T, 1, false>(WL_K_DOT, p.g,
                [=] __device__(long o, int, int, const Pre &) { return VA::load(q.r + o); },
                [=] __device__(long, int, int, int, const VA &rr, const auto &, double *acc, const Pre &) {
_Pragma("unroll")
                    for (int v = 0; v < VA::V; ++v) acc[0] += (double)rr.v[v] * (double)rr.v[v];
                }, (const T *)nullptr, partials, &np, gate);
            if (rcv > 0) return rcv;
        }
    }
    if (rcv != 0)
    WL_TRY((launch_range_red<1>(WL_K_DOT, r_inside(p.g), [=] __device__(int i, int j, int k, double(&acc)[1]) {
        if (after_pcg && st->pcg.r2_valid) return;
        const double v = (double)q.r[q.g.at(i, j, k)];
        acc[0] += v * v;
    }, partials, RED_SUM, 0.0, &np)));
    return launch_finalize<1>(p.g.dist, partials, np, RED_SUM, 0.0, st->red, [=] __device__(const double *v) {
        if (after_pcg && st->pcg.r2_valid) return;
        st->pcg.r2 = (double)(T)v[0];
    });
}

}  // namespace wl
