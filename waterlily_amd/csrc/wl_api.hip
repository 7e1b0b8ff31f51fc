// wl_api.hip -- C ABI (include/wlhip.h) + host orchestration: Vcycle!, solver!, project!, mom_step!.
#include <cstdarg>
#include <cstring>
#include <memory>

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <rccl/rccl.h>

#include "wl_ops.h"
#include "wl_coarse.h"
#include "wl_measure.h"
#include "wl_mesh.h"
#include "wl_stats.h"
#include "wl_budget.h"
#include "wl_probe.h"
#include "wl_integrals.h"
#include "wl_forces.h"
#include "wl_surface.h"
#include "wl_iso.h"
#include "wl_render.h"
#include "wl_downsample.h"
#include "wl_hist.h"
#include "wl_twopoint.h"
#include "wl_regions.h"
#include "wl_region_sums.h"
#include "wl_scene.h"
#include "wl_volume.h"

namespace wl {

// ------------------------------------------------------------------------------------------ communicators
// RCCL over xGMI: neighbour send/recv pairs and world collectives, enqueued on the compute stream (so they are
// ordered with the kernels that produce/consume the planes without host synchronisation).
struct RcclComm : Comm {
    ncclComm_t nc = nullptr;    // world collectives (all-reduce, all-gather), always on the compute stream
    ncclComm_t nch = nullptr;   // halo send/recv: a split of `nc`, so that exchanges running on the comm stream (halo_begin)
                                // never share a communicator with a collective on the compute stream; == nullptr: use nc
    ~RcclComm() override {
        if (nch) ncclCommDestroy(nch);
        if (nc) ncclCommDestroy(nc);
    }
    int chk(ncclResult_t r, const char *what) {
        if (r == ncclSuccess) return 0;
        ctx().err = std::string("rccl: ") + what + ": " + ncclGetErrorString(r);
        return WL_E_STATE;
    }
    int do_allreduce(double *dev, int n, int op) override {
        return chk(ncclAllReduce(dev, dev, (size_t)n, ncclDouble, op == 0 ? ncclSum : ncclMax, nc, ctx().stream), "allreduce");
    }
    int do_sendrecv(const void *slo, void *rlo, const void *shi, void *rhi, size_t bytes, int plo, int phi) override {
        int rc = chk(ncclGroupStart(), "groupStart");
        if (rc) return rc;
        // order: my upper planes go up and fill the lower halo of peer_hi, whose first receive from me is its recv_lo, ...
        // (with a 2-rank ring both peers are the same rank: k-th send must meet the k-th receive of that peer)
        ncclComm_t h = nch ? nch : nc;
        // every call is checked; on an error the group is still closed (an open group would swallow every later call)
        if (!rc && shi) rc = chk(ncclSend(shi, bytes, ncclChar, phi, h, ctx().stream), "send(up)");
        if (!rc && rlo) rc = chk(ncclRecv(rlo, bytes, ncclChar, plo, h, ctx().stream), "recv(from below)");
        if (!rc && slo) rc = chk(ncclSend(slo, bytes, ncclChar, plo, h, ctx().stream), "send(down)");
        if (!rc && rhi) rc = chk(ncclRecv(rhi, bytes, ncclChar, phi, h, ctx().stream), "recv(from above)");
        const std::string first = ctx().err;
        const int rce = chk(ncclGroupEnd(), "groupEnd(sendrecv)");
        if (rc) { ctx().err = first; return rc; }
        return rce;
    }
    int do_allgather(void *buf, size_t bytes) override {
        return chk(ncclAllGather((const char *)buf + (size_t)rank * bytes, buf, bytes, ncclChar, nc, ctx().stream), "allgather");
    }
    int do_group_begin() override { return chk(ncclGroupStart(), "groupStart"); }   // NCCL groups nest
    int do_group_end() override { return chk(ncclGroupEnd(), "groupEnd"); }
};

// Host-callback twin (tests: 2+ ranks sharing one GPU, transport = torch.distributed gloo).  Every operation
// synchronises the stream and stages through pinned host memory: correct, not fast.
struct HostComm : Comm {
    wl_host_sendrecv_fn sr; wl_host_allreduce_fn ar; wl_host_allgather_fn ag; void *user;
    Buf<char, PinnedMem<hipHostMallocDefault>> pin;   // staging, grown to twice what the call needs
    int need(size_t b) { return pin.reserve(b, b * 2); }
    int do_allreduce(double *dev, int n, int op) override {
        double v[8];
        WL_HIP(hipMemcpyAsync(v, dev, sizeof(double) * n, hipMemcpyDeviceToHost, ctx().stream));
        WL_HIP(hipStreamSynchronize(ctx().stream));
        if (ar(user, v, n, op)) return fail(WL_E_STATE, "host allreduce callback failed", __FILE__, __LINE__);
        WL_HIP(hipMemcpyAsync(dev, v, sizeof(double) * n, hipMemcpyHostToDevice, ctx().stream));
        WL_HIP(hipStreamSynchronize(ctx().stream));
        return 0;
    }
    int do_sendrecv(const void *slo, void *rlo, const void *shi, void *rhi, size_t bytes, int plo, int phi) override {
        WL_TRY(need(4 * bytes));
        char *hs_lo = pin.get(), *hr_lo = hs_lo + bytes, *hs_hi = hs_lo + 2 * bytes, *hr_hi = hs_lo + 3 * bytes;
        if (slo) WL_HIP(hipMemcpyAsync(hs_lo, slo, bytes, hipMemcpyDeviceToHost, ctx().stream));
        if (shi) WL_HIP(hipMemcpyAsync(hs_hi, shi, bytes, hipMemcpyDeviceToHost, ctx().stream));
        WL_HIP(hipStreamSynchronize(ctx().stream));
        if (sr(user, slo ? hs_lo : nullptr, slo ? hr_lo : nullptr, shi ? hs_hi : nullptr, shi ? hr_hi : nullptr, (int64_t)bytes, plo, phi))
            return fail(WL_E_STATE, "host sendrecv callback failed", __FILE__, __LINE__);
        if (rlo) WL_HIP(hipMemcpyAsync(rlo, hr_lo, bytes, hipMemcpyHostToDevice, ctx().stream));
        if (rhi) WL_HIP(hipMemcpyAsync(rhi, hr_hi, bytes, hipMemcpyHostToDevice, ctx().stream));
        WL_HIP(hipStreamSynchronize(ctx().stream));
        return 0;
    }
    int do_allgather(void *buf, size_t bytes) override {
        const size_t tot = bytes * (size_t)size;
        WL_TRY(need(tot));
        WL_HIP(hipMemcpyAsync(pin.get() + (size_t)rank * bytes, (char *)buf + (size_t)rank * bytes, bytes, hipMemcpyDeviceToHost, ctx().stream));
        WL_HIP(hipStreamSynchronize(ctx().stream));
        if (ag(user, pin.get(), (int64_t)bytes)) return fail(WL_E_STATE, "host allgather callback failed", __FILE__, __LINE__);
        WL_HIP(hipMemcpyAsync(buf, pin.get(), tot, hipMemcpyHostToDevice, ctx().stream));
        WL_HIP(hipStreamSynchronize(ctx().stream));
        return 0;
    }
};

// Loopback twin (measurement: bench.py --comm loopback): ONE process plays rank `rank` of `size`.  Its neighbours are taken to be
// copies of itself (a periodic stack of this slab): the planes it would send up arrive as the planes from below and vice
// versa (device copies on the stream), a sum over the ranks is `size` times the local value, an all-gather repeats the local
// segment.  Every kernel, split launch and reduction of a rank of the N-GPU run is issued; nothing waits for a wire.
__global__ void k_loop_scale(double *v, int n, double f) { if ((int)threadIdx.x < n) v[threadIdx.x] *= f; }
struct LoopComm : Comm {
    int do_allreduce(double *dev, int n, int op) override {
        if (op != 0) return 0;
        hipLaunchKernelGGL(k_loop_scale, dim3(1), dim3(64), 0, ctx().stream, dev, n, (double)size);
        return (int)hipGetLastError();
    }
    int do_sendrecv(const void *slo, void *rlo, const void *shi, void *rhi, size_t bytes, int, int) override {
        const void *from_below = shi ? shi : slo, *from_above = slo ? slo : shi;
        if (rlo && from_below) WL_HIP(hipMemcpyAsync(rlo, from_below, bytes, hipMemcpyDeviceToDevice, ctx().stream));
        if (rhi && from_above) WL_HIP(hipMemcpyAsync(rhi, from_above, bytes, hipMemcpyDeviceToDevice, ctx().stream));
        return 0;
    }
    int do_allgather(void *buf, size_t bytes) override {
        for (int r = 0; r < size; ++r)
            if (r != rank) WL_HIP(hipMemcpyAsync((char *)buf + (size_t)r * bytes, (const char *)buf + (size_t)rank * bytes, bytes, hipMemcpyDeviceToDevice, ctx().stream));
        return 0;
    }
};

Ctx &ctx() {
    static Ctx c;
    return c;
}
int fail(int code, const char *what, const char *file, int line, const char *who) {
    char buf[512];
    const char *hs = (code > 0 && code < 10000) ? hipGetErrorString((hipError_t)code) : "";
    snprintf(buf, sizeof buf, "wlhip error %d at %s:%d: %s%s%s %s", code, file, line, who ? who : "", who ? ": " : "", what, hs);
    ctx().err = buf;
    return code ? code : WL_E_ARG;
}

Prof::Prof(int kclass, int64_t ncells) : ncell(ncells) {
    Ctx &c = ctx();
    c.launches[kclass] += 1;
    c.cells[kclass] += ncells;
    if (kclass == c.prof_class && ncells >= c.prof_min_cells) {
        auto get = [&c]() {
            hipEvent_t e;
            if (!c.pool.empty()) { e = c.pool.back(); c.pool.pop_back(); }
            else (void)hipEventCreate(&e);
            return e;
        };
        a = get(); b = get();
        timed = true;
        (void)hipEventRecord(a, c.stream);
    }
}
Prof::~Prof() {
    if (timed) {
        Ctx &c = ctx();
        (void)hipEventRecord(b, c.stream);
        c.evts.push_back({a, b, ncell});
    }
}

int check_grid(const wl_grid *g) {
    if (!g) return fail(WL_E_ARG, "null grid", __FILE__, __LINE__);
    if (g->D != 2 && g->D != 3) return fail(WL_E_ARG, "grid.D must be 2 or 3", __FILE__, __LINE__);
    if (g->s[0] != 1) return fail(WL_E_ARG, "grid.s[0] must be 1", __FILE__, __LINE__);
    for (int d = 0; d < g->D; ++d)
        if (g->n[d] < 3) return fail(WL_E_ARG, "grid extents must be >= 3 (one ghost layer per side)", __FILE__, __LINE__);
    if (g->D == 2 && g->n[2] != 1) return fail(WL_E_ARG, "grid.n[2] must be 1 for D==2", __FILE__, __LINE__);
    if (g->s[1] < g->n[0]) return fail(WL_E_ARG, "grid.s[1] < n[0]", __FILE__, __LINE__);
    if (g->D == 3 && g->s[2] < g->s[1] * g->n[1]) return fail(WL_E_ARG, "grid.s[2] < s[1]*n[1]", __FILE__, __LINE__);
    const int64_t sp = g->D == 3 ? g->s[2] * g->n[2] : g->s[1] * g->n[1];
    if (g->sc < sp) return fail(WL_E_ARG, "grid.sc smaller than one component", __FILE__, __LINE__);
    if (g->D == 3 && g->nzg > 0) {
        if (g->own_lo < 0 || g->own_hi >= g->n[2] || g->own_lo > g->own_hi)
            return fail(WL_E_ARG, "grid.own_lo/own_hi outside the local planes", __FILE__, __LINE__);
        if (g->kz0 + g->own_lo < 0 || g->kz0 + g->own_hi > g->nzg - 1)
            return fail(WL_E_ARG, "owned planes outside the global array", __FILE__, __LINE__);
        if (g->zring && (g->kz0 + g->own_lo < 1 || g->kz0 + g->own_hi > g->nzg - 2))
            return fail(WL_E_ARG, "zring: the z ghost planes must not be owned", __FILE__, __LINE__);
    }
    return 0;
}

// ------------------------------------------------------------------------------------------ handles
struct Scratch {
    Buf<double, DevMem> partials;                           // 4 * WL_MAXB doubles
    Buf<State, DevMem> st;                                  // device
    Buf<State, PinnedMem<hipHostMallocDefault>> hst;        // pinned host mirror
    int init() {
        WL_TRY(partials.reserve(4 * WL_MAXB));
        WL_TRY(st.reserve(1));
        WL_HIP(hipMemset(st.get(), 0, sizeof(State)));
        WL_TRY(hst.reserve(1));
        memset(hst.get(), 0, sizeof(State));
        return 0;
    }
    // bring the device scalars to the host (synchronises the stream)
    int fetch() {
        WL_HIP(hipMemcpyAsync(hst.get(), st.get(), sizeof(State), hipMemcpyDeviceToHost, ctx().stream));
        WL_HIP(hipStreamSynchronize(ctx().stream));
        if (ctx().mbox && *ctx().mbox->err_host.get())
            return fail(WL_E_STATE, "mailbox all-reduce: gave up waiting for a peer rank (is every rank still running?)", __FILE__, __LINE__);
        return 0;
    }
};

Scratch &global_scratch(int *rc) {
    // never destroyed: a static's destructor would free device memory at exit, when the HIP runtime may already be gone
    static Scratch &s = *new Scratch();
    static bool ok = false;
    *rc = 0;
    if (!ok) { *rc = s.init(); ok = (*rc == 0); }
    return s;
}

}  // namespace wl

using namespace wl;

struct wl_mg {
    wl_dtype t;
    int D;
    int nlev;
    int permask;
    std::vector<wl_level_desc> lev;
    Scratch sc;
    std::vector<Buf<unsigned char, DevMem>> rowc;   // per level: row constants of L and iD (k_lrow), RC_N values per (j,k) row; D==3 only
    Buf<unsigned char, DevMem> dirty;    // level-0 row flags of wl_mg_update_changed
    bool log_on = false;                 // wl_mg_log: record {n, Linf, L2} per solver iteration
    std::vector<double> log;
    int alloc_rowc() {
        const size_t es = t == WL_F32 ? 4 : 8;
        rowc.resize(nlev);
        for (int l = 0; l < nlev; ++l) {
            const wl_grid &g = lev[l].g;
            if (g.D == 3) WL_TRY(rowc[l].reserve((size_t)g.n[1] * (size_t)g.n[2] * RC_N * es));
        }
        return 0;
    }
};
struct wl_flow {
    wl_dtype t;
    wl_flow_desc d;
    Scratch sc;
    unsigned char *rowfree = nullptr;   // body-free row flags (wl_flow_update); nullptr until built
    Buf<unsigned char, DevMem> rowbuf;  // what rowfree points at once built
    Buf<unsigned char, DevMem> segbuf;  // the same per 64-cell segment of a row (3-D; wl_flow_update's scan only)
    bool seg_valid = false;
    const unsigned char *segfree() const { return (seg_valid && opt(WL_OPT_BDIM_ROWFLAGS)) ? segbuf.get() : nullptr; }
    Buf<int, DevMem> busy;              // compact list of the busy interior rows (j + n1*k), device
    int nbusy = 0;
    int nbusy_lo = 0, nbusy_hi = 0;      // how many of them lie in the first / last owned interior plane (the list is sorted by plane)
    // native measure! (wl_measure.h): per-row band counts / offsets, rows touched by this and by the previous measure!
    Buf<int, DevMem> rowcount;
    Buf<long, DevMem> rowoff;
    Buf<unsigned char, DevMem> touched, prev;
    Buf<unsigned char, DevMem> changed; // rows whose coefficient arrays the last native measure! rewrote (touched now or before)
    bool changed_valid = false;
    bool changed_pending = false;       // `changed` holds rows no update!(pois) has consumed yet: the next measure! ORs into it
    bool prev_valid = false;            // `prev` describes the arrays' current content (else: rewrite every row)
    long nband = -1;                    // result of the last wl_measure_rows (-1: none pending)
};

template <class T> static LevelT<T> lvl(const wl_mg *m, int l) {
    const wl_level_desc &d = m->lev[l];
    LevelT<T> o;
    o.g = mkG(&d.g);
    o.L = (T *)d.L; o.D = (T *)d.D; o.iD = (T *)d.iD; o.x = (T *)d.x; o.eps = (T *)d.eps; o.r = (T *)d.r; o.z = (T *)d.z;
    o.rowc = (opt(WL_OPT_ROW_CONST_L) && l < (int)m->rowc.size()) ? (const T *)m->rowc[l].get() : nullptr;
    return o;
}

// ------------------------------------------------------------------------------------------ MG orchestration
// dirty (optional, D == 3): flags of the level-0 x-rows whose D / iD / row constants can have changed (see
// wl_mg_update_changed); every other row of level 0 keeps what it has.  Levels >= 1 are rebuilt in full (1/8, 1/64 ...).
template <class T, int D> static int mg_update(wl_mg *m, const unsigned char *dirty = nullptr) {
    {
        LevelT<T> p = lvl<T>(m, 0);
        WL_TRY((op_set_diag<T, D>(p.g, p.D, p.iD, p.L, dirty)));
        WL_TRY((halo_exchange<T>(p.g, p.iD, 1, 1)));   // z-slab: the fused smoother evaluates r*iD in the halo planes
        if (D == 3 && m->rowc[0].get()) WL_TRY((op_lrow<T>(p.g, p.L, p.iD, (T *)m->rowc[0].get(), dirty)));
    }
    for (int l = 1; l < m->nlev; ++l) {
        LevelT<T> a = lvl<T>(m, l), b = lvl<T>(m, l - 1);
        WL_TRY((op_restrictL<T, D>(a.g, a.L, b.g, b.L, m->permask)));
        WL_TRY((coarse_L_finish<T, D>(a.g, a.L, b.g, m->permask)));
        WL_TRY((op_set_diag<T, D>(a.g, a.D, a.iD, a.L)));
        WL_TRY((halo_exchange<T>(a.g, a.iD, 1, 1)));
        if (D == 3 && m->rowc[l].get()) WL_TRY((op_lrow<T>(a.g, a.L, a.iD, (T *)m->rowc[l].get())));
    }
    return 0;
}

// Vcycle!  src/MultiLevelPoisson.jl:70-82
// pcg_np (solver! only): receives the partial count when the closing prolongate!+increment! also did the start of the
// pcg! that the caller runs next on level l (eps = r*iD, rho partials), else -1
template <class T, int D> static int mg_vcycle(wl_mg *m, int l, int *pcg_np = nullptr) {
    LevelT<T> fine = lvl<T>(m, l), coarse = lvl<T>(m, l + 1);
    const bool fused = (m->permask == 0) && opt(WL_OPT_SMOOTH_FUSED);   // periodic ghosts of eps are copies, not zeros: keep the two-pass form
    if (fused) WL_TRY((op_smooth_fused<T, D>(fine, fine.eps)));     // r' lives in the eps buffer until the way up
    else WL_TRY((op_jacobi<T, D>(fine, 1, m->permask)));
    // fill!(coarse.x, 0) (MultiLevelPoisson.jl:75) rides in the restriction kernel where the level's ghost cells cannot
    // hold anything but zero (no periodic copy, no halo exchange); otherwise it is a memset of the whole array
    const bool zero_in_restrict = (m->permask == 0) && !coarse.g.dist && !fine.g.dist;
    WL_TRY((op_restrict<T, D>(coarse.g, coarse.r, fine.g, fused ? fine.eps : fine.r, zero_in_restrict ? coarse.x : (T *)nullptr)));
    if (ctx().comm && ctx().comm->size > 1 && fine.g.dist && !coarse.g.dist) {
        // hand-over to the replicated coarse levels: every rank restricted the children it owns
        const int nzl = (fine.g.nzg - 2) / ctx().comm->size / 2;
        WL_TRY(ctx().comm->allgather(coarse.r + coarse.g.s[2], (size_t)nzl * coarse.g.s[2] * sizeof(T)));
    }
    if (!zero_in_restrict) {
        Prof p(WL_K_MISC, coarse.g.cells());
        WL_HIP(hipMemsetAsync(coarse.x, 0, (size_t)span(coarse.g) * sizeof(T), ctx().stream));
    }
    // levels <= 4096 cells: the rest of the recursion + smooth!(coarse) as ONE single-workgroup launch (wl_coarse.h)
    const long tail_cells = coarse_tail_cells();
    bool tail = tail_cells && fused && !coarse.g.dist && coarse.g.interior_cells() <= tail_cells && (m->nlev - (l + 1)) <= CV_MAXLEV;
    if (tail) {
        CoarseArgs<T> ca;
        ca.nlev = m->nlev - (l + 1);
        for (int q = 0; q < ca.nlev; ++q) {
            ca.lev[q] = lvl<T>(m, l + 1 + q);
            if (ca.lev[q].g.dist) tail = false;
        }
        if (tail) {
            Prof p(WL_K_SMOOTH, coarse.g.cells());
            if (opt(WL_OPT_COARSE_PCG_RESIDENT)) hipLaunchKernelGGL((k_coarse_vcycle<T, D, true>), dim3(1), dim3(CV_THREADS), 0, ctx().stream, ca);
            else hipLaunchKernelGGL((k_coarse_vcycle<T, D, false>), dim3(1), dim3(CV_THREADS), 0, ctx().stream, ca);
            WL_HIP(hipGetLastError());
        }
    }
    if (!tail) {
        int pre = -1;
        if (l + 2 < m->nlev) WL_TRY((mg_vcycle<T, D>(m, l + 1, pcg_np ? &pre : nullptr)));
        WL_TRY((op_pcg<T, D>(coarse, 6, m->permask, m->sc.partials.get(), m->sc.st.get(), false, pre)));
    }
    if (pcg_np) *pcg_np = -1;
    if (fused) return op_prolong_increment_fused<T, D>(fine, fine.eps, coarse.g, coarse.x, m->sc.partials.get(), pcg_np);
    WL_TRY((op_prolongate<T, D>(fine.g, fine.eps, coarse.g, coarse.x)));
    return op_increment<T, D>(fine, m->permask);
}

// solver!  src/MultiLevelPoisson.jl:87-99 (nlev>1) / src/Poisson.jl:162-172 (nlev==1).
// One host synchronisation per iteration: the r2 < tol test (:95).
// divu / gu: the right-hand side is div(u) of this velocity field, evaluated inside residual! (project!, single device)
// L∞(p) = maximum(abs, p.r)  src/Poisson.jl:147 -> st->out[1]
template <class T, int D> static int mg_Linf(wl_mg *m, int l) {
    LevelT<T> p = lvl<T>(m, l);
    const T *r = p.r;
    return op_reduce<T, D>(p.g, WL_K_DOT, RED_MAX, 0.0, [=] __device__(long I) { const double v = (double)r[I]; return v < 0 ? -v : v; },
                           m->sc.partials.get(), m->sc.st.get(), 1, true);   // the whole array, ghost cells included
}
// one row of the reference's solver log: `@log ", $n, $(L∞(p)), $r₂\n"` (Poisson.jl:164,167; MultiLevelPoisson.jl:90,94)
template <class T, int D> static int mg_log_row(wl_mg *m, int n, bool have_r2) {
    if (!have_r2) WL_TRY((op_L2<T, D>(lvl<T>(m, 0), m->sc.partials.get(), m->sc.st.get(), false)));
    WL_TRY((mg_Linf<T, D>(m, 0)));
    WL_TRY(m->sc.fetch());
    m->log.push_back((double)n); m->log.push_back(m->sc.hst.get()->out[1]); m->log.push_back(m->sc.hst.get()->pcg.r2);
    return 0;
}
template <class T, int D> static int mg_solve(wl_mg *m, double tol, int itmx, int *n_iter, const T *divu = nullptr, const G *gu = nullptr,
                                              bool halo_begun = false) {
    LevelT<T> p = lvl<T>(m, 0);
    WL_TRY((op_residual<T, D>(p, m->permask, m->sc.partials.get(), m->sc.st.get(), divu, gu, halo_begun)));
    int n = 0;
    if (m->log_on) WL_TRY((mg_log_row<T, D>(m, 0, false)));
    while (n < itmx) {
        int pre = -1;
        if (m->nlev > 1) WL_TRY((mg_vcycle<T, D>(m, 0, &pre)));
        WL_TRY((op_pcg<T, D>(p, 6, m->permask, m->sc.partials.get(), m->sc.st.get(), true, pre, true)));   // (level 1: z ≡ flow.σ)
        WL_TRY((op_L2<T, D>(p, m->sc.partials.get(), m->sc.st.get(), true)));
        WL_TRY(m->sc.fetch());
        ++n;
        const double r2 = m->sc.hst.get()->pcg.r2;
        if (m->log_on) WL_TRY((mg_log_row<T, D>(m, n, true)));
        if (r2 < tol) break;
    }
    WL_TRY((op_bc_per<T, D>(p.g, p.x, m->permask)));
    if (n_iter) *n_iter = n;
    return 0;
}

// project!  src/Flow.jl:137-145
// exchange_u (z-slab runs, mom_step!): the 1-plane halo exchange of u that div needs (it reads u[I+dz]) is issued here on
// the comm stream; x*=dt and div on all owned planes but the last run while it is in flight.
// head_done: `x .*= dt` of this call was already applied (chained onto the previous projection's `x ./= dt`);
// tail_then: instead of this call's own `x ./= dt` pass, run that and the NEXT projection's `x .*= dt'` as one stream.
template <class T> static ScaleOp project_scale(double dt_, double w) {
    const bool dbl = (w != 1.0);
    return ScaleOp{dbl ? w * (double)(T)dt_ : (double)(T)dt_, false, dbl};
}
// uvel: the velocity array to project (mom_step! may hold the predicted velocity in the flow's u0 array; default a->d.u)
template <class T, int D> static int flow_project(wl_flow *a, wl_mg *b, double dt_, double w, int *n_iter, bool exchange_u = false,
                                                  bool head_done = false, const ScaleOp *tail_then = nullptr, const XBc<T> *xbc = nullptr,
                                                  bool *xdone = nullptr, T *uvel = nullptr) {
    const G g = mkG(&a->d.g);
    T *const uv = uvel ? uvel : (T *)a->d.u;
    LevelT<T> p = lvl<T>(b, 0);
    const ScaleOp sc = project_scale<T>(dt_, w);
    const double dts = sc.s;
    const bool dbl = sc.dbl;
    const Range R = r_inside(g);
    // 3-D vector kernels: z = div(u) is formed inside residual! (WL_OPT_DIV_IN_RESIDUAL); p.z stays unwritten
    // (rowvec_fits: a plane's workgroups fit the partial buffer -- the launch below cannot be rejected for its size)
    const bool fused_div = D == 3 && opt(WL_OPT_DIV_IN_RESIDUAL) && pcg_vec_ok<T>(g) && stencil7_ok<T>(p.g) && rowvec_fits<T>(p.g) && b->permask == 0 &&
                           g.s[1] == p.g.s[1] && g.s[2] == p.g.s[2] && g.n[0] == p.g.n[0] && g.n[2] == p.g.n[2] && g.dist == p.g.dist;
    bool begun = false;
    if (fused_div && g.dist) {
        // z-slabs: the plane of u that div reads above the last owned plane and the planes of x that residual! reads travel in ONE
        // batch on the comm stream (x must carry its `.*= dt` first); the fused kernel runs on the inner planes meanwhile
        if (!head_done) WL_TRY((op_scale_all<T, D>(g, p.x, dts, false, dbl)));
        if (exchange_u) { WL_TRY((halo_begin2<T>(g, uv, D, 1, p.g, p.x, 1, 1))); begun = true; }
    } else if (exchange_u && D == 3 && g.dist && overlap_on() && R.hi[2] - R.lo[2] + 1 >= 2) {
        WL_TRY((halo_begin<T>(g, uv, D, 1)));
        int rc = head_done ? 0 : op_scale_all<T, D>(g, p.x, dts, false, dbl);
        if (!rc) rc = op_div<T, D>(g, p.z, (const T *)uv, R.lo[2], R.hi[2] - 1);
        WL_TRY(halo_end());   // (always joined, also on an error above)
        if (rc) return rc;
        WL_TRY((op_div<T, D>(g, p.z, (const T *)uv, R.hi[2], R.hi[2])));
    } else {
        if (exchange_u) WL_TRY((halo_exchange<T>(g, uv, D, 1)));
        if (!fused_div) WL_TRY((op_div<T, D>(g, p.z, (const T *)uv)));
        if (!head_done) WL_TRY((op_scale_all<T, D>(g, p.x, dts, false, dbl)));
    }
    WL_TRY((mg_solve<T, D>(b, 1e-4, 32, n_iter, fused_div ? (const T *)uv : nullptr, &g, begun)));
    WL_TRY((op_correct<T, D>(g, uv, p.L, p.x, p.rowc, xbc, xdone)));
    return op_scale_all<T, D>(g, p.x, dts, true, dbl, tail_then);
}

// mom_step!  src/Flow.jl:153-169
template <class T, int D>
static int flow_mom_step(wl_flow *a, wl_mg *b, double dt, const double *U, const double *gp, const double *gc,
                         double *dt_next, int *n2) {
    const wl_flow_desc &d = a->d;
    const G g = mkG(&d.g);
    T *u = (T *)d.u, *u0 = (T *)d.u0, *f = (T *)d.f, *V = (T *)d.V, *mu0 = (T *)d.mu0, *mu1 = (T *)d.mu1;
    // (z-slab runs: u carries a 2-plane halo for QUICK, f a 1-plane halo for mu_ddn; exchanges are no-ops otherwise)
    // (the x-ghost cells of the interior rows are written by the kernel that produces the row: XBc, WL_OPT_XGHOST_IN_KERNEL)
    const XBc<T> xbc{(D == 3 && d.perdir_mask == 0 && opt(WL_OPT_BC_FUSED) && opt(WL_OPT_XGHOST_IN_KERNEL)) ? 1 : 0, d.exitBC ? 1 : 0, (T)U[0]};
    bool xd = false;
    // `turns`: BDIM! is finished inside conv_diff! on the body-free rows (WL_OPT_BDIM_IN_CONVDIFF, CdFin in wl_convdiff.h).  The kernel
    // that forms f cannot overwrite the velocity its neighbours still read, so the two velocity arrays take turns: the predictor
    // reads `u` (which thereby IS u0: no copy) and writes u' into the flow's u0 array; the corrector reads u' there and u0 in
    // `u`, cell by cell, and writes the new velocity over it.  On return `u` holds the new velocity as always and the u0 ARRAY
    // holds u' instead of the old velocity -- the reference overwrites u0 before it reads it (Flow.jl:154), DESIGN.md 7.8.
    // Otherwise (2-D, periodic directions, convective exit, no row flags): `a.u0 .= a.u` rides in the predictor's conv_diff!
    // and BDIM! #2 is a pass of its own, in place.
    bool turns = false;
    if constexpr (D == 3)
        turns = opt(WL_OPT_BDIM_IN_CONVDIFF) && opt(WL_OPT_BDIM_ROWFLAGS) && a->rowfree && a->busy.get() && d.perdir_mask == 0 && !d.exitBC && conv_diff_tiled<D>(g, 0);
    T *const up = turns ? u0 : u;   // where the predictor's velocity u' lives
    const CdFin<T> fin1{up, a->rowfree, xbc.on, (T)U[0]}, fin2{u, a->rowfree, xbc.on, (T)U[0]};
    (void)fin1; (void)fin2;
    // predictor (:157-161): [u0 .= u (:154)] + conv_diff! + accelerate! + BDIM! #1 in ONE kernel; scale_u!(a,0) is folded into
    // BDIM! #2 (MODE 1: u = ...)
    if (turns) {
        if constexpr (D == 3) {
            WL_TRY((op_conv_diff<T, D, true, false, 1>(g, f, u, d.nu, 0, u, V, dt, gp, gp != nullptr, nullptr, false, &fin1)));
            WL_TRY((op_bdim2_busy<T, 1>(g, up, up, f, V, mu0, mu1, a->busy.get(), a->nbusy, a->nbusy_lo, a->nbusy_hi, xbc, a->segfree())));   // + exchange of f
            xd = xbc.on != 0;
        }
    } else {
        WL_TRY((op_conv_diff<T, D, true, true>(g, f, u, d.nu, d.perdir_mask, nullptr, V, dt, gp, gp != nullptr, u0)));
        // σ's top ghost cells: the flux scratch Φ the reference's conv_diff! leaves there (Flow.jl:157), read by its whole-array
        // z⋅ϵ in the projection that follows (periodic runs only: elsewhere ϵ's ghosts are zero) and by maximum(a.σ) in CFL --
        // which sees the corrector's values, so a non-periodic run skips the predictor's.
        if (d.perdir_mask != 0) WL_TRY((op_sigma_ghosts<T, D>(g, (T *)d.sigma, u, d.nu, d.perdir_mask)));
        WL_TRY((op_bdim2<T, D, 1>(g, u, f, V, mu0, mu1, a->rowfree, a->busy.get(), a->nbusy, true, &xbc, &xd, a->segfree())));   // + exchange of f (overlapped)
    }
    WL_TRY((op_bc_vec<T, D>(g, up, U, d.exitBC, d.perdir_mask, xd)));
    if (d.exitBC) WL_TRY((op_exit_bc<T, D>(g, up, u0, U, dt, a->sc.partials.get(), a->sc.st.get())));
    // (the predictor's closing `x ./= dt` and the corrector's opening `x .*= 0.5dt` are ONE pass over x: nothing in between reads p)
    const ScaleOp corr_head = project_scale<T>(dt, 0.5);
    const bool chain = opt(WL_OPT_SCALE_CHAIN) != 0;
    WL_TRY((flow_project<T, D>(a, b, dt, 1.0, &n2[0], true, false, chain ? &corr_head : nullptr, &xbc, &xd, up)));   // + 1-plane exchange of u' (overlapped)
    WL_TRY((op_bc_vec<T, D>(g, up, U, d.exitBC, d.perdir_mask, xd)));
    // corrector (:164-167); the 2-plane exchange of u' is issued inside op_conv_diff (overlapped with its inner planes);
    // σ's ghost cells: Φ of the corrector (Flow.jl:164), formed from u'; scale_u!(a,0.5) is folded into BDIM! #2 (MODE 2)
    if (turns) {
        if constexpr (D == 3) {
            WL_TRY((op_conv_diff<T, D, true, false, 2>(g, f, up, d.nu, 0, u, V, dt, gc, gc != nullptr, nullptr, true, &fin2)));
            WL_TRY((op_sigma_ghosts<T, D>(g, (T *)d.sigma, up, d.nu, 0)));
            WL_TRY((op_bdim2_busy<T, 2>(g, u, up, f, V, mu0, mu1, a->busy.get(), a->nbusy, a->nbusy_lo, a->nbusy_hi, xbc, a->segfree())));
            xd = xbc.on != 0;
        }
    } else {
        WL_TRY((op_conv_diff<T, D, true>(g, f, u, d.nu, d.perdir_mask, u0, V, dt, gc, gc != nullptr, nullptr, true)));
        WL_TRY((op_sigma_ghosts<T, D>(g, (T *)d.sigma, u, d.nu, d.perdir_mask)));
        WL_TRY((op_bdim2<T, D, 2>(g, u, f, V, mu0, mu1, a->rowfree, a->busy.get(), a->nbusy, true, &xbc, &xd, a->segfree())));
    }
    WL_TRY((op_bc_vec<T, D>(g, u, U, d.exitBC, d.perdir_mask, xd)));
    WL_TRY((flow_project<T, D>(a, b, dt, 0.5, &n2[1], true, chain, nullptr, &xbc, &xd)));
    WL_TRY((op_bc_vec<T, D>(g, u, U, d.exitBC, d.perdir_mask, xd)));
    // push!(a.dt, CFL(a)) (:168); the end-of-step 2-plane exchange of u is issued inside (overlapped with the kernel)
    WL_TRY((op_cfl<T, D>(g, (T *)d.sigma, u, d.nu, a->sc.partials.get(), a->sc.st.get(), true)));
    WL_TRY(a->sc.fetch());
    *dt_next = a->sc.hst.get()->out[0];
    return 0;
}

template <class T, int D> static int red_L2(const G &g, const T *a, Scratch &S) {
    return op_reduce<T, D>(g, WL_K_DOT, RED_SUM, 0.0, [=] __device__(long I) { const double v = (double)a[I]; return v * v; },
                           S.partials.get(), S.st.get(), 0);
}
template <class T, int D> static int red_dot(const G &g, const T *a, const T *b, Scratch &S) {
    return op_reduce<T, D>(g, WL_K_DOT, RED_SUM, 0.0, [=] __device__(long I) { return (double)a[I] * (double)b[I]; },
                           S.partials.get(), S.st.get(), 0, true);
}
template <class T, int D> static int red_sum(const G &g, const T *a, Scratch &S) {
    return op_reduce<T, D>(g, WL_K_DOT, RED_SUM, 0.0, [=] __device__(long I) { return (double)a[I]; }, S.partials.get(), S.st.get(), 0, true);
}
template <class T, int D> static int red_max(const G &g, const T *a, Scratch &S) {
    return op_reduce<T, D>(g, WL_K_DOT, RED_MAX, -1e300, [=] __device__(long I) { return (double)a[I]; }, S.partials.get(), S.st.get(), 0, true);
}
template <class T, int D>
static int bdim_full(const G &g, T *u, const T *u0, T *f, const T *V, const T *mu0, const T *mu1, double dt) {
    WL_TRY((op_bdim1<T, D>(g, f, u0, V, dt)));
    return op_bdim2<T, D, 0>(g, u, f, V, mu0, mu1);
}
// `@inside out[I] = metric(I,u)` (src/Metrics.jl:14-77): the per-cell formula is metric_cell (wl_render.h), shared with
// wl_render_project, which forms the same values without storing them
template <class T, int D>
static int op_metric(const G &g, int kind, T *out, const T *u, int ipar, const double *par, const double *par2) {
    const G gg = g;
    const MetricPar mp = metric_par(D, par, par2);
    return launch_range(WL_K_MISC, r_inside(g), [=] __device__(int i, int j, int k) {
        out[gg.at(i, j, k)] = metric_cell<T, D>(gg, u, kind, ipar, mp, i, j, k);
    });
}

// du_i/dx_j at the centre of cell I (src/Metrics.jl:28-31), in T
template <class T> __device__ inline T dudx(const G &g, const T *u, long I, int i, int j) {
    const T *ui = u + (long)i * g.sc;
    if (i == j) return ui[I + g.s[i]] - ui[I];
    return (ui[I + g.s[j]] + ui[I + g.s[j] + g.s[i]] - ui[I - g.s[j]] - ui[I - g.s[j] + g.s[i]]) / (T)4;
}
// Metrics.jl:109-113 viscous_force over the band
template <class T>
__global__ __launch_bounds__(256) void k_vforce(G g, const T *u, const int64_t *idx, const double *nds, int64_t nband, T nu,
                                                double *partials) {
    double acc[3] = {0, 0, 0};
    const int D = g.D;
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < nband; b += (int64_t)gridDim.x * 256) {
        const long I = idx[b];
        for (int i = 0; i < D; ++i) {
            double s = 0;
            for (int j = 0; j < D; ++j) {
                const T m = -nu * (T)(dudx<T>(g, u, I, i, j) + dudx<T>(g, u, I, j, i));   // (-nu * grad2u)[i,j] in T
                s += (double)m * nds[b * D + j];
            }
            acc[i] += (double)(T)s;                                                        // df[I,:] is a T array
        }
    }
    block_red<3>(acc, RED_SUM);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) partials[(long)c * gridDim.x + blockIdx.x] = acc[c];
}
// Metrics.jl:130-134 pressure_moment over the band
template <class T>
__global__ __launch_bounds__(256) void k_pmoment(G g, const T *p, const int64_t *idx, const double *nds, int64_t nband,
                                                 double x0, double y0, double z0, double *partials) {
    double acc[3] = {0, 0, 0};
    const int D = g.D;
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < nband; b += (int64_t)gridDim.x * 256) {
        const long I = idx[b];
        const long k = D > 2 ? I / g.s[2] : 0, rem = D > 2 ? I - k * g.s[2] : I;
        const long j = rem / g.s[1], i = rem - j * g.s[1];
        const double rx = (double)i - 0.5 - x0, ry = (double)j - 0.5 - y0, rz = (double)(k + g.kz0) - 0.5 - z0;  // loc(0,I)-x0
        const double pv = (double)p[I];
        if (D == 3) {
            const double nx = nds[b * 3], ny = nds[b * 3 + 1], nz = nds[b * 3 + 2];
            acc[0] += (double)(T)(pv * (ry * nz - rz * ny));
            acc[1] += (double)(T)(pv * (rz * nx - rx * nz));
            acc[2] += (double)(T)(pv * (rx * ny - ry * nx));
        } else {
            const double m = (double)(T)(pv * (rx * nds[b * 2 + 1] - ry * nds[b * 2]));
            acc[0] += m; acc[1] += m;
        }
    }
    block_red<3>(acc, RED_SUM);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) partials[(long)c * gridDim.x + blockIdx.x] = acc[c];
}
template <class T>
__global__ __launch_bounds__(256) void k_pforce(const T *p, const int64_t *idx, const double *nds, int64_t nband, int D,
                                                 double *partials) {
    double acc[3] = {0, 0, 0};
    for (int64_t b = (int64_t)blockIdx.x * 256 + threadIdx.x; b < nband; b += (int64_t)gridDim.x * 256) {
        const double pv = (double)p[idx[b]];
        for (int c = 0; c < D; ++c) acc[c] += (double)(T)(pv * nds[b * D + c]);  // df[I,:] is a T array
    }
    block_red<3>(acc, RED_SUM);
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) partials[(long)c * gridDim.x + blockIdx.x] = acc[c];
}
// compact the busy INTERIOR rows of a->rowbuf on the host (n1*n2 bytes; this runs once per measure!, not per step)
static int flow_compact_busy(wl_flow *a, const G &g, int D) {
    a->rowfree = a->rowbuf.get();
    const size_t nrows = (size_t)g.n[1] * (size_t)(D > 2 ? g.n[2] : 1);
    std::vector<unsigned char> fl(nrows);
    WL_HIP(hipMemcpyAsync(fl.data(), a->rowbuf.get(), nrows, hipMemcpyDeviceToHost, ctx().stream));
    WL_HIP(hipStreamSynchronize(ctx().stream));
    const Range R = r_inside(g);
    std::vector<int> list;
    for (int k = R.lo[2]; k <= R.hi[2]; ++k)
        for (int j = 1; j <= g.n[1] - 2; ++j)
            if (!fl[(size_t)j + (size_t)g.n[1] * k]) list.push_back(j + g.n[1] * k);
    const size_t nl = list.size();   // never left without a list: 64 entries for an empty one, 2n + 64 when n do not fit
    WL_TRY(a->busy.reserve(nl ? nl : 1, nl ? nl * 2 + 64 : 64));
    if (!list.empty()) WL_HIP(hipMemcpyAsync(a->busy.get(), list.data(), list.size() * sizeof(int), hipMemcpyHostToDevice, ctx().stream));
    WL_HIP(hipStreamSynchronize(ctx().stream));
    a->nbusy = (int)list.size();
    a->nbusy_lo = a->nbusy_hi = 0;
    if (D > 2 && R.hi[2] > R.lo[2])
        for (int row : list) { a->nbusy_lo += (row / g.n[1] == R.lo[2]); a->nbusy_hi += (row / g.n[1] == R.hi[2]); }
    else
        a->nbusy_lo = a->nbusy;   // a single plane: every row reads both neighbours
    return 0;
}
template <class T, int D> static int flow_update(wl_flow *a) {
    const G g = mkG(&a->d.g);
    WL_TRY((op_rowflags<T, D>(g, (const T *)a->d.V, (const T *)a->d.mu0, (const T *)a->d.mu1, a->rowbuf.get(), a->d.perdir_mask, D == 3 ? a->segbuf.get() : nullptr)));
    a->seg_valid = (D == 3 && a->segbuf.get() != nullptr);
    a->prev_valid = false;   // the arrays were written by someone else: the next native measure! rewrites every row
    return flow_compact_busy(a, g, D);
}
static BodyDev body_dev(const wl_body_desc *bodies) {
    BodyDev o;
    o.n = bodies[0].count > 0 ? bodies[0].count : 1;
    for (int l = 0; l < o.n; ++l) {
        const wl_body_desc *b = bodies + l;
        LeafDev &d = o.leaf[l];
        d.family = b->family; d.ident = b->identity_map != 0; d.op = b->op;
        for (int q = 0; q < 8; ++q) d.p[q] = b->p[q];
        for (int q = 0; q < 9; ++q) { d.A[q] = b->A[q]; d.dA[q] = b->dA[q]; d.Ainv[q] = b->Ainv[q]; }
        for (int q = 0; q < 3; ++q) { d.b[q] = b->b[q]; d.db[q] = b->db[q]; }
    }
    for (int l = o.n; l < WL_BODY_MAXLEAF; ++l) o.leaf[l] = o.leaf[0];
    return o;
}
static int measure_alloc(wl_flow *a, size_t nrows) {
    // one by one: after a failure part-way the next call allocates what is missing instead of trusting the first
    WL_TRY(a->rowcount.reserve(nrows));
    WL_TRY(a->rowoff.reserve(nrows + 1));
    WL_TRY(a->touched.reserve(nrows));
    WL_TRY(a->prev.reserve(nrows));
    WL_TRY(a->changed.reserve(nrows));
    return 0;
}
// The two halves of a native measure! with the body's own kernels passed in: `rows(g, nrows, d2)` launches the sigma / band
// count / touched-flag kernel, `fill(g, nrows, d2, cand)` the coefficient / band-list kernel (parametric: wl_measure.h;
// triangle mesh: wl_mesh.h).  Everything around them does not know what shape the body has.
template <class T, int D, class Rows> static int measure_rows_with(wl_flow *a, double eps, int64_t *nband, Rows rows) {
    const G g = mkG(&a->d.g);
    const size_t nrows = (size_t)g.n[1] * (size_t)(D > 2 ? g.n[2] : 1);
    WL_TRY(measure_alloc(a, nrows));
    const T d2 = (T)((2 + eps) * (2 + eps));
    {
        Prof p(WL_K_MISC, g.cells());
        rows(g, nrows, d2);
        WL_HIP(hipGetLastError());
        hipLaunchKernelGGL(k_scan_rows, dim3(1), dim3(1024), 0, ctx().stream, (const int *)a->rowcount.get(), a->rowoff.get(), (long)nrows);
        WL_HIP(hipGetLastError());
    }
    long tot = 0;
    WL_HIP(hipMemcpyAsync(&tot, a->rowoff.get() + nrows, sizeof(long), hipMemcpyDeviceToHost, ctx().stream));
    WL_HIP(hipStreamSynchronize(ctx().stream));
    a->nband = tot;
    *nband = tot;
    return 0;
}
template <class T, int D> static int measure_rows(wl_flow *a, const wl_body_desc *body, double eps, int64_t *nband) {
    const BodyDev B = body_dev(body);
    return measure_rows_with<T, D>(a, eps, nband, [&](const G &g, size_t nrows, T d2) {
        hipLaunchKernelGGL((k_measure_rows<T, D>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, ctx().stream, g, B, (T *)a->d.sigma, d2,
                           a->rowcount.get(), a->touched.get());
    });
}
template <class T, int D, class Fill> static int measure_fill_with(wl_flow *a, int64_t *cand, Fill fill) {
    const G g = mkG(&a->d.g);
    const size_t nrows = (size_t)g.n[1] * (size_t)(D > 2 ? g.n[2] : 1);
    {
        Prof p(WL_K_MISC, g.cells());
        fill(g, nrows, cand);
        WL_HIP(hipGetLastError());
    }
    a->nband = -1;
    // Body.jl:51-52, then what the host does after the reference's measure!: z-slab halos, body-free row flags
    const double zero[3] = {0, 0, 0};
    WL_TRY((op_bc_vec<T, D>(g, (T *)a->d.mu0, zero, 0, a->d.perdir_mask)));
    WL_TRY((op_bc_vec<T, D>(g, (T *)a->d.V, zero, a->d.exitBC, a->d.perdir_mask)));
    WL_TRY((halo_exchange<T>(g, (T *)a->d.mu0, D, 2)));
    WL_TRY((halo_exchange<T>(g, (T *)a->d.V, D, 2)));
    a->seg_valid = false;   // (the native measure! knows touched ROWS only: every segment of a busy row takes the general statement)
    hipLaunchKernelGGL((k_rowflags_touched<D>), dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, ctx().stream, g,
                       (const unsigned char *)a->touched.get(), a->rowbuf.get(), a->d.perdir_mask);
    WL_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_rows_changed, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, ctx().stream, (const unsigned char *)a->touched.get(),
                       (const unsigned char *)a->prev.get(), !a->prev_valid, a->changed_valid && a->changed_pending, a->changed.get(), (long)nrows);
    WL_HIP(hipGetLastError());
    a->changed_valid = true;
    a->changed_pending = true;
    WL_HIP(hipMemcpyAsync(a->prev.get(), a->touched.get(), nrows, hipMemcpyDeviceToDevice, ctx().stream));
    WL_TRY(flow_compact_busy(a, g, D));
    a->prev_valid = true;
    return 0;
}
template <class T, int D> static int measure_fill(wl_flow *a, const wl_body_desc *body, double eps, int64_t *cand) {
    const BodyDev B = body_dev(body);
    const T d2 = (T)((2 + eps) * (2 + eps));
    return measure_fill_with<T, D>(a, cand, [&](const G &g, size_t nrows, int64_t *cd) {
        hipLaunchKernelGGL((k_measure_fill<T, D>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, ctx().stream, g, B, (const T *)a->d.sigma, d2,
                           (2 + eps) * (2 + eps), eps, (T *)a->d.mu0, (T *)a->d.mu1, (T *)a->d.V, (const unsigned char *)a->touched.get(),
                           (const unsigned char *)a->prev.get(), !a->prev_valid, (const long *)a->rowoff.get(), (long *)cd);
    });
}
// ---- triangle-mesh bodies (wl_mesh.h)
static int mesh_upload(const wl_mesh *m) {
    if (m->d_tri.get()) return 0;
    // the handle's buffers are set only once all four copies are on the device: a failure part-way drops the locals and
    // leaves the handle as it was (not uploaded), so a later call starts again instead of launching with half the arrays
    Buf<double, DevMem> tri;
    Buf<int, DevMem> start, list;
    Buf<signed char, DevMem> sign;
    WL_TRY(tri.reserve(m->tri.size()));
    WL_TRY(start.reserve(m->bin_start.size()));
    WL_TRY(list.reserve(std::max<size_t>(m->bin_tri.size(), 1)));
    WL_TRY(sign.reserve(m->bin_sign.size()));
    hipError_t e = hipMemcpyAsync(tri.get(), m->tri.data(), m->tri.size() * sizeof(double), hipMemcpyHostToDevice, ctx().stream);
    if (e == hipSuccess) e = hipMemcpyAsync(start.get(), m->bin_start.data(), m->bin_start.size() * sizeof(int), hipMemcpyHostToDevice, ctx().stream);
    if (e == hipSuccess && !m->bin_tri.empty())
        e = hipMemcpyAsync(list.get(), m->bin_tri.data(), m->bin_tri.size() * sizeof(int), hipMemcpyHostToDevice, ctx().stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sign.get(), m->bin_sign.data(), m->bin_sign.size(), hipMemcpyHostToDevice, ctx().stream);
    const hipError_t es = hipStreamSynchronize(ctx().stream);   // (also on failure: no copy may still be reading the host arrays)
    if (e == hipSuccess) e = es;
    if (e != hipSuccess) return fail((int)e, "uploading the mesh bins", __FILE__, __LINE__);
    m->d_start = std::move(start); m->d_list = std::move(list); m->d_sign = std::move(sign); m->d_tri = std::move(tri);
    return 0;
}
// the pose as the kernels take it; refuses a map that is not a similarity (A A^T = s^2 I) or whose exact zone R/s is too thin
static int mesh_pose(const wl_mesh *m, const wl_mesh_pose *p, double need, PoseDev &o) {
    if (!m || !p) return fail(WL_E_ARG, "null mesh or pose", __FILE__, __LINE__);
    o.ident = p->identity_map != 0;
    o.s = 1.0;
    for (int q = 0; q < 9; ++q) { o.A[q] = p->A[q]; o.dA[q] = p->dA[q]; o.Ainv[q] = p->Ainv[q]; }
    for (int q = 0; q < 3; ++q) { o.b[q] = p->b[q]; o.db[q] = p->db[q]; }
    if (!o.ident) {
        double gm[9], s2 = 0;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double s = 0;
                for (int q = 0; q < 3; ++q) s += p->A[3 * r + q] * p->A[3 * c + q];
                gm[3 * r + c] = s;
            }
        s2 = (gm[0] + gm[4] + gm[8]) / 3;
        if (!(s2 > 0) || !std::isfinite(s2)) return fail(WL_E_ARG, "mesh pose: the map is singular", __FILE__, __LINE__);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                if (std::fabs(gm[3 * r + c] - (r == c ? s2 : 0.0)) > 1e-10 * s2)
                    return fail(WL_E_ARG, "mesh pose: the map is not a similarity (A A^T != s^2 I)", __FILE__, __LINE__);
        o.s = std::sqrt(s2);
    }
    // (a relative 1e-9 of slack: the caller computes s on its own, and a rotating map's s wanders by an ulp from step to step;
    //  `need` itself carries half a cell more than the faces, the farthest points measured, can be away)
    if (m->R < need * o.s * (1.0 - 1e-9)) return fail(WL_E_ARG, "mesh pose: exact_radius too small for this eps and map scale (needs (2 + eps + 1) * s)", __FILE__, __LINE__);
    return 0;
}
template <class T> static int mesh_rows(wl_flow *a, const wl_mesh *m, const PoseDev &P, double eps, int64_t *nband) {
    WL_TRY(mesh_upload(m));
    const MeshDev M = m->view(true);
    return measure_rows_with<T, 3>(a, eps, nband, [&](const G &g, size_t nrows, T d2) {
        hipLaunchKernelGGL((k_mesh_rows<T>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, ctx().stream, g, M, P, (T *)a->d.sigma, d2,
                           a->rowcount.get(), a->touched.get());
    });
}
template <class T> static int mesh_fill(wl_flow *a, const wl_mesh *m, const PoseDev &P, double eps, int64_t *cand) {
    WL_TRY(mesh_upload(m));
    const MeshDev M = m->view(true);
    const T d2 = (T)((2 + eps) * (2 + eps));
    return measure_fill_with<T, 3>(a, cand, [&](const G &g, size_t nrows, int64_t *cd) {
        hipLaunchKernelGGL((k_mesh_fill<T>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, ctx().stream, g, M, P, (const T *)a->d.sigma, d2,
                           (2 + eps) * (2 + eps), eps, (T *)a->d.mu0, (T *)a->d.mu1, (T *)a->d.V, (const unsigned char *)a->touched.get(),
                           (const unsigned char *)a->prev.get(), !a->prev_valid, (const long *)a->rowoff.get(), (long *)cd);
    });
}
static int check_body(const wl_body_desc *b, int D) {
    if (!b) return fail(WL_E_ARG, "null body", __FILE__, __LINE__);
    const int n = b[0].count > 0 ? b[0].count : 1;
    if (n > WL_BODY_MAXLEAF) return fail(WL_E_ARG, "more than WL_BODY_MAXLEAF leaves in a composite body", __FILE__, __LINE__);
    for (int l = 0; l < n; ++l) {
        const int f = b[l].family;
        if (f != WL_BODY_SPHERE && f != WL_BODY_TORUS && f != WL_BODY_PLATE && f != WL_BODY_CYLINDER)
            return fail(WL_E_ARG, "unknown body family", __FILE__, __LINE__);
        if (f == WL_BODY_TORUS && D != 3) return fail(WL_E_ARG, "the torus family needs D == 3", __FILE__, __LINE__);
        if (l > 0 && (b[l].op < WL_BODY_OP_UNION || b[l].op > WL_BODY_OP_INTERSECT))
            return fail(WL_E_ARG, "unknown composite operation", __FILE__, __LINE__);
    }
    return 0;
}
// shared driver of the band reductions (pressure_force / viscous_force / pressure_moment)
template <class KERNEL> static int band_reduce(const G &gg, Scratch &S, int64_t nband, int D, double out[3], KERNEL launch) {
    out[0] = out[1] = out[2] = 0;
    int nb = (int)((nband + 255) / 256);
    if (nb > 1024) nb = 1024;
    if (nband <= 0) nb = 0;   // a rank whose slab holds no part of the body still joins the all-reduce
    if (nb > 0) {
        Prof pr(WL_K_PFORCE, nband);
        launch(nb);
        WL_HIP(hipGetLastError());
    }
    State *st = S.st.get();
    WL_TRY((launch_finalize<3>(gg.dist, S.partials.get(), nb, RED_SUM, 0.0, st->red, [=] __device__(const double *v) {
        st->out[0] = v[0]; st->out[1] = v[1]; st->out[2] = v[2]; })));
    WL_TRY(S.fetch());
    for (int c = 0; c < D; ++c) out[c] = S.hst.get()->out[c];
    return 0;
}
// Snapshot staging (VTK write / restart): planes klo..khi of a field <-> a DENSE array-of-tuples buffer on the device,
// dst[((kk*n1 + j)*n0 + i)*nct + c] = a_c[i, j, klo+kk] (c < ncomp; 0 for ncomp <= c < nct): the row padding goes, the components
// interleave (VTK's tuple order, ext/WaterLilyWriteVTKExt.jl:79 components_first).  One wavefront per x-row.
template <class T, bool PACK>
__global__ __launch_bounds__(256) void k_snapshot(G g, T *a, int ncomp, int nct, int klo, long nrows, T *buf) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= nrows) return;
    const int j = (int)(row % g.n[1]), kk = (int)(row / g.n[1]);
    const long src = g.at(0, j, klo + kk), dst = row * (long)g.n[0];
    for (int i = threadIdx.x & 63; i < g.n[0]; i += 64)
        for (int c = 0; c < nct; ++c) {
            if (PACK) buf[(dst + i) * nct + c] = c < ncomp ? a[(long)c * g.sc + src + i] : (T)0;
            else if (c < ncomp) a[(long)c * g.sc + src + i] = buf[(dst + i) * nct + c];
        }
}
template <class T> static int snapshot_copy(const G &g, T *a, int ncomp, int nct, int klo, int khi, T *buf, bool pack) {
    const long nrows = (long)g.n[1] * (khi - klo + 1);
    Prof p(WL_K_COPY, nrows * g.n[0] * nct);
    if (pack) hipLaunchKernelGGL((k_snapshot<T, true>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, ctx().stream, g, a, ncomp, nct, klo, nrows, buf);
    else hipLaunchKernelGGL((k_snapshot<T, false>), dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, ctx().stream, g, a, ncomp, nct, klo, nrows, buf);
    return (int)hipGetLastError();
}
template <class T, int D> static int restrictL_full(const G &A, T *a, const G &B, const T *b, int permask) {
    WL_TRY((op_restrictL<T, D>(A, a, B, b, permask)));
    return coarse_L_finish<T, D>(A, a, B, permask);
}

template <class T, int D> static int conv_diff_phi(const G &g, T *r, const T *u, T *Phi, double nu, int permask) {
    WL_TRY((op_conv_diff<T, D, false>(g, r, u, nu, permask, nullptr, nullptr, 0.0, nullptr, false)));
    return Phi ? op_sigma_ghosts<T, D>(g, Phi, u, nu, permask) : 0;
}

// ------------------------------------------------------------------------------------------ argument checks
// What several entry points ask of the same kind of argument is stated here once.  `who` is the entry point's name: the
// message reads "<who>: <what>".  Nothing below touches the device.
#define WL_BAD(who, what) return fail(WL_E_ARG, what, __FILE__, __LINE__, who)
static int check_dtype(const char *who, wl_dtype t, const char *what = "unknown dtype") {
    if (t != WL_F32 && t != WL_F64) WL_BAD(who, what);
    return 0;
}
// kind m = WL_M_* with its component ipar on a D-dimensional grid (wl_metric; WL_R_METRIC + m below)
static bool metric_kind_ok(int m, int ipar, int D) {
    return !(m < 0 || m > WL_M_LAMBDA2 || (m >= WL_M_OMAG && D != 3) || (m == WL_M_CURL && (ipar < 0 || ipar > 2)));
}
// a field kind WL_R_* with its component ipar (wl_render_project; wl_downsample, which alone takes WL_R_FACE)
static int check_kind(const char *who, int kind, int ipar, int D, bool face_ok) {
    if (kind >= WL_R_METRIC) {
        if (!metric_kind_ok(kind - WL_R_METRIC, ipar, D)) WL_BAD(who, "bad metric kind/component for this dimension");
    } else if (face_ok && kind == WL_R_FACE) {
        if (ipar < 0 || ipar >= D) WL_BAD(who, "WL_R_FACE averages component ipar of a vector field (0 <= ipar < D), not a scalar");
    } else if (kind < WL_R_SCALAR || kind > WL_R_CENTRE || (kind != WL_R_SCALAR && (ipar < 0 || ipar >= D))) {
        WL_BAD(who, "bad kind/component for this dimension");
    }
    return 0;
}
// The box lo, hi (given together or not at all) -> l, h: GLOBAL along z, `nd` directions parsed, l = 0, h = 1 in the others.
// No box: 1 .. n - def_inset.  empty_ok: lo == hi passes (a box without cells), else lo < hi is required.
static int parse_box(const char *who, const G &gg, int nd, int def_inset, bool empty_ok, const int32_t *lo, const int32_t *hi, int l[3], int h[3]) {
    if ((lo != nullptr) != (hi != nullptr)) WL_BAD(who, "only one of lo and hi given");
    l[0] = l[1] = l[2] = 0, h[0] = h[1] = h[2] = 1;
    for (int d = 0; d < nd; ++d) {
        const int n = d == 2 ? gg.nzg : gg.n[d];
        l[d] = lo ? lo[d] : 1;
        h[d] = hi ? hi[d] : n - def_inset;
        if (!(0 <= l[d] && (empty_ok ? l[d] <= h[d] : l[d] < h[d]) && h[d] <= n - 1))
            WL_BAD(who, empty_ok ? "bad box (0 <= lo <= hi <= n - 1 in every direction)" : "bad box (0 <= lo < hi <= n - 1 in every direction)");
    }
    return 0;
}
// a metric kind reads every neighbour of a cell: its box stays off the low ghost layer ...
static int check_metric_box(const char *who, int D, const int l[3]) {
    for (int d = 0; d < D; ++d)
        if (l[d] < 1) WL_BAD(who, "the box of a metric kind must lie in inside()");
    return 0;
}
// ... and on a z-slab the planes it is formed on need a plane of the local array on each side: every owned plane (a metric
// kind), or the owned interior planes (interior: the loads and the integrals, which visit inside() alone)
static int check_halo_planes(const char *who, const G &gg, bool interior) {
    const Range R = r_inside(gg);
    const bool some = interior ? (gg.D == 3 && R.count() > 0) : gg.dist;
    const int klo = interior ? R.lo[2] : gg.zlo, khi = interior ? R.hi[2] : gg.zhi;
    if (some && (klo < 1 || khi > gg.n[2] - 2))
        WL_BAD(who, interior ? "an owned interior plane without a halo plane on each side" : "a metric kind on a z-slab needs a halo plane on each side");
    return 0;
}

// ------------------------------------------------------------------------------------------ C ABI
extern "C" {

// ---- communicator
int wl_comm_unique_id(void *out128) {
    ncclUniqueId id;
    ncclResult_t r = ncclGetUniqueId(&id);
    if (r != ncclSuccess) return fail(WL_E_STATE, ncclGetErrorString(r), __FILE__, __LINE__);
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    memcpy(out128, &id, 128);
    return 0;
}
int wl_comm_init_rccl(const void *id128, int rank, int nranks) {
    if (ctx().comm) return fail(WL_E_STATE, "communicator already initialised", __FILE__, __LINE__);
    ncclUniqueId id;
    memcpy(&id, id128, 128);
    RcclComm *c = new RcclComm();
    c->rank = rank; c->size = nranks;
    ncclResult_t r = ncclCommInitRank(&c->nc, nranks, id, rank);
    if (r != ncclSuccess) { delete c; return fail(WL_E_STATE, ncclGetErrorString(r), __FILE__, __LINE__); }
    const char *ov = getenv("WL_OVERLAP");
    if (!(ov && ov[0] == '0')) {   // overlapped exchanges get their own communicator (same ranks); on failure they share `nc`
        ncclComm_t h = nullptr;
        if (ncclCommSplit(c->nc, 0, rank, &h, nullptr) == ncclSuccess && h) c->nch = h;
    }
    ctx().comm = c;
    return 0;
}
int wl_comm_init_host(int rank, int nranks, wl_host_sendrecv_fn sr, wl_host_allreduce_fn ar, wl_host_allgather_fn ag,
                      void *user) {
    if (ctx().comm) return fail(WL_E_STATE, "communicator already initialised", __FILE__, __LINE__);
    if (!sr || !ar || !ag) return fail(WL_E_ARG, "null callback", __FILE__, __LINE__);
    HostComm *c = new HostComm();
    c->rank = rank; c->size = nranks; c->sr = sr; c->ar = ar; c->ag = ag; c->user = user;
    ctx().comm = c;
    return 0;
}
int wl_comm_init_loopback(int rank, int nranks) {
    if (ctx().comm) return fail(WL_E_STATE, "communicator already initialised", __FILE__, __LINE__);
    if (nranks < 1 || rank < 0 || rank >= nranks) return fail(WL_E_ARG, "wl_comm_init_loopback: bad rank", __FILE__, __LINE__);
    LoopComm *c = new LoopComm();
    c->rank = rank; c->size = nranks;
    ctx().comm = c;
    return 0;
}
static void mailbox_release() {
    Mailbox *mb = ctx().mbox;
    if (!mb) return;
    if (mb->host) { (void)hipHostUnregister(mb->host); munmap(mb->host, mb->bytes); }
    delete mb;
    ctx().mbox = nullptr;
}
// Mailbox all-reduce (wl_common.h: Mailbox).  `shm_name` ("/wlhip-...") names a POSIX shared-memory object every rank of the
// node opens; the rank with create != 0 makes and sizes it first (the host orders the calls: create, barrier, open).
int wl_comm_mailbox(const char *shm_name, int create) {
    Comm *cm = ctx().comm;
    if (!cm) return fail(WL_E_STATE, "wl_comm_mailbox: initialise the communicator first", __FILE__, __LINE__);
    if (!shm_name || shm_name[0] != '/') return fail(WL_E_ARG, "wl_comm_mailbox: name must start with '/'", __FILE__, __LINE__);
    if (cm->size > WL_MBOX_MAXRANKS) return fail(WL_E_ARG, "wl_comm_mailbox: too many ranks", __FILE__, __LINE__);
    if (ctx().mbox) { (void)hipStreamSynchronize(ctx().stream); mailbox_release(); }   // (a replacement: nothing may still be polling the old one)
    const size_t bytes = ((2 * (size_t)cm->size * sizeof(MboxSlot) + 4095) / 4096) * 4096;
    const int fd = create ? shm_open(shm_name, O_CREAT | O_EXCL | O_RDWR, 0600) : shm_open(shm_name, O_RDWR, 0600);
    if (fd < 0) return fail(WL_E_STATE, "wl_comm_mailbox: shm_open failed", __FILE__, __LINE__);
    if (create && ftruncate(fd, (off_t)bytes) != 0) { close(fd); return fail(WL_E_STATE, "wl_comm_mailbox: ftruncate failed", __FILE__, __LINE__); }
    struct stat sb;
    if (fstat(fd, &sb) != 0 || (size_t)sb.st_size < bytes) { close(fd); return fail(WL_E_STATE, "wl_comm_mailbox: shared object too small", __FILE__, __LINE__); }
    void *p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);   // (fresh shared memory reads as zero: seq 0 = nothing posted)
    close(fd);
    if (p == MAP_FAILED) return fail(WL_E_STATE, "wl_comm_mailbox: mmap failed", __FILE__, __LINE__);
    Mailbox *mb = new Mailbox();
    mb->bytes = bytes;
    hipError_t e = hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable);
    if (e != hipSuccess) { munmap(p, bytes); delete mb; return fail((int)e, "wl_comm_mailbox: hipHostRegister", __FILE__, __LINE__); }
    mb->host = (MboxSlot *)p;
    void *dp = nullptr;
    e = hipHostGetDevicePointer(&dp, p, 0);
    int rc = e == hipSuccess ? mb->err_host.reserve(1) : (int)e;
    if (!rc) { *mb->err_host.get() = 0; rc = (int)hipHostGetDevicePointer((void **)&mb->err_dev, mb->err_host.get(), 0); }
    if (rc) {
        (void)hipHostUnregister(p); munmap(p, bytes);
        delete mb;
        return fail(rc, "wl_comm_mailbox: device mapping", __FILE__, __LINE__);
    }
    mb->dev = (MboxSlot *)dp;
    if (ctx().wall_khz <= 0.0) {   // ticks per millisecond of wall_clock64() (constant-rate counter: 100 MHz on gfx9)
        int dev = 0, khz = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0)
            ctx().wall_khz = (double)khz;
        else ctx().wall_khz = 1e5;
    }
    ctx().mbox = mb;
    return 0;
}
int wl_comm_mailbox_off(void) {
    if (ctx().mbox) {
        (void)hipStreamSynchronize(ctx().stream);
        mailbox_release();
    }
    return 0;
}
int wl_comm_mailbox_active(int *on) {
    if (!on) return fail(WL_E_ARG, "null output", __FILE__, __LINE__);
    *on = ctx().mbox != nullptr;
    return 0;
}
int wl_comm_finalize(void) {
    if (ctx().comm) {
        (void)hipStreamSynchronize(ctx().stream);
        if (ctx().cstream) (void)hipStreamSynchronize(ctx().cstream);
        mailbox_release();
        delete ctx().comm;
        ctx().comm = nullptr;
    }
    return 0;
}
int wl_comm_rank(int *rank, int *nranks) {
    *rank = ctx().comm ? ctx().comm->rank : 0;
    *nranks = ctx().comm ? ctx().comm->size : 1;
    return 0;
}
int wl_halo_exchange(wl_dtype t, const wl_grid *g, void *a, int ncomp, int depth) {
    WL_TRY(check_dtype("wl_halo_exchange", t));
    WL_TRY(check_grid(g));
    const G gg = mkG(g);
    WL_DISPATCH_T(t, (halo_exchange<T>(gg, (T *)a, ncomp, depth)));
}
int wl_allreduce(double *vals, int n, int op) {
    Comm *cm = ctx().comm;
    if (!cm || cm->size == 1) return 0;
    if (n > 4) return fail(WL_E_ARG, "wl_allreduce: n <= 4", __FILE__, __LINE__);
    int rc = 0;
    Scratch &S = global_scratch(&rc);
    WL_TRY(rc);
    WL_HIP(hipMemcpyAsync(S.st.get()->red, vals, sizeof(double) * n, hipMemcpyHostToDevice, ctx().stream));
    const double init = op == 0 ? 0.0 : -1e300;
    // (np = 1: the "partials" are the values themselves; st->out doubles as the staging so that input and output differ)
    double *in = S.st.get()->red, *out4 = S.st.get()->out;
    int rc2 = 0;
    if (ctx().mbox) {
        WL_HIP(hipMemcpyAsync(out4, in, sizeof(double) * n, hipMemcpyDeviceToDevice, ctx().stream));
        switch (n) {
            case 1: rc2 = reduce_allreduce<1>(out4, 1, op, init, in); break;
            case 2: rc2 = reduce_allreduce<2>(out4, 1, op, init, in); break;
            case 3: rc2 = reduce_allreduce<3>(out4, 1, op, init, in); break;
            default: rc2 = reduce_allreduce<4>(out4, 1, op, init, in); break;
        }
    } else rc2 = cm->allreduce(S.st.get()->red, n, op);
    WL_TRY(rc2);
    WL_HIP(hipMemcpyAsync(vals, S.st.get()->red, sizeof(double) * n, hipMemcpyDeviceToHost, ctx().stream));
    WL_HIP(hipStreamSynchronize(ctx().stream));
    if (ctx().mbox && *ctx().mbox->err_host.get())
        return fail(WL_E_STATE, "mailbox all-reduce: gave up waiting for a peer rank (is every rank still running?)", __FILE__, __LINE__);
    return 0;
}

int wl_abi_version(void) { return WL_ABI_VERSION; }
const char *wl_last_error(void) { return ctx().err.c_str(); }
int wl_device_count(int *n) {
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) { *n = 0; return fail((int)e, "hipGetDeviceCount", __FILE__, __LINE__); }
    *n = c;
    return 0;
}
int wl_set_device(int dev) { WL_HIP(hipSetDevice(dev)); return 0; }
int wl_set_stream(void *s) { ctx().stream = (hipStream_t)s; return 0; }
int wl_sync(void) { WL_HIP(hipStreamSynchronize(ctx().stream)); return 0; }
int wl_malloc(void **p, size_t bytes) { WL_HIP(wl_dev_alloc(p, bytes)); return 0; }
int wl_free(void *p) { WL_HIP(hipFree(p)); return 0; }
int wl_h2d(void *dst, const void *src, size_t bytes) {
    WL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx().stream));
    WL_HIP(hipStreamSynchronize(ctx().stream));
    return 0;
}
int wl_d2h(void *dst, const void *src, size_t bytes) {
    WL_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx().stream));
    WL_HIP(hipStreamSynchronize(ctx().stream));
    return 0;
}
int wl_memset0(void *p, size_t bytes) { WL_HIP(hipMemsetAsync(p, 0, bytes, ctx().stream)); return 0; }
int wl_h2d_2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height) {
    if (width > dpitch || width > spitch) return fail(WL_E_ARG, "wl_h2d_2d: row wider than a pitch", __FILE__, __LINE__);
    WL_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice, ctx().stream));
    WL_HIP(hipStreamSynchronize(ctx().stream));
    return 0;
}
int wl_d2h_2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height) {
    if (width > dpitch || width > spitch) return fail(WL_E_ARG, "wl_d2h_2d: row wider than a pitch", __FILE__, __LINE__);
    WL_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, ctx().stream));
    WL_HIP(hipStreamSynchronize(ctx().stream));
    return 0;
}

// the opening of an entry point that takes (t, g): dtype and grid are checked before the device is touched for the scratch
#define WL_GS()                                  \
    WL_TRY(check_dtype(__func__, t));            \
    WL_TRY(check_grid(g));                       \
    int rc__ = 0;                                \
    Scratch &S = global_scratch(&rc__);          \
    (void)S;                                     \
    WL_TRY(rc__);                                \
    const G gg = mkG(g)
#define WL_GS_OUT() if (!out) WL_BAD(__func__, "null output"); WL_GS()   // ... and that hands its result back through `out`
// ... that takes two grids
#define WL_GS2()                                 \
    WL_TRY(check_dtype(__func__, t));            \
    WL_TRY(check_grid(ga));                      \
    WL_TRY(check_grid(gb));                      \
    const G A = mkG(ga), B = mkG(gb)

int wl_bc_vec(wl_dtype t, const wl_grid *g, void *a, const double A[3], int saveexit, int perdir_mask) {
    WL_GS();
    WL_DISPATCH(t, g->D, (op_bc_vec<T, DD>(gg, (T *)a, A, saveexit, perdir_mask)));
}
int wl_bc_per(wl_dtype t, const wl_grid *g, void *a, int perdir_mask) {
    WL_GS();
    WL_DISPATCH(t, g->D, (op_bc_per<T, DD>(gg, (T *)a, perdir_mask)));
}
int wl_exit_bc(wl_dtype t, const wl_grid *g, void *u, const void *u0, const double U[3], double dt) {
    WL_GS();
    WL_DISPATCH(t, g->D, (op_exit_bc<T, DD>(gg, (T *)u, (const T *)u0, U, dt, S.partials.get(), S.st.get())));
}

#define WL_RED(CALL)                 \
    do {                             \
        int r1__ = [&]() -> int { WL_DISPATCH(t, g->D, CALL); }(); \
        if (r1__) return r1__;       \
        WL_TRY(S.fetch());           \
        *out = S.hst.get()->out[0];        \
        return 0;                    \
    } while (0)

int wl_L2_inside(wl_dtype t, const wl_grid *g, const void *a, double *out) {
    WL_GS_OUT();
    WL_RED((red_L2<T, DD>(gg, (const T *)a, S)));
}
int wl_dot(wl_dtype t, const wl_grid *g, const void *a, const void *b, double *out) {
    WL_GS_OUT();
    WL_RED((red_dot<T, DD>(gg, (const T *)a, (const T *)b, S)));
}
int wl_sum(wl_dtype t, const wl_grid *g, const void *a, double *out) {
    WL_GS_OUT();
    WL_RED((red_sum<T, DD>(gg, (const T *)a, S)));
}
int wl_max(wl_dtype t, const wl_grid *g, const void *a, double *out) {
    WL_GS_OUT();
    WL_RED((red_max<T, DD>(gg, (const T *)a, S)));
}

int wl_conv_diff(wl_dtype t, const wl_grid *g, void *r, const void *u, void *Phi, double nu, int perdir_mask) {
    WL_GS();
    WL_DISPATCH(t, g->D, (conv_diff_phi<T, DD>(gg, (T *)r, (const T *)u, (T *)Phi, nu, perdir_mask)));
}
int wl_accelerate(wl_dtype t, const wl_grid *g, void *r, const double acc[3]) {
    WL_GS();
    WL_DISPATCH(t, g->D, (op_accelerate<T, DD>(gg, (T *)r, acc)));
}
int wl_bdim(wl_dtype t, const wl_grid *g, void *u, const void *u0, void *f, const void *V, const void *mu0,
            const void *mu1, double dt) {
    WL_GS();
    WL_DISPATCH(t, g->D, (bdim_full<T, DD>(gg, (T *)u, (const T *)u0, (T *)f, (const T *)V, (const T *)mu0,
                                           (const T *)mu1, dt)));
}
int wl_scale_u(wl_dtype t, const wl_grid *g, void *u, double scale) {
    WL_GS();
    WL_DISPATCH(t, g->D, (op_scale_u<T, DD>(gg, (T *)u, scale)));
}
int wl_div(wl_dtype t, const wl_grid *g, void *z, const void *u) {
    WL_GS();
    WL_DISPATCH(t, g->D, (op_div<T, DD>(gg, (T *)z, (const T *)u)));
}
int wl_cfl(wl_dtype t, const wl_grid *g, void *sigma, const void *u, double nu, double *out) {
    WL_GS_OUT();
    WL_RED((op_cfl<T, DD>(gg, (T *)sigma, (const T *)u, nu, S.partials.get(), S.st.get())));
}
int wl_set_diag(wl_dtype t, const wl_grid *g, void *Dg, void *iD, const void *L) {
    WL_GS();
    WL_DISPATCH(t, g->D, (op_set_diag<T, DD>(gg, (T *)Dg, (T *)iD, (const T *)L)));
}
int wl_restrictL(wl_dtype t, const wl_grid *ga, void *a, const wl_grid *gb, const void *b, int perdir_mask) {
    WL_GS2();
    WL_DISPATCH(t, ga->D, (restrictL_full<T, DD>(A, (T *)a, B, (const T *)b, perdir_mask)));
}
int wl_restrict(wl_dtype t, const wl_grid *ga, void *a, const wl_grid *gb, const void *b) {
    WL_GS2();
    WL_DISPATCH(t, ga->D, (op_restrict<T, DD>(A, (T *)a, B, (const T *)b)));
}
int wl_prolongate(wl_dtype t, const wl_grid *ga, void *a, const wl_grid *gb, const void *b) {
    WL_GS2();
    WL_DISPATCH(t, ga->D, (op_prolongate<T, DD>(A, (T *)a, B, (const T *)b)));
}

// ---- multigrid handle
int wl_mg_create(wl_mg **out, wl_dtype t, int nlevels, const wl_level_desc *levels, int perdir_mask) {
    WL_TRY(check_dtype("wl_mg_create", t));
    if (!out || !levels || nlevels < 1) return fail(WL_E_ARG, "wl_mg_create: bad arguments", __FILE__, __LINE__);
    if (nlevels == 2) return fail(WL_E_LEVELS, "MultiLevelPoisson requires size=a2^n, where n>2", __FILE__, __LINE__);
    for (int l = 0; l < nlevels; ++l) {
        WL_TRY(check_grid(&levels[l].g));
        const wl_level_desc &d = levels[l];
        if (!d.L || !d.D || !d.iD || !d.x || !d.eps || !d.r || !d.z)
            return fail(WL_E_ARG, "wl_mg_create: null level array", __FILE__, __LINE__);
        if (l > 0)
            for (int k = 0; k < d.g.D; ++k) {
                auto gext = [k](const wl_grid &g) { return (k == 2 && g.nzg > 0) ? g.nzg : g.n[k]; };
                if (gext(d.g) != 1 + gext(levels[l - 1].g) / 2)  // restrictML, src/MultiLevelPoisson.jl:20
                    return fail(WL_E_ARG, "wl_mg_create: level extents must be 1+N/2 of the finer level", __FILE__, __LINE__);
            }
    }
    std::unique_ptr<wl_mg> m(new wl_mg());   // (an error return drops the handle and with it every buffer made so far)
    m->t = t; m->D = levels[0].g.D; m->nlev = nlevels; m->permask = perdir_mask;
    m->lev.assign(levels, levels + nlevels);
    WL_TRY(m->sc.init());
    WL_TRY(m->alloc_rowc());
    WL_TRY(wl_mg_update(m.get()));
    *out = m.release();
    return 0;
}
int wl_mg_destroy(wl_mg *m) {
    if (!m) return 0;
    (void)hipStreamSynchronize(ctx().stream);
    delete m;
    return 0;
}
#define WL_MG_DISPATCH(CALL) WL_DISPATCH(m->t, m->D, CALL)
#define WL_LEVEL_OK() \
    if (!m || level < 0 || level >= m->nlev) return fail(WL_E_ARG, "bad level", __FILE__, __LINE__)

int wl_mg_update(wl_mg *m) { WL_MG_DISPATCH((mg_update<T, DD>(m))); }
int wl_mg_update_changed(wl_mg *m, wl_flow *a) {
    if (!m || !a) return fail(WL_E_ARG, "null handle", __FILE__, __LINE__);
    const wl_grid &gm = m->lev[0].g, &gf = a->d.g;
    // a periodic z across slabs (ring): the ghost plane's source row lives on another rank -> full update
    const bool zper = (m->permask >> 2) & 1, yper = (m->permask >> 1) & 1;
    const bool usable = a->changed_valid && a->changed.get() && m->D == 3 && gf.D == 3 && gm.n[0] == gf.n[0] && gm.n[1] == gf.n[1] &&
                        gm.n[2] == gf.n[2] && m->lev[0].L == a->d.mu0 && !m->rowc.empty() && m->rowc[0].get() && !(zper && gm.nzg > 0);
    a->changed_pending = false;   // consumed (by the partial or by the full update below)
    if (!usable) return wl_mg_update(m);
    const long nrows = (long)gm.n[1] * gm.n[2];
    WL_TRY(m->dirty.reserve((size_t)nrows));
    // D, iD and the row constants of row (j,k) read L of the rows (j,k), (j+1,k), (j,k+1)
    hipLaunchKernelGGL(k_rows_dirty, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, ctx().stream, (const unsigned char *)a->changed.get(),
                       m->dirty.get(), gm.n[1], gm.n[2], (int)yper, (int)zper);
    WL_HIP(hipGetLastError());
    const unsigned char *dirty = m->dirty.get();
    WL_MG_DISPATCH((mg_update<T, DD>(m, dirty)));
}
int wl_mg_mult(wl_mg *m, int level, void *x) {
    WL_LEVEL_OK();
    WL_MG_DISPATCH((op_mult<T, DD>(lvl<T>(m, level), (T *)x, m->permask)));
}
int wl_mg_residual(wl_mg *m, int level) {
    WL_LEVEL_OK();
    WL_MG_DISPATCH((op_residual<T, DD>(lvl<T>(m, level), m->permask, m->sc.partials.get(), m->sc.st.get())));
}
int wl_mg_increment(wl_mg *m, int level) {
    WL_LEVEL_OK();
    WL_MG_DISPATCH((op_increment<T, DD>(lvl<T>(m, level), m->permask)));
}
int wl_mg_jacobi(wl_mg *m, int level, int it) {
    WL_LEVEL_OK();
    WL_MG_DISPATCH((op_jacobi<T, DD>(lvl<T>(m, level), it, m->permask)));
}
int wl_mg_pcg(wl_mg *m, int level, int it, int *n_updates) {
    WL_LEVEL_OK();
    int rc = [&]() -> int { WL_MG_DISPATCH((op_pcg<T, DD>(lvl<T>(m, level), it, m->permask, m->sc.partials.get(), m->sc.st.get(), false, -1, level == 0))); }();
    if (rc) return rc;
    if (n_updates) {
        WL_TRY(m->sc.fetch());
        *n_updates = m->sc.hst.get()->pcg.nupd;
    }
    return 0;
}
int wl_mg_uniform_rows(wl_mg *m, int level, long long *n_uniform, long long *n_rows) {
    WL_LEVEL_OK();
    if (!n_uniform || !n_rows) return fail(WL_E_ARG, "wl_mg_uniform_rows: null output", __FILE__, __LINE__);
    const wl_grid &g = m->lev[level].g;
    *n_uniform = 0;
    *n_rows = (long long)(g.n[1] - 2) * (g.D == 3 ? (g.own_hi > 0 ? g.own_hi - g.own_lo + 1 : g.n[2] - 2) : 1);
    if (g.D != 3 || level >= (int)m->rowc.size() || !m->rowc[level].get()) return 0;
    const size_t es = m->t == WL_F32 ? 4 : 8, cnt = (size_t)g.n[1] * g.n[2] * RC_N;
    std::vector<char> h(cnt * es);
    WL_HIP(hipMemcpyAsync(h.data(), m->rowc[level].get(), cnt * es, hipMemcpyDeviceToHost, ctx().stream));
    WL_HIP(hipStreamSynchronize(ctx().stream));
    for (size_t r = 0; r < cnt; r += RC_N) {
        const double c = m->t == WL_F32 ? (double)reinterpret_cast<const float *>(h.data())[r] : reinterpret_cast<const double *>(h.data())[r];
        if (c == c) ++*n_uniform;
    }
    return 0;
}
int wl_mg_L2(wl_mg *m, int level, double *out) {
    if (!out) return fail(WL_E_ARG, "wl_mg_L2: null output", __FILE__, __LINE__);
    WL_LEVEL_OK();
    int rc = [&]() -> int { WL_MG_DISPATCH((op_L2<T, DD>(lvl<T>(m, level), m->sc.partials.get(), m->sc.st.get()))); }();
    if (rc) return rc;
    WL_TRY(m->sc.fetch());
    *out = m->sc.hst.get()->pcg.r2;
    return 0;
}
int wl_mg_Linf(wl_mg *m, int level, double *out) {
    WL_LEVEL_OK();
    if (!out) return fail(WL_E_ARG, "wl_mg_Linf: null output", __FILE__, __LINE__);
    int rc = [&]() -> int { WL_MG_DISPATCH((mg_Linf<T, DD>(m, level))); }();
    if (rc) return rc;
    WL_TRY(m->sc.fetch());
    *out = m->sc.hst.get()->out[1];
    return 0;
}
int wl_mg_log(wl_mg *m, int on) {
    if (!m) return fail(WL_E_ARG, "null handle", __FILE__, __LINE__);
    m->log_on = on != 0;
    if (!on) m->log.clear();
    return 0;
}
int wl_mg_log_read(wl_mg *m, double *rows, int cap, int *n) {
    if (!m || !n || (cap > 0 && !rows)) return fail(WL_E_ARG, "wl_mg_log_read: null argument", __FILE__, __LINE__);
    const int have = (int)(m->log.size() / 3);
    *n = have;
    if (cap <= 0) return 0;                        // a query: nothing is consumed
    const int take = have < cap ? have : cap;
    for (int q = 0; q < 3 * take; ++q) rows[q] = m->log[q];
    m->log.erase(m->log.begin(), m->log.begin() + 3 * take);   // what did not fit stays for the next read
    return 0;
}
int wl_mg_vcycle(wl_mg *m, int level) {
    if (!m || level < 0 || level + 1 >= m->nlev) return fail(WL_E_ARG, "bad level", __FILE__, __LINE__);
    WL_MG_DISPATCH((mg_vcycle<T, DD>(m, level)));
}
int wl_mg_solve(wl_mg *m, double tol, int itmx, int *n_iter) {
    if (!m) return fail(WL_E_ARG, "null handle", __FILE__, __LINE__);
    WL_MG_DISPATCH((mg_solve<T, DD>(m, tol, itmx, n_iter)));
}

// ---- flow handle
int wl_flow_create(wl_flow **out, wl_dtype t, const wl_flow_desc *d) {
    WL_TRY(check_dtype("wl_flow_create", t));
    if (!out || !d) return fail(WL_E_ARG, "wl_flow_create: bad arguments", __FILE__, __LINE__);
    WL_TRY(check_grid(&d->g));
    if (!d->u || !d->u0 || !d->f || !d->p || !d->sigma || !d->V || !d->mu0 || !d->mu1)
        return fail(WL_E_ARG, "wl_flow_create: null field", __FILE__, __LINE__);
    std::unique_ptr<wl_flow> a(new wl_flow());   // (an error return drops the handle and with it every buffer made so far)
    a->t = t; a->d = *d;
    WL_TRY(a->sc.init());
    const size_t nrows = (size_t)d->g.n[1] * (size_t)(d->g.D > 2 ? d->g.n[2] : 1);
    WL_TRY(a->rowbuf.reserve(nrows));
    if (d->g.D > 2) {
        const size_t ntx = (size_t)(d->g.n[0] - 2 + 63) / 64;
        WL_TRY(a->segbuf.reserve(nrows * (ntx ? ntx : 1)));
    }
    *out = a.release();
    return 0;
}
int wl_flow_destroy(wl_flow *a) {
    if (!a) return 0;
    (void)hipStreamSynchronize(ctx().stream);
    delete a;
    return 0;
}
int wl_flow_update(wl_flow *a) {
    if (!a) return fail(WL_E_ARG, "null handle", __FILE__, __LINE__);
    a->changed_valid = false;   // the arrays were rewritten by the caller: nothing is known about which rows changed
    a->changed_pending = false;
    WL_DISPATCH(a->t, a->d.g.D, (flow_update<T, DD>(a)));
}
int wl_measure_rows(wl_flow *a, const wl_body_desc *body, double eps, int64_t *nband) {
    if (!a || !nband) return fail(WL_E_ARG, "wl_measure_rows: null argument", __FILE__, __LINE__);
    WL_TRY(check_body(body, a->d.g.D));
    if (!(eps > 0)) return fail(WL_E_ARG, "wl_measure_rows: eps must be positive", __FILE__, __LINE__);
    WL_DISPATCH(a->t, a->d.g.D, (measure_rows<T, DD>(a, body, eps, nband)));
}
int wl_measure_fill(wl_flow *a, const wl_body_desc *body, double eps, int64_t *cand_dev) {
    if (!a) return fail(WL_E_ARG, "null handle", __FILE__, __LINE__);
    WL_TRY(check_body(body, a->d.g.D));
    if (a->nband < 0) return fail(WL_E_STATE, "wl_measure_fill: call wl_measure_rows first", __FILE__, __LINE__);
    if (a->nband > 0 && !cand_dev) return fail(WL_E_ARG, "wl_measure_fill: null candidate buffer", __FILE__, __LINE__);
    WL_DISPATCH(a->t, a->d.g.D, (measure_fill<T, DD>(a, body, eps, cand_dev)));
}
int wl_body_nds(const wl_grid *g, const wl_body_desc *body, const int64_t *cand_dev, int64_t n, double *nds_dev) {
    WL_TRY(check_grid(g));
    WL_TRY(check_body(body, g->D));
    if (n <= 0) return 0;
    if (!cand_dev || !nds_dev) return fail(WL_E_ARG, "wl_body_nds: null buffer", __FILE__, __LINE__);
    const G gg = mkG(g);
    const BodyDev B = body_dev(body);
    Prof p(WL_K_PFORCE, n);
    if (g->D == 3) hipLaunchKernelGGL((k_body_nds<3>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx().stream, gg, B, (const long *)cand_dev, (long)n, nds_dev);
    else hipLaunchKernelGGL((k_body_nds<2>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx().stream, gg, B, (const long *)cand_dev, (long)n, nds_dev);
    return (int)hipGetLastError();
}
int wl_mesh_create(wl_mesh **out, const double *vert_host, int64_t nv, const int32_t *tri_host, int64_t nt, double exact_radius) {
    if (!out || !vert_host || !tri_host) return fail(WL_E_ARG, "wl_mesh_create: null argument", __FILE__, __LINE__);
    if (nt <= 0 || nv <= 0) return fail(WL_E_ARG, "wl_mesh_create: empty mesh (nt == 0 or nv == 0)", __FILE__, __LINE__);
    if (nt > (int64_t)0x3fffffff || nv > (int64_t)0x7fffffff) return fail(WL_E_ARG, "wl_mesh_create: mesh too large", __FILE__, __LINE__);
    if (!(exact_radius > 3.0) || !std::isfinite(exact_radius))
        return fail(WL_E_ARG, "wl_mesh_create: exact_radius too small (needs 2 + eps + 1 with eps > 0)", __FILE__, __LINE__);
    std::unique_ptr<wl_mesh> m(new wl_mesh);
    const char *err = mesh_build(*m, vert_host, nv, tri_host, nt, exact_radius);
    if (err) return fail(WL_E_ARG, err, __FILE__, __LINE__);
    *out = m.release();
    return 0;
}
int wl_mesh_destroy(wl_mesh *m) {
    if (!m) return 0;
    if (m->d_tri.get()) (void)hipStreamSynchronize(ctx().stream);
    delete m;
    return 0;
}
int wl_mesh_info(const wl_mesh *m, int64_t out[8]) {
    if (!m || !out) return fail(WL_E_ARG, "wl_mesh_info: null argument", __FILE__, __LINE__);
    out[0] = m->nt; out[1] = m->nv; out[2] = (int64_t)m->bin_sign.size(); out[3] = m->max_per_bin;
    out[4] = (int64_t)m->bin_tri.size(); out[5] = m->nonempty; out[6] = (int64_t)m->device_bytes(); out[7] = m->crossed;
    return 0;
}
int wl_mesh_eval_host(const wl_mesh *m, const wl_mesh_pose *pose, const double *x_host, int64_t n, double fastd2, double *d_host,
                      double *n_host, double *V_host) {
    PoseDev P;
    WL_TRY(mesh_pose(m, pose, 0.0, P));
    if (n > 0 && (!x_host || !d_host)) return fail(WL_E_ARG, "wl_mesh_eval_host: null buffer", __FILE__, __LINE__);
    const MeshDev M = m->view(false);
    for (int64_t q = 0; q < n; ++q) {
        const double x[3] = {x_host[3 * q], x_host[3 * q + 1], x_host[3 * q + 2]};
        double nn[3], V[3];
        mesh_measure(M, P, x, fastd2, d_host[q], nn, V);
        for (int c = 0; c < 3; ++c) {
            if (n_host) n_host[3 * q + c] = nn[c];
            if (V_host) V_host[3 * q + c] = V[c];
        }
    }
    return 0;
}
int wl_measure_rows_mesh(wl_flow *a, const wl_mesh *m, const wl_mesh_pose *pose, double eps, int64_t *nband) {
    if (!a || !nband) return fail(WL_E_ARG, "wl_measure_rows_mesh: null argument", __FILE__, __LINE__);
    if (a->d.g.D != 3) return fail(WL_E_ARG, "wl_measure_rows_mesh: a triangle mesh needs D == 3", __FILE__, __LINE__);
    if (!(eps > 0)) return fail(WL_E_ARG, "wl_measure_rows_mesh: eps must be positive", __FILE__, __LINE__);
    PoseDev P;
    WL_TRY(mesh_pose(m, pose, 2 + eps + 1, P));
    WL_DISPATCH_T(a->t, (mesh_rows<T>(a, m, P, eps, nband)));
}
int wl_measure_fill_mesh(wl_flow *a, const wl_mesh *m, const wl_mesh_pose *pose, double eps, int64_t *cand_dev) {
    if (!a) return fail(WL_E_ARG, "null handle", __FILE__, __LINE__);
    if (a->d.g.D != 3) return fail(WL_E_ARG, "wl_measure_fill_mesh: a triangle mesh needs D == 3", __FILE__, __LINE__);
    if (!(eps > 0)) return fail(WL_E_ARG, "wl_measure_fill_mesh: eps must be positive", __FILE__, __LINE__);
    PoseDev P;
    WL_TRY(mesh_pose(m, pose, 2 + eps + 1, P));
    if (a->nband < 0) return fail(WL_E_STATE, "wl_measure_fill_mesh: call wl_measure_rows_mesh first", __FILE__, __LINE__);
    if (a->nband > 0 && !cand_dev) return fail(WL_E_ARG, "wl_measure_fill_mesh: null candidate buffer", __FILE__, __LINE__);
    WL_DISPATCH_T(a->t, (mesh_fill<T>(a, m, P, eps, cand_dev)));
}
int wl_body_nds_mesh(const wl_grid *g, const wl_mesh *m, const wl_mesh_pose *pose, const int64_t *cand_dev, int64_t n, double *nds_dev) {
    WL_TRY(check_grid(g));
    if (g->D != 3) return fail(WL_E_ARG, "wl_body_nds_mesh: a triangle mesh needs D == 3", __FILE__, __LINE__);
    PoseDev P;
    WL_TRY(mesh_pose(m, pose, 1.0, P));
    if (n <= 0) return 0;
    if (!cand_dev || !nds_dev) return fail(WL_E_ARG, "wl_body_nds_mesh: null buffer", __FILE__, __LINE__);
    WL_TRY(mesh_upload(m));
    const G gg = mkG(g);
    const MeshDev M = m->view(true);
    Prof p(WL_K_PFORCE, n);
    hipLaunchKernelGGL(k_mesh_nds, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx().stream, gg, M, P, (const long *)cand_dev, (long)n, nds_dev);
    return (int)hipGetLastError();
}
static int check_pair(const wl_flow *a, const wl_mg *b) {
    if (!a || !b) return fail(WL_E_ARG, "null handle", __FILE__, __LINE__);
    if (a->t != b->t || a->d.g.D != b->D) return fail(WL_E_ARG, "flow/poisson type mismatch", __FILE__, __LINE__);
    const wl_level_desc &l0 = b->lev[0];
    // src/WaterLily.jl:77: pois.x === flow.p, pois.L === flow.mu0, pois.z === flow.sigma
    if (l0.x != a->d.p || l0.L != a->d.mu0 || l0.z != a->d.sigma)
        return fail(WL_E_ARG, "level-1 (x,L,z) must alias flow (p,mu0,sigma)", __FILE__, __LINE__);
    for (int k = 0; k < 3; ++k)
        if (l0.g.n[k] != a->d.g.n[k] || l0.g.s[k] != a->d.g.s[k]) return fail(WL_E_ARG, "flow/poisson grid mismatch", __FILE__, __LINE__);
    return 0;
}
int wl_project(wl_flow *a, wl_mg *b, double dt, double w, int *n_iter) {
    WL_TRY(check_pair(a, b));
    WL_DISPATCH(a->t, a->d.g.D, (flow_project<T, DD>(a, b, dt, w, n_iter)));
}
int wl_mom_step(wl_flow *a, wl_mg *b, double dt, const double U[3], const double *acc_pred, const double *acc_corr,
                double *dt_next, int n_iter[2]) {
    WL_TRY(check_pair(a, b));
    if (!U || !dt_next || !n_iter) return fail(WL_E_ARG, "wl_mom_step: null output", __FILE__, __LINE__);
    WL_DISPATCH(a->t, a->d.g.D, (flow_mom_step<T, DD>(a, b, dt, U, acc_pred, acc_corr, dt_next, n_iter)));
}

// ---- Metrics.jl:94-100
int wl_vforce(wl_dtype t, const wl_grid *g, const void *u, const int64_t *idx, const double *nds, int64_t nband, double nu,
              double out[3]) {
    WL_GS_OUT();
    return band_reduce(gg, S, nband, g->D, out, [&](int nb) {
        if (t == WL_F32) hipLaunchKernelGGL(k_vforce<float>, dim3(nb), dim3(256), 0, ctx().stream, gg, (const float *)u, idx, nds, nband, (float)nu, S.partials.get());
        else hipLaunchKernelGGL(k_vforce<double>, dim3(nb), dim3(256), 0, ctx().stream, gg, (const double *)u, idx, nds, nband, nu, S.partials.get());
    });
}
int wl_pmoment(wl_dtype t, const wl_grid *g, const void *p, const int64_t *idx, const double *nds, int64_t nband,
               const double x0[3], double out[3]) {
    if (!x0) WL_BAD("wl_pmoment", "null x0");
    WL_GS_OUT();
    const double a = x0[0], b = x0[1], c = g->D > 2 ? x0[2] : 0.0;
    return band_reduce(gg, S, nband, g->D, out, [&](int nb) {
        if (t == WL_F32) hipLaunchKernelGGL(k_pmoment<float>, dim3(nb), dim3(256), 0, ctx().stream, gg, (const float *)p, idx, nds, nband, a, b, c, S.partials.get());
        else hipLaunchKernelGGL(k_pmoment<double>, dim3(nb), dim3(256), 0, ctx().stream, gg, (const double *)p, idx, nds, nband, a, b, c, S.partials.get());
    });
}
// ---- Forces (wl_forces.h): every argument check comes before the first device call
static int check_loads(const char *who, wl_dtype t, const wl_grid *g, const void *p, const void *u, const void *list, int64_t n,
                       const double *x0, const double *rows) {
    if (!g || !p || !u || !x0 || !rows) WL_BAD(who, "null grid, p, u, x0 or rows");
    WL_TRY(check_dtype(who, t));
    if (n < 0) WL_BAD(who, "n < 0");
    if (n > 0 && !list) WL_BAD(who, "null cell list");
    if (g->D != 2 && g->D != 3) WL_BAD(who, "D must be 2 or 3");
    WL_TRY(check_grid(g));
    return check_halo_planes(who, mkG(g), true);
}
int wl_body_loads(wl_dtype t, const wl_grid *g, const void *p, const void *u, double nu, const wl_body_desc *body, const int64_t *cand_dev,
                  int64_t n, const double x0[3], double *rows_dev) {
    WL_TRY(check_loads("wl_body_loads", t, g, p, u, cand_dev, n, x0, rows_dev));
    WL_TRY(check_body(body, g->D));
    WL_GS();
    const int nleaf = body[0].count > 0 ? body[0].count : 1;
    WL_DISPATCH(t, g->D, (op_loads<T, DD>(gg, LoadsBody<DD>{body_dev(body), (const long *)cand_dev}, (const T *)p, (const T *)u, nu, (long)n, x0, nleaf,
                                          S.partials.get(), rows_dev)));
}
int wl_body_loads_mesh(wl_dtype t, const wl_grid *g, const void *p, const void *u, double nu, const wl_mesh *m, const wl_mesh_pose *pose,
                       const int64_t *cand_dev, int64_t n, const double x0[3], double *rows_dev) {
    WL_TRY(check_loads("wl_body_loads_mesh", t, g, p, u, cand_dev, n, x0, rows_dev));
    if (g->D != 3) return fail(WL_E_ARG, "wl_body_loads_mesh: a triangle mesh needs D == 3", __FILE__, __LINE__);
    LoadsMesh src;
    WL_TRY(mesh_pose(m, pose, 1.0, src.P));
    WL_GS();
    WL_TRY(mesh_upload(m));
    src.M = m->view(true);
    src.cand = (const long *)cand_dev;
    WL_DISPATCH_T(t, (op_loads<T, 3>(gg, src, (const T *)p, (const T *)u, nu, (long)n, x0, 1, S.partials.get(), rows_dev)));
}
int wl_band_loads(wl_dtype t, const wl_grid *g, const void *p, const void *u, double nu, const int64_t *idx_dev, const double *nds_dev,
                  int64_t n, const double x0[3], double *rows_dev) {
    WL_TRY(check_loads("wl_band_loads", t, g, p, u, idx_dev, n, x0, rows_dev));
    if (n > 0 && !nds_dev) return fail(WL_E_ARG, "wl_band_loads: null nds", __FILE__, __LINE__);
    WL_GS();
    WL_DISPATCH(t, g->D, (op_loads<T, DD>(gg, LoadsBand<DD>{idx_dev, nds_dev}, (const T *)p, (const T *)u, nu, (long)n, x0, 1, S.partials.get(), rows_dev)));
}
int wl_metric(wl_dtype t, const wl_grid *g, int kind, void *out, const void *u, int ipar, const double par[3],
              const double par2[3]) {
    WL_GS();
    if (!metric_kind_ok(kind, ipar, g->D))
        return fail(WL_E_ARG, "wl_metric: bad kind/component for this dimension", __FILE__, __LINE__);
    WL_DISPATCH(t, g->D, (op_metric<T, DD>(gg, kind, (T *)out, (const T *)u, ipar, par, par2)));
}
int wl_flow_integrals(wl_dtype t, const wl_grid *g, const void *u, const double U[3], double *row_dev) {
    if (!g || !u || !U || !row_dev) return fail(WL_E_ARG, "wl_flow_integrals: null grid, u, U or row", __FILE__, __LINE__);
    if (g->D != 2 && g->D != 3) return fail(WL_E_ARG, "wl_flow_integrals: D must be 2 or 3", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    WL_TRY(check_halo_planes("wl_flow_integrals", mkG(g), true));
    WL_GS();
    WL_DISPATCH(t, g->D, (op_integrals<T, DD>(gg, (const T *)u, U, S.partials.get(), row_dev)));
}
int wl_meanflow_update(wl_dtype t_flow, wl_dtype t_acc, const wl_grid *g, const void *u, const void *p, const wl_grid *ga, void *U,
                       void *P, void *UU, void *pp, double eps, int first) {
    WL_TRY(check_grid(g));
    WL_TRY(check_grid(ga));
    WL_TRY(check_dtype("wl_meanflow_update", t_flow));
    WL_TRY(check_dtype("wl_meanflow_update", t_acc));
    if (t_flow == WL_F64 && t_acc == WL_F32)
        return fail(WL_E_ARG, "wl_meanflow_update: Float32 accumulators on a Float64 flow", __FILE__, __LINE__);
    if (!u || !p || !U || !P) return fail(WL_E_ARG, "wl_meanflow_update: null u, p, U or P", __FILE__, __LINE__);
    bool same = ga->D == g->D && ga->nzg == g->nzg;
    for (int d = 0; d < 3; ++d) same = same && ga->n[d] == g->n[d];
    if (same && g->D == 3 && g->nzg > 0)
        same = ga->kz0 == g->kz0 && ga->own_lo == g->own_lo && ga->own_hi == g->own_hi && ga->zring == g->zring;
    if (!same) return fail(WL_E_ARG, "wl_meanflow_update: the accumulators' grid must have the flow grid's extents and slab", __FILE__, __LINE__);
    if (!(eps > 0.0 && eps <= 1.0)) return fail(WL_E_ARG, "wl_meanflow_update: eps must lie in (0, 1]", __FILE__, __LINE__);
    const G gf = mkG(g), gacc = mkG(ga);
    // the three (flow, accumulator) pairs: Float64 accumulators on either flow, Float32 ones on a Float32 flow (checked above)
#define WL_MEANFLOW(TF, TA, DD) op_meanflow<TF, TA, DD>(gf, gacc, (const TF *)u, (const TF *)p, (TA *)U, (TA *)P, (TA *)UU, (TA *)pp, eps, first)
    if (t_acc == WL_F64) WL_DISPATCH(t_flow, g->D, (WL_MEANFLOW(T, double, DD)));
    if (g->D == 3) return WL_MEANFLOW(float, float, 3);
    return WL_MEANFLOW(float, float, 2);
#undef WL_MEANFLOW
}
// ---- Budget (wl_budget.h): every argument check comes before the first device call
static int check_acc_grid(const char *who, const wl_grid *g, const wl_grid *ga) {
    bool same = ga->D == g->D && ga->nzg == g->nzg;
    for (int d = 0; d < 3; ++d) same = same && ga->n[d] == g->n[d];
    if (same && g->D == 3 && g->nzg > 0)
        same = ga->kz0 == g->kz0 && ga->own_lo == g->own_lo && ga->own_hi == g->own_hi && ga->zring == g->zring;
    if (!same) WL_BAD(who, "the accumulators' grid must have the flow grid's extents and slab");
    return 0;
}
int wl_budget_update(wl_dtype t_flow, wl_dtype t_acc, const wl_grid *g, const void *u, const void *p, const wl_grid *ga, const void *Uf,
                     const void *Pm, void *R, void *PU, void *GG, void *T3, double eps, int first) {
    if (!g || !ga) return fail(WL_E_ARG, "wl_budget_update: null grid", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    WL_TRY(check_grid(ga));
    WL_TRY(check_dtype("wl_budget_update", t_flow));
    WL_TRY(check_dtype("wl_budget_update", t_acc));
    if (t_flow == WL_F64 && t_acc == WL_F32)
        return fail(WL_E_ARG, "wl_budget_update: Float32 accumulators on a Float64 flow", __FILE__, __LINE__);
    if (!u || !p || !Uf || !Pm || !R || !PU || !GG || !T3)
        return fail(WL_E_ARG, "wl_budget_update: null u, p, Uf, Pm, R, PU, GG or T3", __FILE__, __LINE__);
    if (g->D != 2 && g->D != 3) return fail(WL_E_ARG, "wl_budget_update: D must be 2 or 3", __FILE__, __LINE__);
    WL_TRY(check_acc_grid("wl_budget_update", g, ga));
    if (!(eps > 0.0 && eps <= 1.0)) return fail(WL_E_ARG, "wl_budget_update: eps must lie in (0, 1]", __FILE__, __LINE__);
    const G gf = mkG(g), gacc = mkG(ga);
    WL_TRY(check_halo_planes("wl_budget_update", gf, true));
#define WL_BUDGET(TF, TA, DD) op_budget_update<TF, TA, DD>(gf, gacc, (const TF *)u, (const TF *)p, (const TA *)Uf, (const TA *)Pm, (TA *)R, (TA *)PU, (TA *)GG, (TA *)T3, eps, first)
    if (t_acc == WL_F64) WL_DISPATCH(t_flow, g->D, (WL_BUDGET(T, double, DD)));
    if (g->D == 3) return WL_BUDGET(float, float, 3);
    return WL_BUDGET(float, float, 2);
#undef WL_BUDGET
}
int wl_budget_terms(wl_dtype t_acc, const wl_grid *ga, const void *Uf, const void *R, const void *PU, const void *GG, const void *T3,
                    double nu, void *out) {
    if (!ga) return fail(WL_E_ARG, "wl_budget_terms: null grid", __FILE__, __LINE__);
    WL_TRY(check_grid(ga));
    WL_TRY(check_dtype("wl_budget_terms", t_acc));
    if (!Uf || !R || !PU || !GG || !T3 || !out) return fail(WL_E_ARG, "wl_budget_terms: null Uf, R, PU, GG, T3 or out", __FILE__, __LINE__);
    if (ga->D != 2 && ga->D != 3) return fail(WL_E_ARG, "wl_budget_terms: D must be 2 or 3", __FILE__, __LINE__);
    if (!std::isfinite(nu)) return fail(WL_E_ARG, "wl_budget_terms: nu must be finite", __FILE__, __LINE__);
    const G gg = mkG(ga);
    WL_TRY(check_halo_planes("wl_budget_terms", gg, true));
    WL_DISPATCH(t_acc, ga->D, (op_budget_terms<T, DD>(gg, (const T *)Uf, (const T *)R, (const T *)PU, (const T *)GG, (const T *)T3, nu, (T *)out)));
}
int wl_interp(wl_dtype t, const wl_grid *g, const void *a, int ncomp, const double *x_dev, int64_t m, double *out_dev,
              int64_t ldo) {
    WL_TRY(check_grid(g));
    WL_TRY(check_dtype("wl_interp", t));
    if (!a || !x_dev || !out_dev) return fail(WL_E_ARG, "wl_interp: null field, points or output", __FILE__, __LINE__);
    if (ncomp != 0 && ncomp != g->D) return fail(WL_E_ARG, "wl_interp: ncomp must be 0 (scalar) or D (staggered vector)", __FILE__, __LINE__);
    if (m < 0) return fail(WL_E_ARG, "wl_interp: negative number of points", __FILE__, __LINE__);
    if (ldo < (ncomp > 1 ? ncomp : 1)) return fail(WL_E_ARG, "wl_interp: ldo smaller than one row of the result", __FILE__, __LINE__);
    const G gg = mkG(g);
    WL_DISPATCH(t, g->D, (op_interp<T, DD>(gg, (const T *)a, ncomp, x_dev, m, out_dev, ldo)));
}
int wl_surface_sample(wl_dtype t, const wl_grid *g, const void *p, const void *u, const wl_mesh *m, const wl_mesh_pose *pose,
                      double delta, double nu, double *rows_dev, double *geom_dev, double *mean_dev, double w, int first) {
    if (!m || !pose) return fail(WL_E_ARG, "wl_surface_sample: null mesh or pose", __FILE__, __LINE__);
    if (!rows_dev) return fail(WL_E_ARG, "wl_surface_sample: null output rows", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    if (g->D != 3) return fail(WL_E_ARG, "wl_surface_sample: a triangle mesh needs D == 3", __FILE__, __LINE__);
    WL_TRY(check_dtype("wl_surface_sample", t));
    if (!p || !u) return fail(WL_E_ARG, "wl_surface_sample: null p or u", __FILE__, __LINE__);
    if (!(std::isfinite(delta) && delta >= 0.0)) return fail(WL_E_ARG, "wl_surface_sample: delta must be finite and >= 0", __FILE__, __LINE__);
    if (!std::isfinite(nu)) return fail(WL_E_ARG, "wl_surface_sample: nu must be finite", __FILE__, __LINE__);
    if (mean_dev && !first && !(w > 0.0 && w <= 1.0)) return fail(WL_E_ARG, "wl_surface_sample: the mean's weight w must lie in (0, 1]", __FILE__, __LINE__);
    PoseDev P;
    WL_TRY(mesh_pose(m, pose, 0.0, P));
    WL_TRY(mesh_upload(m));
    const G gg = mkG(g);
    const MeshDev M = m->view(true);
    WL_DISPATCH_T(t, (op_surface_sample<T>(gg, M, m->nt, P, (const T *)p, (const T *)u, delta, nu, rows_dev, geom_dev, mean_dev, w, first)));
}
int wl_surface_totals(const double *rows_dev, const double *geom_dev, int64_t nt, const double x0[3], double *out_dev) {
    if (!rows_dev || !geom_dev || !x0 || !out_dev) return fail(WL_E_ARG, "wl_surface_totals: null rows, geometry, x0 or output", __FILE__, __LINE__);
    if (nt <= 0) return fail(WL_E_ARG, "wl_surface_totals: nt must be positive", __FILE__, __LINE__);
    if (!(std::isfinite(x0[0]) && std::isfinite(x0[1]) && std::isfinite(x0[2]))) return fail(WL_E_ARG, "wl_surface_totals: x0 must be finite", __FILE__, __LINE__);
    int rc = 0;
    Scratch &S = global_scratch(&rc);
    WL_TRY(rc);
    return op_surface_totals(rows_dev, geom_dev, nt, x0, S.partials.get(), out_dev);
}
int wl_iso_table(int tet, int mask, int32_t out[7]) {
    if (tet < 0 || tet > 5 || mask < 0 || mask > 15) return fail(WL_E_ARG, "wl_iso_table: tet must lie in 0..5 and mask in 0..15", __FILE__, __LINE__);
    if (!out) return fail(WL_E_ARG, "wl_iso_table: null output", __FILE__, __LINE__);
    const uint32_t w = ISO_TRI[tet][mask];
    const int nt = (int)(w >> 24);
    out[0] = nt;
    for (int k = 0; k < 6; ++k) out[1 + k] = k < 3 * nt ? (int32_t)((w >> (4 * k)) & 15u) : -1;
    return 0;
}
int wl_isosurface(wl_dtype t, const wl_grid *g, const void *a, const void *b, double c, const int32_t lo[3], const int32_t hi[3],
                  double *tri_dev, double *val_dev, int64_t cap, int64_t *count_dev) {
    if (!g || !a || !count_dev) return fail(WL_E_ARG, "wl_isosurface: null grid, field or count", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    if (g->D != 3) return fail(WL_E_ARG, "wl_isosurface: an isosurface needs D == 3", __FILE__, __LINE__);
    WL_TRY(check_dtype("wl_isosurface", t));
    if (!std::isfinite(c)) return fail(WL_E_ARG, "wl_isosurface: the level c must be finite", __FILE__, __LINE__);
    if (cap < 0) return fail(WL_E_ARG, "wl_isosurface: negative capacity", __FILE__, __LINE__);
    if (cap > 0 && !tri_dev) return fail(WL_E_ARG, "wl_isosurface: null triangle buffer with cap > 0", __FILE__, __LINE__);
    if ((b != nullptr) != (val_dev != nullptr))
        return fail(WL_E_ARG, "wl_isosurface: the colour field b and val_dev must be given together", __FILE__, __LINE__);
    const G gg = mkG(g);
    int l[3], h[3];
    WL_TRY(parse_box("wl_isosurface", gg, 3, 2, true, lo, hi, l, h));   // (no box: the cells whose upper corner is in inside())
    WL_DISPATCH_T(t, (op_isosurface<T>(gg, (const T *)a, (const T *)b, c, l, h, tri_dev, val_dev, cap, count_dev)));
}
int wl_render_project(wl_dtype t, const wl_grid *g, const void *f, int kind, int ipar, const double par[3], const double par2[3],
                      int axis, int mode, const int32_t lo[3], const int32_t hi[3], double *img_dev, int64_t ld) {
    if (!g || !f || !img_dev) return fail(WL_E_ARG, "wl_render_project: null grid, field or image", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    WL_TRY(check_dtype("wl_render_project", t));
    const int D = g->D;
    const bool metric = kind >= WL_R_METRIC;
    WL_TRY(check_kind("wl_render_project", kind, ipar, D, false));
    if (mode < WL_R_MAX || mode > WL_R_MEAN) return fail(WL_E_ARG, "wl_render_project: bad mode", __FILE__, __LINE__);
    if (D == 2 ? axis != 2 : (axis < 0 || axis > 2)) return fail(WL_E_ARG, "wl_render_project: bad axis (0..2; a 2-D grid takes 2)", __FILE__, __LINE__);
    const G gg = mkG(g);
    int l[3], h[3];
    WL_TRY(parse_box("wl_render_project", gg, D, 1, true, lo, hi, l, h));
    if (metric) WL_TRY(check_metric_box("wl_render_project", D, l));
    if (metric) WL_TRY(check_halo_planes("wl_render_project", gg, false));
    const int wa = axis == 0 ? 1 : 0;
    if (ld < (int64_t)(h[wa] - l[wa])) return fail(WL_E_ARG, "wl_render_project: ld smaller than the image width", __FILE__, __LINE__);
    WL_DISPATCH(t, D, (op_render_project<T, DD>(gg, (const T *)f, kind, ipar, par, par2, axis, mode, l, h, img_dev, ld)));
}
int wl_render_shade(const double *img_dev, int64_t ld, int nx, int ny, double vmin, double vmax, int levels, const uint8_t *lut_dev,
                    const double *mask_dev, int64_t ldm, double mask_lt, const uint8_t mask_rgba[4], const uint8_t nan_rgba[4], int zoom,
                    int flip_y, uint8_t *rgba_dev) {
    if (!img_dev || !lut_dev || !rgba_dev) return fail(WL_E_ARG, "wl_render_shade: null image, colour table or output", __FILE__, __LINE__);
    if (((uintptr_t)rgba_dev & 3u) != 0) return fail(WL_E_ARG, "wl_render_shade: the output must be 4-byte aligned", __FILE__, __LINE__);
    if (!(std::isfinite(vmin) && std::isfinite(vmax) && vmin < vmax)) return fail(WL_E_ARG, "wl_render_shade: need finite vmin < vmax", __FILE__, __LINE__);
    if (levels < 0 || levels > 256) return fail(WL_E_ARG, "wl_render_shade: levels must lie in 0..256", __FILE__, __LINE__);
    if (zoom < 1) return fail(WL_E_ARG, "wl_render_shade: zoom must be >= 1", __FILE__, __LINE__);
    if (nx < 0 || ny < 0 || ld < nx) return fail(WL_E_ARG, "wl_render_shade: bad image extents or ld smaller than the width", __FILE__, __LINE__);
    if (mask_dev && (!mask_rgba || ldm < nx || std::isnan(mask_lt)))
        return fail(WL_E_ARG, "wl_render_shade: a mask needs its colour, a threshold and ldm >= the width", __FILE__, __LINE__);
    auto word = [](const uint8_t *c) { return c ? (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24) : 0u; };
    ShadeArgs A;
    A.ld = ld; A.ldm = ldm; A.nx = nx; A.ny = ny; A.levels = levels; A.zoom = zoom; A.flip_y = flip_y ? 1 : 0; A.masked = mask_dev ? 1 : 0;
    A.vmin = vmin; A.vmax = vmax; A.mask_lt = mask_lt; A.mask_rgba = mask_dev ? word(mask_rgba) : 0u; A.nan_rgba = word(nan_rgba);
    return op_render_shade(A, img_dev, mask_dev, lut_dev, rgba_dev);
}
// the checks every wl_scene_* entry shares: the image extents
static int scene_size(const char *who, int W, int H) {
    if (W < 1 || W > WL_SCENE_MAX_SIZE || H < 1 || H > WL_SCENE_MAX_SIZE) WL_BAD(who, "W and H must lie in 1..4096");
    return 0;
}
// ... and the triangles of one draw with their ids base .. base + nt - 1
static int scene_tris(const char *who, int64_t nt, uint32_t base, const double *tri_dev, const double M[16], SceneCam *C) {
    if (nt < 0) WL_BAD(who, "negative nt");
    if ((uint64_t)base + (uint64_t)nt > 0xFFFFFFFFull) WL_BAD(who, "base + nt must not exceed 2^32 - 1 (the triangle ids of one picture)");
    if (nt > 0 && !tri_dev) WL_BAD(who, "null triangles with nt > 0");
    if (!M) WL_BAD(who, "null camera matrix");
    for (int k = 0; k < 16; ++k) {
        if (!std::isfinite(M[k])) WL_BAD(who, "the camera matrix must be finite");
        C->m[k] = M[k];
    }
    return 0;
}
int wl_scene_clear(uint64_t *key_dev, int W, int H) {
    if (!key_dev) return fail(WL_E_ARG, "wl_scene_clear: null keys", __FILE__, __LINE__);
    WL_TRY(scene_size("wl_scene_clear", W, H));
    return op_scene_clear((unsigned long long *)key_dev, W, H);
}
int wl_scene_scratch(int64_t nt, int64_t *bytes) {
    if (!bytes || nt < 0 || nt > 0xFFFFFFFFll) return fail(WL_E_ARG, "wl_scene_scratch: null bytes or nt outside 0..2^32 - 1", __FILE__, __LINE__);
    *bytes = scene_scratch_bytes(nt);
    return 0;
}
int wl_scene_draw(uint64_t *key_dev, int W, int H, const double M[16], const double *tri_dev, int64_t nt, uint32_t base, int64_t large_px,
                  void *scratch_dev, int64_t scratch_bytes) {
    if (!key_dev || !scratch_dev) return fail(WL_E_ARG, "wl_scene_draw: null keys or scratch", __FILE__, __LINE__);
    WL_TRY(scene_size("wl_scene_draw", W, H));
    SceneCam C;
    WL_TRY(scene_tris("wl_scene_draw", nt, base, tri_dev, M, &C));
    if (large_px < 0) return fail(WL_E_ARG, "wl_scene_draw: negative large_px", __FILE__, __LINE__);
    if (scratch_bytes < scene_scratch_bytes(nt)) return fail(WL_E_ARG, "wl_scene_draw: scratch_bytes below wl_scene_scratch's", __FILE__, __LINE__);
    if (((uintptr_t)scratch_dev & 3u) != 0) return fail(WL_E_ARG, "wl_scene_draw: the scratch must be 4-byte aligned", __FILE__, __LINE__);
    return op_scene_draw((unsigned long long *)key_dev, W, H, C, tri_dev, nt, base, large_px, (unsigned *)scratch_dev);
}
int wl_scene_shade(const uint64_t *key_dev, int W, int H, uint32_t base, int64_t nt, const double *tri_dev, const double *val_dev,
                   const double M[16], double vmin, double vmax, int levels, const uint8_t *lut_dev, const uint8_t solid_rgba[4],
                   const double light[3], double ambient, const uint8_t nan_rgba[4], uint8_t *rgba_dev) {
    if (!key_dev || !rgba_dev || !light) return fail(WL_E_ARG, "wl_scene_shade: null keys, output or light", __FILE__, __LINE__);
    if (((uintptr_t)rgba_dev & 3u) != 0) return fail(WL_E_ARG, "wl_scene_shade: the output must be 4-byte aligned", __FILE__, __LINE__);
    WL_TRY(scene_size("wl_scene_shade", W, H));
    SceneCam C;
    WL_TRY(scene_tris("wl_scene_shade", nt, base, tri_dev, M, &C));
    if (val_dev) {
        if (!lut_dev) return fail(WL_E_ARG, "wl_scene_shade: vertex values need a colour table", __FILE__, __LINE__);
        if (!(std::isfinite(vmin) && std::isfinite(vmax) && vmin < vmax)) return fail(WL_E_ARG, "wl_scene_shade: need finite vmin < vmax", __FILE__, __LINE__);
        if (levels < 0 || levels > 256) return fail(WL_E_ARG, "wl_scene_shade: levels must lie in 0..256", __FILE__, __LINE__);
    } else if (!solid_rgba) {
        return fail(WL_E_ARG, "wl_scene_shade: no vertex values and no solid colour", __FILE__, __LINE__);
    }
    if (!(ambient >= 0.0 && ambient <= 1.0)) return fail(WL_E_ARG, "wl_scene_shade: ambient must lie in 0..1", __FILE__, __LINE__);
    if (!(std::isfinite(light[0]) && std::isfinite(light[1]) && std::isfinite(light[2])))
        return fail(WL_E_ARG, "wl_scene_shade: the light direction must be finite", __FILE__, __LINE__);
    auto word = [](const uint8_t *c) { return c ? (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24) : 0u; };
    SceneShade A;
    A.W = W; A.H = H; A.levels = levels; A.has_val = val_dev ? 1 : 0; A.base = base; A.nt = (long)nt;
    A.vmin = vmin; A.vmax = vmax; A.ambient = ambient;
    for (int d = 0; d < 3; ++d) A.light[d] = light[d];
    A.solid = word(solid_rgba); A.nan_rgba = word(nan_rgba);
    return op_scene_shade(C, A, (const unsigned long long *)key_dev, tri_dev, val_dev, lut_dev, rgba_dev);
}
int wl_scene_resolve(const uint8_t *rgba_dev, int W, int H, const uint64_t *key_dev, int ssaa, const uint8_t background_rgba[4],
                     uint8_t *out_dev) {
    if (!rgba_dev || !key_dev || !background_rgba || !out_dev)
        return fail(WL_E_ARG, "wl_scene_resolve: null frame, keys, background or output", __FILE__, __LINE__);
    if ((((uintptr_t)rgba_dev | (uintptr_t)out_dev) & 3u) != 0) return fail(WL_E_ARG, "wl_scene_resolve: frame and output must be 4-byte aligned", __FILE__, __LINE__);
    WL_TRY(scene_size("wl_scene_resolve", W, H));
    if (ssaa != 1 && ssaa != 2 && ssaa != 4) return fail(WL_E_ARG, "wl_scene_resolve: bad ssaa (1, 2 or 4)", __FILE__, __LINE__);
    if (W % ssaa != 0 || H % ssaa != 0) return fail(WL_E_ARG, "wl_scene_resolve: W and H must be multiples of ssaa", __FILE__, __LINE__);
    const uint32_t bg = (uint32_t)background_rgba[0] | ((uint32_t)background_rgba[1] << 8) | ((uint32_t)background_rgba[2] << 16) |
                        ((uint32_t)background_rgba[3] << 24);
    return op_scene_resolve(rgba_dev, (const unsigned long long *)key_dev, W, H, ssaa, bg, out_dev);
}
int wl_scene_volume(wl_dtype t, const wl_grid *g, const void *f, const double Minv[16], double ds, const int32_t lo[3], const int32_t hi[3],
                    double vmin, double vmax, int levels, const uint8_t *lut_dev, const double *opac_dev, double t_min,
                    const uint64_t *key_dev, const uint8_t background_rgba[4], uint8_t *rgba_dev, double *acc_dev, int W, int H) {
    const char *who = "wl_scene_volume";
    if (!g || !f || !Minv || !lut_dev || !opac_dev || !key_dev || !background_rgba || !rgba_dev)
        WL_BAD(who, "null grid, field, inverse camera, colour table, opacity table, keys, background or frame");
    WL_TRY(check_grid(g));
    WL_TRY(check_dtype(who, t));
    if (g->D != 3) WL_BAD(who, "a volume needs D == 3");
    if (g->nzg > 0) return fail(WL_E_STATE, "wl_scene_volume: a z-slab decomposition has no distributed picture", __FILE__, __LINE__);
    const G gg = mkG(g);
    int l[3], h[3];
    WL_TRY(parse_box(who, gg, 3, 1, false, lo, hi, l, h));
    for (int d = 0; d < 3; ++d)
        if (h[d] - l[d] < 2) WL_BAD(who, "the box needs two cells or more in every direction (hi - lo >= 2)");
    VolumeArgs A;
    for (int k = 0; k < 16; ++k) {
        if (!std::isfinite(Minv[k])) WL_BAD(who, "the inverse camera matrix must be finite");
        A.mi[k] = Minv[k];
    }
    if (!(ds >= 1.0 / 1048576.0 && ds <= 1.0)) WL_BAD(who, "the step ds must lie in [2^-20, 1]");
    if (!(std::isfinite(vmin) && std::isfinite(vmax) && vmin < vmax)) WL_BAD(who, "need finite vmin < vmax");
    if (levels < 0 || levels > 256) WL_BAD(who, "levels must lie in 0..256");
    if (!(t_min >= 0.0 && t_min < 1.0)) WL_BAD(who, "t_min must lie in [0, 1)");
    WL_TRY(scene_size(who, W, H));
    if (((uintptr_t)rgba_dev & 3u) != 0 || ((uintptr_t)key_dev & 7u) != 0 || ((uintptr_t)acc_dev & 7u) != 0)
        WL_BAD(who, "the frame must be 4-byte aligned, the keys and acc_dev 8-byte aligned");
    A.ds = ds; A.vmin = vmin; A.vmax = vmax; A.t_min = t_min; A.W = W; A.H = H; A.levels = levels;
    for (int d = 0; d < 3; ++d) {
        A.blo[d] = (double)l[d] - 0.5;
        A.bhi[d] = (double)h[d] - 1.5;
    }
    A.bg = (uint32_t)background_rgba[0] | ((uint32_t)background_rgba[1] << 8) | ((uint32_t)background_rgba[2] << 16) |
           ((uint32_t)background_rgba[3] << 24);
    WL_DISPATCH_T(t, (op_scene_volume<T>(gg, A, (const T *)f, lut_dev, opac_dev, (const unsigned long long *)key_dev, rgba_dev, acc_dev)));
}
int wl_scene_average(const uint8_t *rgba_dev, int W, int H, int ssaa, uint8_t *out_dev) {
    const char *who = "wl_scene_average";
    if (!rgba_dev || !out_dev) WL_BAD(who, "null frame or output");
    if ((((uintptr_t)rgba_dev | (uintptr_t)out_dev) & 3u) != 0) WL_BAD(who, "frame and output must be 4-byte aligned");
    WL_TRY(scene_size(who, W, H));
    if (ssaa != 1 && ssaa != 2 && ssaa != 4) WL_BAD(who, "bad ssaa (1, 2 or 4)");
    if (W % ssaa != 0 || H % ssaa != 0) WL_BAD(who, "W and H must be multiples of ssaa");
    return op_scene_average(rgba_dev, W, H, ssaa, out_dev);
}
// the checks wl_downsample and wl_downsample_extent share: factor and box -> l, h (a box without cells is refused here)
static int downsample_box(const char *who, const wl_grid *g, const G &gg, int factor, const int32_t lo[3], const int32_t hi[3], int l[3], int h[3]) {
    if (factor != 1 && factor != 2 && factor != 4 && factor != 8 && factor != 16) WL_BAD(who, "bad factor (1, 2, 4, 8 or 16)");
    WL_TRY(parse_box(who, gg, g->D, 1, false, lo, hi, l, h));
    for (int d = 0; d < g->D; ++d)
        if ((h[d] - l[d]) % factor != 0) WL_BAD(who, "the extents hi - lo of the box must be multiples of factor");
    return 0;
}
int wl_downsample_extent(const wl_grid *g, int factor, const int32_t lo[3], const int32_t hi[3], int32_t nc[3], int32_t *k0) {
    if (!g || !nc || !k0) return fail(WL_E_ARG, "wl_downsample_extent: null grid, nc or k0", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    const G gg = mkG(g);
    int l[3], h[3], n[3], kk, klo;
    WL_TRY(downsample_box("wl_downsample_extent", g, gg, factor, lo, hi, l, h));
    if (!down_extent(gg, factor, l, h, n, &kk, &klo))
        return fail(WL_E_ARG, "wl_downsample_extent: a boundary of this rank's planes inside the box is not at lo_2 + m*factor", __FILE__, __LINE__);
    nc[0] = n[0]; nc[1] = n[1]; nc[2] = n[2];
    *k0 = kk;
    return 0;
}
int wl_downsample(wl_dtype t, const wl_grid *g, const void *f, int kind, int ipar, const double par[3], const double par2[3], int mode,
                  int factor, const int32_t lo[3], const int32_t hi[3], wl_dtype t_out, void *out_dev, int ntuple, int c) {
    if (!g || !f || !out_dev) return fail(WL_E_ARG, "wl_downsample: null grid, field or output", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    WL_TRY(check_dtype("wl_downsample", t, "unknown dtype t"));
    WL_TRY(check_dtype("wl_downsample", t_out, "unknown dtype t_out"));
    const int D = g->D;
    const bool metric = kind >= WL_R_METRIC;
    WL_TRY(check_kind("wl_downsample", kind, ipar, D, true));
    if (mode < WL_R_MAX || mode > WL_R_SAMPLE) return fail(WL_E_ARG, "wl_downsample: bad mode", __FILE__, __LINE__);
    if (ntuple < 1 || ntuple > 9) return fail(WL_E_ARG, "wl_downsample: bad ntuple (1 <= ntuple <= 9)", __FILE__, __LINE__);
    if (c < 0 || c >= ntuple) return fail(WL_E_ARG, "wl_downsample: bad c (0 <= c < ntuple)", __FILE__, __LINE__);
    const G gg = mkG(g);
    int l[3], h[3], nc[3], k0, klo;
    WL_TRY(downsample_box("wl_downsample", g, gg, factor, lo, hi, l, h));
    if (metric) WL_TRY(check_metric_box("wl_downsample", D, l));
    if (metric) WL_TRY(check_halo_planes("wl_downsample", gg, false));
    if (!down_extent(gg, factor, l, h, nc, &k0, &klo))
        return fail(WL_E_ARG, "wl_downsample: a boundary of this rank's planes inside the box is not at lo_2 + m*factor", __FILE__, __LINE__);
    l[2] = klo;
    WL_DISPATCH(t, D, (op_downsample<T, DD>(gg, (const T *)f, kind, ipar, par, par2, mode, factor, l, nc, t_out == WL_F64, out_dev, ntuple, c)));
}
// the checks of one axis of wl_histogram (bins != 0) or of wl_field_range's value (bins == 0)
static int hist_axis_args(const char *who, const wl_hist_axis *a, int D, bool bins) {
    WL_TRY(check_kind(who, a->kind, a->ipar, D, false));
    if (!bins) return 0;
    if (a->nbins < 1) WL_BAD(who, "nbins must be >= 1");
    if (a->range_dev && a->edges_dev) WL_BAD(who, "both range_dev and edges_dev given");
    if (a->edges_dev && a->nbins > HIST_MAXEDGES) WL_BAD(who, "edges take nbins <= 1024");
    if (!a->range_dev && !a->edges_dev && !(std::isfinite(a->lo) && std::isfinite(a->hi) && a->hi > a->lo))
        WL_BAD(who, "a host range needs finite lo < hi");
    return 0;
}
// the box of wl_histogram / wl_field_range -> l, h (a box without cells is refused), with a metric kind's two conditions
static int hist_box_args(const char *who, const G &gg, int D, bool metric, const int32_t lo[3], const int32_t hi[3], int l[3], int h[3]) {
    WL_TRY(parse_box(who, gg, D, 1, false, lo, hi, l, h));
    if (metric) WL_TRY(check_metric_box(who, D, l));
    if (metric) WL_TRY(check_halo_planes(who, gg, false));
    return 0;
}
int wl_histogram(wl_dtype t, const wl_grid *g, const wl_hist_axis *a, const wl_hist_axis *b, const int32_t lo[3], const int32_t hi[3],
                 int accumulate, int64_t *cnt_dev) {
    if (!g || !a || !cnt_dev) return fail(WL_E_ARG, "wl_histogram: null grid, axis or counts", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    WL_TRY(check_dtype("wl_histogram", t));
    if (!a->f || (b && !b->f)) return fail(WL_E_ARG, "wl_histogram: null field of an axis", __FILE__, __LINE__);
    const int D = g->D;
    WL_TRY(hist_axis_args("wl_histogram", a, D, true));
    if (b) WL_TRY(hist_axis_args("wl_histogram", b, D, true));
    if ((int64_t)(a->nbins + 2LL) * (b ? b->nbins + 2LL : 1LL) > HIST_MAXBINS)
        return fail(WL_E_ARG, "wl_histogram: more than 8192 bins ((a->nbins + 2) * (b->nbins + 2))", __FILE__, __LINE__);
    const G gg = mkG(g);
    int l[3], h[3];
    WL_TRY(hist_box_args("wl_histogram", gg, D, a->kind >= WL_R_METRIC || (b && b->kind >= WL_R_METRIC), lo, hi, l, h));
    WL_DISPATCH(t, D, (op_histogram<T, DD>(gg, a, b, l, h, accumulate, cnt_dev)));
}
int wl_field_range_scratch(const wl_grid *g, int64_t *bytes) {
    if (!g || !bytes) return fail(WL_E_ARG, "wl_field_range_scratch: null grid or bytes", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    *bytes = RANGE_SCRATCH;
    return 0;
}
int wl_field_range(wl_dtype t, const wl_grid *g, const void *f, int kind, int ipar, const double par[3], const double par2[3],
                   int absval, const int32_t lo[3], const int32_t hi[3], void *scratch_dev, int64_t scratch_bytes, double *out_dev) {
    if (!g || !f || !out_dev) return fail(WL_E_ARG, "wl_field_range: null grid, field or output", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    WL_TRY(check_dtype("wl_field_range", t));
    const int D = g->D;
    wl_hist_axis a{};
    a.f = f; a.kind = kind; a.ipar = ipar; a.absval = absval;
    for (int d = 0; d < D; ++d) { a.par[d] = par ? par[d] : 0.0; a.par2[d] = par2 ? par2[d] : 0.0; }
    WL_TRY(hist_axis_args("wl_field_range", &a, D, false));
    if (!scratch_dev || scratch_bytes < RANGE_SCRATCH)
        return fail(WL_E_ARG, "wl_field_range: no scratch, or fewer bytes than wl_field_range_scratch asks for", __FILE__, __LINE__);
    const G gg = mkG(g);
    int l[3], h[3];
    WL_TRY(hist_box_args("wl_field_range", gg, D, kind >= WL_R_METRIC, lo, hi, l, h));
    WL_DISPATCH(t, D, (op_field_range<T, DD>(gg, &a, l, h, scratch_dev, out_dev)));
}
// the checks wl_twopoint and wl_twopoint_scratch share: axis, box -> l, h, the line's length and nsep
static int twopoint_line_args(const char *who, const G &gg, int D, bool metric, int axis, int nsep, const int32_t lo[3], const int32_t hi[3], int l[3],
                              int h[3]) {
    if (axis < 0 || axis >= D) WL_BAD(who, "bad axis (0 <= axis < D)");
    WL_TRY(hist_box_args(who, gg, D, metric, lo, hi, l, h));
    const int n = h[axis] - l[axis];
    if (n > TP_MAX_LINE) WL_BAD(who, "the box is longer than WL_TP_MAX_LINE = 1024 cells along axis");
    if (nsep < 1 || nsep > n) WL_BAD(who, "bad nsep (1 <= nsep <= the box's extent along axis)");
    if (axis == 2 && gg.dist) WL_BAD(who, "axis 2 on a z-slab: the lines cross ranks");
    return 0;
}
int wl_twopoint_scratch(const wl_grid *g, int axis, int nsep, const int32_t lo[3], const int32_t hi[3], int64_t *bytes) {
    if (!g || !bytes) return fail(WL_E_ARG, "wl_twopoint_scratch: null grid or bytes", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    const G gg = mkG(g);
    int l[3], h[3];
    WL_TRY(twopoint_line_args("wl_twopoint_scratch", gg, g->D, false, axis, nsep, lo, hi, l, h));
    *bytes = tp_scratch_bytes(tp_box(gg, l, h, axis, nsep, 0));
    return 0;
}
int wl_twopoint(wl_dtype t, const wl_grid *g, const wl_tp_value *a, const wl_tp_value *b, int axis, int nsep, int periodic, const int32_t lo[3],
                const int32_t hi[3], int accumulate, void *scratch_dev, int64_t scratch_bytes, double *out_dev) {
    if (!g || !a || !out_dev) return fail(WL_E_ARG, "wl_twopoint: null grid, value or table", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    WL_TRY(check_dtype("wl_twopoint", t));
    if (!a->f || (b && !b->f)) return fail(WL_E_ARG, "wl_twopoint: null field of a value", __FILE__, __LINE__);
    const int D = g->D;
    WL_TRY(check_kind("wl_twopoint", a->kind, a->ipar, D, false));
    if (b) WL_TRY(check_kind("wl_twopoint", b->kind, b->ipar, D, false));
    const G gg = mkG(g);
    int l[3], h[3];
    WL_TRY(twopoint_line_args("wl_twopoint", gg, D, a->kind >= WL_R_METRIC || (b && b->kind >= WL_R_METRIC), axis, nsep, lo, hi, l, h));
    if (!scratch_dev || scratch_bytes < tp_scratch_bytes(tp_box(gg, l, h, axis, nsep, periodic)))
        return fail(WL_E_ARG, "wl_twopoint: no scratch, or fewer bytes than wl_twopoint_scratch asks for", __FILE__, __LINE__);
    WL_DISPATCH(t, D, (op_twopoint<T, DD>(gg, a, b, axis, nsep, periodic, l, h, accumulate, scratch_dev, out_dev)));
}
// the checks wl_regions and wl_regions_scratch share: one rank, box -> l, h, fewer than 2^31 cells
static int regions_box_args(const char *who, const G &gg, int D, bool metric, const int32_t lo[3], const int32_t hi[3], int l[3], int h[3]) {
    if (gg.dist) WL_BAD(who, "a decomposed flow (z-slabs): regions cross ranks");
    WL_TRY(hist_box_args(who, gg, D, metric, lo, hi, l, h));
    if ((int64_t)(h[0] - l[0]) * (h[1] - l[1]) * (h[2] - l[2]) >= (int64_t)1 << 31) WL_BAD(who, "the box holds 2^31 cells or more");
    return 0;
}
int wl_regions_scratch(const wl_grid *g, const int32_t lo[3], const int32_t hi[3], int64_t *bytes) {
    if (!g || !bytes) return fail(WL_E_ARG, "wl_regions_scratch: null grid or bytes", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    const G gg = mkG(g);
    int l[3], h[3];
    WL_TRY(regions_box_args("wl_regions_scratch", gg, g->D, false, lo, hi, l, h));
    *bytes = rg_scratch_bytes((long)(h[1] - l[1]) * (h[2] - l[2]));
    return 0;
}
int wl_regions(wl_dtype t, const wl_grid *g, const wl_rg_value *v, int cmp, double c, int periodic_mask, const int32_t lo[3],
               const int32_t hi[3], int32_t *label_dev, int64_t cap, int64_t *tab_dev, double *ext_dev, int64_t *n_dev, void *scratch_dev,
               int64_t scratch_bytes) {
    if (!g || !v || !label_dev || !n_dev || !scratch_dev) return fail(WL_E_ARG, "wl_regions: null grid, value, labels, counts or scratch", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    WL_TRY(check_dtype("wl_regions", t));
    if (!v->f) return fail(WL_E_ARG, "wl_regions: null field of the value", __FILE__, __LINE__);
    const int D = g->D;
    WL_TRY(check_kind("wl_regions", v->kind, v->ipar, D, false));
    if (cmp != WL_RG_BELOW && cmp != WL_RG_ABOVE) return fail(WL_E_ARG, "wl_regions: bad cmp (WL_RG_BELOW or WL_RG_ABOVE)", __FILE__, __LINE__);
    if (std::isnan(c)) return fail(WL_E_ARG, "wl_regions: the level c must not be NaN", __FILE__, __LINE__);
    if (periodic_mask < 0 || periodic_mask >= (1 << D)) return fail(WL_E_ARG, "wl_regions: bad periodic_mask (bits 0 .. D - 1)", __FILE__, __LINE__);
    if (cap < 0) return fail(WL_E_ARG, "wl_regions: negative capacity", __FILE__, __LINE__);
    if (cap > 0 && (!tab_dev || !ext_dev)) return fail(WL_E_ARG, "wl_regions: null table or extremes with cap > 0", __FILE__, __LINE__);
    if (cap > ((int64_t)1 << 31)) cap = (int64_t)1 << 31;      // (there are fewer regions than cells)
    if (((uintptr_t)scratch_dev & 7u) || ((uintptr_t)n_dev & 7u) || ((uintptr_t)tab_dev & 7u) || ((uintptr_t)ext_dev & 7u) || ((uintptr_t)label_dev & 3u))
        return fail(WL_E_ARG, "wl_regions: a buffer is not aligned to its element", __FILE__, __LINE__);
    const G gg = mkG(g);
    int l[3], h[3];
    WL_TRY(regions_box_args("wl_regions", gg, D, v->kind >= WL_R_METRIC, lo, hi, l, h));
    if (scratch_bytes < rg_scratch_bytes((long)(h[1] - l[1]) * (h[2] - l[2])))
        return fail(WL_E_ARG, "wl_regions: fewer bytes of scratch than wl_regions_scratch asks for", __FILE__, __LINE__);
    WL_DISPATCH(t, D, (op_regions<T, DD>(gg, v, cmp, c, periodic_mask, l, h, label_dev, cap, tab_dev, ext_dev, n_dev, scratch_dev)));
}
int wl_region_sums(wl_dtype t, const wl_grid *g, const int32_t lo[3], const int32_t hi[3], const int32_t *label_dev, const int64_t *n_dev,
                   int64_t cap, int ncol, const wl_rs_col *cols, int scale_mode, int32_t *scale_dev, int64_t *acc_dev, double *sum_dev,
                   int64_t *over_dev) {
    if (!g || !label_dev || !n_dev || !cols || !scale_dev || !acc_dev || !sum_dev || !over_dev)
        return fail(WL_E_ARG, "wl_region_sums: null grid, labels, counts, columns, scale, limbs, sums or overflow counts", __FILE__, __LINE__);
    WL_TRY(check_grid(g));
    WL_TRY(check_dtype("wl_region_sums", t));
    if (scale_mode != WL_RS_FIND && scale_mode != WL_RS_GIVEN) return fail(WL_E_ARG, "wl_region_sums: bad scale_mode (WL_RS_FIND or WL_RS_GIVEN)", __FILE__, __LINE__);
    if (ncol < 1 || ncol > WL_RS_MAX_COLS) return fail(WL_E_ARG, "wl_region_sums: bad ncol (1 .. WL_RS_MAX_COLS = 8)", __FILE__, __LINE__);
    if (cap < 1) return fail(WL_E_ARG, "wl_region_sums: the capacity must be >= 1", __FILE__, __LINE__);
    if (cap > ((int64_t)1 << 31)) cap = (int64_t)1 << 31;      // (there are fewer regions than cells)
    const int D = g->D;
    bool metric = false;
    for (int c = 0; c < ncol; ++c) {
        if (!cols[c].v.f) return fail(WL_E_ARG, "wl_region_sums: null field of a column's value", __FILE__, __LINE__);
        WL_TRY(check_kind("wl_region_sums", cols[c].v.kind, cols[c].v.ipar, D, false));
        if (cols[c].power != 1 && cols[c].power != 2) return fail(WL_E_ARG, "wl_region_sums: bad power (1 or 2)", __FILE__, __LINE__);
        if (cols[c].moment < -1 || cols[c].moment >= D) return fail(WL_E_ARG, "wl_region_sums: bad moment (-1 or an axis 0 .. D - 1)", __FILE__, __LINE__);
        metric = metric || cols[c].v.kind >= WL_R_METRIC;
    }
    if (((uintptr_t)label_dev & 3u) || ((uintptr_t)scale_dev & 3u) || ((uintptr_t)n_dev & 7u) || ((uintptr_t)acc_dev & 7u) || ((uintptr_t)sum_dev & 7u) ||
        ((uintptr_t)over_dev & 7u))
        return fail(WL_E_ARG, "wl_region_sums: a buffer is not aligned to its element", __FILE__, __LINE__);
    const G gg = mkG(g);
    int l[3], h[3];
    WL_TRY(regions_box_args("wl_region_sums", gg, D, metric, lo, hi, l, h));
    WL_DISPATCH(t, D, (op_region_sums<T, DD>(gg, l, h, label_dev, n_dev, cap, ncol, cols, scale_mode, scale_dev, acc_dev, sum_dev, over_dev)));
}
int wl_tracer_advance(wl_dtype t, const wl_grid *g, const void *u, double *x_dev, int64_t m, double dt, int perdir_mask) {
    WL_TRY(check_grid(g));
    WL_TRY(check_dtype("wl_tracer_advance", t));
    if (!u || !x_dev) return fail(WL_E_ARG, "wl_tracer_advance: null velocity or positions", __FILE__, __LINE__);
    if (m < 0) return fail(WL_E_ARG, "wl_tracer_advance: negative number of particles", __FILE__, __LINE__);
    if (!(std::isfinite(dt) && dt >= 0.0)) return fail(WL_E_ARG, "wl_tracer_advance: dt must be finite and >= 0", __FILE__, __LINE__);
    if (perdir_mask < 0 || perdir_mask >= (1 << g->D)) return fail(WL_E_ARG, "wl_tracer_advance: bad perdir_mask", __FILE__, __LINE__);
    if (g->D == 3 && g->nzg > 0)
        return fail(WL_E_STATE, "wl_tracer_advance: tracers on a z-slab decomposition are not supported", __FILE__, __LINE__);
    const G gg = mkG(g);
    WL_DISPATCH(t, g->D, (op_tracer_advance<T, DD>(gg, (const T *)u, x_dev, m, dt, perdir_mask)));
}
int wl_pforce(wl_dtype t, const wl_grid *g, const void *p, const int64_t *idx, const double *nds, int64_t nband,
              double out[3]) {
    WL_GS_OUT();
    (void)gg;
    out[0] = out[1] = out[2] = 0;
    int nb = (int)((nband + 255) / 256);
    if (nb > 1024) nb = 1024;
    if (nband <= 0) nb = 0;   // a rank whose slab holds no part of the body still joins the all-reduce
    if (nb > 0) {
        Prof pr(WL_K_PFORCE, nband);
        if (t == WL_F32) hipLaunchKernelGGL(k_pforce<float>, dim3(nb), dim3(256), 0, ctx().stream, (const float *)p, idx, nds, nband, g->D, S.partials.get());
        else hipLaunchKernelGGL(k_pforce<double>, dim3(nb), dim3(256), 0, ctx().stream, (const double *)p, idx, nds, nband, g->D, S.partials.get());
        WL_HIP(hipGetLastError());
    }
    State *st = S.st.get();
    WL_TRY((launch_finalize<3>(gg.dist, S.partials.get(), nb, RED_SUM, 0.0, st->red, [=] __device__(const double *v) {
        st->out[0] = v[0]; st->out[1] = v[1]; st->out[2] = v[2]; })));
    WL_TRY(S.fetch());
    for (int c = 0; c < g->D; ++c) out[c] = S.hst.get()->out[c];
    return 0;
}

static int snapshot_args(const wl_grid *g, const void *a, int ncomp, int nct, int klo, int khi, const void *buf) {
    WL_TRY(check_grid(g));
    if (!a || !buf) return fail(WL_E_ARG, "wl_snapshot: null buffer", __FILE__, __LINE__);
    if (ncomp < 1 || nct < ncomp || nct > 9) return fail(WL_E_ARG, "wl_snapshot: need 1 <= ncomp <= ntuple <= 9", __FILE__, __LINE__);
    const int n2 = g->D == 3 ? g->n[2] : 1;
    if (klo < 0 || khi >= n2 || klo > khi) return fail(WL_E_ARG, "wl_snapshot: plane range outside the local array", __FILE__, __LINE__);
    return 0;
}
int wl_snapshot_pack(wl_dtype t, const wl_grid *g, const void *a, int ncomp, int ntuple, int klo, int khi, void *dst) {
    WL_TRY(check_dtype("wl_snapshot_pack", t));
    WL_TRY(snapshot_args(g, a, ncomp, ntuple, klo, khi, dst));
    const G gg = mkG(g);
    WL_DISPATCH_T(t, (snapshot_copy<T>(gg, (T *)const_cast<void *>(a), ncomp, ntuple, klo, khi, (T *)dst, true)));
}
int wl_snapshot_unpack(wl_dtype t, const wl_grid *g, void *a, int ncomp, int ntuple, int klo, int khi, const void *src) {
    WL_TRY(check_dtype("wl_snapshot_unpack", t));
    WL_TRY(snapshot_args(g, a, ncomp, ntuple, klo, khi, src));
    const G gg = mkG(g);
    WL_DISPATCH_T(t, (snapshot_copy<T>(gg, (T *)a, ncomp, ntuple, klo, khi, (T *)const_cast<void *>(src), false)));
}

int wl_set_option(int key, int value) {
    if (key < 0 || key >= 32 || !((WL_OPT_LIVE >> key) & 1u)) return fail(WL_E_ARG, "wl_set_option: no such option", __FILE__, __LINE__);
    ctx().opt.v[key] = value;
    return 0;
}
int wl_get_option(int key, int *value) {
    if (!value || key < 0 || key >= 32 || !((WL_OPT_LIVE >> key) & 1u)) return fail(WL_E_ARG, "wl_get_option: no such option", __FILE__, __LINE__);
    *value = opt(key);
    return 0;
}

// ---- measurement support
static const char *KNAMES[WL_K_COUNT] = {
    "conv_diff", "bdim", "bc", "div", "correct", "cfl", "scale", "residual", "jacobi", "increment", "smooth",
    "restrict", "prolongate", "pcg_init", "pcg_mult_dot", "pcg_update", "pcg_direction", "dot", "scalar", "set_diag",
    "restrictL", "copy", "pforce", "misc"};
const char *wl_kernel_name(int k) { return (k >= 0 && k < WL_K_COUNT) ? KNAMES[k] : "?"; }
int wl_prof_select(int kclass, int64_t min_cells) {
    ctx().prof_class = kclass;
    ctx().prof_min_cells = min_cells;
    return 0;
}
int wl_prof_reset(void) {
    Ctx &c = ctx();
    for (int k = 0; k < WL_K_COUNT; ++k) { c.launches[k] = 0; c.cells[k] = 0; }
    for (auto &e : c.evts) { c.pool.push_back(e.a); c.pool.push_back(e.b); }
    c.evts.clear();
    if (c.comm) for (int q = 0; q < 6; ++q) c.comm->cnt[q] = 0;
    return 0;
}
// back-to-back all-reduces of one double on the library's stream, as the solver issues them (local reduction of a few
// partials + exchange), timed with two events: microseconds per all-reduce.  Every rank calls it with the same `reps`.
int wl_prof_allreduce_us(int reps, double *us_per_op) {
    Comm *cm = ctx().comm;
    if (!us_per_op || reps < 1) return fail(WL_E_ARG, "wl_prof_allreduce_us: bad arguments", __FILE__, __LINE__);
    *us_per_op = 0.0;
    if (!cm || cm->size == 1) return 0;
    int rc = 0;
    Scratch &S = global_scratch(&rc);
    WL_TRY(rc);
    WL_HIP(hipMemsetAsync(S.partials.get(), 0, sizeof(double) * 64, ctx().stream));
    hipEvent_t a, b;
    WL_HIP(hipEventCreate(&a));
    WL_HIP(hipEventCreate(&b));
    for (int w = 0; w < 3 && !rc; ++w) rc = reduce_allreduce<1>(S.partials.get(), 64, RED_SUM, 0.0, S.st.get()->red);   // warm-up
    if (!rc) rc = (int)hipEventRecord(a, ctx().stream);
    for (int q = 0; q < reps && !rc; ++q) rc = reduce_allreduce<1>(S.partials.get(), 64, RED_SUM, 0.0, S.st.get()->red);
    if (!rc) rc = (int)hipEventRecord(b, ctx().stream);
    if (!rc) rc = (int)hipEventSynchronize(b);
    float ms = 0;
    if (!rc) rc = (int)hipEventElapsedTime(&ms, a, b);
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    if (rc) return rc < 10000 ? fail(rc, "wl_prof_allreduce_us", __FILE__, __LINE__) : rc;
    if (ctx().mbox && *ctx().mbox->err_host.get()) return fail(WL_E_STATE, "mailbox all-reduce: gave up waiting for a peer rank", __FILE__, __LINE__);
    *us_per_op = (double)ms * 1e3 / reps;
    return 0;
}
int wl_prof_reset_comm(void) {
    if (ctx().comm) for (int q = 0; q < 6; ++q) ctx().comm->cnt[q] = 0;
    return 0;
}
int wl_prof_comm(int64_t out[6]) {
    if (!out) return fail(WL_E_ARG, "wl_prof_comm: null output", __FILE__, __LINE__);
    for (int q = 0; q < 6; ++q) out[q] = ctx().comm ? ctx().comm->cnt[q] : 0;
    return 0;
}
int wl_prof_allocs(int64_t *count, int64_t *bytes) {
    if (!count || !bytes) return fail(WL_E_ARG, "wl_prof_allocs: null output", __FILE__, __LINE__);
    *count = ctx().n_alloc;
    *bytes = ctx().alloc_bytes;
    return 0;
}
int wl_prof_counts(int kclass, int64_t *launches, int64_t *cells) {
    if (kclass < 0 || kclass >= WL_K_COUNT) return fail(WL_E_ARG, "bad kernel class", __FILE__, __LINE__);
    *launches = ctx().launches[kclass];
    *cells = ctx().cells[kclass];
    return 0;
}
int wl_prof_overlapped(int64_t *count) {
    if (!count) return fail(WL_E_ARG, "wl_prof_overlapped: null output", __FILE__, __LINE__);
    *count = ctx().n_overlapped;
    return 0;
}
int wl_prof_dealt(int64_t *count) {
    if (!count) return fail(WL_E_ARG, "wl_prof_dealt: null output", __FILE__, __LINE__);
    *count = ctx().n_dealt;
    return 0;
}
int wl_prof_timed(int64_t *launches, int64_t *cells, double *ms) {
    Ctx &c = ctx();
    WL_HIP(hipStreamSynchronize(c.stream));
    int64_t n = 0, nc = 0;
    double tot = 0;
    for (auto &e : c.evts) {
        float t = 0;
        WL_HIP(hipEventElapsedTime(&t, e.a, e.b));
        tot += t; ++n; nc += e.cells;
    }
    *launches = n; *cells = nc; *ms = tot;
    return 0;
}

}  // extern "C"
