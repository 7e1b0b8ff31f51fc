/* wlhip.h -- C ABI of libwlhip.so, the MI355X-native backend for WaterLily's `sim_step!` hot path.
 *
 * This header is the drop-in boundary.  Every entry point replaces one method of the reference
 * (/root/reference, file:line cited per function) that a `mem=<device array>` backend overrides at
 * function granularity (precedent: ext/WaterLilyAMDGPUExt.jl:24).
 * The reference-side binding (a Julia package extension made of `ccall`s) is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers, sizes, doubles; no C++/torch types; every function returns
 *     0 on success or a non-zero code (hipError_t, or WL_E_* below); wl_last_error() gives the text.
 *   - arrays follow the reference layout (src/Flow.jl:112-118): column-major, ONE ghost layer per side,
 *     vector fields as separate component blocks (SoA).  Strides are explicit (wl_grid), so both the dense
 *     Julia layout (s = {1, n0, n0*n1}, sc = n0*n1*n2) and a padded/aligned allocation are accepted.
 *   - directions/components are 0-based; `perdir_mask` bit j set = direction j periodic
 *     (reference: 1-based tuple `perdir`).
 *   - scalars cross the ABI as double and are rounded to the field type T where the reference holds a T.
 *   - all work is enqueued on one HIP stream (wl_set_stream; default: the null stream).  Functions that
 *     return a scalar synchronise that stream; all others are asynchronous.
 *   - the caller owns every field array; handles own only internal scratch (reduction partials, solver
 *     scalars).  Aliasing required by the reference is honoured: pois.x === flow.p, pois.L === flow.mu0,
 *     pois.z === flow.sigma (src/WaterLily.jl:77) -- pass the same pointers.
 */
#ifndef WLHIP_H
#define WLHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define WL_ABI_VERSION 6

/* Any other value is refused with WL_E_ARG by every entry point that takes a wl_dtype, and by wl_flow_create / wl_mg_create
 * before anything is allocated. */
typedef enum wl_dtype { WL_F32 = 0, WL_F64 = 1 } wl_dtype;

enum { WL_OK = 0, WL_E_ARG = 10001, WL_E_LEVELS = 10002, WL_E_NOGPU = 10003, WL_E_STATE = 10004 };

/* One grid (= one multigrid level).  n[] INCLUDES the ghost layer (src/Flow.jl:112 `Ng = N .+ 2`). */
typedef struct wl_grid {
    int32_t D;     /* 2 or 3 */
    int32_t n[3];  /* LOCAL extents incl. ghost/halo planes; n[2] = 1 when D == 2 */
    int64_t s[3];  /* element strides; s[0] must be 1 */
    int64_t sc;    /* element stride between the components of a vector field on this grid */
    /* z-slab decomposition (multi-GPU, D == 3).  nzg == 0 means "not decomposed" (the other three are ignored).
     * nzg  : extent along z of the UNDECOMPOSED array, ghosts included (the reference's N[3]+2);
     * kz0  : global z index of local plane 0 (may be negative: unused padding plane below the domain);
     * own_lo, own_hi : LOCAL plane range this rank owns (writes); planes outside are halo copies of a
     *        neighbour's owned planes (filled by wl_halo_exchange) or unused padding. */
    int32_t nzg, kz0, own_lo, own_hi;
    /* zring != 0: z is periodic ACROSS the slabs -- the ranks form a ring, the two z ghost planes are owned by nobody
     * and are filled, like every halo plane, by the neighbour exchange (rank 0 <-> rank P-1 included). */
    int32_t zring;
} wl_grid;

/* ------------------------------------------------------------------ runtime */
int wl_abi_version(void);
const char *wl_last_error(void);
int wl_device_count(int *n);
int wl_set_device(int dev);
int wl_set_stream(void *hip_stream); /* hipStream_t; NULL = null stream */
int wl_sync(void);
/* device memory for hosts without their own allocator (the Julia shim); torch hosts pass data_ptr() */
int wl_malloc(void **p, size_t bytes);
int wl_free(void *p);
int wl_h2d(void *dst, const void *src, size_t bytes);
int wl_d2h(void *dst, const void *src, size_t bytes);
int wl_memset0(void *p, size_t bytes);
/* the same copies between a dense host array and a PITCHED device array (rows of `width` bytes, `height` of them: every x-row of
 * every plane and component): how a host keeps the reference's dense arrays on its side (`Array(a)`, `copyto!`) while the
 * device rows sit on 128-byte boundaries -- the layout the kernels are 5 % faster on */
int wl_h2d_2d(void *dst_dev, size_t dpitch, const void *src_host, size_t spitch, size_t width, size_t height);
int wl_d2h_2d(void *dst_host, size_t dpitch, const void *src_dev, size_t spitch, size_t width, size_t height);

/* ------------------------------------------------------------------ multi-GPU communicator (one per process)
 * z-slab decomposition, one process per GPU.  Production: RCCL over xGMI -- rank 0 calls
 * wl_comm_unique_id, the host broadcasts the 128 bytes (torch.distributed / MPI / files), every rank calls
 * wl_comm_init_rccl.  Testing: wl_comm_init_host routes every collective through host callbacks (device
 * buffers are staged through pinned memory), so any transport (torch.distributed gloo) can carry it. */
int wl_comm_unique_id(void *out128);
int wl_comm_init_rccl(const void *id128, int rank, int nranks);
/* sendrecv: exchange `bytes` with both z-neighbours (host pointers; NULL where there is no neighbour).
 * allreduce: in-place on n doubles, op 0 = sum, 1 = max.  allgather: every rank contributes `bytes` at
 * offset rank*bytes of `buf`. */
typedef int (*wl_host_sendrecv_fn)(void *user, const void *send_lo, void *recv_lo, const void *send_hi, void *recv_hi,
                                   int64_t bytes, int peer_lo, int peer_hi);
typedef int (*wl_host_allreduce_fn)(void *user, double *vals, int n, int op);
typedef int (*wl_host_allgather_fn)(void *user, void *buf, int64_t bytes);
int wl_comm_init_host(int rank, int nranks, wl_host_sendrecv_fn sr, wl_host_allreduce_fn ar, wl_host_allgather_fn ag,
                      void *user);
/* Measurement: ONE process plays rank `rank` of an `nranks`-way z-slab run on one GPU.  Its neighbours are taken to be copies of
 * itself (the planes it would send up arrive from below and vice versa, as device copies), a sum over the ranks is nranks times
 * the local value, an all-gather repeats the local segment: the compute and launch time of a rank, without a wire. */
int wl_comm_init_loopback(int rank, int nranks);
/* Mailbox all-reduce for the run's scalars (dot products, CFL maximum, force sums): after the communicator exists every rank
 * of the NODE opens the same POSIX shared-memory object `shm_name` ("/name"); the one rank that passes create != 0 must
 * have returned before the others call (the host orders it: create on rank 0, barrier, open elsewhere, barrier, then rank 0
 * may shm_unlink the name).  From then on the library sums its scalars through that block of pinned host memory -- one
 * system-scope store + one poll per peer, combined in rank order (bit-identical on every rank) -- instead of one RCCL
 * all-reduce per value; halo planes and the coarse-level all-gather stay on RCCL.  Waits are bounded in wall-clock time
 * (WL_OPT_MBOX_TIMEOUT_S, seconds; 0 = unbounded): a rank that gives up reports WL_E_STATE at the caller's next synchronising
 * call.  Optional: without it scalars use ncclAllReduce. */
int wl_comm_mailbox(const char *shm_name, int create);
int wl_comm_mailbox_off(void);          /* back to the communicator's all-reduce (every rank must call it at the same point) */
int wl_comm_mailbox_active(int *on);
int wl_comm_finalize(void);
int wl_comm_rank(int *rank, int *nranks);
/* fill the halo planes of a (vector) field from the z-neighbours: `depth` planes each side, `ncomp` components */
int wl_halo_exchange(wl_dtype t, const wl_grid *g, void *a, int ncomp, int depth);
/* all-reduce n host doubles over the ranks (op 0 = sum, 1 = max); identity when there is no communicator */
int wl_allreduce(double *vals_host, int n, int op);

/* ------------------------------------------------------------------ util.jl operators */
/* BC!(a,A,saveexit,perdir)            src/util.jl:192-210 */
int wl_bc_vec(wl_dtype t, const wl_grid *g, void *a, const double A[3], int saveexit, int perdir_mask);
/* perBC!(a,perdir)                    src/util.jl:227-231 */
int wl_bc_per(wl_dtype t, const wl_grid *g, void *a, int perdir_mask);
/* exitBC!(u,u0,U,dt)                  src/util.jl:216-222 */
int wl_exit_bc(wl_dtype t, const wl_grid *g, void *u, const void *u0, const double U[3], double dt);
/* L2(a) = sum(abs2, inside(a))        src/util.jl:68 (ext/WaterLilyAMDGPUExt.jl:24) */
int wl_L2_inside(wl_dtype t, const wl_grid *g, const void *a, double *out);
/* dot / sum / maximum over the WHOLE array, ghost cells included: LinearAlgebra.dot, Base.sum, Base.maximum as used at
 * src/Poisson.jl:94,126,131,137,146 and src/Flow.jl:174 (z-slab runs: over the planes the ranks own, all-reduced) */
int wl_dot(wl_dtype t, const wl_grid *g, const void *a, const void *b, double *out);
int wl_sum(wl_dtype t, const wl_grid *g, const void *a, double *out);
int wl_max(wl_dtype t, const wl_grid *g, const void *a, double *out);

/* ------------------------------------------------------------------ Flow.jl operators */
/* conv_diff!(r,u,Phi;nu,perdir)       src/Flow.jl:36-60.  The kernels are in gather form and need no scratch; what the
 * reference's scatter form LEAVES in Phi where a later whole-array reduction reads it -- the top ghost cells (its loops run
 * over inside_u, util.jl:55-57: "top ghost included"; Phi is flow.sigma inside mom_step!, src/Flow.jl:157,164) -- is written
 * to Phi when Phi != NULL: each such cell gets the flux of the last (i,j) loop pair whose range holds it.  Interior cells of
 * Phi (scratch the reference overwrites before reading) are not touched. */
int wl_conv_diff(wl_dtype t, const wl_grid *g, void *r, const void *u, void *Phi, double nu, int perdir_mask);
/* accelerate!(r,dt,g,U)               src/Flow.jl:68-73  (host evaluates g(i,t)+dU_i/dt) */
int wl_accelerate(wl_dtype t, const wl_grid *g, void *r, const double acc[3]);
/* BDIM!(a)                            src/Flow.jl:131-135 */
int wl_bdim(wl_dtype t, const wl_grid *g, void *u, const void *u0, void *f, const void *V, const void *mu0,
            const void *mu1, double dt);
/* scale_u!(a,scale)                   src/Flow.jl:170 */
int wl_scale_u(wl_dtype t, const wl_grid *g, void *u, double scale);
/* @inside z[I] = div(I,u)             src/Flow.jl:139 (div: :11-17) */
int wl_div(wl_dtype t, const wl_grid *g, void *z, const void *u);
/* CFL(a)                              src/Flow.jl:172-182 */
int wl_cfl(wl_dtype t, const wl_grid *g, void *sigma, const void *u, double nu, double *dt_out);

/* ------------------------------------------------------------------ Poisson.jl / MultiLevelPoisson.jl */
/* set_diag!(D,iD,L)                   src/Poisson.jl:42-54 */
int wl_set_diag(wl_dtype t, const wl_grid *g, void *D, void *iD, const void *L);
/* restrictL!(a,b;perdir)              src/MultiLevelPoisson.jl:26-32 */
int wl_restrictL(wl_dtype t, const wl_grid *ga, void *a, const wl_grid *gb, const void *b, int perdir_mask);
/* restrict!(a,b), prolongate!(a,b)    src/MultiLevelPoisson.jl:33-34 */
int wl_restrict(wl_dtype t, const wl_grid *ga, void *a, const wl_grid *gb, const void *b);
int wl_prolongate(wl_dtype t, const wl_grid *ga, void *a, const wl_grid *gb, const void *b);

/* One level of the hierarchy = the fields of `Poisson` (src/Poisson.jl:21-30); caller-owned arrays. */
typedef struct wl_level_desc {
    wl_grid g;
    void *L, *D, *iD, *x, *eps, *r, *z;
} wl_level_desc;

typedef struct wl_mg wl_mg; /* opaque: Poisson (nlevels==1) or MultiLevelPoisson */

/* Poisson(x,L,z) src/Poisson.jl:31-37 / MultiLevelPoisson(x,L,z) src/MultiLevelPoisson.jl:51-59.
 * The host builds the level shapes (`restrictML`, :18-25) and allocates; create() validates them, fills
 * the coarse L by restrictL! and D,iD by set_diag!.  nlevels==2 is rejected with WL_E_LEVELS
 * ("MultiLevelPoisson requires size=a2^n, where n>2"). */
int wl_mg_create(wl_mg **out, wl_dtype t, int nlevels, const wl_level_desc *levels, int perdir_mask);
int wl_mg_destroy(wl_mg *m);
/* update!(ml)                         src/MultiLevelPoisson.jl:62-68 (src/Poisson.jl:46 for one level) */
int wl_mg_update(wl_mg *m);
/* Introspection: how many interior x-rows of `level` carry one coefficient value on all their faces (the 7-point kernels
 * skip the loads of L there, see WL_OPT_ROW_CONST_L) out of how many owned interior rows.  0 for D==2. */
int wl_mg_uniform_rows(wl_mg *m, int level, long long *n_uniform, long long *n_rows);
/* mult!(p,x): p.z = A x               src/Poisson.jl:62-68 */
int wl_mg_mult(wl_mg *m, int level, void *x);
/* residual!(p)                        src/Poisson.jl:91-97 */
int wl_mg_residual(wl_mg *m, int level);
/* increment!(p)                       src/Poisson.jl:99-103 */
int wl_mg_increment(wl_mg *m, int level);
/* Jacobi!(p;it)                       src/Poisson.jl:110-113 */
int wl_mg_jacobi(wl_mg *m, int level, int it);
/* pcg!(p;it)                          src/Poisson.jl:123-143; n_updates = number of (x,r) updates done */
int wl_mg_pcg(wl_mg *m, int level, int it, int *n_updates);
/* L2(p) = r.r                         src/Poisson.jl:146 */
int wl_mg_L2(wl_mg *m, int level, double *out);
/* L∞(p) = maximum(abs, p.r)            src/Poisson.jl:147 (over inside(r): its ghost entries are zero) */
int wl_mg_Linf(wl_mg *m, int level, double *out);
/* Vcycle!(ml;l)                       src/MultiLevelPoisson.jl:70-82 */
int wl_mg_vcycle(wl_mg *m, int level);
/* solver!(p;tol,itmx)                 src/MultiLevelPoisson.jl:87-99 (src/Poisson.jl:162-172 for one
 * level).  n_iter receives the value the reference pushes onto `p.n`. */
int wl_mg_solve(wl_mg *m, double tol, int itmx, int *n_iter);
/* The pressure-solver log of the reference (`@log ", $n, $(L∞(p)), $r₂\n"`, src/Poisson.jl:164,167,
 * src/MultiLevelPoisson.jl:90,94; macro and file format: src/util.jl:4-24).  wl_mg_log(m, 1) makes every later
 * wl_mg_solve / wl_project / wl_mom_step on this hierarchy record one row {n, L∞(p), L₂(p)} for the initial residual
 * (n = 0) and for each iteration -- two extra reductions and a host synchronisation per row, so it is off by default.
 * wl_mg_log_read copies up to `cap` rows (3 doubles each, oldest first) into `rows` and removes
 * them from the record; *n receives the number of rows that were waiting (rows beyond cap stay for the next read; cap = 0 is a
 * query that consumes nothing).  The host prints the "p" / "c"
 * prefixes of src/Flow.jl:158,165 itself. */
int wl_mg_log(wl_mg *m, int on);
int wl_mg_log_read(wl_mg *m, double *rows, int cap, int *n);

/* ------------------------------------------------------------------ Flow (src/Flow.jl:92-122) */
typedef struct wl_flow_desc {
    wl_grid g;
    void *u, *u0, *f, *p, *sigma, *V, *mu0, *mu1; /* mu1[I,i,j] = component i + D*j */
    double nu;
    int32_t exitBC;
    int32_t perdir_mask;
} wl_flow_desc;

typedef struct wl_flow wl_flow; /* opaque */

int wl_flow_create(wl_flow **out, wl_dtype t, const wl_flow_desc *desc);
int wl_flow_destroy(wl_flow *a);
/* Must be called after the coefficient fields mu0, mu1, V were (re)written -- i.e. at the end of measure!(flow,body)
 * (src/Body.jl:31-53), next to update!(pois).  It rebuilds the per-row "body-free" flags (mu1 == 0, V == 0,
 * mu0 == 1 on a whole x-row) that let BDIM! skip those 15 coefficient reads where they are known constants; results
 * are identical with or without the flags.  Until the first call every row takes the general path. */
int wl_flow_update(wl_flow *a);
/* update!(pois) after a native measure! (wl_measure_fill) of the flow whose mu0 is this hierarchy's L: on level 0 only the
 * x-rows that measure! rewrote (and their lower y / z neighbours, whose diagonal reads them) get D, iD and row constants
 * recomputed -- every other row holds the same values already; levels >= 1 are rebuilt in full.  Same results as
 * wl_mg_update (to which it falls back when the flow's last change was not a native measure!, or in 2-D).
 * Periodic y / z: the last interior row also follows the first one (its upper ghost row is that row's periodic copy); a
 * z-periodic ring of slabs takes the full update.  Consumes the flow's changed-row record: flags of several
 * wl_measure_fill calls accumulate until this call has used them -- so ONE hierarchy per flow may be updated this way (the
 * reference builds exactly one, src/WaterLily.jl:77); a second hierarchy on the same mu0 must take wl_mg_update. */
int wl_mg_update_changed(wl_mg *m, wl_flow *a);
/* measure!(flow, body; t, eps)        src/Body.jl:31-53 for a PARAMETRIC body: an sdf family with closed-form gradient
 * (what ForwardDiff.gradient returns, src/AutoBody.jl:119) composed with an affine map xi = A x + b evaluated by the
 * host at the measured time together with its time derivative and inverse (AutoBody.jl:128-130: V = -J \ d(map)/dt).
 * Bodies defined by arbitrary closures stay on the host side of the ABI (waterlily_amd.body: torch).
 *   family WL_BODY_SPHERE: p = {c0, c1, c2, radius}  sdf = sqrt(sum(abs2, xi - c)) - radius   (circle when D == 2)
 *   family WL_BODY_TORUS : p = {c0, c1, c2, R, r}    sdf = norm((xi0-c0, norm((xi1-c1, xi2-c2)) - R)) - r   (D == 3)
 *   family WL_BODY_PLATE : p = {a, thk}              sdf = norm(xi - (clamp(xi0,-a,a), 0[, 0])) - thk   (the reference's
 *                                                    test plate, test/maintests.jl:375: a stadium / capsule about the xi0 axis)
 * Matrices are row-major 3x3 (the upper-left 2x2 block when D == 2). */
enum { WL_BODY_SPHERE = 0, WL_BODY_TORUS = 1, WL_BODY_PLATE = 2, WL_BODY_CYLINDER = 3 };
/*   family WL_BODY_CYLINDER: p = {c0, c1, c2, radius, m0, m1, m2}  sdf = sqrt(sum_a m_a != 0 (xi_a - c_a)^2) - radius: a circle
 *                                                    extruded along the axes whose m_a is 0 (the 3-D cylinder of the reference's
 *                                                    examples/ThreeD_cylinder*.jl)
 * A body may be a COMPOSITE: an array of up to WL_BODY_MAXLEAF descriptors combined left to right like the reference's
 * `Bodies(bodies, ops)` (src/AutoBody.jl:40-110; the AutoBody operators +, ∪, ∩, - of :22-34 build the same thing):
 * element 0 carries `count`, element l > 0 its operation `op` against the composite of the elements before it.  The
 * distance is the min / max of the leaves' distances; normal, map and velocity are those of the ACTIVE leaf (:73-93). */
enum { WL_BODY_OP_UNION = 0, WL_BODY_OP_MINUS = 1, WL_BODY_OP_INTERSECT = 2 };
#define WL_BODY_MAXLEAF 6
typedef struct wl_body_desc {
    int32_t family;
    int32_t identity_map;   /* != 0: xi = x (A, b, dA, db, Ainv are ignored; V = 0) */
    double p[8];
    double A[9], b[3], dA[9], db[3], Ainv[9];
    int32_t op;             /* elements 1.. of a composite: WL_BODY_OP_* */
    int32_t count;          /* element 0: number of descriptors in the array (0 is read as 1) */
} wl_body_desc;
/* Part 1: sigma = sdf at every interior cell centre (Body.jl:34) and the number of band cells d^2 < (2+eps)^2 (:35)
 * this rank will report (synchronises).  Part 2 (same body / eps): mu0, mu1, V (:36-48), then BC!(mu0,0) and
 * BC!(V,0,exitBC) (:51-52), the z-slab halo exchange, and the body-free row flags of wl_flow_update; cand_dev (device,
 * nband entries) receives the band cells as LOCAL dense column-major indices i + n0*(j + n1*k), ascending.
 * Only x-rows that hold a band / inside cell now, or held one at the previous wl_measure_fill, are rewritten. */
int wl_measure_rows(wl_flow *a, const wl_body_desc *body, double eps, int64_t *nband);
int wl_measure_fill(wl_flow *a, const wl_body_desc *body, double eps, int64_t *cand_dev);
/* nds(body, loc(0,I), t) = n * kern(clamp(d,-1,1))  (src/Metrics.jl:84-87, Float64) for n listed cells (indices as
 * written by wl_measure_fill): nds_dev[b*D + c] */
int wl_body_nds(const wl_grid *g, const wl_body_desc *body, const int64_t *cand_dev, int64_t n, double *nds_dev);
/* measure!(flow, body; t, eps) for a body given as a CLOSED TRIANGLE MESH (D == 3 only): the mesh twins of the three
 * entry points above; everything they leave in the flow (sigma, the 15 coefficient arrays of touched-now-or-before rows,
 * both BC! calls, halos, row flags, the changed-row record of wl_mg_update_changed, cand_dev ascending) is the same.
 * The mesh lives in xi = A x + b with A a SIMILARITY (A A^T = s^2 I; anything else is refused), so distances in x are
 * distances in xi divided by s.  Distance contract, in grid units of x, Float64:
 *   exact zone: where the true unsigned distance is < exact_radius / s the value is the Euclidean distance to the closest
 *               point c of the surface, signed by sign((xi - c) . n_pseudo), n_pseudo the angle-weighted pseudonormal of
 *               the feature c lies on (face; sum of the two face normals on an edge; angle-weighted sum at a vertex --
 *               Baerentzen & Aanaes 2005); the normal is (x - c)/d (n_pseudo/|n_pseudo| where |d| < 1e-9);
 *               V = -A^-1 (dA/dt x + db/dt); normal and V are zero where d^2 exceeds the (2+eps)^2 of AutoBody.jl:118;
 *   far zone  : elsewhere sigma only carries the right sign and |sigma| >= exact_radius / s; nothing downstream reads more
 *               (src/Body.jl:35,44).
 * wl_mesh_create (host only: no device is needed) checks its arguments -- nt == 0, indices out of range, non-finite
 * coordinates, exact_radius <= 3 (it must reach 2 + eps + 1: the band test is made at cell centres, measure at faces half
 * a cell away), degenerate triangles, an edge not shared by exactly two triangles, a shared edge traversed twice in the
 * same direction -- then builds pseudonormals and a uniform bin grid (edge exact_radius/2) with per-bin triangle lists and
 * inside/outside flags.  vert_host: nv x 3 doubles in xi space; tri_host: nt x 3 zero-based indices, outward by the
 * right-hand rule.  The device copies are made by the first measure call that uses the handle (one allocation set; no
 * later call allocates).  wl_mesh_info: out = {nt, nv, bins, max triangles per bin, sum of all bin lists, non-empty bins,
 * device bytes, bins the surface crosses}.  wl_mesh_eval_host evaluates the same distance function the kernels use on
 * the host (x_host: n x 3; d_host: n; n_host, V_host: n x 3 or NULL): d, normal and V with normal = V = 0 where
 * d^2 > fastd2 -- for checking a mesh without a device. */
typedef struct wl_mesh wl_mesh;
typedef struct wl_mesh_pose {
    double A[9], b[3], dA[9], db[3], Ainv[9];   /* row-major 3x3, as in wl_body_desc */
    int32_t identity_map;                       /* != 0: xi = x, V = 0 */
} wl_mesh_pose;
int wl_mesh_create(wl_mesh **out, const double *vert_host, int64_t nv, const int32_t *tri_host, int64_t nt, double exact_radius);
int wl_mesh_destroy(wl_mesh *m);
int wl_mesh_info(const wl_mesh *m, int64_t out[8]);
int wl_mesh_eval_host(const wl_mesh *m, const wl_mesh_pose *pose, const double *x_host, int64_t n, double fastd2, double *d_host,
                      double *n_host, double *V_host);
int wl_measure_rows_mesh(wl_flow *a, const wl_mesh *m, const wl_mesh_pose *pose, double eps, int64_t *nband);
int wl_measure_fill_mesh(wl_flow *a, const wl_mesh *m, const wl_mesh_pose *pose, double eps, int64_t *cand_dev);
int wl_body_nds_mesh(const wl_grid *g, const wl_mesh *m, const wl_mesh_pose *pose, const int64_t *cand_dev, int64_t n, double *nds_dev);
/* project!(a,b,w)                     src/Flow.jl:137-145 */
int wl_project(wl_flow *a, wl_mg *b, double dt, double w, int *n_iter);
/* mom_step!(a,b)                      src/Flow.jl:153-169.  dt = a.dt[end]; U = BCTuple(a.U,a.dt,N);
 * acc_pred/acc_corr = g(i,t)+dU_i/dt at t=sum(dt[1:end-1]) and t=sum(dt) (NULL when accelerate! is a
 * no-op, :73).  dt_next receives CFL(a); n_iter[2] the two entries pushed onto pois.n.
 * The u0 ARRAY is scratch across the call, as in the reference (it is overwritten by `a.u⁰ .= a.u` before anything reads
 * it, :154): on return it holds either the velocity the step started from (the reference's copy) or -- 3-D, no periodic
 * direction, no convective exit, WL_OPT_BDIM_IN_CONVDIFF -- the predictor's velocity u', because there the two velocity arrays
 * take turns instead of being copied (the predictor reads u and writes u' into u0, the corrector writes the new velocity
 * back into u).  u, p, f, sigma, the time step and the V-cycle counts are the same bits either way. */
int wl_mom_step(wl_flow *a, wl_mg *b, double dt, const double U[3], const double *acc_pred,
                const double *acc_corr, double *dt_next, int n_iter[2]);

/* ------------------------------------------------------------------ Metrics.jl */
/* pressure_force(p,df,body,t)         src/Metrics.jl:94-100.  nds(body,x,t) (:84-87) runs user closures,
 * so the host evaluates it once per measure! and hands over the compact band of non-zero entries:
 * idx[b] = linear element offset of the cell in p (using g->s), nds[b*D + c] = n_c * kern(d), Float64.
 * out[c] = sum_b Float64( T( p[idx[b]] * nds[b,c] ) ). */
int wl_pforce(wl_dtype t, const wl_grid *g, const void *p, const int64_t *idx_dev, const double *nds_dev,
              int64_t nband, double out[3]);

/* viscous_force(u,nu,df,body,t)       src/Metrics.jl:109-113: out = sum_band Float64( T( -nu * (du_i/dx_j + du_j/dx_i) * nds ) ),
 * same band hand-over as wl_pforce (idx are element offsets into one component of u). */
int wl_vforce(wl_dtype t, const wl_grid *g, const void *u, const int64_t *idx_dev, const double *nds_dev, int64_t nband,
              double nu, double out[3]);
/* pressure_moment(x0,p,df,body,t)    src/Metrics.jl:130-134: out = sum_band Float64( T( p * cross(loc(0,I)-x0, nds) ) );
 * D == 2: the scalar cross product is returned in every component, like the reference's broadcast. */
int wl_pmoment(wl_dtype t, const wl_grid *g, const void *p, const int64_t *idx_dev, const double *nds_dev, int64_t nband,
               const double x0[3], double out[3]);

/* ------------------------------------------------------------------ body loads (Forces, waterlily_amd/forces.py)
 * Force, moment and power of the fluid on a body in ONE sweep over a list of n band cells, nds(body, loc(0,I), t) =
 * n * kern(clamp(d,-1,1)) (src/Metrics.jl:84-87, body_measure with fastd2 = 1) evaluated in registers.  rows_dev (device
 * memory) receives nleaf + 1 rows of 16 doubles: rows 0 .. nleaf-1 the leaves of a composite, row nleaf the total.
 * Per counted cell I, T = the flow's type, everything else Float64:
 *   fp[c] = Float64( T( p[I] * nds[c] ) )                                              the term of wl_pforce
 *   fv[c] = Float64( T( sum_j Float64( T( -nu * (d(c,j) + d(j,c)) ) ) * nds[j] ) )     the term of wl_vforce, d = ∂(i,j,I,u)
 *   r     = loc(0,I) - x0    (z-slabs: the global z)         V = the body's velocity at loc(0,I) (AutoBody.jl:128-130)
 * and every column is the plain sum over the cells of the row:
 *   0-2  Fp = fp        3-5  Fv = fv        6-8  Mp = r x fp    9-11 Mv = r x fv    (double arithmetic on the rounded fp, fv)
 *   12   Wp = fp . V    13   Wv = fv . V    the rate of work of the fluid's load at the body's velocity
 *   14   ncells         15   A = |nds|      counted cells; the surface-measure estimate (area, D == 2: perimeter)
 * D == 2: the z slots of Fp, Fv and the x, y slots of Mp, Mv are 0; the scalar moment r_x f_y - r_y f_x is in slot z (cols 8,
 *   11).  wl_pmoment differs: it writes the scalar into both of its two slots, like the reference's broadcast, and rounds
 *   T(p * (r x nds)) where this rounds fp first.
 * Counted: a cell some component of whose nds is non-zero, i.e. kern(clamp(d)) != 0 with a defined normal -- the cells the
 *   compaction of the composed path (wl_body_nds, then dropping the zero vectors) hands to wl_pforce.  Any other cell is
 *   left before p or u is read: a NaN outside the band |d| < 1 does not enter.  A NaN in p at a counted cell makes NaN in
 *   the sums it enters (Fp, Mp, Wp of that cell's leaf and of the total) and nowhere else; likewise u (Fv, Mv, Wv).
 * Leaves: row q holds the cells whose ACTIVE leaf at the cell centre is q (wl_body_desc: the leaf that supplies distance,
 *   normal and velocity).  For a union of disjoint bodies that is the load on each body; across WL_BODY_OP_MINUS /
 *   _INTERSECT it is only an attribution of surface patches.  Row nleaf = row 0 + row 1 + .. in ascending order, so the
 *   total is reproducible from the leaf rows bit for bit.  nleaf = body[0].count (0 read as 1); 1 for a mesh or a stored band.
 * Sources:  wl_body_loads: a parametric body / composite, D = 2 or 3; cand_dev = LOCAL dense column-major cell indices as
 *   written by wl_measure_fill.  wl_body_loads_mesh: a triangle mesh and its pose (D == 3), the same list.  wl_band_loads: a
 *   stored band as for wl_pforce -- idx_dev element offsets, nds_dev[b*D + c] -- for bodies the device cannot evaluate; it
 *   carries no V, so cols 12 and 13 of both rows are NaN (also when n == 0).  Entries that are not cells of inside(p) are
 *   not counted.
 * z-slabs: a rank counts a candidate only if its plane is owned and globally interior; nothing is communicated, every column
 *   is additive over the ranks (ncells included).
 * Order: each thread walks its cells grid-strided in ascending list order, one masked pass per leaf; wavefront, workgroup,
 *   then one final workgroup sums the workgroups' partials in ascending order.  No floating-point atomics: the same inputs
 *   give the same bits on every call.  n == 0 reads no list and writes zero rows (ncells = 0).
 * Asynchronous: two launches on the library's stream, nothing allocated after the library's first reduction, no
 * synchronisation.  Null pointers, n < 0, D other than 2 / 3, a mesh with D != 3 and count > WL_BODY_MAXLEAF return WL_E_ARG
 * before any device call.  WaterLily v1.3 has no such function to override: the entry points are there for a later binding. */
int wl_body_loads(wl_dtype t, const wl_grid *g, const void *p, const void *u, double nu, const wl_body_desc *body,
                  const int64_t *cand_dev, int64_t n, const double x0[3], double *rows_dev /* (count+1)*16 */);
int wl_body_loads_mesh(wl_dtype t, const wl_grid *g, const void *p, const void *u, double nu, const wl_mesh *m,
                       const wl_mesh_pose *pose, const int64_t *cand_dev, int64_t n, const double x0[3], double *rows_dev /* 2*16 */);
int wl_band_loads(wl_dtype t, const wl_grid *g, const void *p, const void *u, double nu, const int64_t *idx_dev,
                  const double *nds_dev, int64_t n, const double x0[3], double *rows_dev /* 2*16 */);

/* Field metrics over inside(out) (src/Metrics.jl:14-77), `@inside out[I] = metric(I,u)`:
 *   WL_M_KE      ke(I,u,U)            0.125*sum_i (u[I,i]+u[I+d_i,i]-2U_i)^2          (par = U)
 *   WL_M_CURL    curl(i,I,u)          component i=ipar of curl u at the cell EDGE      (D==2: i=3 -> ipar=2)
 *   WL_M_OMAG    omega_mag(I,u)       |curl u| at the cell centre                      (D==3)
 *   WL_M_OTHETA  omega_theta(I,z,c,u) omega . theta, theta = z x (loc(0,I)-c)          (par = z[3], par2 = c[3]; D==3)
 *   WL_M_LAMBDA2 lambda2(I,u)         middle eigenvalue of S^2+Omega^2                 (D==3) */
enum { WL_M_KE = 0, WL_M_CURL = 1, WL_M_OMAG = 2, WL_M_OTHETA = 3, WL_M_LAMBDA2 = 4 };
int wl_metric(wl_dtype t, const wl_grid *g, int kind, void *out, const void *u, int ipar, const double par[3],
              const double par2[3]);

/* ------------------------------------------------------------------ volume integrals (Integrals, waterlily_amd/integrals.py)
 * One sweep over u: sums and maxima over the cells I of inside(p) (z-slabs: this rank's owned interior planes; nothing is
 * communicated, the caller combines the ranks' rows), d(i,j) = the reference's ∂(i,j,I,u) (src/Metrics.jl:28-30).  row_dev
 * receives 6 + D doubles (device memory):
 *   0 E = sum ke(I,u,U)    1 Z = sum |omega|^2 / 2 (D == 2: omega_3 = d(2,1) - d(1,2))    2 S = sum S_ij S_ij, S = sym(d)
 *   3 div2 = sum (sum_i d(i,i))^2    4 divmax = max |sum_i d(i,i)|    5 umax = max_i |u[I,i]|
 *   6.. P_i = sum (u[I,i] + u[I+d_i,i]) / 2
 * Every operand is converted to double before the first operation, for either T; sums and maxima are reduced in a fixed
 * order (same field, same bits; no floating-point atomics).  NaN in u gives NaN in the sums that read it; the maxima skip
 * NaN operands (the comparison of wl_max) and are 0 over an empty range.  No body mask: solid and fluid cells alike.
 * U: the background velocity of ke (D values read).  Reads the ghost cells around the interior and, on a z-slab, the first
 * halo plane on each side (mom_step! leaves them current).  Asynchronous: two launches on the library's stream, nothing
 * allocated after the library's first reduction.  WaterLily v1.3 has no such function to override: the entry point is there
 * for a later binding. */
int wl_flow_integrals(wl_dtype t, const wl_grid *g, const void *u, const double U[3], double *row_dev);

/* ------------------------------------------------------------------ time-averaged statistics (MeanFlow, waterlily_amd/stats.py)
 * One update of running means of u and p, and optionally of the velocity covariance (Reynolds stress) and the pressure
 * variance, over EVERY element of the local arrays (ghost cells and z-slab halo planes included; row padding untouched):
 *   d_c = u_c - U_c;  U_c <- U_c + eps d_c;  UU_ij <- (1-eps)(UU_ij + eps d_i d_j);  the same for P, pp with d = p - P
 * in double arithmetic, each store rounded once to t_acc.  eps = dt / (t - t0) in (0, 1], computed by the host in Float64.
 * first != 0 (the first update of an averaging window, eps == 1): U = u, P = p, UU = pp = 0, and the accumulators are not
 * read.  u, p: the flow's fields on grid g (t_flow); U (D components), P, UU (D(D+1)/2 components in ParaView's
 * symmetric-tensor order: 3-D xx yy zz xy yz xz, 2-D xx yy xy) and pp on grid ga (t_acc: same extents and slab as g, the
 * strides may differ).  UU / pp may be NULL (not collected).  The products pair u[I,i] u[I,j] at the same index I (face
 * values of different faces).  t_flow = WL_F64 with t_acc = WL_F32 is refused.  Asynchronous.  WaterLily v1.3 has no
 * MeanFlow to override: the entry point is there for a later binding. */
int wl_meanflow_update(wl_dtype t_flow, wl_dtype t_acc, const wl_grid *g, const void *u, const void *p, const wl_grid *ga, void *U,
                       void *P, void *UU, void *pp, double eps, int first);

/* ------------------------------------------------------------------ turbulent kinetic energy budget (Budget, waterlily_amd/budget.py)
 * wl_budget_update: one update of the CENTRAL moments the budget of k = 1/2 <u_i'u_i'> is made of, over every cell I of
 * inside() (on a z-slab: this rank's owned interior planes; the first halo plane on each side of u and Uf is read, and must
 * exist).  Uf (D components), Pm: the running means BEFORE this update, the fields U, P of a MeanFlow on grid ga (it averages
 * ghost cells and halo planes too, so they are current without an exchange).  In double arithmetic, every operand converted
 * first, one rounding to t_acc per store, with eps = dt / (t - t0) in (0, 1] as for wl_meanflow_update and keep = 1 - eps:
 *   d[J,i] = u[J,i] - Uf[J,i];   a_i = 0.5 (d[I,i] + d[I+e_i,i])  (the centre fluctuation, as in ke);   q = p[I] - Pm[I]
 *   h_ij = d(i,j,I,d) of src/Metrics.jl:28-30:  h_ii = d[I+e_i,i] - d[I,i],
 *          h_ij = (d[I+e_j,i] + d[I+e_j+e_i,i] - d[I-e_j,i] - d[I-e_j+e_i,i]) / 4, added left to right
 *   s = sum_i a_i a_i;   gg = sum_i sum_j h_ij h_ij (i outer, j inner);   every sum ascending, each term added to the sum so far
 *   T3_j <- (keep T3_j + ((keep eps (1 - 2 eps)) s) a_j) - (eps keep) (2 sum_i a_i R_ij + a_j sum_i R_ii)   with the OLD R,
 *   R_q  <- keep (R_q + (eps a_ia) a_ib);   PU_j <- keep (PU_j + (eps q) a_j);   GG <- keep (GG + eps gg)
 * (the weighted single-sample merge of second and third central moments).  R: the cell-centred covariance <u_i'u_j'>,
 * D(D+1)/2 components in ParaView's order (3-D xx yy zz xy yz xz, 2-D xx yy xy); PU: <p'u_j'>, D components; GG:
 * <h_ij h_ij>; T3: <u_i'u_i'u_j'>, D components -- 13 fields in 3-D, 8 in 2-D, on grid ga (same extents and slab as g, the
 * strides may differ), component stride ga->sc.  first != 0 (eps == 1): every moment becomes 0 and no accumulator, u, p or
 * mean is read.  Cells outside inside() are never written.  t_flow = WL_F64 with t_acc = WL_F32 is refused.
 * The means are NOT advanced: the thread of a neighbouring cell reads Uf at the faces of the cell this thread would write, so
 * the caller follows this launch with wl_meanflow_update (U = Uf, P = Pm), which advances them.  Asynchronous: one launch.
 *
 * wl_budget_terms: the budget terms from the moments, one launch over inside(); arithmetic in double, each value rounded once
 * to t_acc; out has eight components on grid ga (component stride ga->sc).  The cells of inside() shrunk by one on every
 * side (global indices 2 .. n-3) get, with k[J] = 0.5 ((R_0[J] + R_1[J]) + R_2[J]), D_j f = (f[I+e_j] - f[I-e_j]) / 2,
 * G_ij = d(i,j,I,Uf) as above, C_j = 0.5 (Uf[I,j] + Uf[I+e_j,j]):
 *   0  k[I]
 *   1  production           -(sum_i sum_j R_ij G_ij)            i outer, j inner
 *   2  dissipation           nu GG[I]                            (positive)
 *   3  turbulent transport  -0.5 (sum_j D_j T3_j)
 *   4  pressure transport   -(sum_j D_j PU_j)
 *   5  viscous diffusion     nu (sum_j ((k[I+e_j] - 2 k[I]) + k[I-e_j]))
 *   6  convection           -(sum_j C_j D_j k)
 *   7  residual              ((((t1 - t2) + t3) + t4) + t5) + t6  of the unrounded terms: dk/dt plus what the discretisation
 *      and the body do not close
 * every sum ascending, each term added to the sum so far.  The remaining cells of inside() (its rim) get 0; cells outside
 * inside() are not written.  On a z-slab the planes next to a rank boundary read one halo plane of R, PU and T3: the caller
 * exchanges them first (wl_halo_exchange).  Asynchronous.  WaterLily v1.3 has no such function to override: the entry points
 * are there for a later binding. */
int wl_budget_update(wl_dtype t_flow, wl_dtype t_acc, const wl_grid *g, const void *u, const void *p, const wl_grid *ga, const void *Uf,
                     const void *Pm, void *R, void *PU, void *GG, void *T3, double eps, int first);
int wl_budget_terms(wl_dtype t_acc, const wl_grid *ga, const void *Uf, const void *R, const void *PU, const void *GG, const void *T3,
                    double nu, void *out);

/* ------------------------------------------------------------------ point probes and tracers (waterlily_amd/probes.py)
 * interp(x, arr)  src/util.jl:238-257.  x_dev: m*D doubles, point-major, 1-based index coordinates (global z).
 * ncomp == 0: scalar field; ncomp == D: staggered vector field.  Row q of the result at out_dev + q*ldo (ldo >= max(1,ncomp)).
 * With i = floor(x), y = x - i: sum over the 2^D corners J in CartesianIndices order of a[J] * prod_d(J_d == i_d ? 1-y_d : y_d),
 * the product in d order, all in double (Float64 results for either T); component c of a vector field is sampled at
 * x + 0.5 e_c (util.jl:253-256).  A corner of weight exactly 0 is not read; a weighted corner outside the array (ghosts
 * included) gives NaN.  z-slabs: each (point, component) is written by the rank owning its floor plane (the first / last rank
 * for the z ghost planes of a ring and for planes outside the array), every other rank writes 0: a sum over the ranks is the
 * value.  Reads the first halo plane of the owner.  Asynchronous. */
int wl_interp(wl_dtype t, const wl_grid *g, const void *a, int ncomp, const double *x_dev, int64_t m, double *out_dev,
              int64_t ldo);
/* one frozen-field Heun step of m tracers (not on decomposed grids): k1 = u(x), xs = x + dt k1, k2 = u(xs),
 * x <- x + 0.5 dt (k1 + k2) with u interpolated as wl_interp does; directions in perdir_mask wrap xs and x into
 * [1.5, N_d + 1.5); a particle leaving [1.5, N_d + 1.5] in another direction or meeting a NaN velocity gets NaN coordinates
 * (dead) and is skipped from then on.  dt finite and >= 0.  A z-slab grid is refused (WL_E_STATE).  Asynchronous. */
int wl_tracer_advance(wl_dtype t, const wl_grid *g, const void *u, double *x_dev, int64_t m, double dt, int perdir_mask);

/* ------------------------------------------------------------------ surface loads of a mesh body (SurfaceLoads, waterlily_amd/surface.py)
 * Pressure and viscous traction PER TRIANGLE of a wl_mesh at the pose of one instant (D == 3), all in double for either T:
 *   x_v = Ainv (xi_v - b) (x_v = xi_v when identity_map);  x_c = (x_a + x_b + x_c) / 3;  S = (x_b - x_a) x (x_c - x_a) / 2
 *   (area times the outward normal, grid units of x);  n = S / |S|;  V_b = -Ainv (dA x_c + db) (0 for the identity map)
 * and at the sample point x_c + delta n, in index coordinates X = x_c + delta n + 1.5 (wl_interp's convention):
 *   p_t = interp(X, p);   G_ij = u_i(X + e_j/2) - u_i(X - e_j/2), u_i sampled as wl_interp samples component i (at + e_i/2);
 *   tau_i = -nu sum_j (G_ij + G_ji) n_j      (the integrand of viscous_force, src/Metrics.jl:116-119)
 * p_t S is the triangle's pressure load and tau |S| its viscous load, with the signs of wl_pforce / wl_vforce.
 * rows_dev: nt*4 doubles {p_t, tau_x, tau_y, tau_z}; geom_dev: nt*9 doubles {x_c, S, V_b}, or NULL.  A sample with a weighted
 * corner outside the array gives NaN in that triangle's entries only (wl_interp's rule).  z-slabs: each of the 19 interp
 * entries of a triangle follows wl_interp's ownership rule (the owner contributes the value, every other rank 0), so every rank
 * writes a PARTIAL row and the sum over the ranks is the value; geometry rows are the same on every rank.
 * mean_dev (nt*4 doubles, or NULL): the running mean of the row, m <- m + w (v - m), w in (0, 1] computed by the host as
 * wl_meanflow_update's eps is; first != 0: m = v, and m is not read.  Linear too: slab partials sum.
 * Refused with WL_E_ARG before the device is touched: NULL mesh, pose or rows_dev; D != 3; delta negative or not finite; nu not
 * finite; a pose that is not a similarity.  Asynchronous: one launch on the library's stream; nothing is allocated unless this
 * is the first call that uses the mesh handle on the device (it then makes the device copies, as wl_measure_rows_mesh does).
 *
 * wl_surface_totals reduces such rows to out_dev[12] (device memory) about the point x0:
 *   Fp = sum p_t S;  Fv = sum tau |S|;  Mp = sum (x_c - x0) x p_t S;  Mv = sum (x_c - x0) x tau |S|
 * in a fixed order (per thread in ascending triangle order, wavefront, workgroup, one final workgroup; no floating-point
 * atomics: the same rows give the same bits); a NaN row makes the sums it enters NaN.  On z-slabs the totals of partial rows are
 * partial totals.  Asynchronous: two launches, nothing allocated after the library's first reduction.  WaterLily v1.3 has no
 * such functions to override: the entry points are there for a later binding. */
int wl_surface_sample(wl_dtype t, const wl_grid *g, const void *p, const void *u, const wl_mesh *m, const wl_mesh_pose *pose,
                      double delta, double nu, double *rows_dev, double *geom_dev, double *mean_dev, double w, int first);
int wl_surface_totals(const double *rows_dev, const double *geom_dev, int64_t nt, const double x0[3], double *out_dev);

/* ------------------------------------------------------------------ isosurface of a scalar field (Isosurface, waterlily_amd/iso.py)
 * The triangles of the level set a == c of a cell-centred scalar field on a wl_grid (D == 3, either T, pitched or dense), by
 * marching tetrahedra on the Kuhn split of every cube (csrc/wl_iso.h).  Every value is converted to double before its first use.
 *   cube       : the 8 elements J .. J + (1,1,1), J 0-based, its low corner.  Output coordinates are x = J - 0.5 with GLOBAL z:
 *                the frame of loc(0, I), in which MeshBody vertices and SurfaceLoads centroids live.
 *   box        : cubes with lo_d <= J_d < hi_d are visited.  lo == hi == NULL: lo = 1, hi_d = n_d - 2 (nzg - 2 along z), all
 *                corners in inside(a), which is all wl_metric fills.  Any 0 <= lo_d <= hi_d <= n_d - 1 is allowed for a caller
 *                whose ghost cells are current.
 *   tetrahedra : 6 per cube, one per permutation (p0,p1,p2) of the axes in lexicographic order 012, 021, 102, 120, 201, 210, with
 *                local corners v0 = J, v1 = v0 + e_p0, v2 = v1 + e_p1, v3 = J + (1,1,1).  Every edge runs from a corner to a
 *                componentwise >= corner, and the split is translation invariant: neighbouring cubes agree on face diagonals.
 *   inside     : corner q is inside iff a_q < c.  A cube with a NaN corner emits nothing.
 *   vertex     : on the edge between local corners p < q (always the lower linear index first): t = (c - a_p) / (a_q - a_p),
 *                x_d = P_d + t where Q_d != P_d, else P_d.  Both cubes sharing an edge produce the same bits, so the surface is
 *                watertight by bit equality.
 *   triangles  : with I the inside and O the outside local corners, both ascending:  |I| = 1: (I0-O0, I0-O1, I0-O2);
 *                |I| = 3: (I0-O0, I1-O0, I2-O0);  |I| = 2: the quad q0 = I0-O0, q1 = I0-O1, q2 = I1-O1, q3 = I1-O0 as (q0,q1,q2) then
 *                (q0,q2,q3).  The last two vertices of a triangle are swapped where needed so that its normal points to the a >= c
 *                side; whether to swap depends on (tet, inside mask) alone and is decided with every crossing at its edge's
 *                midpoint: the sign of n . (mean(O corners) - mean(I corners)).  A triangle with repeated vertices (some a_q == c)
 *                is emitted as it falls out.
 *   order      : cubes in ascending linear index (x fastest), then tet 0..5, then the order above; at most 12 per cube.  The order
 *                is a function of the field alone.
 *   colour     : b (or NULL): a second field on the same grid with the same T; vertex value b_p + t (b_q - b_p) in double.
 * wl_iso_table (host only) returns the (tet, mask) rule -- bit v of mask: local corner v inside: out[0] = the number of triangles,
 * then 3 entries per triangle, each 4*p + q for the edge between local corners p < q; unused entries are -1.
 * wl_isosurface: tri_dev cap*9 doubles, vertex-major (triangle, vertex, xyz); val_dev cap*3 doubles, required iff b is given;
 * count_dev[0] = the number of triangles the surface has, count_dev[1] = min(that, cap) = the number written.  Triangles with
 * global number >= cap are not written and nothing beyond cap is touched; cap == 0 with tri_dev == NULL is a pure count.
 * Refused with WL_E_ARG before the device is touched: NULL g, a or count_dev; D != 3; a bad box; c NaN or infinite; cap < 0;
 * cap > 0 without tri_dev; b without val_dev or val_dev without b; only one of lo and hi.
 * Asynchronous on the library's stream: a count pass (one wavefront per x-row of cubes), an exclusive scan over the
 * (hi1 - lo1)(hi2 - lo2) rows, an emit pass that leaves rows without triangles before reading the field.  Row counts and
 * offsets live in scratch the library owns, which grows only when a call has more rows than any before it: steady calls
 * allocate nothing (wl_prof_allocs).  No atomics: the same field gives the same bits.
 * z-slabs: a rank visits the cubes whose low-corner plane it owns, the box clipped in global z (rank P-1 visits no cube on the
 * top ghost plane: it would need a plane above; on a ring rank 0 also takes the bottom ghost plane, which nobody owns).  The
 * kernel reads the first halo plane above the owned ones, so THE CALLER MUST HAVE EXCHANGED a AND b TO DEPTH 1
 * (wl_halo_exchange): the output of wl_metric is not exchanged.  The ranks' outputs concatenated in rank order are the
 * undecomposed output bit for bit; nothing is communicated.  WaterLily v1.3 has no such function to override. */
int wl_iso_table(int tet, int mask, int32_t out[7]);
int wl_isosurface(wl_dtype t, const wl_grid *g, const void *a, const void *b, double c, const int32_t lo[3], const int32_t hi[3],
                  double *tri_dev, double *val_dev, int64_t cap, int64_t *count_dev);

/* ------------------------------------------------------------------ slice and projection images (Renderer, waterlily_amd/render.py)
 * The on-device twin of the pictures of ext/WaterLilyPlotsExt.jl (flood, body_plot!, sim_gif!: :17-52), without the volume the
 * reference fills and copies to the host for them.
 *
 * wl_render_project reduces the cells lo_d <= J_d < hi_d (0-based) along `axis` to an image of doubles; the value of a cell is
 * formed on the fly from the field f, converted to double before its first use:
 *   WL_R_SCALAR           f a scalar field: the element as stored
 *   WL_R_UCOMP            f a vector field: component ipar as stored, at its face
 *   WL_R_CENTRE           f a vector field: ((double)f[I,c] + (double)f[I+e_c,c]) / 2, c = ipar
 *   WL_R_METRIC + WL_M_*  f = u: (double)(T)m, m what wl_metric of that kind stores in cell I (ipar, par, par2 as there; the
 *                         same device function evaluates both, so the bits are wl_metric's)
 *   box   : lo == hi == NULL: inside(), lo = 1, hi_d = n_d - 1 (nzg - 1 along z).  Any 0 <= lo_d <= hi_d <= n_d - 1 is allowed
 *           (wl_isosurface's rule; z is global) for a caller whose ghost cells are current; a metric kind reads a 1-cell
 *           neighbourhood, so its box must lie in inside().  D == 2: two entries are read.
 *   image : its axes are the two other than `axis` in ascending order, the lower one fast: pixel (a, b), counted from the
 *           box's low corner, is img_dev[b*ld + a].  D == 2: axis must be 2, the image is the field and every mode gives the
 *           same numbers.  A slice is a box one cell thick along `axis`.
 *   modes : all visit the cells in ascending index along `axis`.  WL_R_MAX, WL_R_MIN: NaN is skipped; WL_R_ABSMAX: the signed
 *           value of largest magnitude, the first one on a tie, NaN skipped; a ray of these three that holds nothing but NaN (or
 *           no cell) gives NaN.  WL_R_SUM: a double accumulator that starts at +0 (NaN propagates); WL_R_MEAN: that sum
 *           divided once by hi_axis - lo_axis.
 *   order : axis 1 or 2: one accumulator per pixel.  axis 0: lane l of 64 takes the cells lo_0 + l, lo_0 + l + 64, ... in
 *           ascending order (a lane without a cell holds the start value), then for off = 32, 16, ..., 1: s_l (+)= s_{l+off} over
 *           the lanes l < off, s_l the earlier operand (on an ABSMAX tie the lower lane stays).  No atomics: a numpy loop in
 *           this order reproduces the bits (tests/render_ref.py).
 *   slabs : a rank visits the planes of the box it owns (the first rank of a ring also takes the bottom ghost plane, as for
 *           wl_isosurface).  axis 0 or 1: z is the image's slow axis; the rank writes the rows of its planes -- row = global z -
 *           lo_2 -- and touches no other row.  axis 2: a partial image over its planes; MEAN still divides by the undecomposed
 *           extent, so SUM and MEAN partials add up and MAX / MIN / ABSMAX partials combine in rank order (a rank without a plane
 *           in the box writes NaN / 0).  A metric kind reads the first halo plane on each side (mom_step! leaves u's current).
 *           Nothing is communicated.
 * Refused with WL_E_ARG before the device is touched: NULL g, f or img_dev; an unknown dtype, kind, component or mode; an axis
 * the dimension does not have (D == 2: any but 2); a bad box; only one of lo and hi; a metric box outside inside(); ld smaller
 * than the image width.  Asynchronous: one launch on the library's stream, nothing allocated.
 *
 * wl_render_shade turns such an image (nx x ny) into RGBA8 through a 256-entry colour table, all in IEEE double:
 *   t = (v - vmin) / (vmax - vmin);  levels == 0: idx = clamp(floor(t*256), 0, 255);  levels = n > 0 (the bands of a filled
 *   contour plot): b = clamp(floor(t*n), 0, n-1), idx = floor((b + 0.5) * 256 / n);  the pixel is lut[idx]; a NaN v gives nan_rgba
 *   (NULL: 0,0,0,0).  With mask_dev (a second image, leading dimension ldm) a pixel whose mask value is < mask_lt gets
 *   mask_rgba, whatever v is.  Every pixel becomes zoom x zoom output pixels; flip_y puts the image's last row first (the
 *   high index at the top, as a plot shows it).  rgba_dev: (ny*zoom) x (nx*zoom) x 4 bytes, dense, 4-byte aligned.
 * lut_dev: 256*4 bytes of device memory; mask_rgba / nan_rgba: host arrays.  Refused with WL_E_ARG: vmin >= vmax or either not
 * finite; levels < 0 or > 256; zoom < 1; a NULL image, table or output; negative extents or ld < nx; a mask without its
 * colour or with ldm < nx.  Asynchronous: one launch.  WaterLily v1.3 draws on the host (Plots.jl): both entry points are there
 * for a later binding. */
enum { WL_R_SCALAR = 0, WL_R_UCOMP = 1, WL_R_CENTRE = 2, WL_R_METRIC = 16 };
enum { WL_R_MAX = 0, WL_R_MIN = 1, WL_R_ABSMAX = 2, WL_R_SUM = 3, WL_R_MEAN = 4 };
int wl_render_project(wl_dtype t, const wl_grid *g, const void *f, int kind, int ipar, const double par[3], const double par2[3],
                      int axis, int mode, const int32_t lo[3], const int32_t hi[3], double *img_dev, int64_t ld);
int wl_render_shade(const double *img_dev, int64_t ld, int nx, int ny, double vmin, double vmax, int levels, const uint8_t *lut_dev,
                    const double *mask_dev, int64_t ldm, double mask_lt, const uint8_t mask_rgba[4], const uint8_t nan_rgba[4], int zoom,
                    int flip_y, uint8_t *rgba_dev);

/* ------------------------------------------------------------------ depth-buffered pictures of triangles (Scene, waterlily_amd/scene.py)
 * A small rasteriser for what wl_isosurface and a posed MeshBody yield: triangles tri_dev[nt][3][3] (doubles, the frame
 * x = J - 0.5), optional vertex values val_dev[nt][3], a camera M (row-major 4x4 doubles made on the host, clip = M (x,y,z,1)), an
 * image of W x H pixels (both 1..WL_SCENE_MAX_SIZE) and a depth buffer key_dev[H*W] of uint64.  Row 0 is the top of the picture.
 * Every double operation below is its own IEEE operation in the order written; coverage and depth order are integers, so the
 * keys are a function of the triangles and the camera alone, bit for bit (tests/scene_ref.py restates all of it).
 *   clear   : wl_scene_clear sets every key to all ones: "nothing".
 *   vertex  : per vertex (x, y, z): c_r = ((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + M[r][3], r = 0..3.  The triangle is dropped whole
 *             when a coordinate or a c is not finite, when a c_3 <= 0, or when a z_ndc = c_2/c_3 is not in [0, 1]: THERE IS NO
 *             CLIPPING -- keep the near and far planes clear of the surface, and the eye outside it.  Then
 *             s_x = ((c_0/c_3)*0.5 + 0.5)*W, s_y = (0.5 - (c_1/c_3)*0.5)*H; dropped unless |s_x| < 2^19 and |s_y| < 2^19;
 *             X = (int64)floor(s_x*256 + 0.5), Y = (int64)floor(s_y*256 + 0.5): 8 sub-pixel bits.
 *   cover   : int64 only.  Pixel (i, j) (column, row) has the centre P = (256 i + 128, 256 j + 128).  E_ab(P) = (X_b - X_a)(P_y - Y_a) -
 *             (Y_b - Y_a)(P_x - X_a).  A2 = E_01(V_2); A2 == 0 drops the triangle; A2 < 0 exchanges vertices 1 and 2 (with their
 *             z_ndc, c_3 and values) and negates A2, so both windings are drawn.  E_0 = E_12(P), E_1 = E_20(P), E_2 = E_01(P) (E_k
 *             is opposite vertex k).  The pixel is covered when every E_k > 0, or == 0 on a top or left edge: edge a -> b is left
 *             when Y_b < Y_a and top when Y_b == Y_a and X_b > X_a (after the exchange; y grows downwards).  A centre on an edge
 *             that two triangles share belongs to exactly one of them.  Pixels visited: the centres inside the bounding box of
 *             the three (X, Y), i from (min X + 127) >> 8 to (max X - 128) >> 8, j likewise, both clamped to the viewport.
 *   key     : b_k = (double)E_k / (double)A2; d = (b_0*z_0 + b_1*z_1) + b_2*z_2 (z_k the z_ndc); zq = floor(d * 2^32) clamped to
 *             [0, 2^32 - 1]; key = (uint64)zq << 32 | (base + t), t the triangle's number in this draw.  The pixel takes the
 *             unsigned minimum (a 64-bit integer atomic): the nearest surface wins, equal depth goes to the lower id.  base + nt
 *             <= 2^32 - 1, so no key is all ones.  Draws with disjoint id ranges share one depth buffer.
 *   paths   : a triangle whose clamped bounding box holds at most large_px pixels is rasterised by one lane; the others are
 *             appended (one integer atomic per wavefront) to a list in scratch_dev and a second launch gives each a whole
 *             wavefront, whose lanes tile the box 8 x 8 pixels at a time.  Neither the choice nor the order of the list shows in
 *             the keys.  large_px == 0: every triangle takes the wavefront path; large_px >= W*H: every triangle its lane.
 *             wl_scene_scratch: the bytes of scratch_dev for nt triangles (16 + 4 nt), host arithmetic.
 *   shade   : wl_scene_shade writes rgba_dev[H*W*4] at the pixels whose key holds an id in [base, base + nt) and touches no other
 *             pixel.  tri_dev, val_dev, M, W, H, base must be the draw's.  The E_k and b_k are recomputed from the same integers.
 *             Value, perspective-correct: q_k = b_k / c_3,k; v = ((q_0*v_0 + q_1*v_1) + q_2*v_2) / ((q_0 + q_1) + q_2).  A NaN v
 *             gives nan_rgba (NULL: 0,0,0,0) as it is, unlit.  Otherwise the colour is lut_dev[idx], idx by wl_render_shade's rule
 *             from (v, vmin, vmax, levels) (one device function serves both); without val_dev it is solid_rgba.  Lighting,
 *             flat and two-sided, from the triangle as stored: a = V_1 - V_0, b = V_2 - V_0, n = (a_y*b_z - a_z*b_y, a_z*b_x - a_x*b_z,
 *             a_x*b_y - a_y*b_x), len = sqrt((n_x*n_x + n_y*n_y) + n_z*n_z), s = ambient + (1 - ambient) * |((n_x*l_x + n_y*l_y) +
 *             n_z*l_z) / len| (len == 0: s = ambient); a channel c becomes floor(c*s + 0.5) clamped to 0..255; alpha is 255.  The
 *             sqrt is the one operation not held to a correctly rounded result.  light: a unit vector, host array.
 *   resolve : wl_scene_resolve: a pixel whose key is "nothing" counts as background_rgba, any other as rgba_dev's; every
 *             ssaa x ssaa block (ssaa 1, 2 or 4; W and H multiples of it) becomes one pixel of out_dev[(H/ssaa)*(W/ssaa)*4], per
 *             channel (sum + n/2) / n in integers, n = ssaa^2.  Anti-aliasing is drawing at ssaa times the size.
 * Refused with WL_E_ARG before the device is touched: a NULL key_dev, scratch_dev, M, light, rgba_dev, out_dev or
 * background_rgba; NULL tri_dev with nt > 0; W or H outside 1..4096; nt < 0; base + nt > 2^32 - 1; a camera entry that is not
 * finite; large_px < 0; scratch_bytes below wl_scene_scratch's; val_dev without lut_dev, with vmin >= vmax or either not finite,
 * or levels outside 0..256; neither val_dev nor solid_rgba; ambient outside [0, 1]; a light that is not finite; ssaa other than
 * 1, 2, 4 or not dividing W and H; an output that is not 4-byte aligned.  Asynchronous on the library's stream; nothing is
 * allocated, no LDS, no float atomics.  The triangles of a draw must stay unchanged until its wl_scene_shade has run.  A
 * decomposed flow has no distributed picture: draw what the ranks' triangles gathered on one rank give.  WaterLily v1.3 draws
 * on the host (Makie): these entry points are there for a later binding. */
enum { WL_SCENE_MAX_SIZE = 4096 };
int wl_scene_clear(uint64_t *key_dev, int W, int H);
int wl_scene_scratch(int64_t nt, int64_t *bytes);
int wl_scene_draw(uint64_t *key_dev, int W, int H, const double M[16], const double *tri_dev, int64_t nt, uint32_t base, int64_t large_px,
                  void *scratch_dev, int64_t scratch_bytes);
int wl_scene_shade(const uint64_t *key_dev, int W, int H, uint32_t base, int64_t nt, const double *tri_dev, const double *val_dev,
                   const double M[16], double vmin, double vmax, int levels, const uint8_t *lut_dev, const uint8_t solid_rgba[4],
                   const double light[3], double ambient, const uint8_t nan_rgba[4], uint8_t *rgba_dev);
int wl_scene_resolve(const uint8_t *rgba_dev, int W, int H, const uint64_t *key_dev, int ssaa, const uint8_t background_rgba[4],
                     uint8_t *out_dev);

/* ------------------------------------------------------------------ ray-marched pictures of a scalar field (Volume, waterlily_amd/volume.py)
 * The field itself seen through Scene's camera: a scalar field f in the flow's layout (p, sigma, a `like` scratch) as an
 * emitting and absorbing cloud, composited front to back over what wl_scene_draw and wl_scene_shade left in key_dev and rgba_dev
 * (both W x H, the draw's size), so that a surface hides the cloud behind it.  wl_scene_volume runs after the last
 * wl_scene_shade and before wl_scene_average, which takes wl_scene_resolve's place in such a picture.  Every double operation
 * below is its own IEEE operation in the order written, and there is no sqrt and no transcendental: acc_dev and rgba_dev are a
 * function of the field, the keys and the camera alone, bit for bit (tests/volume_ref.py restates all of it).
 *   ray     : pixel (i, j) (column, row; row 0 is the top, as for wl_scene_draw): x_n = ((i + 0.5)/W)*2 - 1, y_n = 1 - ((j + 0.5)/H)*2;
 *             h0_r = (Minv[r][0]*x_n + Minv[r][1]*y_n) + Minv[r][3] and g_r = Minv[r][2], r = 0..3, Minv the inverse of the draw's
 *             M (row-major, made on the host).  The homogeneous point at NDC depth z is h_r(z) = h0_r + z*g_r and the world
 *             point P(z)_d = h_d(z) / h_3(z).  P0 = P(0), P1 = P(1), D = P1 - P0.  A ray with a component of P0 or P1 that is
 *             not finite is empty.  The parameter s in [0, 1] of P0 + s D is linear in eye depth along EVERY ray (perspective
 *             included), so the samples of all rays lie on common planes parallel to the picture plane: view-aligned slices.
 *             An oblique ray of a wide perspective therefore walks 1/cos(theta) more world length per step than the central
 *             one; no sqrt is spent on equalising that.
 *   box     : the cells lo_d <= J_d < hi_d (0-based; NULL, NULL: inside()), hi_d - lo_d >= 2.  The frame is x = J - 0.5 (Scene's
 *             and MeshBody's) and X = x + 1.5 in wl_interp's coordinates.  The sampled region is the cell CENTRES of the box:
 *             blo_d = lo_d - 0.5, bhi_d = hi_d - 1.5.  s_in = 0, s_out = 1; for d = 0, 1, 2: when D_d == 0 the ray is empty unless
 *             blo_d <= P0_d <= bhi_d; otherwise ta = (blo_d - P0_d)/D_d, tb = (bhi_d - P0_d)/D_d, s_in = max(s_in, min(ta, tb)),
 *             s_out = min(s_out, max(ta, tb)) (max(a, b) = a > b ? a : b, min likewise).
 *   surface : a pixel whose key is not "nothing": zq = key >> 32, z = (double)zq / 2^32, Ps = P(z), s_stop = (((Ps_0-P0_0)*D_0 +
 *             (Ps_1-P0_1)*D_1) + (Ps_2-P0_2)*D_2) / ((D_0*D_0 + D_1*D_1) + D_2*D_2); otherwise s_stop = +inf.
 *   samples : k = 0, 1, ... while s_k = ((double)k + 0.5)*ds satisfies s_k <= s_out and s_k < s_stop; the sample is taken when
 *             s_k >= s_in (an implementation may start at any k not beyond the first taken one).  Pk_d = P0_d + s_k*D_d;
 *             v = wl_interp's value of f at Pk + 1.5 (a corner of weight 0 is not read, a weighted corner outside the array
 *             gives NaN); a NaN v is skipped.  idx by wl_render_shade's rule from (v, vmin, vmax, levels); a = opac_dev[idx];
 *             w = T*a; C_c = C_c + w*(double)lut_dev[idx][c], c = 0, 1, 2; T = T*(1.0 - a); when T < t_min the march of that
 *             ray stops with T kept as it is.  C = 0, T = 1 at the start.
 *   pixel   : base = background_rgba when the key is "nothing", otherwise rgba_dev's pixel.  A colour channel becomes
 *             floor((C_c + T*(double)base_c) + 0.5) clamped to 0..255, alpha floor(((1.0 - T)*255.0 + T*(double)base_a) + 0.5)
 *             clamped, written in place for EVERY pixel: an empty ray writes base exactly, so afterwards rgba_dev holds the
 *             background too and the keys are no longer needed to finish the picture.  acc_dev[H*W*4], when given, gets
 *             C_r, C_g, C_b, T.  key_dev is only read.
 *   average : wl_scene_average is wl_scene_resolve's block average, (sum + n/2) / n per channel in integers, without the key
 *             test (one device function serves both).
 * opac_dev: 256 doubles in [0, 1], the share absorbed per step; its values are the caller's and are not checked on the device.
 * How tiles of pixels are dealt to wavefronts, and the skip of a sample whose a == 0 before its colour is fetched, show in no
 * bit.  Refused with WL_E_ARG before the device is touched: a NULL g, f, Minv, lut_dev, opac_dev, key_dev, background_rgba or
 * rgba_dev; an unknown dtype; D != 3; a bad box, only one of lo and hi, or an extent below 2; a Minv entry that is not finite;
 * ds outside [2^-20, 1]; vmin >= vmax or either not finite; levels outside 0..256; t_min outside [0, 1); W or H outside
 * 1..WL_SCENE_MAX_SIZE; a frame that is not 4-byte, keys or acc_dev that are not 8-byte aligned; for wl_scene_average: ssaa
 * other than 1, 2, 4 or not dividing W and H, or an unaligned frame or output.  A z-slab grid is refused with WL_E_STATE: it
 * has no distributed picture, as for Scene.  Asynchronous on the library's stream; nothing is allocated, no LDS, no float
 * atomics.  WaterLily v1.3 draws on the host: these entry points are there for a later binding. */
int wl_scene_volume(wl_dtype t, const wl_grid *g, const void *f, const double Minv[16], double ds, const int32_t lo[3], const int32_t hi[3],
                    double vmin, double vmax, int levels, const uint8_t *lut_dev, const double *opac_dev, double t_min,
                    const uint64_t *key_dev, const uint8_t background_rgba[4], uint8_t *rgba_dev, double *acc_dev, int W, int H);
int wl_scene_average(const uint8_t *rgba_dev, int W, int H, int ssaa, uint8_t *out_dev);

/* ------------------------------------------------------------------ box-filtered, cropped volumes (Downsampler, waterlily_amd/downsample.py)
 * The 3-D counterpart of wl_render_project: the fine cells lo_d <= J_d < hi_d (0-based, z global) are cut into blocks of
 * factor^D cells and every block becomes one coarse cell, its value formed on the fly from f.  No volume is filled first: a
 * downsampled metric reads u once and stores 1/factor^D of a field.
 *   kind  : WL_R_SCALAR, WL_R_UCOMP, WL_R_CENTRE, WL_R_METRIC + WL_M_* with ipar, par, par2 exactly as for wl_render_project (the
 *           same device function forms the value).  WL_R_FACE: f a vector field; the f^(D-1) fine faces of component ipar on the
 *           low ipar-face of the block, f[J, ipar] as stored: one fine layer along ipar is read, not f of them.  The coarse
 *           field of MEAN face values is staggered like the fine one, and its divergence over a coarse cell is f^(1-D) times the
 *           sum of the fine divergences of the block: every interior fine face cancels.
 *   box   : lo == hi == NULL: inside().  0 <= lo_d < hi_d <= n_d - 1 (nzg - 1 along z) and every extent a multiple of factor; a
 *           metric kind's box must lie in inside().  D == 2: two entries are read, blocks are f x f.  factor: 1, 2, 4, 8 or 16;
 *           factor 1 is a crop (with a metric kind: the metric of the box, packed, without a scratch field).
 *   modes : WL_R_MAX, WL_R_MIN, WL_R_ABSMAX, WL_R_SUM, WL_R_MEAN combine with wl_render_project's rule acc (+)= v (NaN skipped by the
 *           first three, the first of two equal candidates stays, a block of nothing but NaN gives NaN; SUM and MEAN: a double
 *           sum from +0, NaN propagates).  MEAN multiplies the sum once by the exact power of two 1/f^D (WL_R_FACE: 1/f^(D-1)).
 *           WL_R_SAMPLE: the value of the block's first cell (plain decimation).
 *   order : 64 consecutive fine x of a block row, counted from lo_0, belong to one wavefront; factor divides 64, so a coarse cell
 *           never straddles two.  The lane of fine x walks the f x f rows of its column of the block, z outer and y inner, both
 *           ascending, with one accumulator that starts at +0 (SUM, MEAN) or NaN = "nothing yet".  Then the f lanes of a coarse
 *           cell are combined: for off = f/2, ..., 1: s_l (+)= s_{l+off} over the lanes l < off of the block, s_l the earlier
 *           operand; the result is s_0.  WL_R_FACE visits the low face alone: ipar == 0: only lane 0 of the block walks (the
 *           others enter the tree with the start value); ipar == 1: the first y row of the block; ipar == 2: its first z plane.
 *           No atomics: a numpy loop in this order reproduces the bits (tests/downsample_ref.py).
 *   out   : dense, x fast: coarse cell (I, J, K), counted from the box's low corner (K from this rank's first coarse plane),
 *           goes to out_dev[((K*ncy + J)*ncx + I)*ntuple + c] as t_out (WL_F32 or WL_F64): the double result is rounded once,
 *           at the store.  Entries of other c are not touched, so the components of a vector interleave into one staging buffer
 *           the way wl_snapshot_pack lays them out.  1 <= ntuple <= 9, 0 <= c < ntuple.
 *   slabs : a rank emits the blocks that lie wholly within the planes it owns (the first rank of a ring also takes the bottom
 *           ghost plane, as for wl_isosurface); a boundary of its planes that falls inside the box must be at lo_2 + m*factor,
 *           else WL_E_ARG.  The ranks' outputs concatenated in rank order are the undecomposed output bit for bit; nothing is
 *           communicated.  A metric kind reads the first halo plane on each side, WL_R_CENTRE along z the one above.
 * wl_downsample_extent (host arithmetic only) gives this rank's coarse extents nc (D == 2: nc[2] = 1) and its first coarse
 * plane k0 for a box: what a caller sizes its buffer with and places the part by.  It applies the factor, box and slab checks.
 * Refused with WL_E_ARG before the device is touched: NULL g, f or out_dev; an unknown t, t_out, kind, component or mode; a
 * factor outside the set; extents that are no multiples of it; only one of lo and hi; a bad box; a metric box outside inside();
 * ntuple or c out of range; WL_R_FACE without a vector component (ipar outside 0..D-1).  Asynchronous: one launch on the
 * library's stream, no LDS, nothing allocated.  wl_render_project refuses WL_R_FACE and WL_R_SAMPLE.  WaterLily v1.3 has no
 * such function to override. */
enum { WL_R_FACE = 3 };
enum { WL_R_SAMPLE = 5 };
int wl_downsample(wl_dtype t, const wl_grid *g, const void *f, int kind, int ipar, const double par[3], const double par2[3],
                  int mode, int factor, const int32_t lo[3], const int32_t hi[3], wl_dtype t_out, void *out_dev, int ntuple, int c);
int wl_downsample_extent(const wl_grid *g, int factor, const int32_t lo[3], const int32_t hi[3], int32_t nc[3], int32_t *k0);

/* ------------------------------------------------------------------ histograms and extremes (Histogram, waterlily_amd/hist.py)
 * How the values of a field are distributed over the cells lo_d <= J_d < hi_d (0-based, z global): wl_histogram counts one value
 * per cell into bins (1-D), or a pair of values into a table (joint 2-D); wl_field_range finds the extremes.  The value of a cell
 * is formed on the fly, as for wl_render_project and wl_downsample (the same device function): no volume is filled first.
 *   kind  : per axis: WL_R_SCALAR, WL_R_UCOMP, WL_R_CENTRE, WL_R_METRIC + WL_M_* with ipar, par, par2 exactly as for
 *           wl_render_project; the value is a double, replaced by |v| when absval != 0.  WL_R_FACE is refused.  The two axes of
 *           a joint histogram may read different fields (a->f = p, b->f = u); both lie on the grid g and have dtype t.
 *   box   : lo == hi == NULL: inside().  0 <= lo_d < hi_d <= n_d - 1 (nzg - 1 along z); a metric kind's box must lie in inside()
 *           (of either axis).  D == 2: two entries are read.
 *   bins  : an axis has n = nbins interior bins 1..n, the underflow bin 0 and the overflow bin n + 1.  A cell whose value on
 *           either axis is NaN is counted in cnt_dev[1] and in no bin.  For any other v (+-inf included), three ways:
 *           uniform, host range (range_dev == edges_dev == NULL): lo, hi of the struct, finite, hi > lo.
 *           uniform, device range (range_dev: two doubles on the device, e.g. wl_field_range's output: an auto-ranged histogram
 *             needs no read-back): lo = range_dev[0], hi = range_dev[1], read by the kernel.
 *             Both: v < lo: bin 0; else v > hi: bin n + 1; else, if !(hi > lo) -- only a device range can be so: a constant
 *             field, or NaN, NaN from a box of nothing but NaN -- bin 1 if lo <= v <= hi and bin n + 1 otherwise (so with a NaN
 *             range every non-NaN cell is in bin n + 1; nothing is multiplied); else t = (v - lo) * scale with
 *             scale = (double)n / (hi - lo), every operation an IEEE double operation rounded on its own (no FMA), computed on
 *             the device in both cases, and the bin is 1 + min(n - 1, (int)t), where a t that is not < n - 1 (NaN from an
 *             infinite device range included) takes n - 1 without a conversion.  The top edge is closed: v == hi is in bin n.
 *           edges (edges_dev: n + 1 strictly increasing finite doubles e_0..e_n on the device, n <= 1024): v < e_0: bin 0;
 *             v > e_n: bin n + 1; else 1 + (the number of e_1..e_{n-1} that are <= v): numpy's convention, bin k = [e_{k-1}, e_k)
 *             and the last one closed, v == e_n in bin n.  Comparisons only (a binary search over a copy in LDS).  THAT THE
 *             EDGES INCREASE IS THE CALLER'S PRECONDITION: the library cannot read them before the launch (waterlily_amd.hist
 *             checks its host copy); edges that do not increase give counts that mean nothing, never an access out of bounds.
 *   out   : A = a->nbins + 2, B = b ? b->nbins + 2 : 1.  cnt_dev: 2 + A*B int64: [0] the cells visited (the box's cells in
 *           this rank's planes), [1] the cells dropped for a NaN, [2 + jb*A + ia] the bins: cnt[0] == cnt[1] + the sum of the
 *           bins.  accumulate == 0: the call overwrites (it zeroes the 2 + A*B entries on the library's stream first);
 *           accumulate != 0: it adds to what is there (a PDF over many steps).  A*B <= 8192.
 *   order : none.  Counts are integers: wavefronts count into a workgroup's uint32 table in LDS (a workgroup counts far fewer
 *           than 2^32 cells: csrc/wl_hist.h) and the workgroups add to cnt_dev with 64-bit integer atomics, so the result is a
 *           function of the field and the bins alone, bit for bit, on any launch shape.  No floating-point atomics anywhere.
 *   slabs : a rank counts the cells of the box in the planes it owns (the first rank of a ring also takes the bottom ghost
 *           plane, as for wl_isosurface); a rank without a plane in the box leaves zeros (accumulate == 0).  The ranks' tables
 *           added up are the undecomposed table, exactly; nothing is communicated.  A metric kind reads the first halo plane on
 *           each side, WL_R_CENTRE along z the one above.  A device range is this rank's own: combine ranges before use.
 * wl_field_range: out_dev[0..3] = the minimum, the maximum, the number of non-NaN cells, the number of NaN cells (doubles; the
 * counts are exact below 2^53) of the value (kind, ipar, par, par2, absval as above) over the box.  NaN is skipped, +-inf take
 * part; -0 and +0 compare by the IEEE total order (the minimum of the two is -0, the maximum +0), so the result does not depend
 * on the order of combination; no non-NaN cell (or no cell of this rank's): NaN, NaN, 0, the NaN cells.  Two launches:
 * per-workgroup partials into scratch_dev (at least wl_field_range_scratch's bytes: a constant of the library, whatever the
 * grid), then one workgroup combines them.  No atomics.
 * Refused with WL_E_ARG before the device is touched: wl_histogram: NULL g, a, a->f, cnt_dev, or b->f of a given b; an unknown
 * t, kind or component; WL_R_FACE; nbins < 1; A*B > 8192; edges with nbins > 1024; both range_dev and edges_dev; a host range
 * that is not finite or not hi > lo; only one of lo and hi of the box; a bad box; a metric box outside inside().
 * wl_field_range: NULL g, f, out_dev or scratch_dev; scratch_bytes too small; t, kind, component and box as above.
 * wl_field_range_scratch: NULL g or bytes, a bad grid.  Asynchronous on the library's stream: wl_histogram one launch (after a
 * memset), wl_field_range two; nothing allocated.  WaterLily v1.3 has no such function to override. */
typedef struct {
    const void *f;            /* the field this axis reads */
    int32_t kind, ipar;
    double par[3], par2[3];   /* of a metric kind (wl_metric); unused otherwise */
    int32_t absval;
    int32_t nbins;
    double lo, hi;            /* the host range; unused with range_dev or edges_dev */
    const double *range_dev;  /* NULL, or {lo, hi} on the device */
    const double *edges_dev;  /* NULL, or nbins + 1 edges on the device */
} wl_hist_axis;
int wl_histogram(wl_dtype t, const wl_grid *g, const wl_hist_axis *a, const wl_hist_axis *b, const int32_t lo[3], const int32_t hi[3],
                 int accumulate, int64_t *cnt_dev);
int wl_field_range(wl_dtype t, const wl_grid *g, const void *f, int kind, int ipar, const double par[3], const double par2[3],
                   int absval, const int32_t lo[3], const int32_t hi[3], void *scratch_dev, int64_t scratch_bytes, double *out_dev);
int wl_field_range_scratch(const wl_grid *g, int64_t *bytes);

/* ------------------------------------------------------------------ two-point statistics (TwoPoint, waterlily_amd/twopoint.py)
 * How the value at a cell relates to the value r cells further along one grid axis: for every separation r = 0 .. nsep - 1 the
 * sums from which correlations, structure functions and the 1-D spectrum follow, over the cells lo_d <= J_d < hi_d (0-based, z
 * global).  Both values of a pair are formed on the fly, as for wl_render_project, wl_downsample and wl_histogram (the same
 * device function): no volume is filled first, and a line is read once for all its separations.
 *   kinds : A = a, B = b, each WL_R_SCALAR, WL_R_UCOMP, WL_R_CENTRE or WL_R_METRIC + WL_M_* with ipar, par, par2 exactly as for
 *           wl_render_project; the value is a double (an element is converted before the first operation, for Float32 and
 *           Float64 alike).  WL_R_FACE is refused.  a->f and b->f may be different fields (a->f = p, b->f = u); both lie on the
 *           grid g and have dtype t.  b == NULL: B is A, formed once per cell; the table has the bits of b = a given explicitly.
 *   box   : lo == hi == NULL: inside().  0 <= lo_d < hi_d <= n_d - 1 (nzg - 1 along z); a metric kind's box (of either value)
 *           must lie in inside().  D == 2: two entries are read.  A LINE is the box's cells along `axis` with the other indices
 *           fixed: n = hi_axis - lo_axis cells, n <= WL_TP_MAX_LINE; 1 <= nsep <= n.
 *   pairs : the partner of cell I at separation r is I' with axis index i + r.  periodic != 0: the index wraps inside the box,
 *           lo + ((i - lo + r) mod n) -- no ghost cell is read for the wrap -- and every line has n pairs at every r.
 *           periodic == 0: the pairs with i + r >= hi_axis do not exist; a line has n - r of them.
 *   out   : out_dev[r * 10 + q], doubles.  With a = A(I), b = B(I'), d = b - a, d2 = d * d, every operation an IEEE double
 *           operation rounded on its own (no FMA):
 *             q = 0  N(r): the number of pairs, (lines) * (periodic ? n : n - r), formed by arithmetic, not accumulated
 *             q = 1  sum a            q = 2  sum b            q = 3  sum a*a          q = 4  sum b*b        q = 5  sum a*b
 *             q = 6  sum d2           q = 7  sum d2*d         q = 8  sum d2*d2        q = 9  sum fabs(d)*d2
 *           Sums start at +0; NaN propagates into the rows and columns that read it (N(r) never).  accumulate == 0: the call
 *           overwrites the 10 * nsep entries; accumulate != 0: the call's total, N(r) included, is added ONCE to the entry
 *           that is there, old + new (a statistic over many steps).
 *   order : fixed, and part of the contract.  Line q of the box (q = 0 .. lines - 1) is, for axis 0, the x-row j = lo_1 + q
 *           mod e, k = lo_2 + q div e with e the box's y extent; for axis 1 (2) the line i = lo_0 + q mod e, k (j) = lo + q div e
 *           with e the box's x extent.  L = 16 (n <= 255), 8 (n <= 511) or 4 lines make a ROUND; there are R = ceil(lines / L)
 *           rounds and G = min(512, R) workgroups of 4 wavefronts; workgroup g takes the rounds g, g + G, ..., and of round t
 *           wavefront w takes the lines t*L + w, t*L + w + 4, ... (below lines).  Wavefront v = 4*g + w adds, per separation
 *           and column, the terms of its lines in that order -- ascending q -- and within a line by ascending i, into one
 *           double that starts at +0.  The table's entry is the 4*G wavefront sums (the ones without a line are +0) added in
 *           ascending v to a double that starts at +0.  No floating-point atomics anywhere; the same call gives the same bits.
 *   slabs : axes 0 and 1 of a 3-D flow on z-slabs: a rank takes the lines in the planes it owns (the first rank of a ring
 *           also takes the bottom ghost plane, as for wl_isosurface) with N(r) counting its own lines; a rank without a plane
 *           in the box writes zeros (accumulate == 0).  The ranks' tables added in rank order (waterlily_amd.twopoint.combine)
 *           are the statistic: column 0 is exact, the sums are the decomposed sums, not the undecomposed bits.  Nothing is
 *           communicated.  A metric kind reads the first halo plane on each side, WL_R_CENTRE along z the one above, as for
 *           wl_histogram.  Axis 2 on a z-slab is refused: the lines cross ranks and the halo is 2 planes.
 * wl_twopoint_scratch: the bytes of scratch_dev for this grid (rank), axis, nsep and box: 4*G blocks of 9 * nsep doubles, host
 * arithmetic (at 512^3 and nsep = 256: 38 MB).
 * Refused with WL_E_ARG before the device is touched: NULL g, a, a->f, out_dev or scratch_dev, or b->f of a given b; an unknown
 * t, kind or component; WL_R_FACE; axis outside 0..D-1; nsep outside 1..n; n > WL_TP_MAX_LINE; only one of lo and hi; a bad or
 * empty box; a metric box outside inside(); scratch_bytes below wl_twopoint_scratch's; axis 2 on a z-slab.
 * wl_twopoint_scratch: NULL g or bytes, a bad grid, and axis, nsep and box as above.  Asynchronous on the library's stream: two
 * launches (the wavefront sums into scratch_dev, then one pass that adds them), nothing allocated.  WaterLily v1.3 has no such
 * function to override. */
#define WL_TP_MAX_LINE 1024   /* 4 lines x 2 values x 1024 doubles are the 64 KB of LDS a workgroup stages */
typedef struct {
    const void *f;            /* the field this value reads */
    int32_t kind, ipar;
    double par[3], par2[3];   /* of a metric kind (wl_metric); unused otherwise */
} wl_tp_value;
int wl_twopoint_scratch(const wl_grid *g, int axis, int nsep, const int32_t lo[3], const int32_t hi[3], int64_t *bytes);
int wl_twopoint(wl_dtype t, const wl_grid *g, const wl_tp_value *a, const wl_tp_value *b, int axis, int nsep, int periodic,
                const int32_t lo[3], const int32_t hi[3], int accumulate, void *scratch_dev, int64_t scratch_bytes, double *out_dev);

/* ------------------------------------------------------------------ connected regions of a threshold set (Regions, waterlily_amd/regions.py)
 * How many objects a threshold cuts out of a field, where they are, how big, and which cells belong to which: the cells
 * lo_d <= J_d < hi_d (0-based) whose value lies below (above) a level are grouped into face-connected REGIONS; every cell gets
 * its region's number and every region a row of integers and two extremes.  The value of a cell is formed on the fly, as for
 * wl_render_project, wl_downsample, wl_histogram and wl_twopoint (the same device function): no volume of values is filled first.
 *   value : WL_R_SCALAR, WL_R_UCOMP, WL_R_CENTRE, WL_R_METRIC + WL_M_* with ipar, par, par2 exactly as for wl_render_project; the
 *           value is a double, replaced by |v| when absval != 0.  WL_R_FACE is refused.
 *   set   : a cell is IN when v < c (WL_RG_BELOW) or v > c (WL_RG_ABOVE): strict IEEE double comparisons, so a cell whose value
 *           equals c is out.  A NaN value is never IN; it is counted in n_dev[2].  c must not be NaN; +-inf is allowed.
 *   box   : lo == hi == NULL: inside().  0 <= lo_d < hi_d <= n_d - 1; a metric kind's box must lie in inside().  D == 2: two
 *           entries are read.  The box holds nx*ny*nz < 2^31 cells; the DENSE INDEX of the box cell (i, j, k), counted from the
 *           box's low corner, is q = (k*ny + j)*nx + i.  Cells outside the box do not exist for this call: an IN ghost cell next
 *           to the box joins nothing.
 *   joins : two IN cells are joined when they share a face: 4 neighbours in 2-D, 6 in 3-D; no edge or corner neighbours.  Bit d of
 *           periodic_mask also joins the first and the last cell of every line of the box along axis d (the wrap stays inside
 *           the box: no ghost cell is read, as with wl_twopoint); a bit for an axis the dimension does not have is refused.  A
 *           REGION is a connected component of the IN cells under these joins.
 *   label_dev : nx*ny*nz int32, dense, in the order of q: -1 for a cell that is not IN, else the region's number r.  Regions are
 *           numbered 0 .. R - 1 by the ascending smallest q they contain (their ROOT).  The label volume is a function of the
 *           field, c and the box alone, and is written in full whatever cap is.
 *   n_dev : 4 int64: [0] R, [1] the IN cells, [2] the NaN cells, [3] the cells visited (== nx*ny*nz).
 *   tab_dev : cap x 13 int64.  Row r < min(R, cap): 0 the root q; 1 the cells; 2..4 the sums of i, j, k over the cells, as 0-based
 *           array indices J (ghost offset included: the frame of lo and hi); 5..10 min i, max i, min j, max j, min k, max k in the
 *           same frame (D == 2: k is 0); 11 the smallest q at which the region's minimum value is attained, 12 the same for its
 *           maximum.  With R > cap the first cap rows are filled, rows of higher numbers are not written, and n_dev[0] is still
 *           the true R: the caller grows the table and calls again.  cap == 0 with tab_dev == ext_dev == NULL is allowed (labels
 *           and counts only).
 *   ext_dev : cap x 2 doubles: the region's minimum and maximum value.  -0 < +0 by the IEEE total order (the integer image of
 *           wl_field_range); +-inf take part.  During the call ext_dev holds those integer images.
 *   order : none.  Every column is an integer count, an integer sum, an integer extreme or an extreme of an order-preserving
 *           integer image, formed with integer atomics: the same bits on any launch shape.  No floating-point atomics anywhere.
 *           Value-weighted sums per region (the circulation or the enstrophy of a vortex) are deliberately NOT in this table:
 *           a floating-point sum needs an order contract per region.  wl_region_sums (below) forms them as exact integers.
 *   slabs : a decomposed flow (a z-slab grid, more than one rank) is refused: regions cross ranks, and merging the labels along
 *           the rank boundaries is a later addition.
 * The method: union-find over the dense indices by label equivalence, the parent array being label_dev itself (csrc/wl_regions.h,
 * PAPERS.md).  wl_regions_scratch: the bytes of scratch_dev for this grid and box, host arithmetic: 16 bytes per x-row of the
 * box plus 8 (at 512^3: 4 MB).
 * Refused with WL_E_ARG before the device is touched: NULL g, v, v->f, label_dev, n_dev or scratch_dev; an unknown t, kind,
 * component or cmp; WL_R_FACE; NaN c; a periodic_mask bit >= D; only one of lo and hi; a bad or empty box; a metric box outside
 * inside(); a box of 2^31 cells or more; cap < 0; cap > 0 with a NULL tab_dev or ext_dev; a buffer not aligned to its element;
 * scratch_bytes below wl_regions_scratch's; a z-slab grid.  wl_regions_scratch: NULL g or bytes, a bad grid, a z-slab grid, and
 * the box as above.  Asynchronous on the library's stream: a memset and ten launches (seven with cap == 0), a fixed number;
 * nothing allocated, nothing read back.  WaterLily v1.3 has no such function to override. */
typedef struct {
    const void *f;            /* the field the value reads */
    int32_t kind, ipar;
    double par[3], par2[3];   /* of a metric kind (wl_metric); unused otherwise */
    int32_t absval;
} wl_rg_value;
enum { WL_RG_BELOW = 0, WL_RG_ABOVE = 1 };
int wl_regions_scratch(const wl_grid *g, const int32_t lo[3], const int32_t hi[3], int64_t *bytes);
int wl_regions(wl_dtype t, const wl_grid *g, const wl_rg_value *v, int cmp, double c, int periodic_mask, const int32_t lo[3],
               const int32_t hi[3], int32_t *label_dev, int64_t cap, int64_t *tab_dev, double *ext_dev, int64_t *n_dev, void *scratch_dev,
               int64_t scratch_bytes);

/* ------------------------------------------------------------------ value-weighted sums per region (regions.sums, waterlily_amd/regions.py)
 * How strong the regions of a wl_regions call are: per region and column, the sum over its cells of a TERM -- the circulation,
 * the enstrophy, a weighted moment.  The sum is formed in integers, so it needs no order: the same bits on any launch shape.
 *   inputs : the box is the box of the wl_regions call that wrote label_dev (nx*ny*nz int32, -1 or a region's number < R) and
 *           n_dev (its four counts; n_dev[0] = R is read on the device).  A cell takes part when its label is r >= 0.  The
 *           columns of one call may read different fields (p and u); all of them lie on grid g.
 *   term  : w = v (power 1) or v * v (power 2), v the value of the cell formed by the device function of wl_regions (kinds as
 *           there, absval honoured; WL_R_FACE refused); term = w (moment -1) or w * (double)J_d (moment d in 0..D-1, J_d the
 *           0-based array index of the cell along axis d: the frame of tab_dev's columns 2..4).  Every operation is one IEEE
 *           double operation; nothing is contracted.
 *   scale : per column c an int32 E_c in scale_dev[c].  WL_RS_FIND: the call writes E_c = max(ilogb(M_c), WL_RS_EMIN), M_c the
 *           largest finite |term| over ALL cells with r >= 0 (not only r < cap: the result does not depend on cap), found with
 *           atomicMax on the order-preserving integer image of |term|; no finite term, or M_c == 0: E_c = WL_RS_EMIN.  over_dev
 *           is written as zeros.  WL_RS_GIVEN: scale_dev is read, not written -- the caller fixed the exponents so that the limbs
 *           of several calls or boxes can be added; a value outside WL_RS_EMIN..1023 is taken as the nearer end.  A finite term
 *           with |term| >= 2^(E_c + 1) is not added; it is counted in over_dev[c], a count over the cells with r >= 0 of the
 *           whole box.  A non-zero over_dev[c] means column c is invalid.
 *   fixed point : a finite term maps to the integer n = trunc(term * 2^(126 - E_c)), rounded toward zero: |n| < 2^127; scaling a
 *           double by a power of two is exact, only the bits below the unit 2^(E_c - 126) are cut.  With |n| = d3*2^96 +
 *           d2*2^64 + d1*2^32 + d0, 0 <= d_k < 2^32, the cell adds sign(n)*d_k to limb k of its region's column.  A box has
 *           fewer than 2^31 cells, so |limb| < 2^63.  A term that is not finite (NaN, +-inf) is not added: it adds 1 to the
 *           fifth entry.
 *   acc_dev : cap x ncol x 5 int64, acc_dev[(r*ncol + c)*5 + k]: k = 0..3 the limbs, low to high, k = 4 the count of non-finite
 *           terms.  Rows r < min(R, cap) are initialised by the call, on the device; the other rows are not written, and cells
 *           with a label >= cap are skipped (they still count for the scale and for over_dev).
 *   sum_dev : cap x ncol doubles: with N = sum_k limb_k * 2^(32 k) (a signed integer of up to 159 bits), N * 2^(E_c - 126)
 *           rounded ONCE, to nearest-even; NaN when the count of non-finite terms is not zero; N == 0 gives +0.  The unit is at
 *           least 2^-1020, so a non-zero result is never subnormal; a magnitude beyond the largest double rounds to +-inf.
 *           Hence |sum - sum of the terms| <= cells_r * 2^(E_c - 126) + ulp(sum)/2.  Terms more than 2^74 times smaller than
 *           the column's largest lose low bits; terms more than 2^127 times smaller vanish.
 *   order : none.  Integer atomics only; during a WL_RS_FIND call over_dev holds the integer images of the maxima.
 * Refused with WL_E_ARG before the device is touched: NULL g, label_dev, n_dev, cols, scale_dev, acc_dev, sum_dev or over_dev;
 * ncol outside 1..WL_RS_MAX_COLS; cap < 1; power not 1 or 2; moment outside -1..D-1; a NULL field, an unknown kind or
 * component, WL_R_FACE, a metric box outside inside(); only one of lo and hi, a bad or empty box, a box of 2^31 cells or more; a
 * buffer not aligned to its element; an unknown t or scale_mode; a z-slab grid.  Asynchronous on the library's stream: three
 * launches (WL_RS_GIVEN) or four (WL_RS_FIND), whatever the data; nothing allocated, nothing read back (csrc/wl_region_sums.h).
 * WaterLily v1.3 has no such function to override. */
typedef struct {
    wl_rg_value v;      /* the value, formed by the same device function as everywhere (absval honoured) */
    int32_t power;      /* 1: w = v;  2: w = v*v  (one IEEE double multiply) */
    int32_t moment;     /* -1: term = w;  d in 0..D-1: term = w * (double)J_d  (one more IEEE double multiply) */
} wl_rs_col;
enum { WL_RS_FIND = 0, WL_RS_GIVEN = 1 };
enum { WL_RS_MAX_COLS = 8, WL_RS_EMIN = -894 };
int wl_region_sums(wl_dtype t, const wl_grid *g, const int32_t lo[3], const int32_t hi[3], const int32_t *label_dev,
                   const int64_t *n_dev, int64_t cap, int ncol, const wl_rs_col *cols, int scale_mode, int32_t *scale_dev,
                   int64_t *acc_dev, double *sum_dev, int64_t *over_dev);

/* ------------------------------------------------------------------ snapshots (VTK write / restart,ext/WaterLilyWriteVTKExt.jl:57-66,
 * ext/WaterLilyReadVTKExt.jl:28-45).  The reference copies whole fields to the host (`a.flow.u |> Array`) and permutes the vector
 * components to the front there (components_first, :79).  Here the field's LOCAL planes klo..khi are packed on the device into
 * a dense array-of-tuples staging buffer -- dst[((kk*n1 + j)*n0 + i)*ntuple + c] = a_c[i, j, klo+kk] for c < ncomp, 0 for the
 * padding components ncomp <= c < ntuple (VTK vectors carry 3) -- which the host then moves with ONE asynchronous copy on a
 * side stream while the next time step runs; unpack is the inverse (restart).  Enqueued on the library's stream. */
int wl_snapshot_pack(wl_dtype t, const wl_grid *g, const void *a, int ncomp, int ntuple, int klo, int khi, void *dst);
int wl_snapshot_unpack(wl_dtype t, const wl_grid *g, void *a, int ncomp, int ntuple, int klo, int khi, const void *src);

/* ------------------------------------------------------------------ switches
 * Every key selects between the form of an operator the reference writes and a traffic-saving form of it that produces the
 * same bits (tests flip them one by one, and all at once); a few are tuning values.  The defaults are the measured winners;
 * round 4 retired the keys whose alternative was a recorded loss (11, 12, 20, 21, 24, 25, 28: DESIGN.md, measured dead ends).
 * A key is one of the WL_OPT_* numbers below; any other key: WL_E_ARG.  The numbers are part of the ABI: 11, 12, 20, 21, 24,
 * 25, 28, 29 belonged to retired keys and are never to be reused. */
enum {
    /* 1 = use the 16-B-vectorised z-marching 7-point kernel where it applies (default), 0 = generic range kernel */
    WL_OPT_STENCIL7_VEC = 0,
    /* 1 = fused V-cycle smoothers (default), 0 = the reference's two-pass Jacobi!/increment!/prolongate! */
    WL_OPT_SMOOTH_FUSED = 1,
    /* 1 = LDS-tiled marching conv_diff kernel (default), 0 = generic gather kernel */
    WL_OPT_CONVDIFF_TILED = 2,
    /* 1 = BDIM! uses the body-free row flags (default), 0 = general path everywhere */
    WL_OPT_BDIM_ROWFLAGS = 3,
    /* rows per thread of the vectorised 7-point kernel (a 256-thread workgroup covers 4x that many rows): 1, 2, or 0 (default)
     * = 2 on levels of >= 2^26 interior cells with an even y extent, else 1.  Same values either way. */
    WL_OPT_STENCIL7_ROWS = 4,
    /* != 0 = 16-B vectorised streaming pcg kernels (default), 0 = scalar range kernels */
    WL_OPT_PCG_VEC = 5,
    /* 1 = multigrid levels <= 4096 cells run as one single-workgroup launch per V-cycle (default), 0 = per-op launches */
    WL_OPT_COARSE_TAIL = 6,
    /* 1 = BC! as one closed-form launch (default), 0 = the reference's sequence of plane loops */
    WL_OPT_BC_FUSED = 7,
    /* 1 = pcg! applies x += alpha*eps in the direction kernel instead of the update kernel (default; one array pass less per
     * iteration, identical values), 0 = in the update kernel as the reference orders it */
    WL_OPT_PCG_DEFER_X = 8,
    /* 1 = the 7-point kernels skip the loads of L in rows whose face coefficients are all one number (rows clear of the body
     * and the domain faces; constants recorded by wl_mg_update) (default), 0 = always load L */
    WL_OPT_ROW_CONST_L = 9,
    /* 1 = inside solver! the start of pcg! (eps = r*iD, rho) is evaluated by the prolongate!+increment! kernel that has just
     * produced r (default), 0 = by pcg!'s own first kernel */
    WL_OPT_PCG_START_FUSED = 10,
    /* 1 = pcg! does not store z' = r*iD, the direction kernel recomputes it (default), 0 = stored as in the reference */
    WL_OPT_PCG_RECOMPUTE_PRECOND = 13,
    /* 1 = inside mom_step! the predictor's closing `x ./= dt` and the corrector's opening `x .*= 0.5dt` (Flow.jl:144,139) are
     * one pass over x, each rounding kept (default), 0 = two passes */
    WL_OPT_SCALE_CHAIN = 14,
    /* 1 = on levels of at most 2^25 cells pcg!'s dot products are finished by the kernel that follows (no one-workgroup
     * finalize launches inside a pcg! call; single rank) (default), 2 = on every level, 0 = separate finalize launch after
     * every dot product */
    WL_OPT_PCG_DOTS_IN_KERNEL = 15,
    /* grid size of the 7-point / streaming vector kernels in units of 1024 workgroups (defaults 4 / 16: measured at 512^3, the
     * streaming kernels gain 3-6 % from shorter z-chunks, the 7-point kernels do not) */
    WL_OPT_STENCIL7_GRID_K = 16,
    WL_OPT_STREAM_GRID_K = 17,
    /* 1 = conv_diff! evaluates each interior face flux once and shares it between the two cells (shared-flux LDS kernel on the
     * tiles / planes whose y and z faces are all interior; 64x8 tiles in Float32, 64x4 in Float64) (default), 0 = every cell
     * gathers its six fluxes */
    WL_OPT_CONVDIFF_SHARED_FLUX = 18,
    /* 1 = on levels of 2^22 .. 2^26 cells pcg! does not store z = A*eps: its update kernel is a second 7-point kernel over eps
     * that forms the same A*eps again and applies r -= alpha*(A*eps) (default; 3-D vector kernels), 3 = on every level below
     * 2^26 cells, 2 = on every level, 0 = the mult kernel always stores z */
    WL_OPT_PCG_RECOMPUTE_AEPS = 19,
    /* 1 = inside wl_mom_step / wl_project (3-D, one device) z = div(u) is formed by the residual! kernel itself, the z array is
     * neither written nor read (default), 0 = separate div pass */
    WL_OPT_DIV_IN_RESIDUAL = 22,
    /* 1 = inside wl_mom_step (3-D, x not periodic) the x-ghost cells of the interior rows that BC!(u,U) sets are written by the
     * kernel that has just produced the row (BDIM!, the velocity correction); the BC launch that follows covers the y and z
     * planes only (default), 0 = BC! writes all six planes */
    WL_OPT_XGHOST_IN_KERNEL = 23,
    /* bound of a mailbox all-reduce's wait for a peer in SECONDS of the device's wall clock (default 600; 0 = unbounded, like a
     * collective) */
    WL_OPT_MBOX_TIMEOUT_S = 26,
    /* 1 = inside wl_mom_step (3-D, no periodic direction, no convective exit) the conv_diff! kernels finish BDIM! (Flow.jl:134,
     * scale_u! :166) on the body-free x-rows themselves: the row's new velocity is stored from the registers that hold f, V is
     * not read there, and no separate pass over those rows runs (6T + 9T per cell and step less); the u0 array holds u' on
     * return (see wl_mom_step) (default), 0 = separate BDIM! pass, u0 = the copy of u */
    WL_OPT_BDIM_IN_CONVDIFF = 27,
    /* 1 = consecutive marching kernels sweep their tiles in opposite directions, each XCD starting on the lines the kernel
     * before it touched last (L2 / Infinity Cache) (default), 0 = always ascending.  Two bits: bit 0 is that switch; bit 1
     * chooses which tiles an XCD takes in a z-marching launch: clear = whole z-chunks are dealt round-robin to the eight XCDs
     * (the body's rows, which cost more, are spread over all of them), set = every XCD takes one contiguous slab of z.  So
     * 1 (default) = alternate + dealt, 3 = alternate + slabs, 0 = ascending + dealt, 2 = ascending + slabs.  Same bits in all
     * four: a tile's reduction partial keeps its slot. */
    WL_OPT_SWEEP_ALTERNATE = 30,
    /* 1 = inside the one-workgroup bottom of the V-cycle (levels of <= 4096 cells) pcg! keeps its level in registers and LDS
     * for the whole call (default), 0 = every phase goes through global memory.  Same bits either way. */
    WL_OPT_COARSE_PCG_RESIDENT = 31,
};
int wl_set_option(int key, int value);
int wl_get_option(int key, int *value);

/* ------------------------------------------------------------------ measurement support */
/* Kernel classes for launch counting and HIP-event timing (bench.py roofline leg). */
enum {
    WL_K_CONVDIFF = 0, WL_K_BDIM = 1, WL_K_BC = 2, WL_K_DIV = 3, WL_K_CORRECT = 4, WL_K_CFL = 5,
    WL_K_SCALE = 6, WL_K_RESIDUAL = 7, WL_K_JACOBI = 8, WL_K_INCREMENT = 9, WL_K_SMOOTH = 10,
    WL_K_RESTRICT = 11, WL_K_PROLONG = 12, WL_K_PCG_INIT = 13, WL_K_PCG_MULT = 14, WL_K_PCG_UPDATE = 15,
    WL_K_PCG_DIR = 16, WL_K_DOT = 17, WL_K_SCALAR = 18, WL_K_SETDIAG = 19, WL_K_RESTRICTL = 20,
    WL_K_COPY = 21, WL_K_PFORCE = 22, WL_K_MISC = 23, WL_K_COUNT = 24
};
const char *wl_kernel_name(int kclass);
/* time launches of `kclass` (-1 = none) issued for grids with >= min_cells cells, with hipEvents */
int wl_prof_select(int kclass, int64_t min_cells);
int wl_prof_reset(void);
/* launches / cells processed per class since the last reset (all classes, all levels) */
int wl_prof_counts(int kclass, int64_t *launches, int64_t *cells);
/* device and pinned-host allocations the library itself has made since it was loaded (count, bytes): a steady wl_mom_step makes
 * none (the reference bounds mom_step!'s allocations the same way, test/alloctest.jl:17-27) */
int wl_prof_allocs(int64_t *count, int64_t *bytes);
/* number of stencil launches since start-up that were split to overlap a z-slab halo exchange (comm stream) */
int wl_prof_overlapped(int64_t *count);
/* number of z-marching launches since start-up whose z-chunks were dealt round-robin to the XCDs (WL_OPT_SWEEP_ALTERNATE) */
int wl_prof_dealt(int64_t *count);
/* collectives issued by this rank since the last wl_prof_reset (z-slab runs; all zero without a communicator):
 * out[0] all-reduces, out[1] halo exchanges (one grouped send/recv batch each), out[2] send/recv pairs inside them (one per
 * component and neighbour side), out[3] all-gathers, out[4] bytes this rank sent in halo exchanges, out[5] bytes it
 * contributed to all-gathers */
int wl_prof_comm(int64_t out[6]);
int wl_prof_reset_comm(void);
/* `reps` back-to-back all-reduces of one double, issued the way the solver issues them (mailbox or communicator): microseconds
 * per all-reduce, timed on the device.  Every rank calls it with the same reps; 0 without a communicator. */
int wl_prof_allreduce_us(int reps, double *us_per_op);           /* zero these six counters only (wl_prof_reset zeroes them too) */
/* for the selected class: timed launches, their summed cells, summed milliseconds (synchronises) */
int wl_prof_timed(int64_t *launches, int64_t *cells, double *ms);

#ifdef __cplusplus
}
#endif
#endif /* WLHIP_H */
