"""Independent extended-precision reference of the operators (TEST INFRASTRUCTURE; numpy only).

Written from the operator definitions of the reference WaterLily sources (file:line cited on every function), in GATHER
form: each cell sums the fluxes through its own faces.  The CPU oracle (oracle/wlo_impl.h) uses the reference's scatter
form with a Phi scratch and rounds like the reference; this module rounds nowhere: every operator is evaluated in
np.longdouble (64-bit significand) from the T-valued inputs, and the reductions are exact (math.fsum of exact products).
It imports neither `oracle` nor `waterlily_amd`.

Every operator evaluates at an arbitrary list of cells.  A `Cells` object holds the cell indices (0-based, ghosts
included, one int array per dimension) and a getter that returns the values of a named array at any index tuple; the
same code therefore serves whole small host arrays and cells sampled out of full-size device fields.

Each operator returns (value, M): M is the same expression tree evaluated on the absolute values of every term.  A
product that evaluates the operator in T with any order of its roundings is within a few eps_T * M of `value`; the tests
check |product - value| <= K * eps_T * M with K stated per operator.  Branches (`u > 0 ? ...`, the median limiter, the
`iD == 0` test) are decided on quantities whose sign the product's rounding cannot change or are continuous in their
inputs, so a rounding difference moves the result by a rounding amount only.

Index conventions: arrays are (N1,N2[,N3]) scalars and (...,D) vectors with one ghost layer per side, extents N include
the ghosts; 0-based index q here is the reference's 1-based q+1.
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble

# K per operator: |T result - value| <= K * eps_T * M.  A T evaluation of each expression tree makes at most a handful of
# roundings, each bounded by eps_T/2 of a partial sum whose magnitude M bounds; K leaves a margin of 3-4x over the
# largest ratio measured (oracle 1.13, kernels 1.80).
K = {"conv_diff": 8, "div": 4, "bdim_f": 4, "bdim_u": 8, "flux_out": 4, "accelerate": 1, "scale_u": 1, "diag": 4,
     "iD": 8, "mult": 4, "residual": 8, "jacobi": 8, "alpha": 16, "pcg": 16, "restrict": 4, "restrictL": 4,
     "prolongate": 0,
     # the corrector's f after a whole mom_step! (mom_f below): conv_diff! within 8 eps of its M, which |dt| scales; the
     # acceleration and its rounding to T 1 (r + g, eps/2 of |r| + |g| twice); f = u0 + dt*f - V three roundings of at
     # most eps/2 of M each, rounded up to 3: 8 + 1 + 3
     "mom_f": 12,
     # the coarse V-cycle tail (wl_coarse.h) against its per-level launches: |on - off| <= K * eps_T * (the level's scale
     # of that array, test_xref_step_gpu.py).  Not the rounding bound of one expression: the two group pcg!'s Float64 dot
     # sums differently, so alpha and beta may round apart by an ulp of T and that travels through six iterations and up
     # the levels.  Largest measured: Float32 0 (bit-identical), Float64 4.95; K = 16 is the 3x margin of the others
     "coarse_tail": 16,
     # r + A x = rhs on the level below Vcycle!'s: x and r take 8 updates (smoother, prolongate!+increment!, six pcg!
     # iterations), each rounds x, A*delta (mult: 4) and r; 8 * (1 + 4 + 1) = 48, rounded up to 64
     "coarse_inv": 64,
     # exitBC! (exit_bc below): v = u0 - (U*dt)*(u0 - u0[I-d1]) four roundings (U*dt, the difference, the product, the
     # subtraction), the imbalance three (the sum's cast to T, the division, - U), the final subtraction one; the Float64 sum
     # of n terms adds n*2^-53 of |v|, nothing at these sizes: about 2.5 eps M, K the 3-4x margin of the table
     "exit_bc": 8,
     # u - L*(x[I] - x[I-dc]) (correct below): three roundings, each at most eps/2 of M
     "correct": 4,
     # the velocity a whole mom_step! leaves (mom_u below): bdim_u 8 + correct 4, composed as mom_f is
     "mom_u": 12,
     # x .*= s; x ./= s (Flow.jl:139,144) on a cell nothing else writes: two roundings of |p|; the four passes of a whole
     # step (*dt, /dt, *0.5dt, /0.5dt): four ("scale_x4")
     "scale_x": 2, "scale_x4": 4,
     # the search direction of pcg! iteration k >= 2 (pcg_step_ref below), eps = beta*eps + r*iD with beta = rho1/rho0 in T:
     # six roundings -- rho1 and rho0 to T, the T division, z' = r*iD, beta*eps, the sum -- each counted as a whole eps of
     # M = |beta*eps| + |r*iD| (rho's terms r*(r*iD) share iD's sign, so the roundings of z' inside the sums, eps/2 of rho
     # each, fit into the halves left over): 6, rounded up to 8.  (Float32 sums rho in double; a Float64 sum rounds as it
     # goes, which the count leaves out: the kernels' tree sums stay well inside, the oracle's one sequential sum does so
     # up to about a thousand cells -- DESIGN.md has the figures)
     "pcg_eps": 8}


def K_project(n: int) -> int:
    """K of project_defect after a solve of n solver! iterations: the initial residual 8 (K["residual"]), and per iteration
    eight updates of x and r (Vcycle!'s smoother, prolongate!+increment!, six pcg! iterations) at 8 each, as derived next to
    K["coarse_inv"]: 8 + 64 n"""
    return 8 + 64 * int(n)


def eps(T) -> float:
    return float(np.finfo(np.dtype(T)).eps)


class Cells:
    """The cells `idx` (tuple of D int arrays) of a grid of extents N, reading arrays of extents NA (default N; the fine
    grid for the restrictions) through get(name, index_tuple, comp) -> values.  Indices outside [0, NA) are clamped
    before the fetch: the operators mask what such a fetch feeds."""

    def __init__(self, idx, N, get, NA=None):
        self.idx = tuple(np.asarray(a, dtype=np.int64) for a in idx)
        self.N = tuple(int(n) for n in N)
        self.NA = self.N if NA is None else tuple(int(n) for n in NA)
        self.D = len(self.N)
        self.get = get

    def __len__(self):
        return len(self.idx[0])

    def at(self, name, ix, c=None) -> np.ndarray:
        ix = tuple(np.clip(a, 0, n - 1) for a, n in zip(ix, self.NA))
        return np.asarray(self.get(name, ix, c), dtype=LD)

    def __call__(self, name, off=(), c=None) -> np.ndarray:
        off = tuple(off) + (0,) * (self.D - len(off))
        return self.at(name, tuple(a + o for a, o in zip(self.idx, off)), c)


def host_cells(arrays: dict, idx=None, N=None, NA=None) -> Cells:
    """Cells over host numpy arrays (idx=None: every cell of an array of extents N)."""
    if idx is None:
        idx = tuple(a.ravel(order="F") for a in np.meshgrid(*[np.arange(n) for n in N], indexing="ij"))

    def get(name, ix, c):
        a = arrays[name]
        if a.ndim > len(ix) + 1:                                       # mu1[I,i,j]: component i + D*j
            a = a.reshape(a.shape[:len(ix)] + (-1,), order="F")
        return a[ix + ((c,) if c is not None else ())]
    if N is None:
        N = next(iter(arrays.values())).shape[:len(idx)]
    return Cells(idx, N, get, NA)


def dl(d, D, k=1):
    """offset k along dimension d"""
    return tuple(k if q == d else 0 for q in range(D))


# ------------------------------------------------------------------------------------------------ util.jl

def _pl(N, q, j):
    return tuple(q if d == j else slice(None) for d in range(len(N)))


def BC(a: np.ndarray, A, saveexit=False, perdir=()):
    """util.jl:192-210 BC!(a,A,saveexit,perdir) on a host vector field (N..., n): the reference's plane loops replayed in
    their (i, j) order on a copy -- later loops read ghost cells that earlier ones wrote, so edges and corners hold what the
    reference leaves there.  Pure copies and assignments (A[i] converted to the array's type): the result is exact."""
    a = np.array(a, order="F", copy=True)
    N, n = a.shape[:-1], a.shape[-1]
    for i in range(n):
        for j in range(n):
            pl = lambda q: _pl(N, q, j) + (i,)
            if j in perdir:
                a[pl(0)] = a[pl(N[j] - 2)]                   # :196  a[I,i] = a[CIj(j,I,N[j]-1),i] over slice(N,1,j)
                a[pl(N[j] - 1)] = a[pl(1)]                   # :197  a[I,i] = a[CIj(j,I,2),i] over slice(N,N[j],j)
            elif i == j:
                for q in (0, 1):                             # :200-202  Dirichlet on planes 1 and 2
                    a[pl(q)] = A[i]
                if not saveexit or i > 0:                    # :203  and on plane N unless the exit is saved
                    a[pl(N[j] - 1)] = A[i]
            else:
                a[pl(0)] = a[pl(1)]                          # :205  a[I,i] = a[I+δ(j,I),i] over slice(N,1,j)
                a[pl(N[j] - 1)] = a[pl(N[j] - 2)]            # :206  a[I,i] = a[I-δ(j,I),i] over slice(N,N[j],j)
    return a


def perBC(a: np.ndarray, perdir=()):
    """util.jl:227-231 perBC!(a,perdir) on a host scalar field, the loops in perdir's order on a copy: exact."""
    a = np.array(a, order="F", copy=True)
    N = a.shape
    for j in perdir:
        a[_pl(N, 0, j)] = a[_pl(N, N[j] - 2, j)]            # :229
        a[_pl(N, N[j] - 1, j)] = a[_pl(N, 1, j)]            # :230
    return a


def _sum_ld(v) -> np.longdouble:
    """the sum of longdouble values, exact up to one rounding to longdouble: every value split into two float64 (its
    64-bit significand fits), math.fsum for the leading float64, again for what that left"""
    v = np.asarray(v, LD).ravel()
    hi = v.astype(np.float64)
    parts = np.concatenate([hi, (v - hi).astype(np.float64)]).tolist()
    s0 = math.fsum(parts)
    return LD(s0) + LD(math.fsum(parts + [-s0]))


def exit_bc(C: Cells, U, dt, correction=True):
    """util.jl:216-222 exitBC!(u,u⁰,U,Δt) at the exit cells C (0-based x index N1-1, every other index inside; ALL of
    them: the imbalance is their mean): v = u⁰ - U*Δt*(u⁰ - u⁰[I-δ1]) (:219), ∮u = sum(v)/n - U (:220, the sum exact),
    result v - ∮u (:221).  Reads "u0" (component 0); U = U[1].  M = M1 + mean(M1) + |mean v| + |U| with
    M1 = |u⁰| + |U*Δt|*(|u⁰| + |u⁰[I-δ1]|).  correction=False leaves :220-221 out (the tests' control)."""
    U, dt = LD(U), LD(dt)
    a, b = C("u0", (), 0), C("u0", dl(0, C.D, -1), 0)
    v = a - U * dt * (a - b)
    M1 = abs(a) + abs(U * dt) * (abs(a) + abs(b))
    n = len(C)
    mean = _sum_ld(v) / n
    M = M1 + _sum_ld(M1) / n + abs(mean) + abs(U)
    return (v - (mean - U) if correction else v), M


# ------------------------------------------------------------------------------------------------ Flow.jl

def median(a, b, c):
    """Flow.jl:25-34 (value, M) on (value, M) pairs: the result is one of the arguments, its bound the largest."""
    (av, am), (bv, bm), (cv, cm) = a, b, c
    gt = av > bv
    v = np.where(gt, np.where(bv >= cv, bv, np.where(av > cv, cv, av)),
                 np.where(bv <= cv, bv, np.where(av < cv, cv, av)))
    return v, np.maximum(np.maximum(am, bm), cm)


def quick(u, c, d):
    """Flow.jl:4  quick(u,c,d) = median((5c+2d-u)/6, c, median(10c-9u, c, d))"""
    au, ac, ad = abs(u), abs(c), abs(d)
    a1 = ((5 * c + 2 * d - u) / 6, (5 * ac + 2 * ad + au) / 6)
    a2 = median((10 * c - 9 * u, 10 * ac + 9 * au), (c, ac), (d, ad))
    return median(a1, (c, ac), a2)


def _face_flux(C: Cells, j: int, c: int, F, nu, kind: str):
    """Flux of component c through the j-face at cell index F (Flow.jl:45 / :54 / :55 / :58-59 before the sign of the
    upper boundary): phi-weighted upwind term minus nu * d(u_c)/dx_j.  kind: 'u' (ϕu, :6), 'L' (ϕuL, :8), 'R' (ϕuR, :9),
    'P' (ϕuP, :7 with the far-upwind point at j-index N_j-2)."""
    D = C.D
    sh = lambda k: tuple(a + o for a, o in zip(F, dl(j, D, k)))
    uf_a, uf_b = C.at("u", F, j), C.at("u", tuple(a - o for a, o in zip(F, dl(c, D))), j)
    uf, Muf = (uf_a + uf_b) * LD(0.5), (abs(uf_a) + abs(uf_b)) * LD(0.5)   # ϕ(i,CI(I,j),u)  Flow.jl:3
    b, cc, d = C.at("u", sh(-1), c), C.at("u", F, c), C.at("u", sh(1), c)
    if kind == "P":
        Ip = tuple(np.full_like(a, C.N[j] - 3) if q == j else a for q, a in enumerate(F))
        a = C.at("u", Ip, c)
    else:
        a = C.at("u", sh(-2), c)
    qp, qn = quick(a, b, cc), quick(d, cc, b)
    ph = ((cc + b) * LD(0.5), (abs(cc) + abs(b)) * LD(0.5))              # ϕ(j,I,u_c)
    pos = uf > 0
    if kind == "L":
        lam = (np.where(pos, ph[0], qn[0]), np.where(pos, ph[1], qn[1]))
    elif kind == "R":
        neg = uf < 0
        lam = (np.where(neg, ph[0], qp[0]), np.where(neg, ph[1], qp[1]))
    else:
        lam = (np.where(pos, qp[0], qn[0]), np.where(pos, qp[1], qn[1]))
    nu = LD(nu)
    v = uf * lam[0] - nu * (cc - b)
    M = Muf * lam[1] + abs(nu) * (abs(cc) + abs(b))
    return v, M


def conv_diff(C: Cells, c: int, nu, perdir=()):
    """Flow.jl:36-60 conv_diff!, component c of r at the cells of C, gather form: r[I,c] = sum_j (flux through the lower
    j-face of I) - (flux through its upper j-face).  Which faces exist follows the loop ranges: lower boundary faces on
    j-index 2 (slice(N,2,j,2), :54/:58), interior faces 3:N-1 (inside_u(N,j), :45-47), upper boundary faces on N (:55/:60),
    every other index in 2:N -- so r is 0 on the cells with a 1-based index 1 and gets no j-fluxes where its j-index is N."""
    D = C.D
    v = np.zeros(len(C), LD)
    M = np.zeros(len(C), LD)
    alive = np.all([a >= 1 for a in C.idx], axis=0)
    for j in range(D):
        m, N = C.idx[j], C.N[j]
        per = j in perdir
        has = alive & (m <= N - 2)                          # cell's lower face 1-based m+1 in 2:N-1, upper m+2 in 3:N
        lo_kind = "P" if per else "L"
        for sgn, F, f in ((1, C.idx, m), (-1, tuple(a + o for a, o in zip(C.idx, dl(j, D))), m + 1)):
            fv = np.zeros(len(C), LD)
            fM = np.zeros(len(C), LD)
            for kind, sel in (("u", (f >= 2) & (f <= N - 2)), (lo_kind, f == 1),
                              ("R" if not per else "P", f == N - 1)):
                sel = sel & has
                if not np.any(sel):
                    continue
                FF = F
                if per and kind == "P" and np.any(f == N - 1):
                    # :60  r[I-δ(j),i] -= Φ[CIj(j,I,2)]: the top face repeats the flux of the bottom face
                    FF = tuple(np.where(f == N - 1, 1, a) if q == j else a for q, a in enumerate(F))
                fx = _face_flux(C, j, c, FF, nu, kind)
                fv = np.where(sel, fx[0], fv)
                fM = np.where(sel, fx[1], fM)
            v += sgn * fv
            M += fM
    return v, M


def div(C: Cells):
    """Flow.jl:11-17 with ∂ of Flow.jl:2: sum_i u[I+δi,i] - u[I,i]"""
    v = np.zeros(len(C), LD)
    M = np.zeros(len(C), LD)
    for i in range(C.D):
        a, b = C("u", dl(i, C.D), i), C("u", (), i)
        v += a - b
        M += abs(a) + abs(b)
    return v, M


def flux_out(C: Cells):
    """Flow.jl:176-182 (the σ that CFL, :172-175, maximises)"""
    v = np.zeros(len(C), LD)
    for i in range(C.D):
        v += np.maximum(LD(0), C("u", dl(i, C.D), i)) + np.maximum(LD(0), -C("u", (), i))
    return v, v.copy()


def bdim_f(C: Cells, c: int, dt, off=()):
    """Flow.jl:133  f = u⁰ + dt*f - V (every cell) at C's cells shifted by `off`"""
    u0, f, V = C("u0", off, c), C("f", off, c), C("V", off, c)
    dt = LD(dt)
    return u0 + dt * f - V, abs(u0) + abs(dt) * abs(f) + abs(V)


def bdim_u(C: Cells, c: int, dt, stored=False):
    """Flow.jl:134 with μddn of Flow.jl:18-24: u += 0.5*sum_j μ₁[I,c,j]*(f[I+δj]-f[I-δj]) + V + μ₀*f, f from :133.
    Inside cells only (inside_u(size(p))).  stored=True is :134 alone: "f" is read as the array holds it after :133, ghost
    cells included, instead of being recomposed from u0 (dt is not used then)."""
    D = C.D
    s = np.zeros(len(C), LD)
    Ms = np.zeros(len(C), LD)

    def f_at(off=()):
        if not stored:
            return bdim_f(C, c, dt, off)
        v = C("f", off, c)
        return v, abs(v)
    for j in range(D):
        m1 = C("mu1", (), c + D * j)
        fp, Mp = f_at(dl(j, D))
        fm, Mm = f_at(dl(j, D, -1))
        s += m1 * (fp - fm)
        Ms += abs(m1) * (Mp + Mm)
    f0, M0 = f_at()
    u, V, mu0 = C("u", (), c), C("V", (), c), C("mu0", (), c)
    return u + LD(0.5) * s + V + mu0 * f0, abs(u) + LD(0.5) * Ms + abs(V) + abs(mu0) * M0


def mom_f(C: Cells, c: int, nu, dt, g=0.0, perdir=()):
    """Flow.jl:164-166 + :133: the f that one mom_step! leaves behind -- the corrector's BDIM! value
        f = u_start + dt * (conv_diff(u') + g_corr) - V
    at C's cells.  C reads "u" = u' (the predictor's projected velocity, ghost cells as BC! left them), "us" = u_start (the
    velocity the step started from: Flow.jl:154 copied it into u0) and "V".  M composes the bounds of conv_diff, accelerate
    and bdim_f: |u_start| + |dt| * (M_conv_diff + |g|) + |V|."""
    cv, cM = conv_diff(C, c, nu, perdir)
    us, V = C("us", (), c), C("V", (), c)
    dt, g = LD(dt), LD(g)
    return us + dt * (cv + g) - V, abs(us) + abs(dt) * (cM + abs(g)) + abs(V)


def accelerate(C: Cells, c: int, g):
    """Flow.jl:68-70  r[..,i] .+= g_i (every cell)"""
    r = C("r", (), c)
    return r + LD(g), abs(r) + abs(LD(g))


def scale_u(C: Cells, c: int, s):
    """Flow.jl:170  u *= scale over inside cells"""
    u = C("u", (), c)
    return u * LD(s), abs(u * LD(s))


# ------------------------------------------------------------------------------------------------ Poisson.jl

def diag(C: Cells):
    """Poisson.jl:48-54  D[I] = -sum_i (L[I,i] + L[I+δi,i])"""
    v = np.zeros(len(C), LD)
    M = np.zeros(len(C), LD)
    for i in range(C.D):
        a, b = C("L", (), i), C("L", dl(i, C.D), i)
        v -= a + b
        M += abs(a) + abs(b)
    return v, M


def inv_diag(Dv, DM, T):
    """Poisson.jl:44  iD = abs2(D) < 2eps(T) ? 0 : inv(D).  (value, M) with M = |1/D| * (1 + DM/|D|): the bound of 1/D under
    a relative perturbation DM/|D| of D.  Cells whose exact D sits within the rounding of the threshold have M = inf
    (either answer is right) -- the tests keep away from them."""
    e = LD(eps(T))
    with np.errstate(divide="ignore", invalid="ignore"):
        zero = Dv * Dv < 2 * e
        v = np.where(zero, LD(0), 1 / np.where(zero, LD(1), Dv))
        near = abs(Dv * Dv - 2 * e) <= 8 * e * (DM * DM + abs(Dv * Dv))
        M = np.where(zero, LD(0), abs(v) * (1 + DM / abs(np.where(zero, LD(1), Dv))))
    return v, np.where(near, LD(np.inf), M)


def mult(C: Cells, x="x"):
    """Poisson.jl:69-75  z[I] = x[I]*D[I] + sum_i x[I-δi]*L[I,i] + x[I+δi]*L[I+δi,i]  (D as stored)"""
    D = C.D
    xv, Dv = C(x), C("D")
    v, M = xv * Dv, abs(xv * Dv)
    for i in range(D):
        a = C(x, dl(i, D, -1)) * C("L", (), i)
        b = C(x, dl(i, D)) * C("L", dl(i, D), i)
        v += a + b
        M += abs(a) + abs(b)
    return v, M


def residual_local(C: Cells):
    """Poisson.jl:93  r = iD == 0 ? 0 : z - A x   (before the mean shift)"""
    Av, AM = mult(C)
    z, iD = C("z"), C("iD")
    return np.where(iD == 0, LD(0), z - Av), np.where(iD == 0, LD(0), abs(z) + AM)


def jacobi_increment(C: Cells):
    """Poisson.jl:110-113 + :99-103, one sweep: ϵ = r*iD; r -= A ϵ; x += ϵ.  Returns ((eps, M), (r, M), (x, M)).
    The neighbours' ϵ are r*iD at the neighbours."""
    D = C.D
    e, eM = C("r") * C("iD"), abs(C("r") * C("iD"))
    Ae, AeM = e * C("D"), eM * abs(C("D"))
    for i in range(D):
        for k, Lo in ((-1, ()), (1, dl(i, D))):
            en = C("r", dl(i, D, k)) * C("iD", dl(i, D, k))
            L = C("L", Lo, i)
            Ae += en * L
            AeM += abs(en) * abs(L)
    r, x = C("r"), C("x")
    return (e, eM), (r - Ae, abs(r) + AeM), (x + e, abs(x) + eM)


# ------------------------------------------------------------------------------------------------ Flow.jl: project!, mom_step!

def correct(C: Cells, c: int, x="x"):
    """Flow.jl:142  u[I,c] -= L[I,c]*∂(c,I,x), ∂ of Flow.jl:2: x[I] - x[I-δc].  Reads "u" (before the loop), "L" and the
    scalar `x` (the solver's solution, before `x ./= dt` of :144)."""
    u, L = C("u", (), c), C("L", (), c)
    a, b = C(x), C(x, dl(c, C.D, -1))
    return u - L * (a - b), abs(u) + abs(L) * (abs(a) + abs(b))


def dyadic(s) -> bool:
    """s is a power of two: x * s and x / s are exact"""
    return abs(math.frexp(float(s))[0]) == 0.5


def mom_u(C: Cells, c: int, dt, w=0.5, planted=False):
    """Flow.jl:166-167 with :134 and :142: the velocity one mom_step! leaves in the inside cells,
        0.5*(u' + μddn(μ₁,f) + V + μ₀*f) - L*∂c(w*dt*p)
    C reads "u" = u' (the predictor's projected velocity), the stored "f" (the corrector's :133 value, ghost cells
    included), "V", "mu0", "mu1", "L" and "p" (the final pressure: project! solved for x = p*(w*dt) and divided it out
    again, :144).  w*dt must be a power of two: then x = p*(w*dt) is the solver's x bit for bit.  The normal component on
    its 0-based plane 1 is BC!'s (util.jl:200-202), not this: the caller leaves those cells out.  (planted=True lets a
    control pass a dt that is off on purpose.)"""
    s = LD(w) * LD(dt)
    assert planted or dyadic(s), "mom_u: w*dt must be a power of two"
    bv, bM = bdim_u(C, c, dt, stored=True)
    L = C("L", (), c)
    a, b = s * C("p"), s * C("p", dl(c, C.D, -1))
    return LD(0.5) * bv - L * (a - b), LD(0.5) * bM + abs(L) * (abs(a) + abs(b))


def scale_x(C: Cells, name="p"):
    """Flow.jl:139,144  x .*= dt ... x ./= dt on a cell that nothing in between writes: the value it started with, within
    one rounding per pass of M = |p| (K["scale_x"] for one project!, K["scale_x4"] for the two of a whole step)."""
    p = C(name)
    return p, abs(p)


def project_shift(C: Cells, s, T):
    """Poisson.jl:93-96 for the solve inside project! (Flow.jl:139-140): the mean that residual! subtracts from the initial
    residual r0 = iD == 0 ? 0 : div(u) - A*(s*p), over C's cells (every inside cell); (shift, M) -- (0, M) when the mean is
    within 4 eps of 0, where the reference may skip the shift (:95 tests 2 eps on the rounded mean).  C reads "u", "p" (the
    pressure BEFORE project!), "L", "D", "iD"; s = w*dt."""
    s = LD(s)
    dv, dM = div(C)
    Ax, AM = mult(C, "p")
    live = C("iD") != 0
    r0, rM = np.where(live, dv - s * Ax, LD(0)), np.where(live, dM + abs(s) * AM, LD(0))
    n = len(C)
    sh, shM = _sum_ld(r0) / n, _sum_ld(rM) / n
    return (sh if abs(sh) > 4 * eps(T) else LD(0)), shM


def project_defect(C: Cells, s, shift=0, shiftM=0):
    """The invariant of solver! inside project! (Flow.jl:139-140): from r = z - A x - shift (Poisson.jl:93-96) every update
    x += d, r -= A d (Jacobi!, increment!, pcg!) keeps r + A x = div(u) - shift, so at every inside cell
        r_final + A*(s*p_after) - (div(u_before) - shift) = 0
    in exact arithmetic, whatever the dot products that chose the d's summed to.  Returns (defect, M) with
    M = M_div + shiftM + |s| * M_mult, the bound of the right-hand side and of A x; the check is |defect| <= K_project(n)
    * eps * M.  C reads "r", "p" (after project!: x = p*s, exact as s must be a power of two), "u" (before project!), "L",
    "D" and "iD" (where iD == 0 the residual started from 0 - shift, Poisson.jl:93, and the right-hand side is that)."""
    s = LD(s)
    assert dyadic(s), "project_defect: w*dt must be a power of two"
    dv, dM = div(C)
    Ax, AM = mult(C, "p")
    live = C("iD") != 0
    return C("r") + s * Ax - (np.where(live, dv, s * Ax) - LD(shift)), dM + LD(shiftM) + abs(s) * AM


# ------------------------------------------------------------------------------------------------ MultiLevelPoisson.jl

def restrict(C: Cells, name="b"):
    """MultiLevelPoisson.jl:3-9,33  a[I] = sum of b over up(I) = the 2^D fine cells 2I-2:2I-1 (1-based); C: COARSE cells,
    the getter reads the fine array"""
    v = np.zeros(len(C), LD)
    M = np.zeros(len(C), LD)
    D = C.D
    for corner in np.ndindex(*(2,) * D):
        ix = tuple(2 * a - 1 + o for a, o in zip(C.idx, corner))
        b = C.at(name, ix)
        v += b
        M += abs(b)
    return v, M


def restrictL(C: Cells, c: int, name="b", perdir=()):
    """MultiLevelPoisson.jl:10-16,26-32 restrictL! of component c at COARSE cells: 0.5 * the 2^(D-1) fine faces up(I,c)
    on 2:n-1, then BC!(a, 0, false, perdir) (util.jl:192-210).  Without periodic directions: planes 1, 2 and N of the
    normal direction hold 0, every other ghost cell the value of the nearest inside cell.  With them: _restrictL_per."""
    if perdir:
        return _restrictL_per(C, c, name, tuple(perdir))
    D = C.D
    cl = tuple(np.clip(a, 1, n - 2) for a, n in zip(C.idx, C.N))        # tangential zero-Neumann ghosts
    v = np.zeros(len(C), LD)
    M = np.zeros(len(C), LD)
    for corner in np.ndindex(*(2,) * D):
        if corner[c]:
            continue
        ix = tuple(2 * a - 1 + o for a, o in zip(cl, corner))
        b = C.at(name, ix, c)
        v += b
        M += abs(b)
    m = C.idx[c]
    wall = (m <= 1) | (m == C.N[c] - 1)
    return np.where(wall, LD(0), LD(0.5) * v), np.where(wall, LD(0), LD(0.5) * M)


def _restrictL_per(C: Cells, c: int, name, perdir):
    """restrictL! with periodic directions: the inside values of the whole coarse array, then BC!'s loop over j = 1..D
    for component c (util.jl:194-207) replayed as plane copies in that order -- a periodic j copies plane N-1 into ghost
    plane 1 and plane 2 into ghost plane N (the normal component's plane 2 keeps its restricted value), a wall j zeroes
    (normal) or copies the neighbour plane (tangential) -- so edges and corners hold what the reference leaves there."""
    D, N = C.D, C.N
    full = tuple(a.ravel(order="F") for a in np.meshgrid(*[np.arange(n) for n in N], indexing="ij"))
    ins = np.all([(a >= 1) & (a <= n - 2) for a, n in zip(full, N)], axis=0)
    v = np.zeros(len(full[0]), LD)
    M = np.zeros(len(full[0]), LD)
    for corner in np.ndindex(*(2,) * D):
        if corner[c]:
            continue
        ix = tuple(np.where(ins, 2 * a - 1 + o, 0) for a, o in zip(full, corner))
        b = Cells(full, N, C.get, C.NA).at(name, ix, c)
        v += np.where(ins, b, 0)
        M += np.where(ins, abs(b), 0)
    v, M = (LD(0.5) * a.reshape(N, order="F") for a in (v, M))
    for j in range(D):
        sl = lambda q: tuple(q if d == j else slice(None) for d in range(D))
        n = N[j]
        if j in perdir:
            pairs = ((0, n - 2), (n - 1, 1))
        elif j == c:
            pairs = ((0, None), (1, None), (n - 1, None))
        else:
            pairs = ((0, 1), (n - 1, n - 2))
        for dst, src in pairs:
            for a in (v, M):
                a[sl(dst)] = 0 if src is None else a[sl(src)]
    return v[C.idx], M[C.idx]


def prolongate(C: Cells, name="b"):
    """MultiLevelPoisson.jl:2,34  a[I] = b[down(I)], down(I) = (I+2)÷2 (1-based): a copy, exact.  C: FINE inside cells."""
    v = C.at(name, tuple((a + 1) // 2 for a in C.idx))
    return v, abs(v)


def vcycle_rhs(h0: dict, Nc):
    """The right-hand side Vcycle! hands to the next level (MultiLevelPoisson.jl:72-74): restrict! of the residual after
    one Jacobi!+increment! sweep, from the host arrays L, D, iD, r, x of the level before the call; (value, M) on every
    cell of the coarse grid of extents Nc (0 on its ghost cells)."""
    Ng = h0["r"].shape
    C0 = host_cells({k: h0[k] for k in ("L", "D", "iD", "r", "x")}, N=Ng)
    _, (rv, rM), _ = jacobi_increment(C0)
    ins = np.all([(w >= 1) & (w <= n - 2) for w, n in zip(C0.idx, Ng)], axis=0)
    rv, rM = (np.where(ins, a, 0).reshape(Ng, order="F") for a in (rv, rM))
    Cc = host_cells({"v": rv, "M": rM}, N=Nc, NA=Ng)
    insc = np.all([(w >= 1) & (w <= n - 2) for w, n in zip(Cc.idx, Nc)], axis=0)
    return np.where(insc, restrict(Cc, "v")[0], 0), np.where(insc, restrict(Cc, "M")[0], 0)


def coarse_defect(h: dict, rhs, rhsM):
    """r + A x - rhs at the inside cells of a level (exact, on the stored L and D) and its bound M_rhs + |A||x|: zero in
    exact arithmetic after any sequence of the updates x += d, r -= A d from x = 0, r = rhs (Jacobi!, prolongate! +
    increment!, pcg!) -- whatever the dot products that chose d summed to."""
    N = h["r"].shape
    C = host_cells({"L": h["L"], "D": h["D"], "x": h["x"], "r": h["r"]}, N=N)
    ins = np.all([(w >= 1) & (w <= n - 2) for w, n in zip(C.idx, N)], axis=0)
    Ax, AM = mult(C)
    return (C("r") + Ax - rhs)[ins], (rhsM + AM)[ins]


def pcg1_ref(L, D, iD, r):
    """One pcg! iteration (Poisson.jl:123-135, it=1) from x = 0 on whole host arrays: (alpha, M_alpha, eps, z, x1, r1)
    as (value, M) pairs; rho and z.eps are exact sums over the whole arrays."""
    Ng = r.shape
    C = host_cells({"r": r, "iD": iD}, N=Ng)
    e = (C("r") * C("iD")).reshape(Ng, order="F")
    eM = abs(e)
    Ce = host_cells({"L": L, "D": D, "e": e.astype(np.float64)}, N=Ng)
    ins = np.all([(q >= 1) & (q <= n - 2) for q, n in zip(Ce.idx, Ng)], axis=0)
    zv, zM = mult(Ce, "e")
    zv, zM = np.where(ins, zv, 0), np.where(ins, zM, 0)
    rf = r.ravel(order="F").astype(LD)
    ef = e.ravel(order="F")
    rho = np.sum(rf * ef)
    ze = np.sum(zv * ef)
    Mrho = 2 * np.sum(abs(rf) * eM.ravel(order="F"))
    Mze = 2 * np.sum(zM * eM.ravel(order="F"))
    alpha = rho / ze
    Ma = abs(alpha) * (Mrho / abs(rho) + Mze / abs(ze))
    x1 = (alpha * ef, abs(alpha) * eM.ravel(order="F") + Ma * abs(ef))
    r1 = (rf - alpha * zv, abs(rf) + abs(alpha) * zM + Ma * abs(zv))
    return (alpha, Ma), (ef, eM.ravel(order="F")), (zv, zM), x1, r1, ins


def pcg_step_ref(L, D, iD, z_up, perdir, x, r, e_prev, r_pp, e_k, T, shell=True):
    """Iteration k of pcg! (Poisson.jl:123-143) replayed on its own from stored T values.  pcg! keeps nothing between
    calls and a call of it=k leaves x_k, r_k and eps_k (the last iteration skips :140, so eps_k is the direction iteration
    k used): x = x_{k-1}, r = r_{k-1}, e_prev = eps_{k-1} are the arrays a call of it=k-1 left, r_pp = r_{k-2} those of
    it=k-2 (the start for k = 2), e_k the STORED direction of the call of it=k; k = 1: e_prev = r_pp = None.  z_up is the
    z array as uploaded: pcg! writes z inside only, and z.eps is a whole-array dot (:131), so in the ghost planes that
    perBC! fills with eps (:129) the uploaded z counts (shell=False leaves those cells out: the tests' control).

    Returns a dict of (value, M) pairs in longdouble, whole arrays flattened in Fortran order, scalars as 0-d:
      rho    rho_{k-1} = sum r*(r*iD) (:126,137), M = 2 sum |r*(r*iD)| as in pcg1_ref
      beta   rho_{k-1}/rho_{k-2} (:139; k >= 2)
      eps    beta*eps_{k-1} + r*iD (:140; k = 1: r*iD, :125), M = c*|beta*eps| + |r*iD| with c = 1 when rho's terms share
             a sign (K["pcg_eps"])
      alpha  rho_{k-1}/(z.eps_k) (:131), z = A eps_k inside from mult on perBC(e_k), the uploaded z in the ghost cells
             (K["alpha"])
      x, r   x + alpha*eps_k and r - alpha*A eps_k (:133), M as in pcg1_ref: alpha's own bound enters (K["pcg"])
    and "branch": the scalars pcg! branches on as (name, |value|, threshold, bound) -- |rho| against 10 eps_T (:127 for
    k = 1, :138 of iteration k-1 else), |alpha| against 1e-2 and 1e2 (:132); "exit": None when iteration k updates x and
    r, else ":127" / ":138" (no iteration k: n = k-1 updates were made) or ":132" (eps_k is the new direction, x and r
    stay: n = k-1); "ins": the mask of inside cells; "Aeps" = (A eps_k, M) with zeros outside, "_eps_k" and "_eps_prev" the
    two directions in longdouble (pcg_step_planted builds the controls from them)."""
    Ng = r.shape
    e = LD(eps(T))
    flat = lambda a: np.asarray(a, LD).ravel(order="F")
    rf, idf, xf = flat(r), flat(iD), flat(x)
    zp = rf * idf                                                     # z' = r*iD (:125,136)
    rho, Mrho = _sum_ld(rf * zp), 2 * _sum_ld(abs(rf * zp))
    out = {"rho": (rho, Mrho), "branch": [("rho", abs(rho), LD(10) * e, e * Mrho)], "exit": None}
    C = host_cells({"L": L, "D": D, "e": perBC(e_k, perdir)}, N=Ng)
    ins = np.all([(q >= 1) & (q <= n - 2) for q, n in zip(C.idx, Ng)], axis=0)
    out["ins"] = ins
    if abs(rho) < LD(10) * e:
        out["exit"] = ":127" if e_prev is None else ":138"
        return out
    if e_prev is None:
        out["eps"] = (zp, abs(zp))
    else:
        rp = flat(r_pp)
        tp = rp * (rp * idf)
        rho0, Mrho0 = _sum_ld(tp), 2 * _sum_ld(abs(tp))
        beta = rho / rho0
        c = (Mrho / abs(rho) + Mrho0 / abs(rho0)) / 4
        out["beta"] = (beta, c * abs(beta))
        ep = flat(e_prev)
        out["_eps_prev"] = ep
        out["eps"] = (beta * ep + zp, c * abs(beta * ep) + abs(zp))
    zv, zM = mult(C, "e")
    zg = flat(z_up) if shell else np.zeros(len(ins), LD)
    zv, zM = np.where(ins, zv, 0), np.where(ins, zM, 0)
    ef = C("e")
    ze = _sum_ld(np.where(ins, zv, zg) * ef)
    Mze = 2 * _sum_ld(np.where(ins, zM, abs(zg)) * abs(ef))
    alpha = rho / ze
    Ma = abs(alpha) * (Mrho / abs(rho) + Mze / abs(ze))
    out["alpha"] = (alpha, Ma)
    out["Aeps"] = (zv, zM)
    out["_eps_k"] = ef
    out["branch"] += [("alpha_lo", abs(alpha), LD(1e-2), K["alpha"] * e * Ma), ("alpha_hi", abs(alpha), LD(1e2), K["alpha"] * e * Ma)]
    if abs(alpha) < 1e-2 or abs(alpha) > 1e2:
        out["exit"] = ":132"
        return out
    out["x"] = (xf + alpha * ef, abs(xf) + abs(alpha) * abs(ef) + Ma * abs(ef))
    out["r"] = (rf - alpha * zv, abs(rf) + abs(alpha) * zM + Ma * abs(zv))
    return out


def pcg_step_planted(ref, what, T):
    """`ref` (of pcg_step_ref) with one planted error, for the tests' controls: what = "alpha": alpha off by
    64 K eps M_alpha/|alpha| relative, x and r recomputed with it; "beta": beta off likewise, eps recomputed."""
    out = dict(ref)
    e = LD(eps(T))
    if what == "alpha":
        (a, Ma), (xv, xM), (rv, rM), (zv, _) = ref["alpha"], ref["x"], ref["r"], ref["Aeps"]
        d = a * 64 * K["alpha"] * e * (Ma / abs(a))
        # x = x0 + alpha*eps, r = r0 - alpha*A eps: the planted alpha moves them by d*eps and -d*A eps
        out["x"] = (xv + d * ref["_eps_k"], xM)
        out["r"] = (rv - d * zv, rM)
    else:
        (b, Mb), (ev, eM) = ref["beta"], ref["eps"]
        d = b * 64 * K["pcg_eps"] * e * (Mb / abs(b))
        out["eps"] = (ev + d * ref["_eps_prev"], eM)
    return out


# ------------------------------------------------------------------------------------------------ reductions

def _two_prod(a: np.ndarray, b: np.ndarray):
    """exact a*b = p + e for float64 a, b (Dekker / Veltkamp split)"""
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    p = a * b
    sp = 134217729.0                                                   # 2^27 + 1
    with np.errstate(over="ignore", invalid="ignore"):
        ta, tb = sp * a, sp * b
        ah = ta - (ta - a)
        bh = tb - (tb - b)
    al, bl = a - ah, b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return p, e


def dot(a: np.ndarray, b: np.ndarray):
    """LinearAlgebra.dot over the whole arrays, ghost cells included (Poisson.jl:126,131,137,146): the exact sum, correctly
    rounded to float64, and M = sum |a_i b_i| (also correctly rounded)."""
    p, e = _two_prod(np.ravel(a), np.ravel(b))
    return math.fsum(np.concatenate([p, e])), math.fsum(np.abs(np.concatenate([p, e])))


def L2_inside(a: np.ndarray):
    """util.jl:68  sum(abs2, a[inside])"""
    a = a[tuple(slice(1, n - 1) for n in a.shape)]
    return dot(a, a)


def Linf(a: np.ndarray) -> float:
    """Poisson.jl:147  maximum(abs, p.r) over the whole array: exact"""
    return float(np.max(np.abs(np.asarray(a, np.float64))))


def round_to(x: float, T) -> float:
    """x (a float64 holding the correctly rounded exact value) rounded once more to T"""
    return float(np.dtype(T).type(x))


def ulps(x: float, ref: float, T) -> float:
    """|x - ref| in units of the T spacing at ref"""
    sp = float(np.spacing(np.abs(np.dtype(T).type(ref))))
    return abs(float(x) - float(ref)) / sp


def ratio(got, v, M, T) -> np.ndarray:
    """|got - v| / (eps_T * M) per cell; cells with M == 0 must be exact (ratio 0 or inf)"""
    got = np.asarray(got, dtype=LD)
    d = abs(got - v)
    e = LD(eps(T))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(M > 0, d / (e * M), np.where(d == 0, LD(0), LD(np.inf)))
    return r.astype(np.float64)


def worst(got, v, M, T) -> float:
    r = ratio(got, v, M, T)
    return float(np.max(r)) if r.size else 0.0
