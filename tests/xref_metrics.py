"""Independent extended-precision reference of the Metrics.jl read-outs (TEST INFRASTRUCTURE; numpy only): the field
metrics ke, curl, ω, |ω|, ω_θ, λ₂ and the band sums pressure_force, viscous_force, pressure_moment.

The rules are those of tests/xref.py, whose Cells, K and ratio helpers this module uses: written from the reference
sources (src/Metrics.jl, file:line on every function), evaluated in np.longdouble from the T-valued inputs, every function
returns (value, M) with M the same expression tree on absolute values, sums are exact.  It imports neither `oracle` nor
`waterlily_amd`.

Band sums.  The reference fills `df[I,:]` -- an array of the field type T -- with one term per cell and sums it in Float64
(Metrics.jl:96-99).  A product that does the same is within  eps_T/2 * |term|  per term of the exact term, plus the
Float64 accumulation of n terms in whatever order: at most  n * eps_64/2 * sum|term|.  The band functions return the
exactly summed value, M = sum over the terms of their absolute-value trees, and the tests check
    |got - value| <= (K * eps_T + n * eps_64 / 2) * M                                               (band_tol below).
For a blocked reduction n is replaced by the longest chain of additions a term passes through (tree_adds): past the launch
cap that is about 1000 instead of 2.6e5, which keeps the Float64 check able to see an accumulation done partly in T.
"""
from __future__ import annotations

import math

import numpy as np

import xref as X
from xref import LD, Cells, dl

# K per read-out, by counting the roundings of an evaluation in T (each eps_T/2 of a partial result that M bounds), with the
# margin of xref.K (about 2x the count).  sqrt, sin, cos, acos: 1 ulp (2 half-roundings) is allotted per call.
# Largest ratios measured beside each entry: the oracle's (test_xref_metrics_cpu.py prints them) and the kernels'
# (test_xref_metrics_gpu.py::test_worst_ratios_are_recorded, MI355X); for the band sums as a share of band_tol.
K = {
    # (u + u' - 2U)^2: two roundings inside the square count twice, one for the square: 2.5; D - 1 additions of the sum,
    # each of a partial sum: 1; the factor 0.125 is exact.  3.5 -> 4                        (oracle 1.14, kernels 1.53)
    "ke": 4,
    # (a - b) - (c - d): three roundings, 1.5 -> 4                                           (oracle 0.65, kernels 0.93)
    "curl": 4,
    # ω_c = ∂(k,j) - ∂(j,k): 1.5 per cross derivative (three additions; the division by 4 is exact) + 0.5: 2 eps of M_ω.
    # |Δ sqrt(sum ω²)| <= |Δω|: 2; the squares, the two additions and the sqrt (1 ulp) act on the value: 1.5/2 + 1.  3.75 -> 8
    #                                                                                        (oracle 0.61, kernels 0.99)
    "omega_mag": 8,
    # ω: 2; x = loc - center: 0.5; θ = z × x: 1.5; θ·ω: 1.5; n = |θ|: 2.5 (squares, sums, sqrt 1 ulp), carried by the
    # factor (1 + M_n/n) of M; the division and the rounding of the result to T: 1.  9 -> 16  (oracle 0.06, kernels 0.67)
    "omega_theta": 16,
    # J: 1.5 per entry; S, Ω: 0.5; each product of S² and Ω² carries both factors (4) and its own rounding (0.5), the sum of
    # six terms 2.5: 7 eps of the element-wise bound, whose Frobenius norm is M (Weyl).  The symmetric eigenvalue
    # computations, the product's and numpy's: 4 each (backward stable, a few eps_64 ||A||, at most M); result to T: 0.5.
    # 15.5 -> 16                                                                             (oracle 0.50, kernels 0.96)
    "lambda2": 16,
    # p * nds in Float64 (0.5 eps_64), rounded to T (0.5): 1                                  (oracle 0.43 of the bound, kernels 0.43 of the bound)
    "pforce": 1,
    # ∂(i,j) + ∂(j,i): 1.5 each + 0.5: 2; times ν: 0.5; the Float64 product with nds: eps_64; to T: 0.5.  3 -> 4
    #                                                                                        (oracle 0.12 of the bound, kernels 0.07 of the bound)
    "vforce": 4,
    # r = loc - x₀: 0.5 eps_64; the cross product: 1.5; times p: 0.5; to T: 0.5.  3 -> 4      (oracle 0.16 of the bound, kernels 0.08 of the bound)
    "pmoment": 4,
}


# ------------------------------------------------------------------------------------------------ field metrics

def dudx(C: Cells, a: int, b: int, name="u"):
    """Metrics.jl:28-30  ∂(i,j,I,u): ∂u_a/∂x_b at the centre of cell I; a == b is Flow.jl:2 (u[I+δa,a] - u[I,a]), the
    cross terms average the four faces around the centre: (u[I+δb,a] + u[I+δb+δa,a] - u[I-δb,a] - u[I-δb+δa,a]) / 4"""
    D = C.D
    if a == b:
        p, m = C(name, dl(a, D), a), C(name, (), a)
        return p - m, abs(p) + abs(m)
    ob, oa = np.array(dl(b, D)), np.array(dl(a, D))
    t = [C(name, tuple(ob), a), C(name, tuple(ob + oa), a), C(name, tuple(-ob), a), C(name, tuple(-ob + oa), a)]
    return (t[0] + t[1] - t[2] - t[3]) / 4, (abs(t[0]) + abs(t[1]) + abs(t[2]) + abs(t[3])) / 4


def ke(C: Cells, U=None):
    """Metrics.jl:19-21  ke(I,u,U) = 0.125 * sum_i |u[I,i] + u[I+δi,i] - 2U_i|²"""
    v = np.zeros(len(C), LD)
    M = np.zeros(len(C), LD)
    for i in range(C.D):
        a, b = C("u", (), i), C("u", dl(i, C.D), i)
        Ui = LD(0) if U is None else LD(U[i])
        v += (a + b - 2 * Ui) ** 2
        M += (abs(a) + abs(b) + 2 * abs(Ui)) ** 2
    return LD(0.125) * v, LD(0.125) * M


def curl(C: Cells, i: int):
    """Metrics.jl:54 with permute (:7-10) and the backward difference of Flow.jl:1 on one component:
    curl(i,I,u) = (u[I,k] - u[I-δj,k]) - (u[I,j] - u[I-δk,j]),  j = i+1, k = i+2 cyclically.  In 2-D only i = 2 exists."""
    j, k = (i + 1) % 3, (i + 2) % 3
    D = C.D
    a, b = C("u", (), k), C("u", dl(j, D, -1), k)
    c, d = C("u", (), j), C("u", dl(k, D, -1), j)
    return (a - b) - (c - d), abs(a) + abs(b) + abs(c) + abs(d)


def omega(C: Cells):
    """Metrics.jl:60  ω_i = ∂(k,j,I,u) - ∂(j,k,I,u): (D, n) values and bounds"""
    out = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        (p, Mp), (q, Mq) = dudx(C, k, j), dudx(C, j, k)
        out.append((p - q, Mp + Mq))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def omega_mag(C: Cells):
    """Metrics.jl:66  |ω| = √(ω'ω) (norm2, :6)"""
    w, Mw = omega(C)
    return np.sqrt((w * w).sum(0)), np.sqrt((Mw * Mw).sum(0))


def omega_theta(C: Cells, z, center):
    """Metrics.jl:73-77  θ = z × (loc(0,I) - center), n = |θ|, ω_θ = n <= eps(n) ? 0 : θ'ω / n.  loc(0,I) = I - 1.5 in
    1-based indices (util.jl:160): the 0-based index minus 0.5.  Returns (value, M, n): n == 0 on the axis (value and M
    0 there: exact); M carries the bound of 1/n like xref.inv_diag: (sum M_θ M_ω / n) * (1 + M_n / n)."""
    w, Mw = omega(C)
    z = [LD(q) for q in z]
    x = [C.idx[d].astype(LD) - LD(0.5) - LD(center[d]) for d in range(3)]
    Mx = [abs(C.idx[d].astype(LD) - LD(0.5)) + abs(LD(center[d])) for d in range(3)]
    th, Mth = [], []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        th.append(z[j] * x[k] - z[k] * x[j])
        Mth.append(abs(z[j]) * Mx[k] + abs(z[k]) * Mx[j])
    th, Mth = np.stack(th), np.stack(Mth)
    n = np.sqrt((th * th).sum(0))
    Mn = np.sqrt((Mth * Mth).sum(0))
    on = n == 0
    ns = np.where(on, LD(1), n)
    v = np.where(on, LD(0), (th * w).sum(0) / ns)
    M = np.where(on, LD(0), (Mth * Mw).sum(0) / ns * (1 + Mn / ns))
    return v, M, n


def lambda2(C: Cells):
    """Metrics.jl:40-44  J = [∂(i,j,I,u)], S = (J+J')/2, Ω = (J-J')/2, λ₂ = eigvals(Hermitian(S²+Ω²))[2].  S²+Ω² is formed
    in longdouble and rounded once to Float64, its middle eigenvalue taken by numpy.linalg.eigvalsh (LAPACK: backward
    stable, so without the loss of the trigonometric closed form at coinciding eigenvalues).  By Weyl's inequality an error
    δ of the matrix moves an eigenvalue by at most ||δ||₂ <= ||δ||_F: M is the Frobenius norm of the element-wise bound of
    S²+Ω², built from the bounds of J (|S|, |Ω| <= (M_J + M_J')/2 =: B, so |S²+Ω²| <= 2 B B)."""
    n = len(C)
    J = np.zeros((n, 3, 3), LD)
    MJ = np.zeros((n, 3, 3), LD)
    for a in range(3):
        for b in range(3):
            J[:, a, b], MJ[:, a, b] = dudx(C, a, b)
    Jt = J.transpose(0, 2, 1)
    S, Om = (J + Jt) / 2, (J - Jt) / 2
    A = np.einsum("nac,ncb->nab", S, S) + np.einsum("nac,ncb->nab", Om, Om)
    A = (A + A.transpose(0, 2, 1)) / 2
    B = (MJ + MJ.transpose(0, 2, 1)) / 2
    MA = 2 * np.einsum("nac,ncb->nab", B, B)
    v = np.linalg.eigvalsh(A.astype(np.float64))[:, 1] if n else np.zeros(0)
    return v.astype(LD), np.sqrt((MA * MA).sum((1, 2)))


# ------------------------------------------------------------------------------------------------ band sums

def _exact_sum(t) -> float:
    """the exact sum of longdouble terms, rounded once to Float64: each term splits exactly into two Float64"""
    t = np.asarray(t, LD)
    hi = t.astype(np.float64)
    lo = (t - hi).astype(np.float64)
    return math.fsum(np.concatenate([hi, lo]))


def _band(vals, Ms):
    return (np.array([_exact_sum(v) for v in vals]), np.array([_exact_sum(m) for m in Ms]))


def band_cells(arrays: dict, idx, Ng) -> Cells:
    """Cells over host arrays at the band's cells: idx are column-major linear indices into the extents Ng"""
    return X.host_cells(arrays, idx=np.unravel_index(np.asarray(idx, np.int64), Ng, order="F"), N=Ng)


def pressure_force(p, idx, nds):
    """Metrics.jl:96-99  df[I,:] = p[I] * nds(I), summed over the cells: (value[D], M[D]) over the band (idx, nds[n,D])"""
    C = band_cells({"p": p}, idx, p.shape)
    pv = C("p")
    nds = np.asarray(nds, np.float64).reshape(len(C), C.D).astype(LD)
    return _band([pv * nds[:, c] for c in range(C.D)], [abs(pv * nds[:, c]) for c in range(C.D)])


def viscous_force(u, nu, idx, nds):
    """Metrics.jl:116-119 with ∇²u of :107-108: df[I,i] = sum_j -ν (∂(i,j,I,u) + ∂(j,i,I,u)) nds_j(I)"""
    Ng = u.shape[:-1]
    C = band_cells({"u": u}, idx, Ng)
    D = C.D
    nds = np.asarray(nds, np.float64).reshape(len(C), D).astype(LD)
    nu = LD(nu)
    d = {(a, b): dudx(C, a, b) for a in range(D) for b in range(D)}
    vals, Ms = [], []
    for i in range(D):
        v = np.zeros(len(C), LD)
        M = np.zeros(len(C), LD)
        for j in range(D):
            v += -nu * (d[i, j][0] + d[j, i][0]) * nds[:, j]
            M += abs(nu) * (d[i, j][1] + d[j, i][1]) * abs(nds[:, j])
        vals.append(v)
        Ms.append(M)
    return _band(vals, Ms)


def pressure_moment(p, x0, idx, nds):
    """Metrics.jl:137-140  df[I,:] = p[I] * cross(loc(0,I) - x₀, nds(I)).  3-D: the three components.  2-D: the cross
    product of two 2-vectors is the scalar r_x n_y - r_y n_x, which the broadcast `df[I,:] .= ` writes into both columns, so
    the reference returns that one moment twice; wl_pmoment's out[:2] holds it twice in the same way."""
    C = band_cells({"p": p}, idx, p.shape)
    D = C.D
    pv = C("p")
    nds = np.asarray(nds, np.float64).reshape(len(C), D).astype(LD)
    r = [C.idx[d].astype(LD) - LD(0.5) - LD(x0[d]) for d in range(D)]
    Mr = [abs(C.idx[d].astype(LD) - LD(0.5)) + abs(LD(x0[d])) for d in range(D)]
    if D == 2:
        v = pv * (r[0] * nds[:, 1] - r[1] * nds[:, 0])
        M = abs(pv) * (Mr[0] * abs(nds[:, 1]) + Mr[1] * abs(nds[:, 0]))
        return _band([v, v], [M, M])
    vals, Ms = [], []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        vals.append(pv * (r[j] * nds[:, k] - r[k] * nds[:, j]))
        Ms.append(abs(pv) * (Mr[j] * abs(nds[:, k]) + Mr[k] * abs(nds[:, j])))
    return _band(vals, Ms)


def tree_adds(n, cap, block=256):
    """the longest chain of Float64 additions a term passes through in a blocked reduction of n terms: the grid-stride loop
    of one thread (ceil(n / (blocks * block)) terms), log2(block) levels of the block's tree, and the sum over the blocks'
    partials in whatever order (at most `blocks` additions), with blocks = min(ceil(n / block), cap)"""
    if n <= 0:
        return 0
    blocks = min(-(-n // block), cap)
    return -(-n // (blocks * block)) + int(math.log2(block)) + blocks


def band_tol(name, n, M, T, adds=None):
    """the bound of a band sum of n terms (module docstring).  `adds`: the longest chain of Float64 additions a term
    passes through (default n: a serial sum, the oracle's and the reference's); a blocked reduction passes tree_adds"""
    adds = n if adds is None else adds
    return (K[name] * X.eps(T) + adds * X.eps(np.float64) / 2) * np.asarray(M, np.float64)


def band_ratio(name, got, v, M, n, T, adds=None) -> float:
    """max over the components of |got - v| / band_tol; 0 where both vanish, inf where only the bound does"""
    tol = band_tol(name, n, M, T, adds)
    d = np.abs(np.asarray(got, np.float64) - v)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, d / tol, np.where(d == 0, 0.0, np.inf))
    return float(np.max(r))


# ------------------------------------------------------------------------------------------------ inputs

KINDS = ["random", "ties", "scaled-up", "scaled-down"]                     # the xref_inputs.field kinds the metrics run on
SPECIAL = ["uniform", "diagonal", "rotation", "shear", "rotation-noise", "shear-noise"]       # special_fields below
X0 = (3.3, -1.7, 2.1)                                                      # pressure_moment's x₀: asymmetric, off the half-integers


def inside(C, Ng):
    return np.all([(x >= 1) & (x <= n - 2) for x, n in zip(C.idx, Ng)], axis=0)


def synthetic_band(Ng, nband, seed):
    """`nband` inside cells of a grid of extents Ng (column-major linear indices; the cells next to every ghost layer come
    first, then random ones, repeated when nband exceeds the grid) and nds uniform in [-1, 1]"""
    rng = np.random.default_rng(seed)
    D = len(Ng)
    sub = np.stack(np.meshgrid(*[np.arange(1, n - 1) for n in Ng], indexing="ij")).reshape(D, -1)
    edge = np.any([(s == 1) | (s == n - 2) for s, n in zip(sub, Ng)], axis=0)
    lin = np.ravel_multi_index(tuple(sub), Ng, order="F")
    first = np.concatenate([rng.permutation(lin[edge]), rng.permutation(lin[~edge])])
    idx = first[:nband] if nband <= first.size else np.concatenate([first, rng.choice(lin, nband - first.size)])
    return idx.astype(np.int64), rng.random((nband, D)) * 2 - 1


def linear_field(Ng, T, A, b=(0.0, 0.0, 0.0), noise=0.0, seed=0):
    """u_c = (A x + b)_c sampled at the face positions loc(c,I) (util.jl:160: the 0-based index minus 0.5, minus another
    0.5 along c), plus uniform noise of the given amplitude, rounded to T"""
    D = len(Ng)
    ix = np.indices(Ng).astype(np.float64) - 0.5
    u = np.zeros(Ng + (D,))
    rng = np.random.default_rng(seed)
    for c in range(D):
        x = ix.copy()
        x[c] -= 0.5
        u[..., c] = np.tensordot(np.asarray(A, np.float64)[c, :D], x, axes=(0, 0)) + b[c]
        if noise:
            u[..., c] += noise * (2 * rng.random(Ng) - 1)
    return np.asfortranarray(u.astype(T))


def _skew(a):
    return np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])


def special_fields(Ng, T, seed=0, scale=1.0):
    """The fields on which λ₂, ω and curl take their special paths, {name: u}:
      uniform     u_c constant: J ≡ 0, so λ₂, ω and curl are exactly 0
      diagonal    u_c a function of x_c alone: S²+Ω² is diagonal (λ₂ sorts the diagonal, no rotation)
      rotation    solid rotation 0.7 a × x about the tilted axis a: S²+Ω² has a double eigenvalue -0.49, which is λ₂
      shear       0.7 a b' x with a ⊥ b, both tilted: S²+Ω² = 0 in exact arithmetic, a triple eigenvalue
      *-noise     the last two with noise of 2^-30: the eigenvalues split by that much
    `scale` multiplies the rate 0.7 of the last four (the tests' control)."""
    rng = np.random.default_rng(seed)
    a = np.array([0.48, -0.6, 0.64])                                   # a unit vector, no component zero
    b = np.cross(a, [0.3, 0.9, -0.2])
    b /= np.linalg.norm(b)
    out = {"uniform": np.asfortranarray(np.broadcast_to(np.array([1.0, 0.5, -0.25], T), Ng + (3,)).copy())}
    diag = np.zeros(Ng + (3,))
    for c in range(3):
        prof = rng.random(Ng[c]) * 2 - 1
        diag[..., c] = prof.reshape([-1 if d == c else 1 for d in range(3)])
    out["diagonal"] = np.asfortranarray(diag.astype(T))
    for nm, A in (("rotation", 0.7 * scale * _skew(a)), ("shear", 0.7 * scale * np.outer(a, b))):
        out[nm] = linear_field(Ng, T, A, (0.3, -0.1, 0.2))
        out[nm + "-noise"] = linear_field(Ng, T, A, (0.3, -0.1, 0.2), noise=2.0 ** -30, seed=seed + 1)
    return out
