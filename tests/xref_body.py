"""Independent extended-precision reference of the body measurement (TEST INFRASTRUCTURE; numpy only): the Body.jl /
AutoBody.jl leg of tests/xref.py for the closed-form families and affine maps that the HIP `measure!` kernels take.  It
imports neither `oracle` nor `waterlily_amd`.  Sources (reference tree): src/AutoBody.jl:73-93 (composite rules),
:115-131 (measure), src/Body.jl:31-53 (measure!), :56-61 (kern, kern0, kern1), src/Metrics.jl:84-87 (nds), src/util.jl:160
(loc).  ForwardDiff's gradient / jacobian / derivative are replaced by the closed forms of each family and of an affine map.

A body is a list of leaves `leaf(family, p, map, op)`; `map` is (A, b, dA/dt, db/dt) at the measured time, as Float64
arrays (the builders below evaluate them; sin and cos are taken in Float64, 1 ulp each, which the bound M carries through
|A| and |b|).  Everything else is evaluated in np.longdouble from the exact half-integer positions.

The measure kernels evaluate in Float64 and round once to T, so the check is sharper than K * eps_T * M:
    |got - ref| <= ulp_T(ref) / 2 + K * eps_64 * M                                        (tol below)
K = 32 for every quantity: the longest chain is d at a mapped torus point -- the map (2D roundings), e = xi - c (1), two
nested norms (2 (D+1) and two sqrt at 1 ulp = 2 roundings each), two subtractions (2), the chain rule and |grad| (2D + D + 3),
d / m (1): about 30 half-ulps = 15 eps of the partial results that M bounds; 32 is the usual 2x margin.  kern0, kern1 and
kern call sin or cos once or twice (1 ulp each, of values at most 1): their M below adds 1 per call.
Largest shares of the bound measured, oracle / kernels (test_worst_ratios_are_recorded of the CPU and the GPU file, MI355X):
    Float64   sigma 0.032 / 0.032   mu0 0.000 / 0.000   mu1 0.000 / 0.000   V 0.012 / 0.013   nds 0.000 / 0.000
    Float32   sigma 1.000 / 1.000   mu0 0.996 / 0.997   mu1 0.475 / 0.475   V 0.976 / 1.000
None exceeds 1.  In Float64 the K = 32 term decides and is used to a thirtieth at most: M carries the cancellation of xi - c
as if both operands were rounded, and they are exact half-integers and constants.  In Float32 the bound is ulp_T/2 to within
1e-7 of itself, so a share of 1.000 is a value whose exact counterpart lies half an ulp_T from a Float32 number, rounded
correctly: the Float64 evaluation erred by less than the K eps_64 M that separates 1.000 from above 1, and a kernel that
evaluated in Float32 would show shares of several units.

Every function also returns its distance from each branch it takes, so that a test can assert that no compared point sits
nearer to a branch than its error bound:
    band   | sigma_T^2 - (2+eps)^2 |  (Body.jl:35, on the stored T value)         fast  | d^2 - fastd2 |  (AutoBody.jl:118)
    clamp  | |d/eps| - 1 |            (Body.jl:57-61 through clamp)               plate | |xi_0| - a |    (the plate's clamp)
    tie    the gap between the two leaves that compete for a composite's value    nds   | |d| - 1 |       (Metrics.jl:86)
"""
from __future__ import annotations

import math

import numpy as np

LD = np.longdouble
K = 32
PI = LD(np.pi) + LD(1.2246467991473532e-16)                              # pi to longdouble precision (hi + lo)


def leaf(family, p, map=None, op="+"):
    """family in sphere | cylinder | torus | plate.  p: sphere (c[D], R); cylinder (c[D], R, axes); torus (c[3], R, r);
    plate (a, thk).  op joins this leaf to the composite of the ones before it: "+" union, "-" minus, "&" intersection."""
    return {"family": family, "p": p, "map": map, "op": op}


# ------------------------------------------------------------------------------------------------ affine maps at a time t

def translate(D, t, v=0.0, a=0.0, s0=0.0):
    """xi = x - (s0 + v t + a t^2)"""
    v, a, s0 = (np.broadcast_to(np.asarray(q, np.float64), (D,)) for q in (v, a, s0))
    return np.eye(D), -(s0 + v * t + a * t * t), np.zeros((D, D)), -(v + 2 * a * t)


def rotate3d(center, axis, w, t, th0=0.0):
    """xi = R (x - c), R = I - sin(th) K + (1 - cos(th)) K^2 (Rodrigues, rotation by -th about the unit axis), th = w t + th0"""
    c = np.broadcast_to(np.asarray(center, np.float64), (3,))
    k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    s, co = math.sin(w * t + th0), math.cos(w * t + th0)
    R, dR = np.eye(3) - s * Kx + (1 - co) * (Kx @ Kx), (-co * Kx + s * (Kx @ Kx)) * w
    return R, -R @ c, dR, -dR @ c


def rotate2d(center, w, t, th0=0.0):
    """xi = R (x - c), R = [c s; -s c]"""
    s, co = math.sin(w * t + th0), math.cos(w * t + th0)
    R, dR = np.array([[co, s], [-s, co]]), np.array([[-s, co], [-co, -s]]) * w
    c = np.full(2, float(center))
    return R, -R @ c, dR, -dR @ c


def scale(m, s):
    return tuple(s * q for q in m)


# ------------------------------------------------------------------------------------------------ one leaf

def _norm(e, Me):
    return np.sqrt((e * e).sum(0)), np.sqrt((Me * Me).sum(0))


def _leaf(L, x):
    """sdf and its gradient with respect to x at the points x (D, n) of one leaf, before the division by |grad|:
    (d, M_d, g, M_g, branch distances)"""
    D, n = x.shape
    if L["map"] is None:
        A, b = np.eye(D).astype(LD), np.zeros(D, LD)
    else:
        A, b = L["map"][0].astype(LD), L["map"][1].astype(LD)
    xi = A @ x + b[:, None]
    Mxi = abs(A) @ abs(x) + abs(b)[:, None]
    br = {}
    fam, p = L["family"], L["p"]
    if fam in ("sphere", "cylinder"):
        c = np.broadcast_to(np.asarray(p[0], np.float64), (D,)).astype(LD)
        mask = np.ones(D) if fam == "sphere" else np.array([1.0 if a in p[2] else 0.0 for a in range(D)])
        e, Me = (xi - c[:, None]) * mask[:, None], (Mxi + abs(c)[:, None]) * mask[:, None]
        rho, Mrho = _norm(e, Me)
        d, Md = rho - LD(p[1]), Mrho + abs(LD(p[1]))
        gxi, Mgxi = e / rho, Me / rho * (1 + Mrho / rho)
    elif fam == "torus":
        c = np.broadcast_to(np.asarray(p[0], np.float64), (3,)).astype(LD)
        e, Me = xi - c[:, None], Mxi + abs(c)[:, None]
        s, Ms = _norm(e[1:], Me[1:])
        q, Mq = s - LD(p[1]), Ms + abs(LD(p[1]))
        rho, Mrho = np.sqrt(e[0] ** 2 + q ** 2), np.sqrt(Me[0] ** 2 + Mq ** 2)
        d, Md = rho - LD(p[2]), Mrho + abs(LD(p[2]))
        gxi = np.stack([e[0] / rho, (q / rho) * (e[1] / s), (q / rho) * (e[2] / s)])
        cr, cs = 1 + Mrho / rho, 1 + Ms / s
        Mgxi = np.stack([Me[0] / rho * cr, (Mq / rho * cr) * (Me[1] / s * cs), (Mq / rho * cr) * (Me[2] / s * cs)])
    elif fam == "plate":
        a = LD(p[0])
        e, Me = xi.copy(), Mxi.copy()
        e[0] = xi[0] - np.clip(xi[0], -a, a)
        Me[0] = Mxi[0] + a
        rho, Mrho = _norm(e, Me)
        d, Md = rho - LD(p[1]), Mrho + abs(LD(p[1]))
        with np.errstate(invalid="ignore", divide="ignore"):
            gxi, Mgxi = e / rho, Me / rho * (1 + Mrho / rho)
        gxi[0] = np.where(abs(xi[0]) > a, gxi[0], 0 * gxi[0])            # (0 * NaN keeps the NaN of rho = 0)
        br["plate"] = abs(abs(xi[0]) - a)
    else:
        raise ValueError(fam)
    return d, Md, A.T @ gxi, abs(A).T @ Mgxi, br


def _composite(body, x):
    """AutoBody.jl:73-93: the composite's sdf at x, per point the active leaf and its sign, and the gap to the runner-up"""
    ev = [_leaf(L, x) for L in body]
    d, act, sgn = ev[0][0].copy(), np.zeros(x.shape[1], int), np.ones(x.shape[1], LD)
    tie = np.full(x.shape[1], np.inf, LD)
    for q, L in enumerate(body[1:], start=1):
        dq = ev[q][0]
        if L["op"] == "+":
            new, take, s = dq, dq < d, 1
        elif L["op"] == "-":
            new, take, s = -dq, -dq > d, -1
        else:
            new, take, s = dq, dq > d, 1
        tie = np.minimum(np.where(take, LD(np.inf), tie), abs(new - d))   # a later winner only competes with later leaves
        d, act, sgn = np.where(take, new, d), np.where(take, q, act), np.where(take, LD(s), sgn)
    return d, act, sgn, tie, ev


def sdf(body, x):
    """(d, M_d, {tie}) of the composite at x (D, n)"""
    x = np.asarray(x, LD)
    d, act, sgn, tie, ev = _composite(body, x)
    Md = np.choose(act, [e[1] for e in ev]) if len(body) > 1 else ev[0][1]
    return d, Md, {"tie": tie}


def measure(body, x, fastd2=np.inf):
    """AutoBody.jl:115-131 (for a composite :107-110, the active leaf): ((d, M), (n, M), (V, M), branch distances);
    n = V = 0 where d^2 > fastd2 (:118) or the gradient holds a NaN (:120)"""
    x = np.asarray(x, LD)
    D, npts = x.shape
    d, act, sgn, tie, ev = _composite(body, x)
    br = {"tie": tie, "fast": abs(d * d - LD(fastd2)), "plate": np.full(npts, np.inf, LD)}
    Md = np.zeros(npts, LD)
    n, Mn, V, MV = (np.zeros((D, npts), LD) for _ in range(4))
    for q, L in enumerate(body):
        sel = act == q
        if not sel.any():
            continue
        dq, Mdq, g, Mg, b = ev[q]
        if "plate" in b:
            br["plate"] = np.where(sel, b["plate"], br["plate"])
        near = sel & ~(d * d > LD(fastd2))
        g = g * sgn
        ok = near & ~np.isnan(g).any(0)
        with np.errstate(invalid="ignore", divide="ignore"):
            m, Mm = _norm(g, Mg)
            cm = 1 + Mm / m
        Md = np.where(sel, Mdq, Md)
        d = np.where(ok, d / m, d)
        Md = np.where(ok, Mdq / m * cm, Md)
        n = np.where(ok, g / m, n)
        Mn = np.where(ok, Mg / m * cm, Mn)
        if L["map"] is not None:
            A, dA, db = L["map"][0].astype(LD), L["map"][2].astype(LD), L["map"][3].astype(LD)
            Ai = _inv(A)
            dot, Mdot = dA @ x + db[:, None], abs(dA) @ abs(x) + abs(db)[:, None]
            V = np.where(ok, -(Ai @ dot), V)
            MV = np.where(ok, abs(Ai) @ Mdot, MV)
    return (d, Md), (n, Mn), (V, MV), br


def _inv(A):
    """inverse of a 2x2 or 3x3 longdouble matrix by cofactors"""
    D = A.shape[0]
    if D == 2:
        det = A[0, 0] * A[1, 1] - A[0, 1] * A[1, 0]
        return np.array([[A[1, 1], -A[0, 1]], [-A[1, 0], A[0, 0]]], LD) / det
    C = np.array([[A[(i + 1) % 3, (j + 1) % 3] * A[(i + 2) % 3, (j + 2) % 3] - A[(i + 1) % 3, (j + 2) % 3] * A[(i + 2) % 3, (j + 1) % 3]
                   for j in range(3)] for i in range(3)], LD)
    return C.T / (A[0] * C[0]).sum()


# ------------------------------------------------------------------------------------------------ Body.jl:56-61

def kern(d):
    return LD(0.5) + LD(0.5) * np.cos(PI * d)


def kern0(d):
    return LD(0.5) + LD(0.5) * d + LD(0.5) * np.sin(PI * d) / PI


def kern1(d):
    return LD(0.25) * (1 - d * d) - LD(0.5) * (d * np.sin(PI * d) + (1 + np.cos(PI * d)) / PI) / PI


def loc(i, idx):
    """util.jl:160 for 0-based indices idx (D, n): the index minus 0.5, and another 0.5 less along i for the face i (i = -1:
    the cell centre)"""
    x = np.asarray(idx).astype(LD) - LD(0.5)
    if i >= 0:
        x[i] -= LD(0.5)
    return x


def fields(body, idx, eps, T):
    """Body.jl:31-53 (the fill loop, before BC!) at the inside cells idx (D, n).  Returns a dict name -> (value, M) with
    sigma (n), mu0 (D, n), V (D, n), mu1 (D*D, n) (component i + D*j as the arrays hold it), the band mask, and the branch
    distances {band, tie, fast, clamp, plate} (min over the faces of a cell)."""
    T = np.dtype(T).type
    idx = np.asarray(idx)
    D, n = idx.shape
    d, Md, br0 = sdf(body, loc(-1, idx))
    sT = d.astype(np.float64).astype(T)
    d2 = T((2 + eps) ** 2)
    band = sT * sT < d2
    out = {"sigma": (d, Md), "band": band}
    br = {"band": abs(d * d - LD((2 + eps) ** 2)), "tie": br0["tie"]}
    mu0, Mmu0 = np.where(d < 0, LD(0), LD(1))[None].repeat(D, 0), np.zeros((D, n), LD)
    V, MV = np.zeros((D, n), LD), np.zeros((D, n), LD)
    mu1, Mmu1 = np.zeros((D * D, n), LD), np.zeros((D * D, n), LD)
    for k in ("fast", "clamp", "plate"):
        br[k] = np.full(n, np.inf, LD)
    ib = idx[:, band]
    e = LD(eps)
    for i in range(D):
        (di, Mdi), (ni, Mni), (Vi, MVi), b = measure(body, loc(i, ib), fastd2=(2 + eps) ** 2)
        q = np.clip(di / e, -1, 1)
        Mq = Mdi / e
        V[i, band], MV[i, band] = Vi[i], MVi[i]
        mu0[i, band], Mmu0[i, band] = kern0(q), 1 + Mq                       # |kern0'| = kern <= 1; one sin
        k1, Mk1 = e * kern1(q), e * (2 + Mq)                               # |kern1'| = |q| kern0 <= 1; sin and cos
        for j in range(D):
            mu1[i + D * j, band], Mmu1[i + D * j, band] = k1 * ni[j], Mk1 * Mni[j] + abs(k1) * Mni[j]
        br["fast"][band] = np.minimum(br["fast"][band], b["fast"])
        br["plate"][band] = np.minimum(br["plate"][band], b["plate"])
        br["tie"][band] = np.minimum(br["tie"][band], b["tie"])
        br["clamp"][band] = np.minimum(br["clamp"][band], abs(abs(di / e) - 1))
    out.update(mu0=(mu0, Mmu0), V=(V, MV), mu1=(mu1, Mmu1))
    return out, br


def nds(body, idx):
    """Metrics.jl:84-87  n * kern(clamp(d,-1,1)) with measure(...; fastd2 = 1) at the cell centres idx (D, n):
    ((value (D, n), M), {nds, fast, tie, plate})"""
    (d, Md), (n, Mn), _, br = measure(body, loc(-1, np.asarray(idx)), fastd2=1.0)
    w = kern(np.clip(d, -1, 1))
    br["nds"] = abs(abs(d) - 1)
    return (n * w, Mn * (1 + PI / 2 * Md) + abs(n * w)), br                 # |kern'| <= pi/2; one cos


def tol(ref, M, T):
    """ulp_T(ref)/2 + K * eps_64 * M"""
    T = np.dtype(T).type
    r64 = np.asarray(ref, np.float64)
    return np.spacing(np.abs(r64.astype(T))).astype(np.float64) / 2 + K * np.finfo(np.float64).eps * np.asarray(M, np.float64)


def ratio(got, ref, M, T):
    """max |got - ref| / tol (0 for empty input); an exact zero (ref = M = 0) must be met exactly"""
    d = np.abs(np.asarray(got, LD) - ref).astype(np.float64)
    t = tol(ref, M, T)
    exact = (np.asarray(ref, np.float64) == 0) & (np.asarray(M, np.float64) == 0)
    r = np.where(exact, np.where(d == 0, 0.0, np.inf), d / np.where(exact, 1.0, t))
    return float(np.max(r)) if d.size else 0.0


# ------------------------------------------------------------------------------------------------ the tests' bodies

# name -> (dims, times, leaves); a leaf is (family, p, map spec, op), a map spec None, ("translate", v, s0),
# ("rotate3d", center, axis, w, th0), ("rotate2d", center, w, th0) or ("scaled", spec, s).  Centres, radii and times are not representable offsets (64.3,
# 7.37 ...), so that no face or cell sits on a branch; the tests assert that from the branch distances.
C3 = (10.3, 9.2, 8.1)
CASES = {
    # a sphere of radius 4 near x = 64.3: its band lies across the seam between the 64-cell x chunks (i = 64 | 65) in
    # every row it touches
    "seam-3d": ((130, 12, 10), (0.0,), [("sphere", ((64.3, 6.2, 5.1), 4.0), None, "+")]),
    # the same sphere translating along x: short of the seam at t = 0 (centre 55.3), across it at t = 7.37 (centre 64.95)
    "seam-3d-moving": ((130, 12, 10), (0.0, 7.37), [("sphere", ((55.3, 6.2, 5.1), 4.0), ("translate", (1.31, 0.0, 0.0), 0.0), "+")]),
    "seam-2d": ((130, 20), (0.0,), [("sphere", ((64.3, 10.2), 4.0), None, "+")]),
    "seam-2d-moving": ((130, 20), (0.0, 7.37), [("sphere", ((55.3, 10.2), 4.0), ("translate", (1.31, 0.0), 0.0), "+")]),
    "torus": ((20, 18, 16), (0.0,), [("torus", (C3, 4.3, 1.4), None, "+")]),
    "cylinder": ((20, 18, 16), (0.0,), [("cylinder", (C3, 3.1, (0, 1)), None, "+")]),
    "rotating-plate": ((20, 18, 16), (0.0, 7.37), [("plate", (3.3, 1.2), ("rotate3d", C3, (0.3, -0.5, 0.8), 0.21, 0.4), "+")]),
    "scaled": ((20, 18, 16), (0.0, 7.37), [("sphere", ((20.6, 18.4, 16.2), 7.1), ("scaled", ("translate", (0.11, 0.0, 0.07), 0.0), 2.0), "+")]),
    # the reference's test plate (2-D) turning about a pivot: the |xi_0| = a branch with the oracle's closed forms as well
    "plate-2d": ((26, 22), (0.0, 7.37), [("plate", (4.3, 1.2), ("rotate2d", 12.3, 0.21, 0.4), "+")]),
    "composite": ((20, 18, 16), (0.0, 7.37), [("sphere", (C3, 5.23), ("translate", (0.21, 0.0, 0.0), 0.0), "+"),
                                              ("cylinder", (C3, 1.73, (0, 1)), None, "-"),
                                              ("sphere", ((10.3, 9.2, 11.43), 5.17), None, "&")]),
}


def _map_at(spec, D, t):
    if spec is None:
        return None
    if spec[0] == "translate":
        return translate(D, t, v=spec[1], s0=spec[2])
    if spec[0] == "rotate3d":
        return rotate3d(spec[1], spec[2], spec[3], t, spec[4])
    if spec[0] == "rotate2d":
        return rotate2d(spec[1], spec[2], t, spec[3])
    return scale(_map_at(spec[1], D, t), spec[2])


def body_at(name, t):
    """the reference's leaves of CASES[name] at time t"""
    dims, _, leaves = CASES[name]
    return [leaf(f, p, _map_at(m, len(dims), t), op) for f, p, m, op in leaves]


def inside_cells(dims):
    """0-based indices (D, n) of the inside cells of a grid of interior extents dims, column-major (ascending linear index)"""
    g = np.meshgrid(*[np.arange(1, n + 1) for n in dims], indexing="ij")
    return np.stack([a.ravel(order="F") for a in g])


# ------------------------------------------------------------------------------------------------ the tests' controls

def moved(name, t, D, shift=0.0, rate=1.0):
    """the reference's leaves with the body moved by `shift` along x and its map's time derivative scaled by `rate`"""
    out = body_at(name, t)
    for L in out:
        A, b, dA, db = L["map"] if L["map"] is not None else translate(D, 0.0)
        L["map"] = (A, b + shift * A[:, 0], rate * dA, rate * db)
    return out


def controls(name, t, idx, T, D, Ng, got, got_list, got_nds, keep):
    """what must FAIL: sigma against the body moved by 64 K eps_T of the grid along x; V against a map whose velocity is
    off by 64 K eps_T (bodies that move); mu0, mu1, the band list and nds against the body moved by one cell (their M
    carries the cancellation of xi - c through the normal, so a move of 64 K eps is inside their bound)"""
    cell = tuple(idx)
    e = 64 * K * float(np.finfo(T).eps)
    ref2, _ = fields(moved(name, t, D, shift=e * max(Ng)), idx, 1.0, T)
    assert ratio(got["sigma"], *ref2["sigma"], T) > 1
    ref3, _ = fields(moved(name, t, D, rate=1 + e), idx, 1.0, T)
    if any(np.any(r != 0) for r in ref3["V"][0]):
        assert max(ratio(got["V"][cell + (c,)], ref3["V"][0][c], ref3["V"][1][c], T) for c in range(D)) > 1
    one = moved(name, t, D, shift=1.0)
    ref1 = fields(one, idx, 1.0, T)[0]
    band1 = ref1["band"]
    assert max(ratio(got["mu0"][cell + (c,)], ref1["mu0"][0][c], ref1["mu0"][1][c], T) for c in range(D)) > 1
    assert max(ratio(got["mu1"][cell + (q,)], ref1["mu1"][0][q], ref1["mu1"][1][q], T) for q in range(D * D)) > 1
    lin = np.ravel_multi_index(cell, Ng, order="F")
    assert not np.array_equal(got_list, lin[band1])
    (nv, nM), _ = nds(one, idx[:, keep])
    assert ratio(got_nds, nv, nM, np.float64) > 1
