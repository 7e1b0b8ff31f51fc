"""Independent extended-precision reference of the Forces rows (TEST INFRASTRUCTURE; numpy only): the 16 columns that
wl_body_loads / wl_body_loads_mesh / wl_band_loads write per leaf (include/wlhip.h), restated in the style of
tests/xref_metrics.py, whose band sums it reuses for the three quantities the two share:

    cols 0-2  Fp  xref_metrics.pressure_force    K["pforce"]  = 1
    cols 3-5  Fv  xref_metrics.viscous_force     K["vforce"]  = 4
    cols 6-8  Mp  xref_metrics.pressure_moment   K["pmoment"] = 4   (2-D: the scalar, in slot z)

Every function returns (value, M): the exactly summed value in np.longdouble from the T-valued fields and the Float64 band
(nds, V), and the same expression tree on absolute values.  The check is that of xref_metrics.band_tol,
    |got - value| <= (K * eps_T + adds * eps_64 / 2) * M,
with `adds` the longest chain of Float64 additions a term passes through (xref_metrics.tree_adds for the kernels' blocked
reduction, plus one per leaf for the total row).  It imports neither `oracle` nor `waterlily_amd`.

The kernel's Mp is r x T(p nds) in double where the reference's is T(p (r x nds)): against the exact p (r x nds) the first
carries 0.5 eps_T of each product p nds_k |r_j| (the rounding of fp) and 2 eps_64 (r, product, difference), the second
the 3 counted in xref_metrics.  Both are inside K["pmoment"] = 4.

The constants of the four new columns, by counting the roundings of an evaluation whose every step is made in T = Float64
(the worst case: for Float32 the double steps vanish against eps_T), each eps_T/2 of a partial result that M bounds, doubled
for margin and rounded up to a power of two like xref_metrics.K:
    Mv  r x fv.  fv: the 3 of K["vforce"] (d + d: 2, times nu: 0.5, the product with nds in double, to T: 0.5).  r = loc - x0:
        0.5; the two products and their difference: 1.5.  5 -> 8.                     M = Mr_j Mfv_k + Mr_k Mfv_j
    Wp  fp . V.  fp: the 1 of K["pforce"]; each product with V: 0.5; D - 1 additions of partial sums: 1.  2.5 -> 4.
                                                                                      M = sum_c |p nds_c| |V_c|
    Wv  fv . V.  fv: 3; product: 0.5; additions: 1.  4.5 -> 8.                        M = sum_c Mfv_c |V_c|
    A   |nds| = sqrt(sum nds_c^2), all in Float64 whatever T: squares 0.5, D - 1 additions 1, the square root halves the
        relative error and adds 1 ulp (two half-roundings): 1.5 / 2 + 1 = 1.75 -> 4, in units of eps_64.   M = |nds|
    ncells: an integer count in double, exact (K = 0, M = 0).
V is an input here (Float64, as the kernel's registers hold it): the geometry -- nds, V and the active leaf of a composite --
comes from tests/xref_body.py (geometry() below) or from a stored band; its own error is xref_body's subject, not this one's.

Counted cells: those with a non-zero component of nds.  A leaf row holds the cells whose active leaf it is; the last row is
the total over all counted cells.  Without V (a stored band) Wp and Wv are NaN, which the kernel must return as NaN.
"""
from __future__ import annotations

import numpy as np

import xref as X
import xref_body as XB
import xref_metrics as XM
from xref import LD

NV = 16
COLUMNS = ("Fp_x", "Fp_y", "Fp_z", "Fv_x", "Fv_y", "Fv_z", "Mp_x", "Mp_y", "Mp_z", "Mv_x", "Mv_y", "Mv_z", "Wp", "Wv", "ncells", "area")
K = dict(XM.K, Mv=8, Wp=4, Wv=8, A=4, ncells=0)
COLK = ("pforce",) * 3 + ("vforce",) * 3 + ("pmoment",) * 3 + ("Mv",) * 3 + ("Wp", "Wv", "ncells", "A")


def _fv_terms(u, nu, idx, nds):
    """per cell the exact viscous term and its bound, (D, n) each (xref_metrics.viscous_force before the sum)"""
    Ng = u.shape[:-1]
    C = XM.band_cells({"u": u}, idx, Ng)
    D = C.D
    nds = np.asarray(nds, np.float64).reshape(len(C), D).astype(LD)
    nu = LD(nu)
    d = {(a, b): XM.dudx(C, a, b) for a in range(D) for b in range(D)}
    v, M = np.zeros((D, len(C)), LD), np.zeros((D, len(C)), LD)
    for i in range(D):
        for j in range(D):
            v[i] += -nu * (d[i, j][0] + d[j, i][0]) * nds[:, j]
            M[i] += abs(nu) * (d[i, j][1] + d[j, i][1]) * abs(nds[:, j])
    return v, M, C


def row(p, u, nu, x0, idx, nds, V=None):
    """One row over the band (idx: column-major linear indices into p's extents; nds [n, D] Float64; V [n, D] Float64 or
    None): (value[16], M[16], n) with n the number of counted cells"""
    D = p.ndim
    idx = np.asarray(idx, np.int64).reshape(-1)
    nds = np.asarray(nds, np.float64).reshape(idx.size, D)
    keep = (nds != 0).any(1)
    idx, nds = idx[keep], nds[keep]
    n = int(idx.size)
    v, M = np.zeros(NV), np.zeros(NV)
    v[0:D], M[0:D] = XM.pressure_force(p, idx, nds)
    v[3:3 + D], M[3:3 + D] = XM.viscous_force(u, nu, idx, nds)
    mv, mM = XM.pressure_moment(p, x0, idx, nds)
    if D == 3:
        v[6:9], M[6:9] = mv, mM
    else:
        v[8], M[8] = mv[0], mM[0]
    fv, Mfv, C = _fv_terms(u, nu, idx, nds)
    r = [C.idx[d].astype(LD) - LD(0.5) - LD(x0[d]) for d in range(D)]
    Mr = [abs(C.idx[d].astype(LD) - LD(0.5)) + abs(LD(x0[d])) for d in range(D)]
    if D == 3:
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            v[9 + i] = XM._exact_sum(r[j] * fv[k] - r[k] * fv[j])
            M[9 + i] = XM._exact_sum(Mr[j] * Mfv[k] + Mr[k] * Mfv[j])
    else:
        v[11] = XM._exact_sum(r[0] * fv[1] - r[1] * fv[0])
        M[11] = XM._exact_sum(Mr[0] * Mfv[1] + Mr[1] * Mfv[0])
    if V is None:
        v[12:14], M[12:14] = np.nan, np.nan
    else:
        Vl = np.asarray(V, np.float64).reshape(-1, D)[keep].astype(LD)
        pv = XM.band_cells({"p": p}, idx, p.shape)("p")
        ndl = nds.astype(LD)
        v[12] = XM._exact_sum(sum(pv * ndl[:, c] * Vl[:, c] for c in range(D)) if n else np.zeros(0, LD))
        M[12] = XM._exact_sum(sum(abs(pv * ndl[:, c] * Vl[:, c]) for c in range(D)) if n else np.zeros(0, LD))
        v[13] = XM._exact_sum(sum(fv[c] * Vl[:, c] for c in range(D)) if n else np.zeros(0, LD))
        M[13] = XM._exact_sum(sum(Mfv[c] * abs(Vl[:, c]) for c in range(D)) if n else np.zeros(0, LD))
    v[14] = n
    a = np.sqrt((nds.astype(LD) ** 2).sum(1))
    v[15] = M[15] = XM._exact_sum(a)
    return v, M, n


def rows(p, u, nu, x0, idx, nds, V=None, leaf=None, nleaf=1):
    """The nleaf + 1 rows: (value[nleaf+1, 16], M[nleaf+1, 16], n[nleaf+1]); leaf[b] = the active leaf of band entry b"""
    idx = np.asarray(idx, np.int64).reshape(-1)
    leaf = np.zeros(idx.size, int) if leaf is None else np.asarray(leaf, int).reshape(-1)
    nds = np.asarray(nds, np.float64).reshape(idx.size, p.ndim)
    out = []
    for q in range(nleaf):
        s = leaf == q
        out.append(row(p, u, nu, x0, idx[s], nds[s], None if V is None else np.asarray(V).reshape(idx.size, -1)[s]))
    out.append(row(p, u, nu, x0, idx, nds, V))
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out]), np.array([o[2] for o in out])


def tol(n, M, T, adds=None):
    """the bound of every column of a row of n counted cells (module docstring); column 15 in units of eps_64 whatever T"""
    adds = n if adds is None else adds
    M = np.asarray(M, np.float64)
    e64 = X.eps(np.float64)
    t = np.array([(K[k] * (e64 if k == "A" else X.eps(T)) + adds * e64 / 2) for k in COLK]) * M
    return t


def ratios(got, v, M, n, T, adds=None):
    """per column |got - v| / tol: 0 where both vanish (or both are NaN), inf where only the bound does"""
    got = np.asarray(got, np.float64)
    t = tol(n, M, T, adds)
    out = np.zeros(NV)
    for c in range(NV):
        if np.isnan(v[c]):
            out[c] = 0.0 if np.isnan(got[c]) else np.inf
            continue
        d = abs(got[c] - v[c])
        out[c] = d / t[c] if t[c] > 0 else (0.0 if d == 0 else np.inf)
        if np.isnan(got[c]):
            out[c] = np.inf
    return out


def geometry(body, idx_dn):
    """(nds [n, D], V [n, D], leaf [n]) in Float64 of xref_body's leaves `body` at the cell centres idx_dn (D, n), 0-based:
    nds of Metrics.jl:84-87 (measure with fastd2 = 1), the velocity and the active leaf of AutoBody.jl:73-131"""
    idx_dn = np.asarray(idx_dn)
    x = XB.loc(-1, idx_dn)
    (nv, _), _ = XB.nds(body, idx_dn)
    _, _, (V, _), _ = XB.measure(body, x, fastd2=1.0)
    _, act, _, _, _ = XB._composite(body, np.asarray(x, LD))
    return nv.T.astype(np.float64), V.T.astype(np.float64), np.asarray(act, int)
