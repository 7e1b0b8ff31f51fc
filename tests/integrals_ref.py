"""numpy restatement of the Integrals row (waterlily_amd/integrals.py, include/wlhip.h: wl_flow_integrals) in np.longdouble,
gather form, independent of the oracle and of the library.

u: dense host array (Ng..., D), ghosts included.  Cells I of inside(p); d(i,j) = the reference's ∂(i,j,I,u)
(src/Metrics.jl:28-30).  Columns: E, Z, S, div2, divmax, umax, P_1..P_D."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


def names(D):
    return ("E", "Z", "S", "div2", "divmax", "umax") + tuple(f"P{i + 1}" for i in range(D))


def _sh(a, off):
    """a at I + off for every inside cell I"""
    return a[tuple(slice(1 + o, n - 1 + o) for o, n in zip(off, a.shape))]


def _delta(i, D, s=1):
    return tuple(s if d == i else 0 for d in range(D))


def _add(a, b):
    return tuple(x + y for x, y in zip(a, b))


def grad(i, j, u):
    """∂(i,j,I,u) over the inside cells (longdouble)"""
    D = u.ndim - 1
    ui = u[..., i]
    di, dj, mj = _delta(i, D), _delta(j, D), _delta(j, D, -1)
    if i == j:
        return _sh(ui, di) - _sh(ui, (0,) * D)
    return (_sh(ui, dj) + _sh(ui, _add(dj, di)) - _sh(ui, mj) - _sh(ui, _add(mj, di))) / 4


def terms(u, U=None):
    """per-cell terms of the four sums and of P (dict name -> array over inside cells), the divergence, and max_i |u[I,i]|"""
    u = np.asarray(u).astype(LD)
    D = u.ndim - 1
    U = np.zeros(D, LD) if U is None else np.asarray(U, dtype=LD)
    zero = (0,) * D
    cen2 = [_sh(u[..., i], zero) + _sh(u[..., i], _delta(i, D)) for i in range(D)]       # twice the cell-centred velocity
    J = [[grad(i, j, u) for j in range(D)] for i in range(D)]
    t = {"E": sum((cen2[i] - 2 * U[i]) ** 2 for i in range(D)) * LD(0.125)}
    if D == 2:
        om = [J[1][0] - J[0][1]]
    else:   # Metrics.jl:60: omega_i = ∂(k,j) - ∂(j,k), (i,j,k) cyclic
        om = [J[(i + 2) % 3][(i + 1) % 3] - J[(i + 1) % 3][(i + 2) % 3] for i in range(3)]
    t["Z"] = sum(w * w for w in om) / 2
    t["S"] = sum(((J[i][j] + J[j][i]) / 2) ** 2 for i in range(D) for j in range(D))
    div = sum(J[i][i] for i in range(D))
    t["div2"] = div * div
    for i in range(D):
        t[f"P{i + 1}"] = cen2[i] / 2
    uabs = np.stack([np.abs(_sh(u[..., i], zero)) for i in range(D)])
    facesum = sum(np.abs(_sh(u[..., i], zero)) + np.abs(_sh(u[..., i], _delta(i, D))) for i in range(D))
    return t, div, uabs, facesum


def integrals(u, U=None):
    """(row, bound, n): row[6+D] in longdouble; bound[q] = sum |term| of a summed column, the face sum
    sum_i (|u[I+d_i,i]| + |u[I,i]|) at the maximising cell for divmax, 0 for umax; n = number of inside cells.
    The maxima skip NaN operands (the device's comparison) and are 0 over no cell."""
    D = np.asarray(u).ndim - 1
    t, div, uabs, facesum = terms(u, U)
    nm = names(D)
    row, bound = np.zeros(6 + D, LD), np.zeros(6 + D, LD)
    n = int(div.size)
    for q, name in enumerate(nm):
        if name in t:
            row[q] = t[name].sum(dtype=LD)
            bound[q] = np.abs(t[name]).sum(dtype=LD)
    ad = np.abs(div)
    if n and not np.isnan(ad).all():
        k = np.nanargmax(ad)
        row[4], bound[4] = ad.ravel()[k], facesum.ravel()[k]
    if n and not np.isnan(uabs).all():
        row[5] = np.nanmax(uabs)
    return row, bound, n


def tolerance(bound, n):
    """derived, not measured: any summation order of n doubles is within (n-1) u sum|x_i|, and a term is at most a few dozen
    double operations from exactly converted inputs -> (n + 48) 2^-53 sum|term|; divmax 8 * 2^-53 * its face sum; umax exact"""
    tol = (n + 48) * U53 * np.asarray(bound, dtype=np.float64)
    tol[4] = 8 * U53 * float(bound[4])
    tol[5] = 0.0
    return tol


def check(got, u, U=None, n=None):
    """assert |got - ref| <= tolerance column by column; returns the worst ratio (for -s output)"""
    row, bound, ni = integrals(u, U)
    tol = tolerance(bound, ni if n is None else n)
    err = np.abs(np.asarray(got, dtype=LD) - row).astype(np.float64)
    worst = 0.0
    for q, name in enumerate(names(np.asarray(u).ndim - 1)):
        assert err[q] <= tol[q], f"{name}: |got - ref| = {err[q]:.3g} > {tol[q]:.3g} (got {got[q]!r}, ref {float(row[q])!r})"
        if tol[q] > 0:
            worst = max(worst, err[q] / tol[q])
    return worst


# ---- fields with closed-form rows: small integers over the WHOLE array, ghosts included (exact in Float32)

def index_field(Ng, f, T=np.float64):
    """u[I, i] = f(i, I) with I the 0-based index arrays"""
    ix = np.indices(Ng)
    u = np.zeros(tuple(Ng) + (len(Ng),), dtype=T)
    for i in range(len(Ng)):
        u[..., i] = f(i, ix)
    return u


def pins(D):
    """[(label, Ng, f(i, I), U, {column: value / n})] -- n = number of inside cells; every column not named is 0"""
    out = []
    if D == 2:
        Ng, U0, Om, a = (9, 7), (3.0, -2.0), 2.0, 3.0
        out.append(("uniform", Ng, lambda i, I: U0[i] + 0 * I[0], None, {"E": 6.5, "umax": "3", "P1": 3.0, "P2": -2.0}))
        out.append(("uniform-U", Ng, lambda i, I: U0[i] + 0 * I[0], U0, {"E": 0.0, "umax": "3", "P1": 3.0, "P2": -2.0}))
        out.append(("rotation", Ng, lambda i, I: -Om * I[1] if i == 0 else Om * I[0], None, {"Z": 2 * Om ** 2}))
        out.append(("shear", Ng, lambda i, I: a * I[1] if i == 0 else 0 * I[0], None, {"Z": a * a / 2, "S": a * a / 2}))
    else:
        Ng, U0, Om, a = (8, 7, 6), (3.0, -2.0, 1.0), 2.0, 3.0
        out.append(("uniform", Ng, lambda i, I: U0[i] + 0 * I[0], None, {"E": 7.0, "umax": "3", "P1": 3.0, "P2": -2.0, "P3": 1.0}))
        out.append(("uniform-U", Ng, lambda i, I: U0[i] + 0 * I[0], U0, {"E": 0.0, "umax": "3", "P1": 3.0, "P2": -2.0, "P3": 1.0}))
        for ax in range(3):
            b, c = (ax + 1) % 3, (ax + 2) % 3
            out.append((f"rotation-{ax}", Ng, (lambda i, I, b=b, c=c: -Om * I[c] if i == b else (Om * I[b] if i == c else 0 * I[0])),
                        None, {"Z": 2 * Om ** 2}))
        out.append(("strain", Ng, lambda i, I: a * I[0] if i == 0 else (-a * I[1] if i == 1 else 0 * I[0]), None,
                    {"S": 2 * a * a}))
    return out


def check_pin(row, spec, Ng, what=""):
    """the exact row of a pin: column value = spec * n for the sums named, Z / S / div2 / divmax = 0 unless named; E, umax and P
    (which depend on the indices for the non-uniform fields) are only checked where the spec names them"""
    D = len(Ng)
    n = int(np.prod([m - 2 for m in Ng]))
    for q, name in enumerate(names(D)):
        if name in spec:
            want = float(spec[name]) if isinstance(spec[name], str) else spec[name] * n
            assert float(row[q]) == want, (what, name, float(row[q]), want)
        elif 1 <= q <= 4:
            assert float(row[q]) == 0.0, (what, name, float(row[q]))
