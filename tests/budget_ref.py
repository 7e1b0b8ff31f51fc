"""numpy restatement of Budget's two rules (waterlily_amd/budget.py; include/wlhip.h: wl_budget_update, wl_budget_terms), written
from the rules themselves, operation by operation in the stated order: double arithmetic on converted operands, one rounding to
the accumulator type A (float32 or float64) per stored value.  Arrays are whole local host arrays (ghost cells included); the
moments are written on inside() and the terms on inside() shrunk by one, zeros elsewhere.  Also the DIRECT moments: long double,
two passes over the kept samples, which the incremental rule must reproduce."""
import numpy as np

from meanflow_ref import ORDER, RefMean, eps_schedule

COLUMNS = ("k", "production", "dissipation", "turbulent_transport", "pressure_transport", "viscous_diffusion", "convection", "residual")


def sym(D, i, j):
    """index of R_ij in ParaView's order"""
    i, j = min(i, j), max(i, j)
    return ORDER[D].index((i, j))


def _sh(f, off, m=1):
    """f at I + off for every I of the array shrunk by m on every side"""
    return f[tuple(slice(m + o, n - m + o) for o, n in zip(off, f.shape))]


def _e(D, *js):
    o = [0] * D
    for j in js:
        o[abs(j) - 1] += 1 if j > 0 else -1
    return tuple(o)


def grad(d, i, j, m=1, dt=np.float64):
    """the reference's d(i,j,I,d) on the array shrunk by m: d is the whole array of component i"""
    D = d.ndim
    if i == j:
        return _sh(d, _e(D, i + 1), m) - _sh(d, _e(D), m)
    return (_sh(d, _e(D, j + 1), m) + _sh(d, _e(D, j + 1, i + 1), m) - _sh(d, _e(D, -(j + 1)), m) - _sh(d, _e(D, -(j + 1), i + 1), m)) / dt(4)


def centre(d, i, m=1, dt=np.float64):
    D = d.ndim
    return dt(0.5) * (_sh(d, _e(D), m) + _sh(d, _e(D, i + 1), m))


class RefBudget:
    """host arrays R (N..., D(D+1)/2), PU (N..., D), GG (N...), T3 (N..., D) of dtype A, and mean: a RefMean (U, P)"""

    def __init__(self, D, A, t_init):
        self.D, self.A = D, np.dtype(A)
        self.mean = RefMean(D, A, t_init, uu=False, pp=False)
        self.R = self.PU = self.GG = self.T3 = None

    @property
    def t(self):
        return self.mean.t

    def reset(self, t_init=None):
        self.mean.reset(t_init)

    def update(self, u, p, t):
        eps = eps_schedule(self.mean.t, t)
        if eps is None:
            return None
        D, A = self.D, self.A
        u64, p64 = np.asarray(u, dtype=np.float64), np.asarray(p, dtype=np.float64)
        N = p64.shape
        I = tuple(slice(1, n - 1) for n in N)
        if len(self.mean.t) == 1:                              # first: every moment 0, nothing read
            self.R = np.zeros(N + (len(ORDER[D]),), dtype=A)
            self.PU, self.GG, self.T3 = np.zeros(N + (D,), dtype=A), np.zeros(N, dtype=A), np.zeros(N + (D,), dtype=A)
        else:
            keep = 1.0 - eps
            U, P = self.mean.U.astype(np.float64), self.mean.P.astype(np.float64)
            d = [u64[..., c] - U[..., c] for c in range(D)]
            a = [centre(d[c], c) for c in range(D)]
            q = (p64 - P)[I]
            gg = None
            for i in range(D):
                for j in range(D):
                    h = grad(d[i], i, j)
                    gg = h * h if gg is None else gg + h * h
            s = a[0] * a[0]
            for i in range(1, D):
                s = s + a[i] * a[i]
            R = [self.R[I + (k,)].astype(np.float64) for k in range(len(ORDER[D]))]
            tr = R[0]
            for i in range(1, D):
                tr = tr + R[i]
            c1, c2 = keep * eps * (1.0 - 2.0 * eps), eps * keep
            for j in range(D):
                sr = a[0] * R[sym(D, 0, j)]
                for i in range(1, D):
                    sr = sr + a[i] * R[sym(D, i, j)]
                t3 = self.T3[I + (j,)].astype(np.float64)
                self.T3[I + (j,)] = ((keep * t3 + c1 * s * a[j]) - c2 * (2.0 * sr + a[j] * tr)).astype(A)
            for k, (ia, ib) in enumerate(ORDER[D]):
                self.R[I + (k,)] = (keep * (R[k] + eps * a[ia] * a[ib])).astype(A)
            for j in range(D):
                self.PU[I + (j,)] = (keep * (self.PU[I + (j,)].astype(np.float64) + eps * q * a[j])).astype(A)
            self.GG[I] = (keep * (self.GG[I].astype(np.float64) + eps * gg)).astype(A)
        self.mean.update(u, p, t)
        return eps

    def terms(self, nu, R=None, PU=None, GG=None, T3=None, U=None):
        return terms(self.D, self.A, nu, self.R if R is None else R, self.PU if PU is None else PU, self.GG if GG is None else GG,
                     self.T3 if T3 is None else T3, self.mean.U if U is None else U)


def terms(D, A, nu, R, PU, GG, T3, U):
    """the eight terms (N..., 8) of dtype A from moment arrays and the mean velocity (any float dtype: converted first)"""
    A = np.dtype(A)
    R, PU, GG, T3, U = (np.asarray(x, dtype=np.float64) for x in (R, PU, GG, T3, U))
    N = GG.shape
    J = tuple(slice(2, n - 2) for n in N)
    k = R[..., 0]
    for i in range(1, D):
        k = k + R[..., i]
    k = 0.5 * k
    k0 = _sh(k, _e(D), 2)
    prod = None
    for i in range(D):
        for j in range(D):
            t = _sh(R[..., sym(D, i, j)], _e(D), 2) * grad(U[..., i], i, j, 2)
            prod = t if prod is None else prod + t
    tt = pt = vd = cv = None
    for j in range(D):
        ep, em = _e(D, j + 1), _e(D, -(j + 1))
        kp, km = _sh(k, ep, 2), _sh(k, em, 2)
        t3 = (_sh(T3[..., j], ep, 2) - _sh(T3[..., j], em, 2)) / 2.0
        pu = (_sh(PU[..., j], ep, 2) - _sh(PU[..., j], em, 2)) / 2.0
        lap = (kp - 2.0 * k0) + km
        adv = centre(U[..., j], j, 2) * ((kp - km) / 2.0)
        tt, pt = (t3, pu) if tt is None else (tt + t3, pt + pu)
        vd, cv = (lap, adv) if vd is None else (vd + lap, cv + adv)
    t1, t2, t3_, t4, t5, t6 = -prod, nu * _sh(GG, _e(D), 2), -0.5 * tt, -pt, nu * vd, -cv
    out = np.zeros(N + (8,), dtype=A)
    for c, v in enumerate((k0, t1, t2, t3_, t4, t5, t6, ((((t1 - t2) + t3_) + t4) + t5) + t6)):
        out[J + (c,)] = v.astype(A)
    return out


def direct_moments(us, ps, dts):
    """time-weighted two-pass central moments of the samples in long double, on inside(): dict U, P (whole arrays) and R, PU,
    GG, T3 (inside() only), the last axis the component"""
    L = np.longdouble
    w = np.asarray(dts, dtype=L)
    W = w.sum()
    us, ps = [np.asarray(u, dtype=L) for u in us], [np.asarray(p, dtype=L) for p in ps]
    D = us[0].shape[-1]
    U = sum(wi * u for wi, u in zip(w, us)) / W
    P = sum(wi * p for wi, p in zip(w, ps)) / W
    I = tuple(slice(1, n - 1) for n in P.shape)
    shape = tuple(n - 2 for n in P.shape)
    R, PU = np.zeros(shape + (len(ORDER[D]),), dtype=L), np.zeros(shape + (D,), dtype=L)
    GG, T3 = np.zeros(shape, dtype=L), np.zeros(shape + (D,), dtype=L)
    for wi, u, p in zip(w, us, ps):
        d = [u[..., c] - U[..., c] for c in range(D)]
        a = [centre(d[c], c, 1, L) for c in range(D)]
        q = (p - P)[I]
        s = sum(x * x for x in a)
        for k, (ia, ib) in enumerate(ORDER[D]):
            R[..., k] += wi * a[ia] * a[ib]
        for j in range(D):
            PU[..., j] += wi * q * a[j]
            T3[..., j] += wi * s * a[j]
        GG += wi * sum(grad(d[i], i, j, 1, L) ** 2 for i in range(D) for j in range(D))
    return dict(U=U, P=P, R=R / W, PU=PU / W, GG=GG / W, T3=T3 / W)
