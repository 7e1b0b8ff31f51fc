"""numpy restatement of MeanFlow's update rule (waterlily_amd/stats.py, include/wlhip.h: wl_meanflow_update), written from the
rule itself, not from the kernel: with eps = dt / (t - t0) (Float64, exactly 1 on the first update of a window),
per element, in double arithmetic with one rounding to the accumulator type A per stored value,

    d = u - U;  U <- U + eps d;  UU_ij <- (1 - eps) (UU_ij + eps d_i d_j);  the same for P, pp with d = p - P;

on the first update U = u, P = p, UU = pp = 0.  Also the NAIVE form <uu> - <u><u> (running means of u and u*u in A
arithmetic), used only to show what storing the covariance avoids."""
import numpy as np

ORDER = {1: ((0, 0),), 2: ((0, 0), (1, 1), (0, 1)), 3: ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))}


def eps_schedule(t_seen, t):
    """None when dt == 0, eps otherwise; dt < 0 raises ValueError"""
    dt = float(t) - float(t_seen[-1])
    if dt < 0:
        raise ValueError("time went back")
    if dt == 0:
        return None
    return dt / (float(t) - float(t_seen[0]))


class RefMean:
    """host arrays U (N..., D), P (N...), UU (N..., D(D+1)/2), pp (N...) of dtype A"""

    def __init__(self, D, A, t_init, uu=True, pp=True):
        self.D, self.A = D, np.dtype(A)
        self.t = [float(t_init)]
        self.uu, self.ppf = uu, pp
        self.U = self.P = self.UU = self.pp = None

    def reset(self, t_init=None):
        self.t = [self.t[-1] if t_init is None else float(t_init)]

    def update(self, u, p, t):
        eps = eps_schedule(self.t, t)
        if eps is None:
            return None
        A = self.A
        u64, p64 = np.asarray(u, dtype=np.float64), np.asarray(p, dtype=np.float64)
        if len(self.t) == 1:
            self.U, self.P = u64.astype(A), p64.astype(A)
            self.UU = np.zeros(u64.shape[:-1] + (len(ORDER[self.D]),), dtype=A) if self.uu else None
            self.pp = np.zeros(p64.shape, dtype=A) if self.ppf else None
        else:
            U = self.U.astype(np.float64)
            d = u64 - U
            self.U = (U + eps * d).astype(A)
            if self.uu:
                S = self.UU.astype(np.float64)
                for q, (a, b) in enumerate(ORDER[self.D]):
                    S[..., q] = (1.0 - eps) * (S[..., q] + eps * d[..., a] * d[..., b])
                self.UU = S.astype(A)
            P = self.P.astype(np.float64)
            dp = p64 - P
            self.P = (P + eps * dp).astype(A)
            if self.ppf:
                self.pp = ((1.0 - eps) * (self.pp.astype(np.float64) + eps * dp * dp)).astype(A)
        self.t.append(float(t))
        return eps


def naive_variance(xs, dts, A=np.float32):
    """<x^2> - <x>^2 from running means of x and x*x kept in A arithmetic (the form MeanFlow does NOT use)"""
    A = np.dtype(A).type
    m1 = m2 = A(0)
    T = 0.0
    for x, dt in zip(xs, dts):
        T += dt
        e = A(dt / T)
        x = A(x)
        m1 = A(m1 + e * A(x - m1))
        m2 = A(m2 + e * A(A(x * x) - m2))
    return float(A(m2 - A(m1 * m1)))


def robust_variance(xs, dts, A=np.float32):
    """the rule above on one element (times t_n = t_{n-1} + dt_n from t_0 = 0): double arithmetic, A storage"""
    A = np.dtype(A).type
    U = S = None
    seen = [0.0]
    for x, dt in zip(xs, dts):
        t = seen[-1] + dt
        e = eps_schedule(seen, t)
        x = float(A(x))
        if len(seen) == 1:
            U, S = A(x), A(0)
        else:
            d = x - float(U)
            U = A(float(U) + e * d)
            S = A((1.0 - e) * (float(S) + e * d * d))
        seen.append(t)
    return float(S)


def exact_variance(xs, dts, A=np.float32):
    """the dt-weighted variance of the A-rounded samples, two-pass in long double"""
    x = np.asarray([A(v) for v in xs], dtype=np.longdouble)
    w = np.asarray(dts, dtype=np.longdouble)
    m = (w * x).sum() / w.sum()
    return float((w * (x - m) ** 2).sum() / w.sum())


def cancellation_signal(n=2000, a=5.0, b=5e-3):
    """u_n = a + b s_n (a / b = 1e3) with a fixed zero-mean, unit-variance sequence s_n, and uneven dt_n"""
    k = np.arange(n, dtype=np.float64)
    s = np.sqrt(2.0) * np.sin(0.7 * k + 0.3)
    dts = 0.1 + 0.05 * np.cos(0.37 * k) ** 2
    return a + b * s, dts
