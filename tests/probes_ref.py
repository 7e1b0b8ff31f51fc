"""References for waterlily_amd.probes (wl_interp, wl_tracer_advance):

* `interp` / `interp_vec`: a restatement of util.jl:238-257 in the kernel's exact operation order (Python floats are IEEE
  doubles, every operation rounded once): i = floor(x), y = x - i, corners in CartesianIndices order, weight = product of
  the per-direction factors in d order, s = 0.0 then s = s + a[J] * w; a corner of weight exactly 0 is not read; a weighted
  corner outside the array gives NaN.  Vector fields sample component c at x + 0.5 e_c (one double addition).
* `exact`: the same interpolation in exact rational arithmetic (fractions.Fraction) from the Float64-shifted point, with
  the bound sum |a_J| w_J a rounding analysis is scaled by.
* `heun`: one frozen-field Heun step of the tracers, the kernel's rule and order.
Arrays are dense host arrays in the reference's layout (first index fastest; vector components on the last axis)."""
import math
from fractions import Fraction

import numpy as np

NAN = float("nan")


def interp(x, a):
    """scalar field a (D axes) at the 1-based index coordinate x (D floats)"""
    D = a.ndim
    i0, y = [], []
    for d in range(D):
        v = float(x[d])
        if v != v:
            return NAN
        f = math.floor(v)
        if not (0 <= f <= a.shape[d]):
            return NAN
        i0.append(f - 1)
        y.append(v - float(f))
    s = 0.0
    for c in range(1 << D):
        w = 1.0
        J = []
        for d in range(D):
            up = (c >> d) & 1
            wd = y[d] if up else 1.0 - y[d]
            w = wd if d == 0 else w * wd
            J.append(i0[d] + up)
        if w == 0.0:
            continue
        if any(j < 0 or j >= n for j, n in zip(J, a.shape)):
            return NAN
        s = s + float(a[tuple(J)]) * w
    return s


def shifted(x, c):
    p = [float(v) for v in x]
    p[c] = p[c] + 0.5
    return p


def interp_vec(x, u):
    """staggered vector field u (D axes + component axis) at x: component c at x + 0.5 e_c"""
    D = u.ndim - 1
    return np.array([interp(shifted(x, c), u[..., c]) for c in range(D)])


def interp_many(X, a, vector):
    X = np.asarray(X, dtype=np.float64).reshape(-1, (a.ndim - 1) if vector else a.ndim)
    if vector:
        return np.array([interp_vec(x, a) for x in X]).reshape(len(X), -1)
    return np.array([interp(x, a) for x in X])


def exact(x, a, c=None):
    """(value, bound) of the interpolation of the scalar field a (component c of a vector field: a[..., c] at the
    Float64-shifted x + 0.5 e_c) in exact arithmetic; (nan, 0) out of range"""
    if c is not None:
        x = shifted(x, c)
        a = a[..., c]
    D = a.ndim
    X = [Fraction(float(v)) for v in x]
    i0 = [math.floor(v) - 1 for v in X]
    y = [v - math.floor(v) for v in X]
    s, b = Fraction(0), Fraction(0)
    for k in range(1 << D):
        w = Fraction(1)
        J = []
        for d in range(D):
            up = (k >> d) & 1
            w *= y[d] if up else 1 - y[d]
            J.append(i0[d] + up)
        if w == 0:
            continue
        if any(j < 0 or j >= n for j, n in zip(J, a.shape)):
            return NAN, 0.0
        v = Fraction(float(a[tuple(J)]))
        s += v * w
        b += abs(v) * w
    return float(s), float(b)


def wrap(v, N):
    if v < 1.5:
        v = v + N
    if v >= N + 1.5:
        v = v - N
    return v


def heun(X, u, dt, perdir=()):
    """one frozen-field Heun step of the particles X (M, D) on the staggered velocity u (with ghosts)"""
    X = np.array(X, dtype=np.float64, copy=True)
    D = X.shape[1]
    N = [n - 2 for n in u.shape[:D]]
    h = 0.5 * dt
    for q in range(X.shape[0]):
        x = [float(v) for v in X[q]]
        if any(v != v for v in x):
            continue
        k1 = interp_vec(x, u)
        p = []
        for d in range(D):
            v = x[d] + dt * float(k1[d])
            p.append(wrap(v, N[d]) if d in perdir else v)
        k2 = interp_vec(p, u)
        dead, out = False, []
        for d in range(D):
            v = x[d] + h * (float(k1[d]) + float(k2[d]))
            if d in perdir:
                v = wrap(v, N[d])
            elif not (1.5 <= v <= N[d] + 1.5):
                dead = True
            dead = dead or k1[d] != k1[d] or k2[d] != k2[d]
            out.append(v)
        X[q] = NAN if dead else out
    return X


def fill_faces(shape_cells, f, T=np.float64):
    """apply!((i,x)->f(i,x), u) (util.jl:171) on a dense array of extents shape_cells (ghosts included): face i of cell I sits
    at loc(i,I) = I - 1.5 - 0.5 e_i (1-based I)"""
    D = len(shape_cells)
    u = np.zeros(tuple(shape_cells) + (D,), dtype=T, order="F")
    idx = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) + 1 for n in shape_cells], indexing="ij"))
    for i in range(D):
        x = idx - 1.5
        x[i] -= 0.5
        u[..., i] = f(i, x)
    return u


def fill_centres(shape_cells, f, T=np.float64):
    """apply!(x->f(x), a): cell centres at I - 1.5"""
    idx = np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) + 1 for n in shape_cells], indexing="ij"))
    return np.asfortranarray(f(idx - 1.5).astype(T))
