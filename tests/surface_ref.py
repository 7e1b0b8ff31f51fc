"""Reference for waterlily_amd.surface (wl_surface_sample, wl_surface_totals): the formulas of the SurfaceLoads issue in numpy
Float64, written from their statement and not from the kernel.

Triangle t of a mesh in xi = A x + b, at one pose (A, b, dA, db, Ainv), or the identity map (pose None):
    x_v = Ainv (xi_v - b);  x_c = (x_a + x_b + x_c) / 3;  S = (x_b - x_a) x (x_c - x_a) / 2;  n = S / |S|
    V_b = -Ainv (dA x_c + db)                                        (0 for the identity map)
    X = x_c + delta n + 1.5                                          (index coordinates, probes_ref's convention)
    p_t = interp(X, p);  G_ij = u_i(X + e_j/2) - u_i(X - e_j/2), u_i = component i of probes_ref.interp_vec (sampled at + e_i/2)
    tau = -nu (G + G^T) n
    Fp = sum p_t S;  Fv = sum tau |S|;  Mp = sum (x_c - x0) x p_t S;  Mv = sum (x_c - x0) x tau |S|
Fields are dense host arrays with ghost cells (first index fastest, components last); interpolation is probes_ref.interp, so
a weighted corner outside the array gives NaN, which spreads through the arithmetic exactly as IEEE spreads it."""
import numpy as np

import probes_ref as R


def geometry(vertices, triangles, pose=None):
    """dict of x-space vertices xv [nt, 3, 3], centroid, S, area, n, Vb for pose = (A, b, dA, db, Ainv, ...) or None"""
    xi = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles)]
    if pose is None:
        xv = xi.copy()
    else:
        b, Ai = np.asarray(pose[1], dtype=np.float64), np.asarray(pose[4], dtype=np.float64)
        xv = (xi - b) @ Ai.T
    xc = (xv[:, 0] + xv[:, 1] + xv[:, 2]) / 3.0
    S = 0.5 * np.cross(xv[:, 1] - xv[:, 0], xv[:, 2] - xv[:, 0])
    area = np.linalg.norm(S, axis=1)
    n = S / area[:, None]
    if pose is None:
        Vb = np.zeros_like(xc)
    else:
        dA, db = np.asarray(pose[2], dtype=np.float64), np.asarray(pose[3], dtype=np.float64)
        Vb = -((xc @ dA.T + db) @ Ai.T)
    return {"xv": xv, "centroid": xc, "S": S, "area": area, "n": n, "Vb": Vb}


def sample(geo, p, u, delta, nu):
    """(p_t [nt], tau [nt, 3], G [nt, 3, 3]) at x_c + delta n"""
    X = geo["centroid"] + delta * geo["n"] + 1.5
    nt = len(X)
    pt, G = np.empty(nt), np.empty((nt, 3, 3))
    for t in range(nt):
        x = [float(v) for v in X[t]]
        pt[t] = R.interp(x, p)
        for j in range(3):
            hi, lo = list(x), list(x)
            hi[j] = x[j] + 0.5
            lo[j] = x[j] - 0.5
            G[t, :, j] = R.interp_vec(hi, u) - R.interp_vec(lo, u)
    with np.errstate(invalid="ignore"):
        tau = -nu * np.einsum("tij,tj->ti", G + np.swapaxes(G, 1, 2), geo["n"])
    return pt, tau, G


def totals(geo, pt, tau, x0):
    """(Fp, Fv, Mp, Mv), each [3]"""
    fp = pt[:, None] * geo["S"]
    fv = tau * geo["area"][:, None]
    d = geo["centroid"] - np.asarray(x0, dtype=np.float64)
    return fp.sum(0), fv.sum(0), np.cross(d, fp).sum(0), np.cross(d, fv).sum(0)


def linear_fields(shape_cells, g, c, M, cu, T):
    """p = g . x + c at the cell centres and u_i = (M x)_i + cu_i at the faces of component i, rounded to T (ghosts included)"""
    g, M, cu = np.asarray(g, dtype=np.float64), np.asarray(M, dtype=np.float64), np.asarray(cu, dtype=np.float64)
    p = R.fill_centres(shape_cells, lambda x: np.tensordot(g, x, 1) + c, T)
    u = R.fill_faces(shape_cells, lambda i, x: np.tensordot(M[i], x, 1) + cu[i], T)
    return p, u
