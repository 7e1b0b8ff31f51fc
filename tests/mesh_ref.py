"""The checker for MeshBody: signed distance to a closed triangle mesh by brute force in numpy Float64 over ALL triangles
for every query point -- no bins, no early exit, and a different closest-point formulation from the product's (projection
onto the face plane + an inside test, else the nearest of the three clamped edge projections; the product classifies
Voronoi regions).  Pinned on the CPU by closed forms in tests/test_mesh_cpu.py."""
import numpy as np

FACE, EDGE, VERTEX = 0, 1, 2


class Ref:
    def __init__(self, vertices, triangles):
        self.v = np.asarray(vertices, dtype=np.float64)
        self.t = np.asarray(triangles, dtype=np.int64)
        a, b, c = (self.v[self.t[:, k]] for k in range(3))
        self.a, self.b, self.c = a, b, c
        nf = np.cross(b - a, c - a)
        self.nf = nf / np.linalg.norm(nf, axis=1, keepdims=True)
        # edge pseudonormals: the sum of the two faces' unit normals, keyed by the undirected edge
        en = {}
        for q, tri in enumerate(self.t):
            for k in range(3):
                key = (min(tri[k], tri[(k + 1) % 3]), max(tri[k], tri[(k + 1) % 3]))
                en[key] = en.get(key, 0.0) + self.nf[q]
        self.en = np.zeros((len(self.t), 3, 3))
        for q, tri in enumerate(self.t):
            for k in range(3):
                s = en[(min(tri[k], tri[(k + 1) % 3]), max(tri[k], tri[(k + 1) % 3]))]
                self.en[q, k] = s / np.linalg.norm(s)
        # vertex pseudonormals: face normals weighted by the face's angle at the vertex
        vn = np.zeros_like(self.v)
        P = np.stack([a, b, c], axis=1)
        for k in range(3):
            u, w = P[:, (k + 1) % 3] - P[:, k], P[:, (k + 2) % 3] - P[:, k]
            cosang = np.einsum("ij,ij->i", u, w) / (np.linalg.norm(u, axis=1) * np.linalg.norm(w, axis=1))
            np.add.at(vn, self.t[:, k], np.arccos(np.clip(cosang, -1, 1))[:, None] * self.nf)
        self.vn = vn / np.linalg.norm(vn, axis=1, keepdims=True)

    def _closest(self, x):
        """x (q,3) -> closest points (q,nt,3), kind (q,nt), local feature index (q,nt)"""
        a, b, c, nf = self.a[None], self.b[None], self.c[None], self.nf[None]
        X = x[:, None, :]
        hgt = np.einsum("qtk,qtk->qt", X - a, np.broadcast_to(nf, (len(x),) + nf.shape[1:]))
        p0 = X - hgt[..., None] * nf
        inside = np.ones(hgt.shape, dtype=bool)
        for p, q in ((a, b), (b, c), (c, a)):
            inside &= np.einsum("qtk,qtk->qt", np.cross(np.broadcast_to(q - p, p0.shape), p0 - p), np.broadcast_to(nf, p0.shape)) >= 0
        best = np.where(inside[..., None], p0, 0.0)
        kind = np.where(inside, FACE, -1)
        loc = np.zeros(hgt.shape, dtype=np.int64)
        bd = np.where(inside, 0.0, np.inf)           # only used to choose among the edges of non-inside points
        for k, (p, q) in enumerate(((a, b), (b, c), (c, a))):
            e = q - p
            s = np.clip(np.einsum("qtk,qtk->qt", X - p, np.broadcast_to(e, p0.shape)) / np.einsum("qtk,qtk->qt", e, e), 0.0, 1.0)
            cp = p + s[..., None] * e
            dd = np.einsum("qtk,qtk->qt", X - cp, X - cp)
            take = (~inside) & (dd < bd)
            best = np.where(take[..., None], cp, best)
            bd = np.where(take, dd, bd)
            kind = np.where(take, np.where((s == 0.0) | (s == 1.0), VERTEX, EDGE), kind)
            loc = np.where(take, np.where(s == 1.0, (k + 1) % 3, k), loc)
        return best, kind, loc

    def query(self, x, chunk=None):
        """dict of d (signed), c (closest point), kind, pn (unit pseudonormal of the closest feature), n (gradient: (x-c)/d,
        pn where |d| < 1e-9), gap (to the second-closest triangle whose closest point is farther than 1e-6 from the first's)"""
        x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
        chunk = chunk or max(1, int(2e6) // max(1, len(self.t)))
        out = {k: [] for k in ("d", "c", "kind", "pn", "n", "gap")}
        for lo in range(0, len(x), chunk):
            xs = x[lo:lo + chunk]
            cp, kind, loc = self._closest(xs)
            dist = np.linalg.norm(xs[:, None, :] - cp, axis=2)
            w = np.argmin(dist, axis=1)
            r = np.arange(len(xs))
            c, k, l, du = cp[r, w], kind[r, w], loc[r, w], dist[r, w]
            pn = np.where((k == FACE)[:, None], self.nf[w],
                          np.where((k == EDGE)[:, None], self.en[w, l], self.vn[self.t[w, l]]))
            sgn = np.where(np.einsum("ij,ij->i", xs - c, pn) < 0, -1.0, 1.0)
            d = sgn * du
            with np.errstate(invalid="ignore", divide="ignore"):
                n = np.where((du < 1e-9)[:, None], pn, (xs - c) / d[:, None])
            other = np.linalg.norm(cp - c[:, None, :], axis=2) > 1e-6
            gap = np.min(np.where(other, dist, np.inf), axis=1) - du
            for key, val in (("d", d), ("c", c), ("kind", k), ("pn", pn), ("n", n), ("gap", gap)):
                out[key].append(val)
        return {k: np.concatenate(v) for k, v in out.items()}


def kern(d):
    return 0.5 + 0.5 * np.cos(np.pi * d)


def kern0(d):
    return 0.5 + 0.5 * d + 0.5 * np.sin(np.pi * d) / np.pi


def kern1(d):
    return 0.25 * (1 - d * d) - 0.5 * (d * np.sin(np.pi * d) + (1 + np.cos(np.pi * d)) / np.pi) / np.pi


def measure(ref: Ref, pose, x, fastd2=np.inf):
    """measure(body, x, t; fastd2) (src/AutoBody.jl:115-131) with the mesh as the sdf of xi = A x + b, A = s * rotation:
    (d, n, V, gap) in x units; n = V = 0 where d^2 > fastd2.  pose = (A, b, dA, db, Ainv, s)."""
    A, b, dA, db, Ai, s = pose
    x = np.asarray(x, dtype=np.float64).reshape(-1, 3)
    q = ref.query(x @ A.T + b)
    d = q["d"] / s
    n = (q["n"] @ A) / s
    V = -((x @ dA.T + db) @ Ai.T)
    far = d * d > fastd2
    n[far] = 0.0
    V[far] = 0.0
    return d, n, V, q["gap"] / s
