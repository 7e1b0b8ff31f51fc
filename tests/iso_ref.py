"""The isosurface definition of include/wlhip.h (wl_isosurface) restated in numpy: marching tetrahedra on the Kuhn split.

Independent of the device table: the (tet, mask) rule is built here from the text -- inside / outside corners ascending, the
three cases, orientation by the midpoint rule -- and compared with wl_iso_table by tests/test_iso_cpu.py.

    tri, val, edge, cube = extract(a, c, b=None, lo=None, hi=None)
        tri  [nt, 3, 3] Float64 vertices (x = J - 0.5), val [nt, 3] or None,
        edge [nt, 3, 2, 3] the 0-based array indices (P, Q) of the edge every vertex lies on,
        cube [nt, 3] the low corner J of the cube every triangle comes from
"""
import itertools

import numpy as np

PERMS = list(itertools.permutations(range(3)))        # lexicographic: 012, 021, 102, 120, 201, 210


def tet_corners(tet):
    """offsets (4, 3) of the local corners v0..v3 of tetrahedron `tet` from the cube's low corner"""
    p0, p1, _ = PERMS[tet]
    v = np.zeros((4, 3), dtype=np.int64)
    v[1, p0] = 1
    v[2] = v[1]
    v[2, p1] = 1
    v[3] = 1
    return v


def rule(tet, mask):
    """triangles of (tet, mask) as lists of three (p, q) local-corner edges, p < q, oriented towards the outside"""
    V = tet_corners(tet).astype(np.float64)
    I = [v for v in range(4) if (mask >> v) & 1]
    O = [v for v in range(4) if not (mask >> v) & 1]
    e = lambda a, b: (a, b) if a < b else (b, a)
    if len(I) == 1:
        tris = [[e(I[0], O[0]), e(I[0], O[1]), e(I[0], O[2])]]
    elif len(I) == 3:
        tris = [[e(I[0], O[0]), e(I[1], O[0]), e(I[2], O[0])]]
    elif len(I) == 2:
        q = [e(I[0], O[0]), e(I[0], O[1]), e(I[1], O[1]), e(I[1], O[0])]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    else:
        return []
    out = []
    towards = V[O].mean(0) - V[I].mean(0)
    for t in tris:
        m = np.array([(V[p] + V[q]) / 2 for p, q in t])                 # exact in halves
        s = float(np.dot(np.cross(m[1] - m[0], m[2] - m[0]), towards))
        assert s != 0.0
        out.append(t if s > 0 else [t[0], t[2], t[1]])
    return out


TABLE = [[rule(tet, mask) for mask in range(16)] for tet in range(6)]
CORNERS = [tet_corners(tet) for tet in range(6)]


def table_row(tet, mask):
    """what wl_iso_table returns: [ntri, 4p+q ..., -1 ...]"""
    t = TABLE[tet][mask]
    codes = [4 * p + q for tri in t for p, q in tri]
    return [len(t)] + codes + [-1] * (6 - len(codes))


def extract(a, c, b=None, lo=None, hi=None):
    A = np.asarray(a, dtype=np.float64)
    Bf = None if b is None else np.asarray(b, dtype=np.float64)
    n = A.shape
    lo = (1, 1, 1) if lo is None else tuple(int(x) for x in lo)
    hi = tuple(x - 2 for x in n) if hi is None else tuple(int(x) for x in hi)
    assert all(0 <= l <= h <= m - 1 for l, h, m in zip(lo, hi, n)) and np.isfinite(c)
    c = float(c)
    keys, tri, val, edge, cube = [], [], [], [], []
    if all(h > l for l, h in zip(lo, hi)):
        ext = tuple(h - l for l, h in zip(lo, hi))
        m = np.zeros(ext, dtype=np.int64)
        nan = np.zeros(ext, dtype=bool)
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    s = A[lo[0] + dx:hi[0] + dx, lo[1] + dy:hi[1] + dy, lo[2] + dz:hi[2] + dz]
                    m |= (s < c).astype(np.int64) << (dx + 2 * dy + 4 * dz)
                    nan |= np.isnan(s)
        rel = np.argwhere((m != 0) & (m != 255) & ~nan)
        mm = m[rel[:, 0], rel[:, 1], rel[:, 2]]
        lin = rel[:, 0] + ext[0] * (rel[:, 1] + ext[1] * rel[:, 2])         # ascending linear index, x fastest
        J = rel + np.array(lo)
        at = lambda F, I: F[I[..., 0], I[..., 1], I[..., 2]]
        for tet in range(6):
            V = CORNERS[tet]
            m4 = sum(((mm >> int(V[v, 0] + 2 * V[v, 1] + 4 * V[v, 2])) & 1) << v for v in range(4))
            for mask in range(1, 15):
                sel = m4 == mask
                if not sel.any():
                    continue
                for s, t in enumerate(TABLE[tet][mask]):
                    P = J[sel][:, None, :] + V[[p for p, _ in t]][None]                 # [ns, 3 vertices, 3]
                    Q = J[sel][:, None, :] + V[[q for _, q in t]][None]
                    ap, aq = at(A, P), at(A, Q)
                    with np.errstate(divide="ignore", invalid="ignore"):
                        tt = (c - ap) / (aq - ap)
                    tri.append(np.where(Q != P, (P - 0.5) + tt[..., None], P - 0.5))
                    edge.append(np.stack([P, Q], axis=2))
                    cube.append(J[sel])
                    keys.append(lin[sel] * 12 + 2 * tet + s)
                    if Bf is not None:
                        bp, bq = at(Bf, P), at(Bf, Q)
                        with np.errstate(invalid="ignore"):
                            val.append(bp + tt * (bq - bp))
    if not keys:
        return (np.zeros((0, 3, 3)), None if Bf is None else np.zeros((0, 3)), np.zeros((0, 3, 2, 3), dtype=np.int64),
                np.zeros((0, 3), dtype=np.int64))
    order = np.argsort(np.concatenate(keys), kind="stable")
    cat = lambda parts: np.concatenate(parts)[order]
    return cat(tri), (None if Bf is None else cat(val)), cat(edge), cat(cube)


def edges_of(tri):
    """Recover the edge (P, Q) every vertex lies on from its position alone: P = floor(x + 0.5), Q = P + 1 in the non-integer
    components of x + 0.5 (an edge, a face diagonal or the body diagonal: they all share the one t).  [nt, 3, 2, 3] int64; a
    vertex without a non-integer component gives -1."""
    y = np.asarray(tri, dtype=np.float64) + 0.5
    P = np.floor(y)
    frac = y != P
    out = np.stack([P, P + frac], axis=2).astype(np.int64)
    out[frac.sum(-1) == 0] = -1
    return out


def closed(tri):
    """every directed edge occurs once and its reverse once, compared by bits"""
    t = np.ascontiguousarray(tri, dtype=np.float64).view(np.uint64).reshape(-1, 3, 3)
    d = np.concatenate([np.concatenate([t[:, k], t[:, (k + 1) % 3]], axis=1) for k in range(3)])     # [3 nt, 6]
    r = np.concatenate([d[:, 3:], d[:, :3]], axis=1)
    ud, cd = np.unique(d, axis=0, return_counts=True)
    ur = np.unique(r, axis=0)
    return len(d) > 0 and bool(np.all(cd == 1)) and ud.shape == ur.shape and bool(np.array_equal(ud, ur))


def area(tri):
    t = np.asarray(tri, dtype=np.float64)
    return float(0.5 * np.linalg.norm(np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]), axis=1).sum())


def normals(tri):
    t = np.asarray(tri, dtype=np.float64)
    return np.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0])


def volume(tri):
    t = np.asarray(tri, dtype=np.float64)
    return float(np.einsum("ij,ij->i", t[:, 0], np.cross(t[:, 1], t[:, 2])).sum() / 6.0)
