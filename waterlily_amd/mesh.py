"""MeshBody: a closed triangle mesh as an immersed body, measured by the HIP kernels of csrc/wl_mesh.h.

The mesh lives in xi = A(t) x + b(t) (an `AffineMap` of waterlily_amd.body, as for the parametric bodies) and the map
must be a similarity at every measured time, so that distances in x are distances in xi divided by the scale factor.
There is no torch path for a mesh: `Simulation(..., geometry="host")` and 2-D are refused.
"""
from __future__ import annotations

import ctypes as C
import struct
from typing import Optional

import numpy as np

from . import _lib
from .body import AffineMap


def _directed_edges(tri: np.ndarray) -> np.ndarray:
    return np.concatenate([tri[:, [0, 1]], tri[:, [1, 2]], tri[:, [2, 0]]]).astype(np.int64)


def enclosed_volume(vertices, triangles) -> float:
    """divergence theorem on the triangles, Float64: sum a . (b x c) / 6"""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(triangles)[:, k]] for k in range(3))
    return float(np.sum(np.einsum("ij,ij->i", a, np.cross(b, c))) / 6.0)


def centroid(vertices, triangles) -> np.ndarray:
    """centre of volume of the enclosed solid (signed tetrahedra against the origin)"""
    v = np.asarray(vertices, dtype=np.float64)
    a, b, c = (v[np.asarray(triangles)[:, k]] for k in range(3))
    w = np.einsum("ij,ij->i", a, np.cross(b, c)) / 6.0
    return np.sum(w[:, None] * (a + b + c) / 4.0, axis=0) / np.sum(w)


def validate(vertices: np.ndarray, triangles: np.ndarray) -> None:
    """Raise a ValueError that names the defect: NaN coordinates, indices out of range, degenerate triangles, not closed,
    inconsistently oriented, inside-out."""
    if vertices.ndim != 2 or vertices.shape[1] != 3 or triangles.ndim != 2 or triangles.shape[1] != 3 or len(triangles) == 0:
        raise ValueError("MeshBody: vertices must be (nv,3) and triangles a non-empty (nt,3)")
    if not np.all(np.isfinite(vertices)):
        raise ValueError("MeshBody: NaN (or infinite) vertex coordinates")
    if triangles.min() < 0 or triangles.max() >= len(vertices):
        raise ValueError("MeshBody: triangle indices out of range (0-based, < number of vertices)")
    a, b, c = (vertices[triangles[:, k]] for k in range(3))
    area2 = np.linalg.norm(np.cross(b - a, c - a), axis=1)
    if np.any(area2 == 0.0):
        raise ValueError(f"MeshBody: degenerate (zero-area) triangles, the first at index {int(np.argmax(area2 == 0.0))}")
    e = _directed_edges(triangles)
    nv = int(len(vertices))
    und = np.minimum(e[:, 0], e[:, 1]) * nv + np.maximum(e[:, 0], e[:, 1])
    _, cnt = np.unique(und, return_counts=True)
    if np.any(cnt != 2):
        raise ValueError(f"MeshBody: the mesh is not closed: {int(np.sum(cnt != 2))} edges are not shared by exactly two triangles")
    _, dcnt = np.unique(e[:, 0] * nv + e[:, 1], return_counts=True)
    if np.any(dcnt != 1):
        raise ValueError("MeshBody: inconsistently oriented triangles: a shared edge is traversed twice in the same direction")
    if enclosed_volume(vertices, triangles) < 0:
        raise ValueError("MeshBody: negative enclosed volume: the mesh is inside-out (normals point inwards); pass flip=True")


def read_stl(path):
    """(vertices (nv,3) float64, triangles (nt,3) int32) of a binary or ASCII STL file; vertices welded by exact
    coordinate equality."""
    raw = open(path, "rb").read()
    nt_bin = struct.unpack("<I", raw[80:84])[0] if len(raw) >= 84 else -1
    if len(raw) == 84 + 50 * nt_bin:
        rec = np.frombuffer(raw, dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]), offset=84, count=nt_bin)
        pts = rec["v"].reshape(-1, 3).astype(np.float64)
    else:
        rows = [ln.split()[1:4] for ln in raw.decode("ascii", errors="replace").splitlines() if ln.strip().startswith("vertex")]
        pts = np.array(rows, dtype=np.float64).reshape(-1, 3)
        if len(pts) == 0 or len(pts) % 3:
            raise ValueError(f"{path}: neither a binary STL (size != 84 + 50 * count) nor an ASCII STL with 3 vertices per facet")
    pts = pts + 0.0                                        # -0.0 welds with 0.0
    verts, inv = np.unique(pts, axis=0, return_inverse=True)
    return verts, inv.reshape(-1, 3).astype(np.int32)


def write_stl(path, vertices, triangles) -> None:
    """binary STL (Float32 coordinates, facet normals by the right-hand rule)"""
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles)
    p = v[t]
    n = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    ln = np.linalg.norm(n, axis=1, keepdims=True)
    n = np.divide(n, ln, out=np.zeros_like(n), where=ln > 0)
    rec = np.zeros(len(t), dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    rec["n"], rec["v"] = n, p
    with open(path, "wb") as f:
        f.write(b"waterlily_amd binary STL".ljust(80, b" "))
        f.write(struct.pack("<I", len(t)))
        f.write(rec.tobytes())


def similarity_scale(A: np.ndarray) -> float:
    """s with A A^T = s^2 I (Float64); a ValueError for anything that is not rotation x uniform scale"""
    A = np.asarray(A, dtype=np.float64)
    G = A @ A.T
    s2 = float(np.trace(G)) / 3.0
    if not (s2 > 0 and np.isfinite(s2)) or np.max(np.abs(G - s2 * np.eye(3))) > 1e-10 * s2:
        raise ValueError("MeshBody: the map is not a similarity (A A^T != s^2 I): only rotation x uniform scale + translation "
                         "keeps distances, shear or non-uniform scaling is refused")
    return float(np.sqrt(s2))


class MeshBody:
    """`MeshBody(vertices, triangles, map=None, scale=1.0)`: vertices (nv,3) float, triangles (nt,3) int, 0-based, outward by
    the right-hand rule; `map` an AffineMap giving xi = A(t) x + b(t); the mesh lives in xi space, multiplied by `scale`."""

    def __init__(self, vertices, triangles, map: Optional[AffineMap] = None, scale: float = 1.0, flip: bool = False):
        if map is not None and not isinstance(map, AffineMap):
            raise TypeError("MeshBody: `map` must be an AffineMap (body.translation, body.rotation3d, ...)")
        v = np.array(vertices, dtype=np.float64)
        t = np.array(triangles)
        if t.size and not np.issubdtype(t.dtype, np.integer):
            raise ValueError("MeshBody: triangles must be integers")
        t = t.astype(np.int64)
        if flip and t.ndim == 2:
            t = t[:, ::-1]
        validate(v, t)
        self.vertices = np.ascontiguousarray(v * float(scale))
        self.triangles = np.ascontiguousarray(t.astype(np.int32))
        self.amap = map
        self.identity_map = map is None
        self._h, self._R = None, 0.0

    @classmethod
    def from_stl(cls, path, map=None, scale=1.0, flip=False):
        v, t = read_stl(path)
        return cls(v, t, map=map, scale=scale, flip=flip)

    @property
    def volume(self) -> float:
        return enclosed_volume(self.vertices, self.triangles)

    @property
    def centroid(self) -> np.ndarray:
        return centroid(self.vertices, self.triangles)

    def coeffs(self, t: float):
        """(A, b, dA/dt, db/dt, A^-1, s) at time t, Float64; refuses a map that is not a similarity"""
        if self.amap is None:
            I, Z = np.eye(3), np.zeros((3, 3))
            return I, np.zeros(3), Z, np.zeros(3), I, 1.0
        A, b, dA, db = (np.asarray(q, dtype=np.float64) for q in self.amap.coeffs(float(t)))
        if A.shape != (3, 3):
            raise ValueError("MeshBody: the map must be 3-D")
        s = similarity_scale(A)
        inv = getattr(self.amap, "inverse", None)
        Ai = np.asarray(inv(float(t)), dtype=np.float64) if inv is not None else A.T / (s * s)
        return A, b, dA, db, Ai, s

    def pose(self, t: float):
        """(wl_mesh_pose, s) at time t"""
        A, b, dA, db, Ai, s = self.coeffs(t)
        p = _lib.MeshPose()
        for name, M in (("A", A), ("dA", dA), ("Ainv", Ai)):
            getattr(p, name)[:] = list(M.ravel())
        for name, vec in (("b", b), ("db", db)):
            getattr(p, name)[:] = list(vec)
        p.identity_map = int(self.amap is None)
        return p, s

    def handle(self, need: float):
        """the wl_mesh handle whose exact radius (xi units) is at least `need`; (re)built only when it is not.  It is built
        with a relative margin of 1e-6 over `need`: the scale factor of a rotating map, computed in floating point at every
        measure!, wanders by an ulp from step to step, and that must neither rebuild the bins nor be refused by the library."""
        if self._h is None or self._R < need:
            self.close()
            R = max(float(need) * (1.0 + 1e-6), 3.5)
            h = C.c_void_p()
            _lib.check(_lib.lib().wl_mesh_create(C.byref(h), self.vertices.ctypes.data_as(C.c_void_p), len(self.vertices),
                                                 self.triangles.ctypes.data_as(C.c_void_p), len(self.triangles), R))
            self._h, self._R = h, R
        return self._h

    def native(self, t: float, eps: float):
        """(handle, pose) for a measure! at time t: the exact zone reaches 2 + eps + 1 cells in x"""
        p, s = self.pose(t)
        return self.handle((3.0 + float(eps)) * s), p

    def info(self) -> dict:
        out = (C.c_int64 * 8)()
        _lib.check(_lib.lib().wl_mesh_info(self._h, out))
        keys = ("nt", "nv", "bins", "max_per_bin", "entries", "nonempty_bins", "device_bytes", "crossed_bins")
        return dict(zip(keys, (int(v) for v in out)))

    def eval_host(self, x, t: float = 0.0, eps: float = 1.0, fastd2: float = np.inf):
        """(d, n, V) at the points x (n,3) from the library's host twin of the kernels' distance function (no device)"""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, 3))
        h, p = self.native(t, eps)
        d, n, V = np.empty(len(x)), np.empty((len(x), 3)), np.empty((len(x), 3))
        _lib.check(_lib.lib().wl_mesh_eval_host(h, C.byref(p), x.ctypes.data_as(C.c_void_p), len(x), float(min(fastd2, 1e300)),
                                                d.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p)))
        return d, n, V

    def close(self) -> None:
        if self._h is not None:
            _lib.lib().wl_mesh_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _refuse(self, *_):
        raise TypeError("MeshBody does not combine with other bodies: concatenate disjoint meshes into one MeshBody")

    __add__ = __or__ = __and__ = __sub__ = __neg__ = _refuse
