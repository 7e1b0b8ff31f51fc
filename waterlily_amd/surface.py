"""Where on a MeshBody the load acts: pressure and viscous traction per triangle, their sums and moments recorded during a run,
time averages, and a surface file ParaView opens.

    sl = SurfaceLoads(sim, mean=True)                # sim.body is a MeshBody; delta = sim.eps + 1, x0 = the centroid at t = 0
    for _ in range(n):
        sim_step(sim)
        record(sl, sim)                              # two C calls (three kernel launches), no synchronisation
    t, v = series(sl)                                # v[k] = (Fp, Fv, Mp, Mv) after step k, columns(sl) names them
    f = fields(sl)                                   # numpy: centroid, area_vector, body_velocity, p, traction, mean_p, ..
    write_vtp("hull.vtp", sl)                        # the triangles with those arrays as cell data
    tot = loads(sim)                                 # one-off, synchronous: {"Fp_x": .., .., "Mv_z": ..}

Triangle t is sampled at x_c + delta n (centroid, outward unit normal, at the pose of time(sim.flow)): p_t = interp(p) and
tau = -nu (G + G^T) n with G the central difference of the interpolated velocity over one cell.  p_t S (S = area n) is the
triangle's pressure load and tau |S| its viscous load, with the signs of pressure_force / viscous_force, so Fp and Fv are
their surface counterparts.  Formulas, the NaN rule and slab ownership: include/wlhip.h (wl_surface_sample,
wl_surface_totals) and csrc/wl_surface.h.  Lengths are grid units of x, values Float64 for either flow type.  On z-slabs
every rank holds partial rows and partial totals and nothing is communicated per step; series(), fields() and loads()
sum the ranks at the host and must be called by every rank.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Tuple

import numpy as np
import torch

from . import _lib
from . import sim as S
from ._lib import check
from .mesh import MeshBody
from ._series import _rank_sum
from .stats import weight
from .vtk import data_array

COLUMNS = tuple(f"{k}_{a}" for k in ("Fp", "Fv", "Mp", "Mv") for a in "xyz")


def _to_x(body: MeshBody, xi: np.ndarray, t: float) -> np.ndarray:
    """points of xi space in x space at time t: Ainv (xi - b)"""
    if body.amap is None:
        return np.array(xi, dtype=np.float64, copy=True)
    _, b, _, _, Ai, _ = body.coeffs(t)
    return (np.asarray(xi, dtype=np.float64) - b) @ Ai.T


class SurfaceLoads:
    """Sampler and recorder of the surface loads of sim.body.  rows [nt, 4] = (p, tau_x, tau_y, tau_z), geom [nt, 9] =
    (centroid, area vector, body velocity) and mean [nt, 4] (mean=True: the time average of rows since the object was made or
    reset) are Float64 device arrays of the last sample; buf [capacity, 12] is a device ring of the recorded totals, t the
    host list of their times (the ring keeps the last `capacity` records)."""

    def __init__(self, sim, delta=None, x0=None, mean: bool = False, capacity: int = 4096):
        body = getattr(sim, "body", None)
        if not isinstance(body, MeshBody):
            raise TypeError(f"SurfaceLoads: sim.body must be a MeshBody, not {type(body).__name__}")
        if capacity < 1:
            raise ValueError("SurfaceLoads: capacity must be >= 1")
        self.delta = float(sim.eps) + 1.0 if delta is None else float(delta)
        if not (np.isfinite(self.delta) and self.delta >= 0):
            raise ValueError("SurfaceLoads: delta must be finite and >= 0")
        self.body, self.nt = body, len(body.triangles)
        self.x0 = _to_x(body, body.centroid, 0.0) if x0 is None else np.asarray(x0, dtype=np.float64).reshape(3)
        self._x03 = _lib.d3(self.x0)
        flow = sim.flow
        self.slab = flow.layout.slab
        z = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=flow.device)
        self.rows, self.geom = z(self.nt, 4), z(self.nt, 9)
        self.mean = z(self.nt, 4) if mean else None
        self.buf = z(int(capacity), 12)
        self.t: List[float] = []
        self.time = None                      # time of the last sample
        self._tm = [S.time(flow)]             # the averaging window: its start, then the times blended in


def columns(sl: SurfaceLoads) -> Tuple[str, ...]:
    return COLUMNS


def sample(sl: SurfaceLoads, sim) -> None:
    """Sample every triangle at time(sim.flow) into sl.rows / sl.geom and blend the rows into sl.mean (weight dt / (t - t0),
    MeanFlow's; a repeated time is not blended twice): one kernel launch, no synchronisation."""
    if sim.body is not sl.body or sim.flow.layout.slab is not sl.slab:
        raise ValueError("SurfaceLoads: the simulation's body or slab differs from the one the object was made for")
    flow = sim.flow
    t = S.time(flow)
    w = weight(sl._tm, t) if sl.mean is not None else None
    h, pose = sl.body.native(t, sim.eps)
    g = flow.layout.grid()
    check(_lib.lib().wl_surface_sample(S._WLT[flow.T], C.byref(g), S._ptr(flow.p), S._ptr(flow.u), h, C.byref(pose), sl.delta,
                                       flow.nu, S._ptr(sl.rows), S._ptr(sl.geom), None if w is None else S._ptr(sl.mean),
                                       1.0 if w is None else w, int(len(sl._tm) == 1)))
    if w is not None:
        sl._tm.append(t)
    sl.time = t


def _totals(sl: SurfaceLoads, out: torch.Tensor) -> None:
    check(_lib.lib().wl_surface_totals(S._ptr(sl.rows), S._ptr(sl.geom), sl.nt, sl._x03, S._ptr(out)))


def record(sl: SurfaceLoads, sim) -> None:
    """sample, then the twelve totals about sl.x0 into the next row of the ring, with the time: no synchronisation."""
    sample(sl, sim)
    _totals(sl, sl.buf[len(sl.t) % sl.buf.shape[0]])
    sl.t.append(sl.time)


def series(sl: SurfaceLoads) -> Tuple[np.ndarray, np.ndarray]:
    """(t[K], totals[K, 12]) of the last K <= capacity records, oldest first (synchronises; on z-slabs every rank must call
    it: the ranks' partial totals are summed once, here)."""
    n, cap = len(sl.t), sl.buf.shape[0]
    K = min(n, cap)
    order = [(n - K + k) % cap for k in range(K)]
    v = _rank_sum(sl.buf.cpu().numpy()[order], sl.slab)
    return np.asarray(sl.t[n - K:], dtype=np.float64), v


def reset(sl: SurfaceLoads) -> None:
    """Forget the records and start a new averaging window at the last time seen (the buffers keep their size)."""
    sl.t = []
    sl._tm = [sl._tm[-1]]


def fields(sl: SurfaceLoads) -> Dict[str, np.ndarray]:
    """The last sample as numpy arrays over the triangles: centroid, area_vector, body_velocity [nt, 3], p [nt], traction
    [nt, 3], and mean_p, mean_traction when the mean is kept (synchronises; every rank of a slab run must call it)."""
    if sl.time is None:
        raise ValueError("SurfaceLoads: nothing sampled yet")
    g = sl.geom.cpu().numpy()
    r = _rank_sum(sl.rows.cpu().numpy(), sl.slab)
    out = {"centroid": g[:, 0:3].copy(), "area_vector": g[:, 3:6].copy(), "body_velocity": g[:, 6:9].copy(),
           "p": r[:, 0].copy(), "traction": r[:, 1:4].copy()}
    if sl.mean is not None:
        m = _rank_sum(sl.mean.cpu().numpy(), sl.slab)
        out["mean_p"], out["mean_traction"] = m[:, 0].copy(), m[:, 1:4].copy()
    return out


def loads(sim, delta=None, x0=None) -> Dict[str, float]:
    """The twelve totals now, by name (synchronous; on z-slabs every rank must call it)."""
    sl = SurfaceLoads(sim, delta=delta, x0=x0, capacity=1)
    record(sl, sim)
    return dict(zip(COLUMNS, (float(x) for x in series(sl)[1][0])))


def write_vtp(path, sl) -> None:
    """The triangles at the sampled time as a VTK PolyData file (XML, ascii arrays): points = the vertices in x space, cell data =
    p, traction, area_vector, body_velocity and the means when kept.  On z-slabs every rank must call it; rank 0 writes."""
    f = fields(sl)
    if sl.slab is not None and sl.slab.rank != 0:
        return
    pts = _to_x(sl.body, sl.body.vertices, sl.time)
    tri = np.asarray(sl.body.triangles, dtype=np.int64)
    nt = len(tri)
    cells = "".join(data_array(k, f[k], "Float64") for k in ("p", "traction", "area_vector", "body_velocity", "mean_p", "mean_traction")
                    if k in f)
    with open(path, "w") as o:
        o.write('<?xml version="1.0"?>\n<VTKFile type="PolyData" version="1.0" byte_order="LittleEndian">\n<PolyData>\n'
                f'<Piece NumberOfPoints="{len(pts)}" NumberOfVerts="0" NumberOfLines="0" NumberOfStrips="0" NumberOfPolys="{nt}">\n'
                "<Points>\n" + data_array("Points", pts, "Float64") + "</Points>\n"
                '<CellData Scalars="p" Vectors="traction">\n' + cells + "</CellData>\n"
                "<Polys>\n" + data_array("connectivity", tri.ravel(), "Int64") + data_array("offsets", 3 * np.arange(1, nt + 1), "Int64")
                + "</Polys>\n</Piece>\n</PolyData>\n</VTKFile>\n")
