"""The load of the fluid on the body, recorded during a run: pressure and viscous force, their moments about x0, the power
they exchange with a moving body, and -- for a `Bodies` composite -- the share of every leaf.

    fr = Forces(sim, x0=(cx, cy, cz))                # x0: the point the moments are taken about, default the origin
    for _ in range(n):
        sim_step(sim)
        record(fr, sim)                              # one C call (two kernel launches), no synchronisation
    t, v = series(fr)                                # v[k, q] = the 16 columns of leaf q after step k; v[k, -1] the total
    CD = coefficients(v[:, -1, 0] + v[:, -1, 3], U, L)
    row = loads(sim, x0)                             # one-off, synchronous: {"Fp": .., "Fv": .., "Mp": .., ..}

Columns (columns()): Fp[3], Fv[3], Mp[3], Mv[3] (2-D: the force's z slot and the moment's x, y slots are 0, the scalar moment is
in slot z), Wp = sum fp.V and Wv = sum fv.V (the rate of work of the fluid's load at the body's own velocity V: minus the
power the body spends on the fluid), ncells and A = sum |nds| (the surface measure the band represents).  Definitions,
arithmetic, summation order, the NaN rule and the slab rule: include/wlhip.h (wl_body_loads) and csrc/wl_forces.h.

Which body, which cells: exactly what pressure_force(sim) uses -- the body at time(sim.flow), the candidate cells the last
measure! listed (flow._band_cells), and for a body declared static (sim_step(remeasure=False)) the pose the cached band was
built at -- so loads(sim)["Fp"] is pressure_force(sim) up to the order of the sum.  Native bodies (parametric, composites,
meshes) are evaluated in the kernel's registers: no nds array, no compaction.  Any other body (torch closures) goes through
the stored band of sim._band_of, whose build runs torch and SYNCHRONISES when the body moved; such a band carries no body
velocity, so Wp and Wv are NaN.

Leaves: row q sums the cells whose active leaf is q.  For a union of disjoint bodies that is the load on each of them; across
"-" and "&" it is only an attribution of surface patches.  The last row is the total, row 0 + row 1 + .. in that order.

On z-slabs every rank records the rows of its own planes and nothing is communicated per step; series() and loads() add the
ranks' rows at the host, in rank order (every column is additive; NaN stays NaN).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import _series
from . import body as B
from . import sim as S
from ._lib import check
from .mesh import MeshBody
from ._series import _rank_parts

NV = 16
_COLUMNS = ("Fp_x", "Fp_y", "Fp_z", "Fv_x", "Fv_y", "Fv_z", "Mp_x", "Mp_y", "Mp_z", "Mv_x", "Mv_y", "Mv_z", "Wp", "Wv", "ncells", "area")


def columns() -> Tuple[str, ...]:
    """The names of the 16 columns of a row."""
    return _COLUMNS


def _x0(x0, D: int) -> Tuple[float, ...]:
    if x0 is None:
        return (0.0,) * D
    x0 = tuple(float(v) for v in np.asarray(x0, dtype=np.float64).ravel())
    if len(x0) != D:
        raise ValueError(f"Forces: x0 must have {D} components, got {len(x0)}")
    return x0


def _native(sim: S.Simulation) -> bool:
    """the condition under which _ensure_band evaluates the body with the library's kernels"""
    return getattr(sim.flow, "_band_cells", None) is not None and sim.geometry == "device" and B.is_native(sim.body)


def nleaf(sim: S.Simulation) -> int:
    """Rows before the total: the leaves of a native `Bodies` composite, else 1."""
    return len(sim.body.bodies) if _native(sim) and isinstance(sim.body, B.Bodies) else 1


def combine(parts: Sequence[np.ndarray]) -> np.ndarray:
    """The ranks' rows [..., 16] -> the rows of the whole domain: addition in rank order.  Pure host code."""
    out = np.array(parts[0], dtype=np.float64, copy=True)
    for p in parts[1:]:
        out += np.asarray(p, dtype=np.float64)
    return out


def _pose_time(sim: S.Simulation) -> float:
    """The body time _ensure_band would use: now, or -- body declared static and a band cached -- that band's"""
    if sim._band is not None and not getattr(sim, "_moving", True):
        return sim._band[0]
    return S.time(sim.flow)


def _call(sim: S.Simulation, x03, rows: torch.Tensor) -> None:
    flow = sim.flow
    L = _lib.lib()
    wt, nu = S._WLT[flow.T], float(flow.nu)
    g = S._grid_of(flow.p, flow.D)
    if _native(sim):
        t = _pose_time(sim)
        cand = flow._band_cells[1]
        if isinstance(sim.body, MeshBody):
            h, pose = sim.body.native(t, sim.eps)
            check(L.wl_body_loads_mesh(wt, C.byref(g), S._ptr(flow.p), S._ptr(flow.u), nu, h, C.byref(pose), S._ptr(cand), cand.numel(),
                                       x03, S._ptr(rows)))
        else:
            desc = sim.body.native_desc(t, flow.D)
            check(L.wl_body_loads(wt, C.byref(g), S._ptr(flow.p), S._ptr(flow.u), nu, desc, S._ptr(cand), cand.numel(), x03, S._ptr(rows)))
        return
    idx, nds = S._band_of(sim)
    check(L.wl_band_loads(wt, C.byref(g), S._ptr(flow.p), S._ptr(flow.u), nu, S._ptr(idx), S._ptr(nds), idx.numel(), x03, S._ptr(rows)))


class Forces(_series.Series):
    """Recorder of the loads.  buf: Float64 device buffer [capacity, nleaf+1, 16], slot k = the k-th record; t: host list of
    the times."""

    def __init__(self, sim: S.Simulation, x0=None, capacity: int = 256):
        flow = sim.flow
        self.nleaf = nleaf(sim)
        super().__init__(("Forces", "the recorder was"), flow.D, flow.layout.slab, (self.nleaf + 1, NV), capacity, flow.device)
        self.x0 = _x0(x0, self.D)
        self._x03 = _lib.d3(self.x0)


def record(fr: Forces, sim: S.Simulation) -> None:
    """Append the loads on sim.body: one wl_*_loads call into the next slot of the buffer, no synchronisation for a native
    body.  A full buffer is doubled by a device copy."""
    row = _series.next_row(fr, sim.flow.D, sim.flow.layout.slab)
    if nleaf(sim) != fr.nleaf:
        raise ValueError("Forces: the body's number of leaves differs from the one the recorder was made for")
    _call(sim, fr._x03, row)
    fr.t.append(S.time(sim.flow))


def series(fr: Forces) -> Tuple[np.ndarray, np.ndarray]:
    """(t[K], values[K, nleaf+1, 16]) of the K records so far (synchronises; on z-slabs every rank must call it: the ranks'
    buffers are added once, here)."""
    t, parts = _series.rank_rows(fr)
    return t, combine(parts)


reset = _series.reset


def loads(sim: S.Simulation, x0=None) -> Dict[str, object]:
    """The loads on sim.body now (synchronous; on z-slabs every rank must call it): Fp, Fv, Mp, Mv as arrays of D components
    (2-D moments: the scalar), Wp, Wv, ncells, area of the whole body, and "leaves": the rows [nleaf+1, 16] as recorded."""
    D = sim.flow.D
    rows = torch.zeros((nleaf(sim) + 1, NV), dtype=torch.float64, device=sim.flow.device)
    _call(sim, _lib.d3(_x0(x0, D)), rows)
    v = combine(_rank_parts(rows.cpu().numpy(), sim.flow.layout.slab))
    tot = v[-1]
    mom = (lambda a: a.copy()) if D == 3 else (lambda a: float(a[2]))
    return {"Fp": tot[0:D].copy(), "Fv": tot[3:3 + D].copy(), "Mp": mom(tot[6:9]), "Mv": mom(tot[9:12]), "Wp": float(tot[12]),
            "Wv": float(tot[13]), "ncells": int(tot[14]), "area": float(tot[15]), "leaves": v}


def coefficients(v, U: float, L_or_area: float) -> np.ndarray:
    """2 F / (U^2 A): force (or, with A = area * length, moment) columns -> coefficients.  Host helper."""
    return 2.0 * np.asarray(v, dtype=np.float64) / (float(U) ** 2 * float(L_or_area))
