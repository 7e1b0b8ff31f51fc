"""Time-averaged statistics of a Flow on the device: mean velocity and pressure, Reynolds stresses, pressure variance.

    mf = MeanFlow(sim.flow, uu_stats=True, pp_stats=True)
    for _ in range(n):
        sim_step(sim)
        update(mf, sim.flow)          # one kernel launch, asynchronous

The averages are weighted by the time step: with t the flow time and dt = t - t_last, each update blends the current fields
in with weight eps = dt / (t - t0) (West's weighted incremental form; include/wlhip.h: wl_meanflow_update).  `UU` holds the
COVARIANCE <u_i' u_j'>, not <u_i u_j>: in a wake with mean ~1 and fluctuations ~0.1 the difference <uu> - <u><u> loses about
two digits to cancellation in Float32, the stored covariance does not.  The products pair u[I,i] and u[I,j] at the same index
I, i.e. the face values of DIFFERENT faces of cell I (the convention of WaterLily's later MeanFlow); a cell-centred covariance
is not provided.  Every element of the local arrays is updated, ghost cells and z-slab halo planes included, so the fields can
be handed to `sim.gather`, `sim.metric` and `vtk.write` like the flow's own.  No collective is needed on z-slabs: every rank
updates its own planes and eps is the same everywhere (the time step comes out of an all-reduce).
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Optional, Sequence

import numpy as np

from . import _lib
from . import sim as S
from ._lib import check

# ParaView's symmetric-tensor component order of UU
UU_ORDER = {2: ((0, 0), (1, 1), (0, 1)), 3: ((0, 0), (1, 1), (2, 2), (0, 1), (1, 2), (0, 2))}


class MeanFlow:
    """Running time averages of `flow`.  Fields (device, allocated by the flow's layout rule -- pitched when the flow is, the
    same slab): U (N..., D) mean of u (face values: the same field type as u); P (N...) mean of p; UU (N..., D(D+1)/2) the
    velocity covariance, only with uu_stats; pp (N...) the variance of p, only with pp_stats.  t: host list of the times
    seen, t[0] = start of the averaging window (default: time(flow)).  dtype: accumulator type (default: the flow's T;
    Float64 is allowed on a Float32 flow, Float32 on a Float64 flow is refused)."""

    def __init__(self, flow: S.Flow, *, t_init: Optional[float] = None, uu_stats: bool = False, pp_stats: bool = False,
                 dtype=None):
        T = np.dtype(flow.T)
        A = T if dtype is None else np.dtype(dtype)
        if A not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise ValueError(f"MeanFlow: the accumulator dtype must be float32 or float64, not {A}")
        if T == np.float64 and A == np.float32:
            raise ValueError("MeanFlow: Float32 accumulators on a Float64 flow are refused (they would lose the flow's precision)")
        self.D, self.T, self.flow_T = flow.D, A, T
        lay = flow.layout
        self.layout = S.Layout(lay.Ng_global, A, padded=lay.lead > 0, slab=lay.slab)
        al = lambda nc: self.layout.alloc(nc, flow.device)
        self.U = al((flow.D,))
        self.P = al(())
        self.UU = al((flow.D * (flow.D + 1) // 2,)) if uu_stats else None
        self.pp = al(()) if pp_stats else None
        self.t = [S.time(flow) if t_init is None else float(t_init)]


def time(mf: MeanFlow) -> float:
    """length of the averaging window"""
    return mf.t[-1] - mf.t[0]


def weight(t_seen: Sequence[float], t: float) -> Optional[float]:
    """eps of an update at flow time t after the times `t_seen` (t_seen[0] = start of the window), in Float64:
    None when dt = t - t_seen[-1] == 0 (nothing to do), else dt / (t - t_seen[0]) -- exactly 1 on the first update of a
    window.  dt < 0 raises."""
    t = float(t)
    dt = t - float(t_seen[-1])
    if dt < 0:
        raise ValueError(f"MeanFlow: the flow time went back ({t} < {t_seen[-1]})")
    if dt == 0:
        return None
    return dt / (t - float(t_seen[0]))


def update(mf: MeanFlow, flow: S.Flow) -> None:
    """Blend the flow's current u and p into the averages: one kernel launch on the library's stream, no synchronisation."""
    eps = weight(mf.t, S.time(flow))
    if eps is None:
        return
    if flow.D != mf.D or tuple(flow.p.shape) != tuple(mf.P.shape) or flow.layout.slab is not mf.layout.slab:
        raise ValueError("MeanFlow: the flow's grid or slab differs from the one the averages were made for")
    gf, ga = flow.layout.grid(), mf.layout.grid()
    ptr = lambda a: None if a is None else C.c_void_p(a.data_ptr())
    check(_lib.lib().wl_meanflow_update(S._WLT[mf.flow_T], S._WLT[mf.T], C.byref(gf), ptr(flow.u), ptr(flow.p), C.byref(ga),
                                        ptr(mf.U), ptr(mf.P), ptr(mf.UU), ptr(mf.pp), eps, int(len(mf.t) == 1)))
    mf.t.append(S.time(flow))


def reset(mf: MeanFlow, t_init: Optional[float] = None) -> None:
    """Start a new averaging window at t_init (default: the last time seen); the next update overwrites the fields."""
    mf.t = [mf.t[-1] if t_init is None else float(t_init)]


def mean_attrib(mf: MeanFlow) -> Dict[str, Callable]:
    """Attributes for vtk.vtkWriter(attrib=...): MeanVelocity, MeanPressure, and ReynoldsStress / PressureVariance when they
    are collected.  vtk.write packs every attribute with the flow's T, so the accumulators must have that type."""
    if mf.T != mf.flow_T:
        raise TypeError(f"mean_attrib: the averages are {mf.T}, the flow is {mf.flow_T}, and vtk.write packs with the flow's "
                        "type -- make the MeanFlow with the flow's dtype to write it")
    out = {"MeanVelocity": lambda sim: mf.U, "MeanPressure": lambda sim: mf.P}
    if mf.UU is not None:
        out["ReynoldsStress"] = lambda sim: mf.UU
    if mf.pp is not None:
        out["PressureVariance"] = lambda sim: mf.pp
    return out
