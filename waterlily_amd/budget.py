"""Time-averaged turbulent kinetic energy budget of a Flow on the device: where k = 1/2 <u_i'u_i'> is produced, transported
and dissipated.

    bg = Budget(sim.flow)
    for _ in range(n):
        sim_step(sim)
        update(bg, sim.flow)          # two kernel launches, asynchronous
    T = terms(bg, sim.flow.nu)        # (N..., 8): k, production, dissipation, ..., residual (columns())

    dk/dt = -U_j d_j k - <u_i'u_j'> d_j U_i - nu <d_j u_i' d_j u_i'> - 1/2 d_j <u_i'u_i'u_j'> - d_j <p'u_j'> + nu lap k

Every update adds the current step to CENTRAL moments of the cell-centred fluctuation a_i = (u - U) averaged to the cell
centre (include/wlhip.h: wl_budget_update): R = <a_i a_j> (the cell-centred Reynolds stress, which MeanFlow.UU is not), PU =
<p'a_j>, GG = <d_j u_i' d_j u_i'> and the triple correlation T3_j = <a_i a_i a_j>, the last by the weighted incremental merge
of third central moments -- formed as <uuu> - ... it would cancel in Float32, as <uu> - <u><u> does (stats.py).  The
fluctuation is taken against the running mean BEFORE the update, which `bg.mean` (a MeanFlow without statistics) holds; the
second launch advances it.  Memory: 13 moment fields + the 4 of the mean = 17 fields of the grid in 3-D (8 + 3 = 11 in 2-D);
`terms` adds 8 for its result.  The moments live on the cells of inside() (on z-slabs: of this rank's owned planes); ghost
cells stay zero.  No body mask: the velocity in a solid cell does not fluctuate, so it contributes zeros.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import sim as S
from . import stats
from ._lib import check

COLUMNS = ("k", "production", "dissipation", "turbulent_transport", "pressure_transport", "viscous_diffusion", "convection",
           "residual")


def columns() -> Tuple[str, ...]:
    """names of the eight components of `terms`; residual = production - dissipation + the four transport terms"""
    return COLUMNS


class Budget:
    """Running central moments of `flow` for the budget of k.  mean: the MeanFlow (U, P) the fluctuations are taken against;
    R (N..., D(D+1)/2) cell-centred covariance in ParaView's order (stats.UU_ORDER); PU (N..., D); GG (N...); T3 (N..., D):
    device fields allocated by the flow's layout rule (pitched when the flow is, the same slab).  dtype: accumulator type,
    with MeanFlow's rule (default the flow's T; Float32 on a Float64 flow is refused)."""

    def __init__(self, flow: S.Flow, t_init: Optional[float] = None, dtype=None):
        self.mean = stats.MeanFlow(flow, t_init=t_init, dtype=dtype)
        self.D, self.T, self.flow_T = self.mean.D, self.mean.T, self.mean.flow_T
        self.layout = self.mean.layout
        al = lambda nc: self.layout.alloc(nc, flow.device)
        self.R = al((flow.D * (flow.D + 1) // 2,))
        self.PU = al((flow.D,))
        self.GG = al(())
        self.T3 = al((flow.D,))

    @property
    def t(self):
        return self.mean.t


def time(bg: Budget) -> float:
    """length of the averaging window"""
    return stats.time(bg.mean)


def _ptr(a):
    return C.c_void_p(a.data_ptr())


def update(bg: Budget, flow: S.Flow) -> None:
    """Blend the flow's current u and p into the moments, then into the means: two launches on the library's stream, no
    synchronisation."""
    mf = bg.mean
    eps = stats.weight(mf.t, S.time(flow))
    if eps is None:
        return
    if flow.D != bg.D or tuple(flow.p.shape) != tuple(mf.P.shape) or flow.layout.slab is not bg.layout.slab:
        raise ValueError("Budget: the flow's grid or slab differs from the one the moments were made for")
    gf, ga = flow.layout.grid(), bg.layout.grid()
    check(_lib.lib().wl_budget_update(S._WLT[bg.flow_T], S._WLT[bg.T], C.byref(gf), _ptr(flow.u), _ptr(flow.p), C.byref(ga), _ptr(mf.U),
                                      _ptr(mf.P), _ptr(bg.R), _ptr(bg.PU), _ptr(bg.GG), _ptr(bg.T3), eps, int(len(mf.t) == 1)))
    stats.update(mf, flow)


def reset(bg: Budget, t_init: Optional[float] = None) -> None:
    """Start a new averaging window at t_init (default: the last time seen); the next update overwrites the moments."""
    stats.reset(bg.mean, t_init)


def terms(bg: Budget, nu: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The budget terms (N..., 8) in the order of columns(), a device field of the accumulator type: values on the cells of
    inside() shrunk by one on every side, zeros on the rest of a fresh result (a given `out` keeps what it held outside
    inside()).  On a decomposed flow the moments' halo planes are exchanged first (a collective: every rank calls)."""
    if out is None:
        out = bg.layout.alloc((8,), bg.R.device)
    elif tuple(out.shape) != tuple(bg.GG.shape) + (8,) or out.dtype != bg.GG.dtype or out.stride() != bg.GG.stride() + (bg.layout.sc,):
        raise ValueError("Budget.terms: out must be a field of 8 components in the moments' layout and type")
    if bg.layout.slab is not None:
        for a in (bg.R, bg.PU, bg.T3):
            S.halo_exchange(a)
    ga = bg.layout.grid()
    check(_lib.lib().wl_budget_terms(S._WLT[bg.T], C.byref(ga), _ptr(bg.mean.U), _ptr(bg.R), _ptr(bg.PU), _ptr(bg.GG), _ptr(bg.T3),
                                     float(nu), _ptr(out)))
    return out


def integrate(terms: torch.Tensor, box: Optional[Sequence[Sequence[int]]] = None) -> torch.Tensor:
    """Float64 sum of every column of `terms` (..., 8) over the cells lo <= I < hi of box = (lo, hi), 0-based indices of the
    local array (default: all of it -- outside the cells `terms` fills the result is zero).  A torch operation, on the tensor's
    device; no synchronisation."""
    D = terms.ndim - 1
    if box is not None:
        lo, hi = box
        if len(lo) != D or len(hi) != D:
            raise ValueError(f"Budget.integrate: the box needs {D} indices per corner")
        terms = terms[tuple(slice(int(a), int(b)) for a, b in zip(lo, hi))]
    return terms.sum(dim=tuple(range(D)), dtype=torch.float64)


def attrib(bg: Budget, sim) -> Dict[str, Callable]:
    """Attributes for vtk.vtkWriter(attrib=...): TKEBudget (8 components, columns(), with sim.flow.nu; formed when the file is
    written) and the mean's MeanVelocity and MeanPressure.  vtk.write packs with the flow's T, so the accumulators must have
    that type."""
    if bg.T != bg.flow_T:
        raise TypeError(f"Budget.attrib: the moments are {bg.T}, the flow is {bg.flow_T}, and vtk.write packs with the flow's type "
                        "-- make the Budget with the flow's dtype to write it")
    out = {"TKEBudget": lambda s: terms(bg, sim.flow.nu)}
    out.update(stats.mean_attrib(bg.mean))
    return out
