"""Volume integrals of the flow, recorded during a run: kinetic energy, enstrophy, strain (dissipation), divergence norms,
the largest velocity component and the momentum -- the validation curves of the Taylor-Green case and of any other run.

    ig = Integrals(sim.flow)                         # U = background velocity subtracted in E, default 0
    for _ in range(n):
        sim_step(sim)
        record(ig, sim.flow)                         # one C call (two kernel launches), no synchronisation
    t, v = series(ig)                                # v[k] = (E, Z, S, div2, divmax, umax, P_1, .., P_D) after step k
    row = integrals(sim.flow)                        # one-off, synchronous: {"E": .., "Z": .., ..}

All cells of inside(p) count, solid and fluid alike (no body mask).  The resolved dissipation rate is 2 nu S.  Definitions,
arithmetic (double throughout, fixed summation order) and the NaN rule: include/wlhip.h (wl_flow_integrals) and
csrc/wl_integrals.h.  On z-slabs every rank records the row of its own planes and nothing is communicated per step; series()
and integrals() combine the ranks at the host, in rank order.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import _series
from . import sim as S
from ._lib import check
from ._series import _rank_parts

MAX_COLUMNS = (4, 5)            # divmax, umax: combined by maximum; every other column by addition


def _names(D: int) -> Tuple[str, ...]:
    return ("E", "Z", "S", "div2", "divmax", "umax") + tuple(f"P{i + 1}" for i in range(D))


def _background(U, D: int) -> Tuple[float, ...]:
    if U is None:
        return (0.0,) * D
    U = tuple(float(v) for v in np.asarray(U, dtype=np.float64).ravel())
    if len(U) != D:
        raise ValueError(f"Integrals: U must have {D} components, got {len(U)}")
    return U


def combine(parts: Sequence[np.ndarray]) -> np.ndarray:
    """The ranks' rows [..., 6+D] -> the rows of the whole domain: sums by addition in rank order, columns 4 and 5 by
    maximum (the device's comparison: a NaN never replaces a number).  Pure host code."""
    out = np.array(parts[0], dtype=np.float64, copy=True)
    for p in parts[1:]:
        p = np.asarray(p, dtype=np.float64)
        mx = {c: np.where(p[..., c] > out[..., c], p[..., c], out[..., c]) for c in MAX_COLUMNS}
        out += p
        for c in MAX_COLUMNS:
            out[..., c] = mx[c]
    return out


def _call(flow: S.Flow, U3, row: torch.Tensor) -> None:
    g = flow.layout.grid()
    check(_lib.lib().wl_flow_integrals(S._WLT[flow.T], C.byref(g), S._ptr(flow.u), U3, S._ptr(row)))


class Integrals(_series.Series):
    """Recorder of the integrals.  buf: Float64 device buffer [capacity, 6+D], row k = the k-th record; t: host list of the
    times."""

    def __init__(self, flow: S.Flow, U=None, capacity: int = 256):
        super().__init__(("Integrals", "the recorder was"), flow.D, flow.layout.slab, (6 + flow.D,), capacity, flow.device)
        self.U = _background(U, flow.D)
        self._U3 = _lib.d3(self.U)


def columns(ig: Integrals) -> Tuple[str, ...]:
    return _names(ig.D)


def record(ig: Integrals, flow: S.Flow) -> None:
    """Append the integrals of flow.u: one wl_flow_integrals call into the next row of the buffer, no synchronisation.  A
    full buffer is doubled by a device copy."""
    _call(flow, ig._U3, _series.next_row(ig, flow.D, flow.layout.slab))
    ig.t.append(S.time(flow))


def series(ig: Integrals) -> Tuple[np.ndarray, np.ndarray]:
    """(t[K], values[K, 6+D]) of the K records so far (synchronises; on z-slabs every rank must call it: the ranks' buffers
    are combined once, here)."""
    t, parts = _series.rank_rows(ig)
    return t, combine(parts)


reset = _series.reset


def integrals(flow: S.Flow, U=None) -> Dict[str, float]:
    """The integrals of flow.u now, by name (synchronous; on z-slabs every rank must call it)."""
    row = torch.zeros(6 + flow.D, dtype=torch.float64, device=flow.device)
    _call(flow, _lib.d3(_background(U, flow.D)), row)
    v = combine(_rank_parts(row.cpu().numpy(), flow.layout.slab))
    return dict(zip(_names(flow.D), (float(x) for x in v)))
