"""What the recorders beside the stepper share (Probes, Integrals, Forces; SurfaceLoads for the ranks alone): a Float64 buffer of
rows that grows, the host list of the times, the flow the recorder was made for, and the ranks' parts of a z-slab run at the host
(the read-outs' gather() functions start from them too).
Works on any torch device.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch


def _rank_parts(v: np.ndarray, slab) -> list:
    """The ranks' arrays in rank order, at the host (one all-gather; [v] when not decomposed)."""
    if slab is None or slab.size == 1:
        return [v]
    import torch.distributed as dist
    parts = [None] * slab.size
    dist.all_gather_object(parts, v)
    return parts


def host_parts(x, slab) -> Tuple[list, bool]:
    """How every gather() of a read-out starts: (the ranks' host copies of the tensor or array x in rank order, whether this
    rank is the one that returns the result: rank 0, or the only one).  Every rank must call it."""
    v = x.detach().cpu().numpy().copy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return _rank_parts(v, slab), slab is None or slab.size == 1 or slab.rank == 0


def _add(parts: list) -> np.ndarray:
    """parts[0] + parts[1] + .. in that order (the one part itself when not decomposed)"""
    if len(parts) == 1:
        return parts[0]
    out = parts[0].copy()
    for p in parts[1:]:
        out += p
    return out


def _rank_sum(v: np.ndarray, slab) -> np.ndarray:
    """Sum of the ranks' arrays (every entry is non-zero on at most its owner), in rank order, at the host."""
    return _add(_rank_parts(v, slab))


class Series:
    """buf: Float64 buffer [capacity, *row_shape] on `device`, row k = the k-th record; t: host list of the times; D, slab: the
    dimension and the z-slab of the flow the recorder was made for.  who = (class name, "the recorder was"): the error texts."""

    def __init__(self, who: Tuple[str, str], D: int, slab, row_shape, capacity: int, device):
        if capacity < 1:
            raise ValueError(f"{who[0]}: capacity must be >= 1")
        self._who = who
        self.D, self.slab = D, slab
        self.buf = torch.zeros((int(capacity),) + tuple(row_shape), dtype=torch.float64, device=device)
        self.t: List[float] = []


def next_row(sr: Series, D: int, slab) -> torch.Tensor:
    """The row the next record goes to, for a flow of dimension D on `slab`; a full buffer is doubled by a device copy.  The
    caller fills the row and then appends the time to sr.t."""
    if D != sr.D or slab is not sr.slab:
        raise ValueError(f"{sr._who[0]}: the flow's dimension or slab differs from the one {sr._who[1]} made for")
    k = len(sr.t)
    if k == sr.buf.shape[0]:
        grown = torch.empty((2 * k,) + tuple(sr.buf.shape[1:]), dtype=sr.buf.dtype, device=sr.buf.device)
        grown[:k].copy_(sr.buf)
        sr.buf = grown
    return sr.buf[k]


def rank_rows(sr: Series) -> Tuple[np.ndarray, list]:
    """(t[K], the first K rows of every rank's buffer in rank order) at the host (synchronises; every rank must call it)."""
    return np.asarray(sr.t, dtype=np.float64), _rank_parts(sr.buf[:len(sr.t)].cpu().numpy(), sr.slab)


def reset(sr: Series) -> None:
    """Forget the records (the buffer keeps its size)."""
    sr.t = []
