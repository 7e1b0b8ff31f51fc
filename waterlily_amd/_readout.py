"""What the read-outs beside the stepper share (Render, Downsample, Histogram, TwoPoint, Regions, Scene, Isosurface): the device
buffer each of them owns, the library's numbers of the kinds and modes, the one descriptor of "the value of a cell", the box
rule and the layout check of a field.  It imports nothing from the family.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _lib
from . import sim as S
from ._lib import check

R_SCALAR, R_UCOMP, R_CENTRE, R_FACE, R_METRIC = 0, 1, 2, 3, 16
MODE = {"max": 0, "min": 1, "absmax": 2, "sum": 3, "mean": 4}
KIND = {"scalar": R_SCALAR, "ucomp": R_UCOMP, "centre": R_CENTRE, "center": R_CENTRE}       # ("face": Downsample's alone)
KIND.update({k: R_METRIC + v for k, v in S._METRIC.items()})


def code(table: dict, name) -> int:
    """the library's number of a kind or mode given by name (a number passes through)"""
    return table[name] if isinstance(name, str) else int(name)


def i3(v):
    return (C.c_int32 * 3)(*([int(x) for x in v] + [0] * 3)[:3])


class DevBuf:
    """A block of device memory from the library's allocator (wl_malloc: counted by wl_prof_allocs), freed with the object.
    torch views it through __cuda_array_interface__ and keeps the object alive for as long as a view exists."""

    def __init__(self, nbytes: int):
        self.nbytes = max(1, int(nbytes))
        p = C.c_void_p()
        check(_lib.lib().wl_malloc(C.byref(p), C.c_size_t(self.nbytes)))
        self.ptr = p.value
        check(_lib.lib().wl_memset0(C.c_void_p(self.ptr), C.c_size_t(self.nbytes)))
        self.__cuda_array_interface__ = {"shape": (self.nbytes,), "typestr": "|u1", "data": (self.ptr, False), "version": 2}

    def tensor(self, dtype, device) -> torch.Tensor:
        return torch.as_tensor(self, device=device).view(dtype)

    def __del__(self):
        if getattr(self, "ptr", None):
            _lib.lib().wl_free(C.c_void_p(self.ptr))
            self.ptr = None


class Value:
    """The value of a cell.  kind: "scalar" (a scalar field), "ucomp" / "centre" (component i of a vector field, as stored /
    averaged to the cell centre) or a metric of u: "ke", "curl", "omega_mag", "omega_theta", "lambda2" (i, par, par2 as
    waterlily_amd.sim.metric).  absval: |v| in place of v (Histogram and Regions read it; TwoPoint refuses it)."""

    def __init__(self, kind="scalar", i: int = 0, par=None, par2=None, absval: bool = False):
        self.kind, self.i, self.par, self.par2, self.absval = code(KIND, kind), int(i), par, par2, bool(absval)

    def fill(self, s):
        """The leading fields of the ctypes struct s (HistAxis, TpValue, RgValue, RsCol.v) but the field's pointer f: an absent
        par or par2 is three zeros there.  Returns s."""
        s.kind, s.ipar = self.kind, self.i
        s.par[:] = list(_lib.d3(() if self.par is None else self.par))
        s.par2[:] = list(_lib.d3(() if self.par2 is None else self.par2))
        if hasattr(s, "absval"):
            s.absval = int(self.absval)
        return s

    def flat(self):
        """(kind, ipar, par, par2) as wl_render_project, wl_downsample and wl_field_range take them: an absent par is NULL"""
        return self.kind, self.i, None if self.par is None else _lib.d3(self.par), None if self.par2 is None else _lib.d3(self.par2)


def inside(N):
    """the default box (lo, hi): inside() of arrays of extents N"""
    return (1,) * len(N), tuple(int(n) - 1 for n in N)


def sides(box):
    """(lo, hi) of a given box as tuples of ints; two empty tuples for what is no pair of sequences of integers"""
    try:
        lo, hi = (tuple(int(x) for x in side) for side in box)
    except (TypeError, ValueError):
        return (), ()
    return lo, hi


def box_ok(lo, hi, N) -> bool:
    """the box rule: the cells lo_d <= J_d < hi_d of arrays of extents N, one entry per dimension"""
    return len(lo) == len(hi) == len(N) and all(0 <= l < h <= n - 1 for l, h, n in zip(lo, hi, N))


def box_of(who: str, N, box):
    """((lo, hi), given): the validated box, inside() when none was given; who: the class named in the error"""
    if box is None:
        return inside(N), False
    lo, hi = sides(box)
    if not box_ok(lo, hi, N):
        raise ValueError(f"{who}: a box is (lo, hi) with {len(N)} entries each, 0 <= lo < hi <= n - 1")
    return (lo, hi), True


def box_args(box):
    """the two int32[3] the library takes for (lo, hi); two NULLs (the library's default, inside()) for None"""
    return (None, None) if box is None else (i3(box[0]), i3(box[1]))


def laid_out_like(f: torch.Tensor, ref: torch.Tensor) -> bool:
    return tuple(f.shape) == tuple(ref.shape) and f.stride() == ref.stride() and f.dtype == ref.dtype


def field_grid(flow, f: torch.Tensor, vector: bool, who: str):
    """the grid descriptor of `f`, which must be laid out like the flow's u (vector) or p; who: the class named in the error"""
    if not laid_out_like(f, flow.u if vector else flow.p):
        raise ValueError(f"{who}: the field must have the layout of flow.{'u' if vector else 'p'} (use waterlily_amd.sim.like)")
    return S._grid_of(f, flow.D)
