"""Isosurfaces on the device: the triangles of a scalar field's level set, optionally coloured by a second field -- the λ₂ or |ω|
picture of a wake without writing the volume.

    isf = Isosurface(sim.flow)                        # owns the triangle / value buffers and the two-element count
    tri, val = lambda2(isf, sim, -0.01, color="omega_mag")   # device views [nt, 3, 3] and [nt, 3] (Float64)
    tri, _ = extract(isf, field, 0.5)                 # any cell-centred scalar field on the flow's grid
    n = count(isf, field, 0.5)                        # the number of triangles only
    write_vtp("wake.vtp", tri, val, name="omega_mag") # welded PolyData ParaView opens
    area(tri), enclosed_volume(tri)                   # torch, double

The surface is marching tetrahedra on the Kuhn split of every cube of 8 neighbouring cells; the definition -- tetrahedra,
vertices, orientation (normals towards a >= c), order, the NaN rule, the box -- is in include/wlhip.h (wl_isosurface) and
csrc/wl_iso.h.  Coordinates are x = J - 0.5 with global z, the frame of loc(0, I) in which MeshBody vertices live.  Vertices on
a shared edge are bit-equal, so weld() needs no tolerance.  The order of the triangles is a function of the field alone.

The views returned by extract / lambda2 alias the object's buffers: the next call overwrites them.  On z-slabs every rank
extracts the part whose low-corner planes it owns (the field must be exchanged to depth 1; lambda2 does that) and
gather() concatenates the parts in rank order on rank 0: the undecomposed surface bit for bit.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib
from . import _readout as R
from . import _series
from . import sim as S
from ._lib import check
from .vtk import data_array


class Isosurface:
    """Device buffers of one extraction: tri [capacity, 3, 3] and, once a colour is asked for, val [capacity, 3] (Float64), and
    cnt = (triangles the surface has, triangles written).  extract() grows them when a surface does not fit."""

    def __init__(self, flow, capacity: int = 1 << 20):
        if flow.D != 3:
            raise ValueError("Isosurface: a 3-D flow is needed")
        if int(capacity) < 1:
            raise ValueError("Isosurface: capacity must be >= 1")
        self.flow = flow
        self.capacity = int(capacity)
        self.tri = torch.empty((self.capacity, 3, 3), dtype=torch.float64, device=flow.device)
        self.val: Optional[torch.Tensor] = None
        self.cnt = torch.zeros(2, dtype=torch.int64, device=flow.device)
        self.field: Optional[torch.Tensor] = None     # lambda2's scratch scalar fields (made on first use)
        self.cfield: Optional[torch.Tensor] = None

    def _grow(self, capacity: int, color: bool) -> None:
        if capacity > self.capacity:
            self.capacity = int(capacity)
            self.tri = torch.empty((self.capacity, 3, 3), dtype=torch.float64, device=self.flow.device)
            self.val = None
        if color and self.val is None:
            self.val = torch.empty((self.capacity, 3), dtype=torch.float64, device=self.flow.device)


def _check_field(isf: Isosurface, a: torch.Tensor, what: str) -> None:
    if not R.laid_out_like(a, isf.flow.p):
        raise ValueError(f"Isosurface: {what} must be a scalar field with the layout of flow.p (use waterlily_amd.sim.like)")


def _run(isf: Isosurface, a: torch.Tensor, c: float, color, box, cap: int) -> Tuple[int, int]:
    """one wl_isosurface call and the read of its count (the one synchronisation): (total, written)"""
    lo, hi = R.box_args(box)
    g = S._grid_of(a, 3)
    check(_lib.lib().wl_isosurface(S._WLT[S._T(a)], C.byref(g), S._ptr(a), None if color is None else S._ptr(color), float(c), lo, hi,
                                   S._ptr(isf.tri) if cap else None, S._ptr(isf.val) if (cap and color is not None) else None,
                                   int(cap), S._ptr(isf.cnt)))
    total, written = (int(x) for x in isf.cnt.cpu())
    return total, written


def extract(isf: Isosurface, a: torch.Tensor, c: float, color: Optional[torch.Tensor] = None, box=None):
    """The surface a == c inside `box` = (lo, hi) (default: the cubes of inside(a)), coloured by the field `color`: device views
    tri [nt, 3, 3] and val [nt, 3] (None without a colour).  One call and one read of the count; when the surface does not fit,
    the buffers grow to the count and the call is made once more."""
    _check_field(isf, a, "the field")
    if color is not None:
        _check_field(isf, color, "the colour")
    isf._grow(isf.capacity, color is not None)
    total, written = _run(isf, a, c, color, box, isf.capacity)
    if total > written:
        isf._grow(total, color is not None)
        total, written = _run(isf, a, c, color, box, isf.capacity)
    return isf.tri[:written], (None if color is None else isf.val[:written])


def count(isf: Isosurface, a: torch.Tensor, c: float, box=None) -> int:
    """the number of triangles extract would return (on z-slabs: this rank's); nothing is written"""
    _check_field(isf, a, "the field")
    lo, hi = R.box_args(box)
    g = S._grid_of(a, 3)
    check(_lib.lib().wl_isosurface(S._WLT[S._T(a)], C.byref(g), S._ptr(a), None, float(c), lo, hi, None, None, 0, S._ptr(isf.cnt)))
    return int(isf.cnt[0].item())


def lambda2(isf: Isosurface, sim, c: float, color=None):
    """extract() of λ₂(u) of sim.flow, computed into a scratch field the object owns.  color: None, "omega_mag" (a second scratch
    field), "pressure" (sim.flow.p) or a scalar field.  On z-slabs both fields are exchanged to depth 1 first."""
    flow = sim.flow
    if flow is not isf.flow:
        raise ValueError("Isosurface: the simulation's flow differs from the one the object was made for")
    if isf.field is None:
        isf.field = S.like(flow.p)
    S.metric(isf.field, "lambda2", flow.u)
    if isinstance(color, str):
        if color == "pressure":
            b = flow.p
        elif color == "omega_mag":
            if isf.cfield is None:
                isf.cfield = S.like(flow.p)
            b = S.metric(isf.cfield, "omega_mag", flow.u)
        else:
            raise ValueError(f'Isosurface: color must be "omega_mag", "pressure" or a field, not {color!r}')
    else:
        b = color
    if flow.layout.slab is not None:
        S.halo_exchange(isf.field, 1)
        if b is not None:
            S.halo_exchange(b, 1)
    return extract(isf, isf.field, c, color=b)


# --------------------------------------------------------------------------- what one does with the triangles

def area(tri: torch.Tensor) -> torch.Tensor:
    """the surface's area (a 0-dim Float64 tensor on tri's device)"""
    t = tri.to(torch.float64)
    return 0.5 * torch.linalg.cross(t[:, 1] - t[:, 0], t[:, 2] - t[:, 0]).norm(dim=1).sum()


def enclosed_volume(tri: torch.Tensor) -> torch.Tensor:
    """the volume a closed surface encloses, positive where a < c is inside (divergence theorem; a 0-dim Float64 tensor)"""
    t = tri.to(torch.float64)
    return (t[:, 0] * torch.linalg.cross(t[:, 1], t[:, 2])).sum() / 6.0


def weld(tri) -> Tuple[np.ndarray, np.ndarray]:
    """points [nv, 3] (the distinct vertices, by bits) and connectivity [nt, 3]: canonical edges make equal vertices bit-equal,
    so np.unique on the rows is the whole job."""
    t = tri.detach().cpu().numpy() if isinstance(tri, torch.Tensor) else np.asarray(tri)
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(-1, 3)
    if len(t) == 0:
        return np.zeros((0, 3)), np.zeros((0, 3), dtype=np.int64)
    t = t + 0.0                                        # -0.0 and 0.0 are one point
    _, first, inv = np.unique(t.view(np.uint64), axis=0, return_index=True, return_inverse=True)
    return t[first], inv.reshape(-1, 3).astype(np.int64)


def write_vtp(path, tri, val=None, name: str = "color") -> None:
    """The welded surface as a VTK PolyData file (XML, ascii arrays): Float32 points, the triangles, and `val` [nt, 3] as the
    point-data array `name`."""
    pts, conn = weld(tri)
    nt = len(conn)
    if nt == 0:
        raise ValueError("Isosurface: the surface has no triangles (nothing to write)")
    point_data = ""
    if val is not None:
        v = val.detach().cpu().numpy() if isinstance(val, torch.Tensor) else np.asarray(val)
        pv = np.zeros(len(pts), dtype=np.float64)
        pv[conn.ravel()] = np.asarray(v, dtype=np.float64).ravel()          # equal vertices carry equal values
        point_data = f'<PointData Scalars="{name}">\n' + data_array(name, pv.astype(np.float32), "Float32") + "</PointData>\n"
    with open(path, "w") as o:
        o.write('<?xml version="1.0"?>\n<VTKFile type="PolyData" version="1.0" byte_order="LittleEndian">\n<PolyData>\n'
                f'<Piece NumberOfPoints="{len(pts)}" NumberOfVerts="0" NumberOfLines="0" NumberOfStrips="0" NumberOfPolys="{nt}">\n'
                "<Points>\n" + data_array("Points", pts.astype(np.float32), "Float32") + "</Points>\n" + point_data
                + "<Polys>\n" + data_array("connectivity", conn.ravel(), "Int64") + data_array("offsets", 3 * np.arange(1, nt + 1), "Int64")
                + "</Polys>\n</Piece>\n</PolyData>\n</VTKFile>\n")


def gather(tri, val=None, slab=None):
    """The ranks' parts concatenated in rank order on rank 0 as numpy arrays (tri, val); (None, None) on the other ranks.  Every
    rank of a slab run must call it; without a slab it is a copy to the host."""
    t, root = _series.host_parts(tri, slab)
    v = None if val is None else _series.host_parts(val, slab)[0]                        # (val is None on every rank or on none)
    if not root:
        return None, None
    return np.concatenate(t, axis=0), None if v is None else np.concatenate(v, axis=0)
