"""The HIP `measure!` kernels (csrc/wl_measure.h: k_measure_rows, k_measure_fill, k_body_nds) against the independent
extended-precision reference tests/xref_body.py on the native bodies of xref_body.CASES, at several times, in both types:
sigma, mu0, mu1, V within ulp_T(ref)/2 + K * eps_64 * M (the kernels evaluate in Float64 and round once to T: in Float32 this
passes only if they do), the band-cell list equal AS A SEQUENCE to the reference's cells with sigma_T^2 < (2+eps)^2 in
ascending order, and wl_body_nds on that list.  The seam cases put the band across the boundary of the 64-cell x chunks
(i = 64 | 65) over which k_measure_fill carries the list position.  From the reference's branch distances alone every
case asserts that no compared cell is nearer to a branch than its error bound (no cell is left out; how the margins follow
from the bounds: test_xref_body_cpu.branch_margin's twin below; the inputs were moved on the CPU until this held)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import xref_body as XB
from waterlily_amd import body as B
from waterlily_amd import sim as S

TYPES = [np.float32, np.float64]
WORST = {}


def native_map(spec, D):
    if spec is None:
        return None
    if spec[0] == "translate":
        return B.translation(D, v=spec[1], s0=spec[2])
    if spec[0] == "rotate3d":
        return B.rotation3d(spec[1], spec[2], spec[3], spec[4])
    if spec[0] == "rotate2d":
        return B.rotation2d(spec[1], spec[2], spec[3])
    return B.scaled(native_map(spec[1], D), spec[2])


def native_body(name):
    dims, _, leaves = XB.CASES[name]
    D = len(dims)
    out = None
    for fam, p, m, op in leaves:
        mp = native_map(m, D)
        b = {"sphere": lambda: B.Sphere(p[0], p[1], D, map=mp), "cylinder": lambda: B.Cylinder(p[0], p[1], D, axes=p[2], map=mp),
             "torus": lambda: B.Torus(p[0], p[1], p[2], map=mp), "plate": lambda: B.Plate(p[0], p[1], D, map=mp)}[fam]()
        out = b if out is None else {"+": out.__add__, "-": out.__sub__, "&": out.__and__}[op](b)
    assert B.is_native(out)
    return out


def branch_margin(key, T, scale):
    """the band test is made on sigma rounded to T (sigma_T^2 within 3 ulp_T of d^2 = 9): 16 eps_T * 9; every other branch
    is decided in Float64 on quantities within K eps_64 M of the reference, M of the order of the coordinates: 1024 K eps_64 scale"""
    f64 = 1024 * XB.K * float(np.finfo(np.float64).eps) * scale
    return f64 + (16 * 9 * float(np.finfo(T).eps) if key == "band" else 0.0)


def record(key, T, r):
    k = f"{key} {np.dtype(T).name}"
    WORST[k] = max(WORST.get(k, 0.0), r)
    assert r <= 1, f"{k}: |hip-ref| = {r:.3g} of its bound"


@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("name", list(XB.CASES))
def test_measure_hip_vs_xref(T, name):
    dims, times, _ = XB.CASES[name]
    D = len(dims)
    Ng = tuple(n + 2 for n in dims)
    idx = XB.inside_cells(dims)
    cell = tuple(idx)
    lin = np.ravel_multi_index(cell, Ng, order="F")
    body = native_body(name)
    # (a Flow and measure_flow, what Simulation and measure call: the multigrid solver a Simulation also builds wants
    # extents a*2^n, which the seam grids are not)
    f = S.Flow(dims, (1.0,) + (0.0,) * (D - 1), T=T, nu=0.01)
    lists = []
    for t in times:
        S.measure_flow(f, body, t=t, eps=1.0, geometry="device")
        ref, br = XB.fields(XB.body_at(name, t), idx, 1.0, T)
        for k in ("band", "tie", "fast", "clamp", "plate"):
            assert float(np.min(br[k])) > branch_margin(k, T, max(Ng)), (k, float(np.min(br[k])))
        h = {k: S.to_host(getattr(f, k)) for k in ("sigma", "mu0", "mu1", "V")}
        assert not np.isnan(ref["mu1"][0]).any()                          # (no face on the plate's rho = 0 line)
        record("sigma", T, XB.ratio(h["sigma"][cell], *ref["sigma"], T))
        band = ref["band"]
        assert band.sum() > 100
        got_list = f._band_cells[1].cpu().numpy()
        assert np.array_equal(got_list, lin[band]), "band-cell list differs from the reference's as a sequence"
        lists.append(lin[band])
        if name.startswith("seam"):
            i = idx[0][band]
            rows = lin[band] // Ng[0]
            straddle = np.intersect1d(rows[i == 64], rows[i == 65]).size
            assert straddle > 0 if (t > 0 or "moving" not in name) else straddle == 0
        for c in range(D):
            ok = idx[c] >= 2                                              # BC!(mu0, 0) and BC!(V, 0) rewrite the normal
            record("mu0", T, XB.ratio(h["mu0"][cell + (c,)][ok], ref["mu0"][0][c][ok], ref["mu0"][1][c][ok], T))     # component on plane 2
            record("V", T, XB.ratio(h["V"][cell + (c,)][ok], ref["V"][0][c][ok], ref["V"][1][c][ok], T))
            for j in range(D):
                record("mu1", T, XB.ratio(h["mu1"].reshape(Ng + (D * D,), order="F")[cell + (c + D * j,)],
                                           ref["mu1"][0][c + D * j], ref["mu1"][1][c + D * j], T))
        # wl_body_nds on the kernel's list
        cand = f._band_cells[1]
        nds = torch.empty((cand.numel(), D), dtype=torch.float64, device=cand.device)
        S.check(S._lib.lib().wl_body_nds(C.byref(S._grid_of(f.p, D)), body.native_desc(t, D), C.c_void_p(cand.data_ptr()),
                                         cand.numel(), C.c_void_p(nds.data_ptr())))
        (nv, nM), brn = XB.nds(XB.body_at(name, t), idx[:, band])
        for k in ("nds", "fast", "tie", "plate"):
            assert float(np.min(brn[k])) > branch_margin(k, np.float64, max(Ng)), (k, float(np.min(brn[k])))
        assert (nv != 0).any(0).sum() > 20
        record("nds", np.float64, XB.ratio(nds.cpu().numpy().T, nv, nM, np.float64))
        # controls that must fail (xref_body.controls): sigma against the body moved by 64 K eps_T of the grid, V against a
        # velocity off by 64 K eps_T, mu0, mu1, the list and nds against the body moved by one cell
        XB.controls(name, t, idx, T, D, Ng, dict(sigma=h["sigma"][cell], mu0=h["mu0"], mu1=h["mu1"].reshape(Ng + (D * D,), order="F"),
                                                 V=h["V"]), got_list, nds.cpu().numpy().T, band)
    if len(lists) == 2:
        assert not np.array_equal(lists[0], lists[1])                     # the body moved between the two times


def test_worst_ratios_are_recorded():
    """(prints the largest |hip-ref| as a share of ulp_T/2 + K eps_64 M per quantity: -s shows it)"""
    print("\nworst hip vs xref_body:", {k: round(v, 3) for k, v in sorted(WORST.items())})
