"""Isosurface without a GPU: the device's (tet, mask) table against the one tests/iso_ref.py derives from the text, the
argument checks of wl_isosurface, the numpy restatement against closed forms (an oblique plane, two spheres, a torus), and the
weld / .vtp round trip.

Bounds (EPS = 2^-52), as the definition gives them:
  * plane g.x = c, |g_z| dominant, field exact in either T (g in eighths, coordinates in halves): a vertex has
    |g.x - c| <= 16 EPS sum |g_d| n_d; the area is footprint |g| / |g_z| within nt EPS area; normals have n.g > 0;
  * distance fields: | |x - x0| - R | <= 3 / (8 (R - sqrt 3)), the linear-interpolation error of a distance (second derivative
    along a line <= 1 / distance) over an edge of length <= sqrt 3.
"""
import ctypes as C
import functools
import os
import sys
import xml.etree.ElementTree as ET

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import iso_ref as IR  # noqa: E402

from waterlily_amd import _lib, iso  # noqa: E402

EPS = 2.0 ** -52
LEVEL = 0.1 + 2.0 ** -30                              # the level of the random-field tests: equals no field value
SHAPES = [(70, 9, 7), (33, 12, 10), (64, 5, 5)]       # interior cells: > one 64-chunk and no multiple; short rows; one chunk + ghosts
G_LIN = np.array([0.375, -0.25, 1.5])                 # |g_z| dominant; eighths, so g.x is exact in Float32 on half-integer x
C_LIN = 12.1 + 2.0 ** -30


def coords(Ng):
    """x = I - 0.5 for every array index: [3, n0, n1, n2]"""
    return np.stack(np.meshgrid(*[np.arange(n, dtype=np.float64) - 0.5 for n in Ng], indexing="ij"))


def linear_field(Ng, g=G_LIN, c0=0.0, T=np.float64):
    x = coords(Ng)
    return np.asfortranarray((g[0] * x[0] + g[1] * x[1] + g[2] * x[2] + c0).astype(T))


def random_field(shape, T, seed=3):
    Ng = tuple(n + 2 for n in shape)
    a = np.asfortranarray(np.random.default_rng(seed).standard_normal(Ng).astype(T))
    assert not (a.astype(np.float64) == LEVEL).any()
    return a


def check_plane(tri, Ng, lo=None, hi=None, g=G_LIN, c=C_LIN):
    """the three identities of the oblique plane on a triangle list"""
    lo = (1, 1, 1) if lo is None else lo
    hi = tuple(n - 2 for n in Ng) if hi is None else hi
    nt = len(tri)
    assert nt > 0
    tol = 16 * EPS * float(np.sum(np.abs(g) * np.array(Ng)))
    d = np.abs(tri.reshape(-1, 3) @ g - c).max()
    n = IR.normals(tri)
    foot = (hi[0] - lo[0]) * (hi[1] - lo[1])
    want = foot * np.linalg.norm(g) / abs(g[2])
    got = IR.area(tri)
    print(f"\nplane: {nt} triangles, max |g.x - c| = {d:.3e} (bound {tol:.3e}), area {got!r} want {want!r} (bound {nt * EPS * want:.3e})")
    assert d <= tol
    assert np.all(n @ g > 0)
    assert abs(got - want) <= nt * EPS * want
    z = tri[..., 2]
    assert z.min() > lo[2] - 0.5 and z.max() < hi[2] - 0.5                           # the plane crosses only the side walls


# ---------------------------------------------------------------------------------------------------- the table
def test_table_equals_the_rule_of_the_text():
    L = _lib.lib()
    out = (C.c_int32 * 7)()
    for tet in range(6):
        for mask in range(16):
            assert L.wl_iso_table(tet, mask, out) == 0
            assert list(out) == IR.table_row(tet, mask), (tet, mask)
        for mask in (0, 15):
            assert L.wl_iso_table(tet, mask, out) == 0 and out[0] == 0
    for tet, mask in ((-1, 3), (6, 3), (2, -1), (2, 16)):
        assert L.wl_iso_table(tet, mask, out) == _lib.WL_E_ARG and b"tet must lie in 0..5" in L.wl_last_error()
    assert L.wl_iso_table(0, 1, None) == _lib.WL_E_ARG and b"null output" in L.wl_last_error()


# ---------------------------------------------------------------------------------------------------- argument checks
def _grid3():
    g = _lib.Grid()
    g.D = 3
    g.n[:] = [8, 8, 8]
    g.s[:] = [1, 8, 64]
    g.sc = 512
    return g


def test_entry_point_rejects_bad_calls_before_the_device():
    L = _lib.lib()
    g = _grid3()
    buf = (C.c_double * 64)()
    f = C.cast(buf, C.c_void_p)
    i3 = lambda *v: (C.c_int32 * 3)(*v)
    base = dict(t=_lib.WL_F64, g=C.byref(g), a=f, b=None, c=0.5, lo=None, hi=None, tri=f, val=None, cap=4, cnt=f)
    call = lambda **k: (lambda d: L.wl_isosurface(d["t"], d["g"], d["a"], d["b"], d["c"], d["lo"], d["hi"], d["tri"], d["val"], d["cap"],
                                                  d["cnt"]))({**base, **k})
    g2 = _lib.Grid()
    g2.D = 2
    g2.n[:] = [8, 8, 1]
    g2.s[:] = [1, 8, 64]
    g2.sc = 64
    cases = [({"g": None}, b"null grid, field or count"), ({"a": None}, b"null grid, field or count"), ({"cnt": None}, b"null grid, field or count"),
             ({"g": C.byref(g2)}, b"D == 3"),
             ({"lo": i3(-1, 1, 1), "hi": i3(6, 6, 6)}, b"bad box"), ({"lo": i3(1, 1, 1), "hi": i3(6, 8, 6)}, b"bad box"),
             ({"lo": i3(1, 5, 1), "hi": i3(6, 4, 6)}, b"bad box"),
             ({"c": float("nan")}, b"must be finite"), ({"c": float("inf")}, b"must be finite"), ({"c": float("-inf")}, b"must be finite"),
             ({"cap": -1}, b"negative capacity"), ({"tri": None}, b"null triangle buffer"),
             ({"b": f}, b"given together"), ({"val": f}, b"given together"),
             ({"lo": i3(1, 1, 1)}, b"only one of lo and hi"), ({"hi": i3(6, 6, 6)}, b"only one of lo and hi")]
    for kw, msg in cases:
        assert call(**kw) == _lib.WL_E_ARG and msg in L.wl_last_error(), (kw, L.wl_last_error())


# ---------------------------------------------------------------------------------------------------- the reference against closed forms
def test_reference_on_an_oblique_plane():
    Ng = (14, 12, 16)
    a = linear_field(Ng)
    assert not (a == C_LIN).any()
    assert np.array_equal(linear_field(Ng, T=np.float32).astype(np.float64), a)     # exact in Float32 too
    tri, _, edge, _ = IR.extract(a, C_LIN)
    check_plane(tri, Ng)
    assert np.array_equal(IR.edges_of(tri), edge)


X0 = np.array([11.3, 11.7, 11.45])                    # off-lattice centre (coordinates x = J - 0.5) in a 24^3 box


@functools.lru_cache(maxsize=None)
def solid(kind):
    """(field, level, tri, edge) of a distance field on 26^3 (computed once, read-only)"""
    x = coords((26, 26, 26)) - X0[:, None, None, None]
    if kind == "torus":
        a, c = np.sqrt((np.sqrt(x[0] ** 2 + x[1] ** 2) - 7.0) ** 2 + x[2] ** 2), 2.6
    else:
        a, c = np.sqrt(x[0] ** 2 + x[1] ** 2 + x[2] ** 2), float(kind)
    assert not (a == c).any()
    tri, _, edge, _ = IR.extract(a, c)
    return a, c, tri, edge


def euler(tri):
    pts, conn = iso.weld(tri)
    e = np.sort(np.concatenate([conn[:, [0, 1]], conn[:, [1, 2]], conn[:, [2, 0]]]), axis=1)
    return len(pts) - len(np.unique(e, axis=0)) + len(conn)


@pytest.mark.parametrize("R", [3.7, 9.2])
def test_reference_on_a_sphere(R):
    _, _, tri, _ = solid(R)
    assert IR.closed(tri)
    assert euler(tri) == 2
    vol = IR.volume(tri)
    r = np.linalg.norm(tri.reshape(-1, 3) - X0, axis=1)
    bound = 3.0 / (8.0 * (R - np.sqrt(3.0)))
    print(f"\nsphere R={R}: {len(tri)} triangles, volume {vol:.4f} (ball {4 / 3 * np.pi * R ** 3:.4f}), max | |x-x0| - R | = {np.abs(r - R).max():.3e} "
          f"(bound {bound:.3e})")
    assert vol > 0
    assert np.abs(r - R).max() <= bound
    import torch
    t = torch.from_numpy(tri)
    assert abs(float(iso.enclosed_volume(t)) - vol) <= 1e-12 * vol and abs(float(iso.area(t)) - IR.area(tri)) <= 1e-12 * IR.area(tri)


def test_reference_on_a_torus():
    _, _, tri, _ = solid("torus")
    assert IR.closed(tri)
    assert euler(tri) == 0
    assert IR.volume(tri) > 0


# ---------------------------------------------------------------------------------------------------- weld and the surface file
def _array(node):
    a = np.array(node.text.split(), dtype=np.float64 if node.get("type").startswith("Float") else np.int64)
    nc = int(node.get("NumberOfComponents"))
    return a if nc == 1 else a.reshape(-1, nc)


@pytest.mark.parametrize("color", [False, True])
def test_weld_and_write_vtp_round_trip(tmp_path, color):
    a, c, tri, _ = solid(3.7)
    val = None
    if color:
        b = linear_field(a.shape, np.array([0.3, -0.2, 0.7]), 1.5)
        _, val, _, _ = IR.extract(a, c, b=b)
    pts, conn = iso.weld(tri)
    assert len(np.unique(pts.view(np.uint64), axis=0)) == len(pts) == len(np.unique(tri.reshape(-1, 3), axis=0))
    assert np.array_equal(pts[conn], tri)
    path = tmp_path / "s.vtp"
    iso.write_vtp(path, tri, val, name="b")
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.get("type") == "PolyData"
    piece = root.find("PolyData/Piece")
    assert int(piece.get("NumberOfPolys")) == len(tri) and int(piece.get("NumberOfPoints")) == len(pts)
    pnode = piece.find("Points/DataArray")
    assert pnode.get("type") == "Float32"
    fp = _array(pnode)
    assert np.array_equal(fp, pts.astype(np.float32).astype(np.float64))
    polys = {d.get("Name"): _array(d) for d in piece.findall("Polys/DataArray")}
    assert np.array_equal(polys["offsets"], 3 * np.arange(1, len(tri) + 1))
    assert np.array_equal(fp[polys["connectivity"].reshape(-1, 3)], tri.astype(np.float32).astype(np.float64))
    pd = {d.get("Name"): _array(d) for d in piece.findall("PointData/DataArray")}
    if color:
        assert list(pd) == ["b"]
        assert np.array_equal(pd["b"][polys["connectivity"].reshape(-1, 3)], val.astype(np.float32).astype(np.float64))
    else:
        assert pd == {}
