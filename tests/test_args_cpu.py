"""The argument checks the entry points of libwlhip.so share, without a GPU: every entry point that takes a wl_dtype refuses an
unknown one, the older reducers refuse a null output, the three box parsers hold one rule (and their two stated differences), and
the recorders' shared series buffer grows, resets and refuses a foreign flow on CPU tensors.  Pointers are fake: every call fails
validation before anything is dereferenced."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from waterlily_amd import _lib, _series

E = _lib.WL_E_ARG
FAKE = C.c_void_p(0x1000)


def grid(n=8):
    g = _lib.Grid()
    g.D = 3
    g.n[:] = [n, n, n]
    g.s[:] = [1, n, n * n]
    g.sc = n ** 3
    return g


def dtype_params():
    """{entry point: positions of its wl_dtype parameters}, read from the declarations of include/wlhip.h"""
    txt = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER).read(), flags=re.S)
    out = {}
    for name, params in re.findall(r"\bint\s+(wl_\w+)\s*\(([^()]*)\)\s*;", txt):
        pos = [k for k, p in enumerate(params.split(",")) if p.strip().startswith("wl_dtype")]
        if pos:
            out[name] = pos
    return out


def descriptors():
    """valid descriptors of a flow and of a three-level multigrid (fields: one host array, never reached)"""
    host = (C.c_float * (3 * 18 ** 3))()
    fd = _lib.FlowDesc()
    fd.g = grid(18)
    for k in ("u", "u0", "f", "p", "sigma", "V", "mu0", "mu1"):
        setattr(fd, k, C.addressof(host))
    fd.nu = 0.01
    levels = (_lib.LevelDesc * 3)()
    for lv, n in zip(levels, (18, 10, 6)):
        lv.g = grid(n)
        for k in ("L", "D", "iD", "x", "eps", "r", "z"):
            setattr(lv, k, C.addressof(host))
    return host, fd, levels


def plain_args(fn, g, keep):
    """one unobjectionable value per parameter, by its ctypes type"""
    body = (_lib.BodyDesc * 2)()
    body[0].family, body[0].count = _lib.WL_BODY_SPHERE, 1
    pose = _lib.MeshPose()
    pose.identity_map = 1
    keep += [body, pose]
    by_type = {C.POINTER(_lib.Grid): C.byref(g), C.c_void_p: FAKE, C.POINTER(C.c_double): (C.c_double * 3)(), C.c_double: 0.5, C.c_int: 0,
               C.c_int64: 0, C.POINTER(C.c_int32): None, C.POINTER(_lib.BodyDesc): body, C.POINTER(_lib.MeshPose): C.byref(pose)}
    return [by_type[t] for t in fn.argtypes]


def test_every_entry_point_refuses_an_unknown_dtype():
    L = _lib.lib()
    table = dtype_params()
    assert len(table) >= 37 and {"wl_pforce", "wl_snapshot_pack", "wl_halo_exchange", "wl_meanflow_update", "wl_downsample"} <= set(table)
    g, keep = grid(), []
    host, fd, levels = descriptors()
    for name, positions in sorted(table.items()):
        fn = getattr(L, name)
        for pos in positions:
            h = C.c_void_p()
            if name == "wl_flow_create":
                args = [C.byref(h), 0, C.byref(fd)]
            elif name == "wl_mg_create":
                args = [C.byref(h), 0, 3, levels, 0]
            else:
                args = plain_args(fn, g, keep)
            args[pos] = 7
            rc = fn(*args)
            assert rc == E and b"dtype" in L.wl_last_error(), (name, pos, rc, L.wl_last_error())
            assert h.value is None, name


def test_reducers_refuse_a_null_output():
    L = _lib.lib()
    g = grid()
    gp, d3 = C.byref(g), (C.c_double * 3)()
    calls = {
        "wl_L2_inside": lambda: L.wl_L2_inside(0, gp, FAKE, None),
        "wl_dot": lambda: L.wl_dot(0, gp, FAKE, FAKE, None),
        "wl_sum": lambda: L.wl_sum(0, gp, FAKE, None),
        "wl_max": lambda: L.wl_max(0, gp, FAKE, None),
        "wl_cfl": lambda: L.wl_cfl(0, gp, FAKE, FAKE, 0.1, None),
        "wl_pforce": lambda: L.wl_pforce(0, gp, FAKE, FAKE, FAKE, 4, None),
        "wl_vforce": lambda: L.wl_vforce(0, gp, FAKE, FAKE, FAKE, 4, 0.1, None),
        "wl_pmoment": lambda: L.wl_pmoment(0, gp, FAKE, FAKE, FAKE, 4, d3, None),
        "wl_pmoment (x0)": lambda: L.wl_pmoment(0, gp, FAKE, FAKE, FAKE, 4, None, d3),
        "wl_mg_L2": lambda: L.wl_mg_L2(None, 0, None),
    }
    for name, call in calls.items():
        assert call() == E and b"null" in L.wl_last_error() and name.split()[0].encode() in L.wl_last_error(), (name, L.wl_last_error())


def i3(*v):
    return (C.c_int32 * 3)(*v)


def test_one_box_rule_through_three_entry_points():
    """the same boxes on an 8 x 8 x 8 grid: lo and hi come together, 0 <= lo <= hi <= n - 1; only wl_downsample refuses an empty
    extent (lo == hi), and only wl_isosurface's default stops at n - 2 (which none of the rules below can tell apart)"""
    L = _lib.lib()
    g = grid()
    gp = C.byref(g)
    nc, k0 = (C.c_int32 * 3)(), C.c_int32()
    cnt = (C.c_int64 * 1)()
    iso = lambda lo, hi: L.wl_isosurface(0, gp, FAKE, None, 0.5, lo, hi, None, None, 0, cnt)
    # ld = -1 is refused AFTER the box: "ld" in the message says that the box passed
    ren = lambda lo, hi: L.wl_render_project(0, gp, FAKE, 0, 0, None, None, 2, 0, lo, hi, FAKE, -1)
    ext = lambda lo, hi: L.wl_downsample_extent(gp, 1, lo, hi, nc, C.byref(k0))

    def refused(call, lo, hi, word):
        assert call(lo, hi) == E and word in L.wl_last_error(), (lo and list(lo), hi and list(hi), L.wl_last_error())

    def render_accepts(lo, hi):
        assert ren(lo, hi) == E and b"ld" in L.wl_last_error() and b"box" not in L.wl_last_error(), L.wl_last_error()

    for call in (iso, ren, ext):
        refused(call, i3(1, 1, 1), None, b"only one")
        refused(call, None, i3(4, 4, 4), b"only one")
        refused(call, i3(1, 1, 1), i3(8, 4, 4), b"box")               # hi = n
        refused(call, i3(1, 1, 1), i3(4, 4, 8), b"box")
        refused(call, i3(-1, 1, 1), i3(4, 4, 4), b"box")
        refused(call, i3(5, 1, 1), i3(4, 4, 4), b"box")
    # lo == hi in one direction: the documented difference
    refused(ext, i3(4, 1, 1), i3(4, 4, 4), b"box")
    render_accepts(i3(4, 1, 1), i3(4, 4, 4))
    # a box with cells and the default box
    for lo, hi in ((i3(1, 1, 1), i3(4, 4, 7)), (None, None)):
        assert ext(lo, hi) == 0, L.wl_last_error()
        render_accepts(lo, hi)
    assert list(nc) == [6, 6, 6] and k0.value == 0                     # the default of wl_downsample_extent: 1 .. n - 1
    if not torch.cuda.is_available():
        # wl_isosurface has no check behind the box: acceptance shows as the device's refusal (a HIP error number), seen only
        # where there is no device -- with one, the call would run on the fake pointers
        for lo, hi in ((i3(4, 1, 1), i3(4, 4, 4)), (i3(1, 1, 1), i3(4, 4, 7)), (None, None)):
            rc = iso(lo, hi)
            assert rc != 0 and rc != E, (rc, L.wl_last_error())


# --------------------------------------------------------------------------- the recorders' series buffer, on CPU tensors

def test_series_grows_resets_and_refuses_a_foreign_flow():
    slab = object()
    sr = _series.Series(("Thing", "the recorder was"), 3, slab, (2, 3), 2, "cpu")
    assert tuple(sr.buf.shape) == (2, 2, 3) and sr.buf.dtype == torch.float64 and sr.t == [] and sr.D == 3 and sr.slab is slab
    rng = np.random.default_rng(0)
    rows = rng.standard_normal((5, 2, 3))
    for k in range(5):
        row = _series.next_row(sr, 3, slab)
        assert row.data_ptr() == sr.buf[k].data_ptr()
        row.copy_(torch.from_numpy(rows[k]))
        sr.t.append(0.5 * k)
    assert sr.buf.shape[0] == 8                                        # 2 -> 4 -> 8
    assert np.array_equal(sr.buf[:4].numpy().view(np.uint64), rows[:4].view(np.uint64))      # bit for bit through two growths
    assert np.array_equal(sr.buf[4].numpy(), rows[4])
    with pytest.raises(ValueError, match="dimension or slab"):
        _series.next_row(sr, 2, slab)
    with pytest.raises(ValueError, match="dimension or slab"):
        _series.next_row(sr, 3, None)
    with pytest.raises(ValueError, match="Thing: capacity"):
        _series.Series(("Thing", "the recorder was"), 3, None, (1,), 0, "cpu")
    _series.reset(sr)
    assert sr.t == [] and sr.buf.shape[0] == 8


def test_single_rank_combination_returns_the_rows():
    sr = _series.Series(("Thing", "the recorder was"), 2, None, (4,), 2, "cpu")
    vals = np.arange(12, dtype=np.float64).reshape(3, 4)
    vals[1, 2] = -0.0
    for k in range(3):
        _series.next_row(sr, 2, None).copy_(torch.from_numpy(vals[k]))
        sr.t.append(float(k))
    t, parts = _series.rank_rows(sr)
    assert np.array_equal(t, [0.0, 1.0, 2.0]) and t.dtype == np.float64 and len(parts) == 1
    assert np.array_equal(parts[0].view(np.uint64), vals.view(np.uint64))
    assert _series._add(parts) is parts[0]
    v = np.ones(3)
    assert _series._rank_parts(v, None)[0] is v and _series._rank_sum(v, None) is v
    from waterlily_amd import probes
    assert probes._rank_parts is _series._rank_parts and probes._rank_sum is _series._rank_sum
