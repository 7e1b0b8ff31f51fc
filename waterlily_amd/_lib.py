"""ctypes binding of libwlhip.so (the C ABI declared in include/wlhip.h).

There is NO fallback: if the HIP library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import enum
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("WLHIP_LIB") or os.path.join(_HERE, "libwlhip.so")   # (WLHIP_LIB: an alternative build, A/B measurements)
HEADER = os.path.join(os.path.dirname(_HERE), "include", "wlhip.h")
_lib = None

WL_F32, WL_F64 = 0, 1
WL_E_ARG, WL_E_LEVELS, WL_E_NOGPU, WL_E_STATE = 10001, 10002, 10003, 10004


class WlError(RuntimeError):
    pass


class Grid(C.Structure):
    _fields_ = [("D", C.c_int32), ("n", C.c_int32 * 3), ("s", C.c_int64 * 3), ("sc", C.c_int64),
                ("nzg", C.c_int32), ("kz0", C.c_int32), ("own_lo", C.c_int32), ("own_hi", C.c_int32),
                ("zring", C.c_int32)]


class LevelDesc(C.Structure):
    _fields_ = [("g", Grid)] + [(k, C.c_void_p) for k in ("L", "D", "iD", "x", "eps", "r", "z")]


class FlowDesc(C.Structure):
    _fields_ = [("g", Grid)] + [(k, C.c_void_p) for k in ("u", "u0", "f", "p", "sigma", "V", "mu0", "mu1")] + [
        ("nu", C.c_double), ("exitBC", C.c_int32), ("perdir_mask", C.c_int32)]


class BodyDesc(C.Structure):
    """wl_body_desc (include/wlhip.h): a parametric body at one instant"""
    _fields_ = [("family", C.c_int32), ("identity_map", C.c_int32), ("p", C.c_double * 8), ("A", C.c_double * 9),
                ("b", C.c_double * 3), ("dA", C.c_double * 9), ("db", C.c_double * 3), ("Ainv", C.c_double * 9),
                ("op", C.c_int32), ("count", C.c_int32)]


class MeshPose(C.Structure):
    """wl_mesh_pose (include/wlhip.h): the affine map of a mesh body at one instant"""
    _fields_ = [("A", C.c_double * 9), ("b", C.c_double * 3), ("dA", C.c_double * 9), ("db", C.c_double * 3),
                ("Ainv", C.c_double * 9), ("identity_map", C.c_int32)]


# how wl_hist_axis, wl_tp_value and wl_rg_value (include/wlhip.h) all begin: the field and which value of a cell is formed from it
_VALUE_FIELDS = [("f", C.c_void_p), ("kind", C.c_int32), ("ipar", C.c_int32), ("par", C.c_double * 3), ("par2", C.c_double * 3)]


class HistAxis(C.Structure):
    """wl_hist_axis (include/wlhip.h): one axis of a histogram"""
    _fields_ = _VALUE_FIELDS + [("absval", C.c_int32), ("nbins", C.c_int32), ("lo", C.c_double), ("hi", C.c_double),
                                ("range_dev", C.c_void_p), ("edges_dev", C.c_void_p)]


class TpValue(C.Structure):
    """wl_tp_value (include/wlhip.h): one of the two values of a two-point statistic"""
    _fields_ = _VALUE_FIELDS


class RgValue(C.Structure):
    """wl_rg_value (include/wlhip.h): the value whose threshold set wl_regions labels"""
    _fields_ = _VALUE_FIELDS + [("absval", C.c_int32)]


WL_RG_BELOW, WL_RG_ABOVE = 0, 1


class RsCol(C.Structure):
    """wl_rs_col (include/wlhip.h): one column of wl_region_sums: the value, its power and the index it is weighted with"""
    _fields_ = [("v", RgValue), ("power", C.c_int32), ("moment", C.c_int32)]


WL_RS_FIND, WL_RS_GIVEN = 0, 1
WL_RS_MAX_COLS, WL_RS_EMIN = 8, -894


WL_BODY_SPHERE, WL_BODY_TORUS, WL_BODY_PLATE, WL_BODY_CYLINDER = 0, 1, 2, 3
WL_BODY_OP_UNION, WL_BODY_OP_MINUS, WL_BODY_OP_INTERSECT = 0, 1, 2
WL_BODY_MAXLEAF = 6


class Opt(enum.IntEnum):
    """wl_set_option keys: the WL_OPT_* enumerators of include/wlhip.h (tests/test_options.py holds the two together).
    SWEEP_ALTERNATE holds two bits: bit 0 = consecutive marching kernels sweep in opposite directions, bit 1 = every XCD keeps
    one contiguous slab of z instead of z-chunks dealt round-robin (1: default, 3: alternate + slabs, 0 / 2: ascending)."""
    STENCIL7_VEC = 0
    SMOOTH_FUSED = 1
    CONVDIFF_TILED = 2
    BDIM_ROWFLAGS = 3
    STENCIL7_ROWS = 4
    PCG_VEC = 5
    COARSE_TAIL = 6
    BC_FUSED = 7
    PCG_DEFER_X = 8
    ROW_CONST_L = 9
    PCG_START_FUSED = 10
    PCG_RECOMPUTE_PRECOND = 13
    SCALE_CHAIN = 14
    PCG_DOTS_IN_KERNEL = 15
    STENCIL7_GRID_K = 16
    STREAM_GRID_K = 17
    CONVDIFF_SHARED_FLUX = 18
    PCG_RECOMPUTE_AEPS = 19
    DIV_IN_RESIDUAL = 22
    XGHOST_IN_KERNEL = 23
    MBOX_TIMEOUT_S = 26
    BDIM_IN_CONVDIFF = 27
    SWEEP_ALTERNATE = 30
    COARSE_PCG_RESIDENT = 31


def opt_key(key) -> int:
    """A wl_set_option key given as an Opt, a number, or a name ("PCG_VEC", "WL_OPT_PCG_VEC", "5"): the number.
    Numbers pass unchecked (the library refuses the ones it does not know)."""
    if isinstance(key, str) and not key.strip().lstrip("+-").isdigit():
        name = key.strip().upper()
        name = name[len("WL_OPT_"):] if name.startswith("WL_OPT_") else name
        if name not in Opt.__members__:
            raise WlError(f"no such option: {key!r} (one of {', '.join(Opt.__members__)})")
        return int(Opt[name])
    return int(key)


def opt_name(key) -> str:
    """How a tool prints a key: NAME (number)"""
    k = opt_key(key)
    return f"{Opt(k).name} ({k})" if k in Opt._value2member_map_ else str(k)


SENDRECV_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int)
ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_double), C.c_int, C.c_int)
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64)


def build(force: bool = False) -> str:
    """Compile waterlily_amd/libwlhip.so for gfx950 with hipcc (cross-compiles without a GPU)."""
    csrc = os.path.join(_HERE, "csrc")
    srcs = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [HEADER]
    stale = (not os.path.exists(LIB_PATH)) or any(os.path.getmtime(s) > os.path.getmtime(LIB_PATH) for s in srcs)
    if force or stale:
        r = subprocess.run(["make", "-C", csrc], capture_output=True, text=True)
        if r.returncode != 0:
            raise WlError("building libwlhip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


def declared_symbols() -> list[str]:
    """Every function the public header declares (used by the CPU-side export test)."""
    txt = open(HEADER).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(wl_[a-zA-Z0-9_]+)\s*\(", txt)))


def lib() -> C.CDLL:
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise WlError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "(waterlily_amd has no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    vp, gp, dp, i, d, i64 = C.c_void_p, C.POINTER(Grid), C.POINTER(C.c_double), C.c_int, C.c_double, C.c_int64
    ip = C.POINTER(C.c_int)
    sig = {
        "wl_abi_version": (i, []),
        "wl_last_error": (C.c_char_p, []),
        "wl_device_count": (i, [ip]),
        "wl_set_device": (i, [i]),
        "wl_set_stream": (i, [vp]),
        "wl_sync": (i, []),
        "wl_malloc": (i, [C.POINTER(vp), C.c_size_t]),
        "wl_free": (i, [vp]),
        "wl_h2d": (i, [vp, vp, C.c_size_t]),
        "wl_d2h": (i, [vp, vp, C.c_size_t]),
        "wl_memset0": (i, [vp, C.c_size_t]),
        "wl_h2d_2d": (i, [vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t]),
        "wl_d2h_2d": (i, [vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, C.c_size_t]),
        "wl_comm_unique_id": (i, [vp]),
        "wl_comm_init_rccl": (i, [vp, i, i]),
        "wl_comm_init_host": (i, [i, i, SENDRECV_FN, ALLREDUCE_FN, ALLGATHER_FN, vp]),
        "wl_comm_init_loopback": (i, [i, i]),
        "wl_comm_mailbox": (i, [C.c_char_p, i]),
        "wl_comm_mailbox_off": (i, []),
        "wl_comm_mailbox_active": (i, [ip]),
        "wl_comm_finalize": (i, []),
        "wl_comm_rank": (i, [ip, ip]),
        "wl_halo_exchange": (i, [i, gp, vp, i, i]),
        "wl_allreduce": (i, [dp, i, i]),
        "wl_bc_vec": (i, [i, gp, vp, dp, i, i]),
        "wl_bc_per": (i, [i, gp, vp, i]),
        "wl_exit_bc": (i, [i, gp, vp, vp, dp, d]),
        "wl_L2_inside": (i, [i, gp, vp, dp]),
        "wl_dot": (i, [i, gp, vp, vp, dp]),
        "wl_sum": (i, [i, gp, vp, dp]),
        "wl_max": (i, [i, gp, vp, dp]),
        "wl_conv_diff": (i, [i, gp, vp, vp, vp, d, i]),
        "wl_accelerate": (i, [i, gp, vp, dp]),
        "wl_bdim": (i, [i, gp, vp, vp, vp, vp, vp, vp, d]),
        "wl_scale_u": (i, [i, gp, vp, d]),
        "wl_div": (i, [i, gp, vp, vp]),
        "wl_cfl": (i, [i, gp, vp, vp, d, dp]),
        "wl_set_diag": (i, [i, gp, vp, vp, vp]),
        "wl_restrictL": (i, [i, gp, vp, gp, vp, i]),
        "wl_restrict": (i, [i, gp, vp, gp, vp]),
        "wl_prolongate": (i, [i, gp, vp, gp, vp]),
        "wl_mg_create": (i, [C.POINTER(vp), i, i, C.POINTER(LevelDesc), i]),
        "wl_mg_destroy": (i, [vp]),
        "wl_mg_update": (i, [vp]),
        "wl_mg_update_changed": (i, [vp, vp]),
        "wl_mg_uniform_rows": (i, [vp, i, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]),
        "wl_mg_mult": (i, [vp, i, vp]),
        "wl_mg_residual": (i, [vp, i]),
        "wl_mg_increment": (i, [vp, i]),
        "wl_mg_jacobi": (i, [vp, i, i]),
        "wl_mg_pcg": (i, [vp, i, i, ip]),
        "wl_mg_L2": (i, [vp, i, dp]),
        "wl_mg_Linf": (i, [vp, i, dp]),
        "wl_mg_log": (i, [vp, i]),
        "wl_mg_log_read": (i, [vp, dp, i, ip]),
        "wl_mg_vcycle": (i, [vp, i]),
        "wl_mg_solve": (i, [vp, d, i, ip]),
        "wl_flow_create": (i, [C.POINTER(vp), i, C.POINTER(FlowDesc)]),
        "wl_flow_destroy": (i, [vp]),
        "wl_flow_update": (i, [vp]),
        "wl_measure_rows": (i, [vp, C.POINTER(BodyDesc), d, C.POINTER(i64)]),
        "wl_measure_fill": (i, [vp, C.POINTER(BodyDesc), d, vp]),
        "wl_body_nds": (i, [gp, C.POINTER(BodyDesc), vp, i64, vp]),
        "wl_mesh_create": (i, [C.POINTER(vp), vp, i64, vp, i64, d]),
        "wl_mesh_destroy": (i, [vp]),
        "wl_mesh_info": (i, [vp, C.POINTER(i64)]),
        "wl_mesh_eval_host": (i, [vp, C.POINTER(MeshPose), vp, i64, d, vp, vp, vp]),
        "wl_measure_rows_mesh": (i, [vp, vp, C.POINTER(MeshPose), d, C.POINTER(i64)]),
        "wl_measure_fill_mesh": (i, [vp, vp, C.POINTER(MeshPose), d, vp]),
        "wl_body_nds_mesh": (i, [gp, vp, C.POINTER(MeshPose), vp, i64, vp]),
        "wl_project": (i, [vp, vp, d, d, ip]),
        "wl_mom_step": (i, [vp, vp, d, dp, dp, dp, dp, ip]),
        "wl_metric": (i, [i, gp, i, vp, vp, i, dp, dp]),
        "wl_pforce": (i, [i, gp, vp, vp, vp, i64, dp]),
        "wl_vforce": (i, [i, gp, vp, vp, vp, i64, d, dp]),
        "wl_pmoment": (i, [i, gp, vp, vp, vp, i64, dp, dp]),
        "wl_body_loads": (i, [i, gp, vp, vp, d, C.POINTER(BodyDesc), vp, i64, dp, vp]),
        "wl_body_loads_mesh": (i, [i, gp, vp, vp, d, vp, C.POINTER(MeshPose), vp, i64, dp, vp]),
        "wl_band_loads": (i, [i, gp, vp, vp, d, vp, vp, i64, dp, vp]),
        "wl_flow_integrals": (i, [i, gp, vp, dp, vp]),
        "wl_meanflow_update": (i, [i, i, gp, vp, vp, gp, vp, vp, vp, vp, d, i]),
        "wl_budget_update": (i, [i, i, gp, vp, vp, gp, vp, vp, vp, vp, vp, vp, d, i]),
        "wl_budget_terms": (i, [i, gp, vp, vp, vp, vp, vp, d, vp]),
        "wl_interp": (i, [i, gp, vp, i, vp, i64, vp, i64]),
        "wl_tracer_advance": (i, [i, gp, vp, vp, i64, d, i]),
        "wl_surface_sample": (i, [i, gp, vp, vp, vp, C.POINTER(MeshPose), d, d, vp, vp, vp, d, i]),
        "wl_surface_totals": (i, [vp, vp, i64, dp, vp]),
        "wl_iso_table": (i, [i, i, C.POINTER(C.c_int32)]),
        "wl_isosurface": (i, [i, gp, vp, vp, d, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp, i64, vp]),
        "wl_render_project": (i, [i, gp, vp, i, i, dp, dp, i, i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, i64]),
        "wl_render_shade": (i, [vp, i64, i, i, d, d, i, vp, vp, i64, d, C.POINTER(C.c_uint8), C.POINTER(C.c_uint8), i, i, vp]),
        "wl_scene_clear": (i, [vp, i, i]),
        "wl_scene_scratch": (i, [i64, C.POINTER(i64)]),
        "wl_scene_draw": (i, [vp, i, i, dp, vp, i64, C.c_uint32, i64, vp, i64]),
        "wl_scene_shade": (i, [vp, i, i, C.c_uint32, i64, vp, vp, dp, d, d, i, vp, C.POINTER(C.c_uint8), dp, d, C.POINTER(C.c_uint8), vp]),
        "wl_scene_resolve": (i, [vp, i, i, vp, i, C.POINTER(C.c_uint8), vp]),
        "wl_scene_volume": (i, [i, gp, vp, dp, d, C.POINTER(C.c_int32), C.POINTER(C.c_int32), d, d, i, vp, vp, d, vp, vp, vp, vp, i, i]),
        "wl_scene_average": (i, [vp, i, i, i, vp]),
        "wl_downsample": (i, [i, gp, vp, i, i, dp, dp, i, i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), i, vp, i, i]),
        "wl_downsample_extent": (i, [gp, i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        "wl_histogram": (i, [i, gp, vp, vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), i, vp]),      # (a, b: byref(HistAxis))
        "wl_field_range": (i, [i, gp, vp, i, i, dp, dp, i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, i64, vp]),
        "wl_field_range_scratch": (i, [gp, C.POINTER(C.c_int64)]),
        "wl_twopoint": (i, [i, gp, vp, vp, i, i, i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), i, vp, i64, vp]),      # (a, b: byref(TpValue))
        "wl_twopoint_scratch": (i, [gp, i, i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
        "wl_regions": (i, [i, gp, vp, i, d, i, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, i64, vp, vp, vp, vp, i64]),      # (v: byref(RgValue))
        "wl_regions_scratch": (i, [gp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]),
        "wl_region_sums": (i, [i, gp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), vp, vp, i64, i, vp, i, vp, vp, vp, vp]),      # (cols: an array of RsCol)
        "wl_snapshot_pack": (i, [i, gp, vp, i, i, i, i, vp]),
        "wl_snapshot_unpack": (i, [i, gp, vp, i, i, i, i, vp]),
        "wl_set_option": (i, [i, i]),
        "wl_get_option": (i, [i, ip]),
        "wl_kernel_name": (C.c_char_p, [i]),
        "wl_prof_select": (i, [i, i64]),
        "wl_prof_reset": (i, []),
        "wl_prof_overlapped": (i, [C.POINTER(i64)]),
        "wl_prof_dealt": (i, [C.POINTER(i64)]),
        "wl_prof_counts": (i, [i, C.POINTER(i64), C.POINTER(i64)]),
        "wl_prof_allocs": (i, [C.POINTER(i64), C.POINTER(i64)]),
        "wl_prof_comm": (i, [C.POINTER(i64)]),
        "wl_prof_reset_comm": (i, []),
        "wl_prof_allreduce_us": (i, [i, dp]),
        "wl_prof_timed": (i, [C.POINTER(i64), C.POINTER(i64), dp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(L, name)
        fn.restype = res
        fn.argtypes = args
    if L.wl_abi_version() != 6:
        raise WlError("libwlhip.so ABI version mismatch; rebuild it")
    _lib = L
    return L


def check(rc: int) -> None:
    if rc != 0:
        msg = lib().wl_last_error().decode(errors="replace")
        if rc == WL_E_LEVELS:
            raise AssertionError("MultiLevelPoisson requires size=a2ⁿ, where n>2")
        raise WlError(f"libwlhip call failed ({rc}): {msg}")


def set_option(key, value: int):
    """Tuning / A-B switches of the library (include/wlhip.h, wl_set_option); key: an Opt, its number or its name."""
    check(lib().wl_set_option(opt_key(key), int(value)))


def get_option(key) -> int:
    v = C.c_int()
    check(lib().wl_get_option(opt_key(key), C.byref(v)))
    return v.value


@contextlib.contextmanager
def options(values):
    """`with options({Opt.PCG_DEFER_X: 0, ...}):` sets the given keys and puts the values they HAD back on the way out,
    exception or not."""
    keep = {k: get_option(k) for k in values}
    try:
        for k, v in values.items():
            set_option(k, v)
        yield
    finally:
        for k, v in keep.items():
            set_option(k, v)


def d3(v):
    import numpy as np
    v = list(np.asarray(v, dtype=np.float64).ravel()) + [0.0] * 3
    return (C.c_double * 3)(*v[:3])
