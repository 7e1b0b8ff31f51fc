"""Regions without a GPU: every refusal of wl_regions / wl_regions_scratch comes back WL_E_ARG through the C ABI before the
device is touched (pointers are fake: nothing is dereferenced but the value struct), the scratch arithmetic, the yardstick
tests/regions_ref.py against hand-written 2-D cases whose answers are known, and the torch functions of the table on CPU
tensors."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import regions_ref as RR  # noqa: E402

from waterlily_amd import _lib, regions  # noqa: E402
from waterlily_amd.twopoint import TwoPoint, Value  # noqa: E402

E = _lib.WL_E_ARG
FAKE = C.c_void_p(0x1000)
R_METRIC, M_OMAG, M_LAMBDA2, M_CURL = 16, 2, 4, 1


def grid(n=(10, 9, 8)):
    g = _lib.Grid()
    g.D = len(n)
    nn = list(n) + [1] * (3 - len(n))
    g.n[:] = nn
    g.s[:] = [1, nn[0], nn[0] * nn[1]]
    g.sc = nn[0] * nn[1] * nn[2]
    return g


def i3(*v):
    return (C.c_int32 * 3)(*(list(v) + [0] * 3)[:3])


def value(kind=0, ipar=0, f=0x1000, absval=0):
    v = _lib.RgValue()
    v.f, v.kind, v.ipar, v.absval = f, kind, ipar, absval
    return v


def call(g=None, v=None, t=0, cmp=0, c=0.5, mask=0, lo=None, hi=None, label=FAKE, cap=0, tab=None, ext=None, n=FAKE, scratch=FAKE, nbytes=1 << 40,
         null_g=False, null_v=False):
    g = grid() if g is None else g
    v = value() if v is None else v
    return _lib.lib().wl_regions(t, None if null_g else C.byref(g), None if null_v else C.byref(v), cmp, c, mask, lo, hi, label, cap, tab, ext, n,
                                 scratch, nbytes)


def refused(word, **kw):
    rc = call(**kw)
    err = _lib.lib().wl_last_error()
    assert rc == E and b"wl_regions" in err and word in err, (kw, rc, err)


def test_every_refusal_comes_back_before_the_device_is_touched():
    refused(b"null", null_g=True)
    refused(b"null", null_v=True)
    refused(b"null", label=None)
    refused(b"null", n=None)
    refused(b"null", scratch=None)
    refused(b"null field", v=value(f=None))
    refused(b"dtype", t=7)
    refused(b"kind", v=value(kind=3))                                  # WL_R_FACE
    refused(b"kind", v=value(kind=9))
    refused(b"kind", v=value(kind=1, ipar=3))                          # a component the dimension does not have
    refused(b"kind", v=value(kind=1, ipar=2), g=grid((10, 9)))
    refused(b"metric", v=value(kind=R_METRIC + 7))
    refused(b"metric", v=value(kind=R_METRIC + M_CURL, ipar=3))
    refused(b"metric", v=value(kind=R_METRIC + M_LAMBDA2), g=grid((10, 9)))     # lambda2 is 3-D
    refused(b"cmp", cmp=2)
    refused(b"cmp", cmp=-1)
    refused(b"NaN", c=float("nan"))
    refused(b"periodic_mask", mask=8)
    refused(b"periodic_mask", mask=-1)
    refused(b"periodic_mask", mask=4, g=grid((10, 9)))                 # a bit for an axis a 2-D grid does not have
    refused(b"only one", lo=i3(1, 1, 1))
    refused(b"only one", hi=i3(4, 4, 4))
    refused(b"box", lo=i3(1, 1, 1), hi=i3(10, 4, 4))                   # hi = n
    refused(b"box", lo=i3(-1, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(4, 1, 1), hi=i3(4, 4, 4))                    # empty
    refused(b"box", lo=i3(5, 1, 1), hi=i3(4, 4, 4))
    refused(b"inside()", v=value(kind=R_METRIC + M_OMAG), lo=i3(0, 1, 1), hi=i3(4, 4, 4))
    refused(b"capacity", cap=-1)
    refused(b"null table", cap=4, tab=None, ext=FAKE)
    refused(b"null table", cap=4, tab=FAKE, ext=None)
    refused(b"aligned", scratch=C.c_void_p(0x1004))
    refused(b"aligned", label=C.c_void_p(0x1002))
    refused(b"scratch", nbytes=16 * 7 * 6 + 7)                         # one byte short of wl_regions_scratch's
    refused(b"scratch", nbytes=0)
    big = grid((2050, 1026, 1026))                                     # 2048 * 1024 * 1024 = 2^31 cells in inside()
    refused(b"2^31", g=big)
    slab = grid()
    slab.nzg, slab.kz0, slab.own_lo, slab.own_hi = 14, 0, 1, 6        # a z-slab of a decomposed array
    refused(b"decomposed", g=slab)


def test_what_passes_every_check_reaches_the_device():
    """the mirror of the refusals: the same calls with nothing wrong pass validation, which shows as the device's own refusal (a
    HIP error number) where there is no device -- with one, the call would run on the fake pointers"""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    for kw in (dict(), dict(c=float("inf")), dict(c=float("-inf"), cmp=1), dict(mask=7), dict(lo=i3(0, 0, 0), hi=i3(9, 8, 7)),
               dict(v=value(kind=R_METRIC + M_LAMBDA2), lo=i3(1, 1, 1), hi=i3(9, 8, 7)), dict(cap=4, tab=FAKE, ext=FAKE),
               dict(nbytes=16 * 7 * 6 + 8), dict(g=grid((10, 9)), mask=3, v=value(kind=2, ipar=1))):
        rc = call(**kw)
        assert rc != 0 and rc != E, (kw, rc, _lib.lib().wl_last_error())


def test_scratch_is_sixteen_bytes_per_row_plus_eight():
    L = _lib.lib()
    nb = C.c_int64(-1)
    g = grid()
    assert L.wl_regions_scratch(C.byref(g), None, None, C.byref(nb)) == 0 and nb.value == 16 * 7 * 6 + 8
    assert L.wl_regions_scratch(C.byref(g), i3(0, 2, 1), i3(9, 5, 7), C.byref(nb)) == 0 and nb.value == 16 * 3 * 6 + 8      # x does not count
    g2 = grid((40, 24))
    assert L.wl_regions_scratch(C.byref(g2), None, None, C.byref(nb)) == 0 and nb.value == 16 * 22 + 8
    assert L.wl_regions_scratch(C.byref(g2), i3(3, 2), i3(39, 23), C.byref(nb)) == 0 and nb.value == 16 * 21 + 8
    assert L.wl_regions_scratch(None, None, None, C.byref(nb)) == E
    assert L.wl_regions_scratch(C.byref(g), None, None, None) == E
    assert L.wl_regions_scratch(C.byref(g), i3(1, 1, 1), None, C.byref(nb)) == E
    assert L.wl_regions_scratch(C.byref(g), i3(1, 1, 1), i3(1, 4, 4), C.byref(nb)) == E
    assert L.wl_regions_scratch(C.byref(grid((2050, 1026, 1026))), None, None, C.byref(nb)) == E and b"2^31" in L.wl_last_error()


# --------------------------------------------------------------------------- the yardstick against answers known by hand

def pic(*rows):
    """a 2-D box from a picture: rows are y (the first row is j = 0), columns x; '#' = -1 (IN for below 0), '.' = +1"""
    return np.array([[-1.0 if ch == "#" else 1.0 for ch in row] for row in rows], dtype=np.float64).T


def test_ref_two_blobs():
    v = pic("##...",
            "##..#",
            "....#")
    lab, tab, ext, n = RR.regions(v, 0.0, lo=(3, 2))
    assert n.tolist() == [2, 6, 0, 15]
    assert lab.T.tolist() == [[0, 0, -1, -1, -1], [0, 0, -1, -1, 1], [-1, -1, -1, -1, 1]]
    #                     root cells  sum i        sum j   sum k  i-range  j-range  k     argmin argmax
    assert tab[0].tolist() == [0, 4, 3 + 4 + 3 + 4, 2 + 2 + 3 + 3, 0, 3, 4, 2, 3, 0, 0, 0, 0]
    assert tab[1].tolist() == [9, 2, 7 + 7, 3 + 4, 0, 7, 7, 3, 4, 0, 0, 9, 9]
    assert ext.tolist() == [[-1.0, -1.0], [-1.0, -1.0]]


def test_ref_ring_and_the_hole_it_encloses():
    v = pic(".....",
            ".###.",
            ".#.#.",
            ".###.",
            ".....")
    lab, tab, ext, n = RR.regions(v, 0.0)
    assert n.tolist() == [1, 8, 0, 25] and tab[0, 1] == 8 and tab[0, 0] == 6 and tab[0, 5:9].tolist() == [2, 4, 2, 4]
    lab, tab, ext, n = RR.regions(v, 0.0, above=True)          # the complement: the outside and the hole, not joined
    assert n.tolist() == [2, 17, 0, 25] and tab[:, 1].tolist() == [16, 1] and tab[1, 0] == 12 and lab[2, 2] == 1 and lab[0, 0] == 0


def test_ref_a_diagonal_pair_does_not_join():
    v = pic("#.",
            ".#")
    lab, tab, ext, n = RR.regions(v, 0.0)
    assert n[0] == 2 and lab.T.tolist() == [[0, -1], [-1, 1]]
    lab, tab, ext, n = RR.regions(v, 0.0, periodic=(0, 1))     # nor through the wrap of a line of two cells
    assert n[0] == 2


def test_ref_a_wrap_join():
    v = pic("#..#",
            "....",
            ".#..",
            ".#..")
    assert RR.regions(v, 0.0)[3][0] == 3
    lab, tab, ext, n = RR.regions(v, 0.0, periodic=(0,))       # x: the two cells of the first row are one region
    assert n[0] == 2 and lab[0, 0] == lab[3, 0] == 0 and tab[0, 1] == 2 and tab[0, 5:7].tolist() == [1, 4]
    lab, tab, ext, n = RR.regions(v, 0.0, periodic=(1,))       # y: (1, 3) is joined to (1, 0), which is out: nothing changes
    assert n[0] == 3
    v[1, 0] = -1.0
    lab, tab, ext, n = RR.regions(v, 0.0, periodic=(1,))       # now the column joins the first row's left cells through the wrap
    assert n[0] == 2 and lab[1, 3] == lab[0, 0] == 0 and tab[:, 1].tolist() == [4, 1]


def test_ref_a_cell_equal_to_c_is_out_and_nan_is_counted():
    v = np.array([[0.25, 0.5, 0.75], [0.5, np.nan, 0.5], [-0.0, 0.0, -np.inf]]).T
    lab, tab, ext, n = RR.regions(v, 0.5)
    assert n.tolist() == [2, 4, 1, 9] and lab.T.tolist() == [[0, -1, -1], [-1, -1, -1], [1, 1, 1]]
    assert np.array_equal(ext[1].view(np.uint64), np.array([-np.inf, 0.0]).view(np.uint64)) and tab[1, 11] == 8 and tab[1, 12] == 7
    lab, tab, ext, n = RR.regions(v, 0.5, above=True)
    assert n.tolist() == [1, 1, 1, 9] and lab[2, 0] == 0
    lab, tab, ext, n = RR.regions(v[:2, 2:], 0.5)              # -0 < +0: the minimum is -0, the maximum +0
    assert np.array_equal(ext[0].view(np.uint64), np.array([-0.0, 0.0]).view(np.uint64)) and tab[0, 11:].tolist() == [0, 1]


# --------------------------------------------------------------------------- the functions of the table, on CPU tensors

def result(v, c, lo, **kw):
    lab, tab, ext, n = RR.regions(v, c, lo=lo, **kw)
    t = [torch.tensor(int(x)) for x in n]
    return regions.Result(torch.from_numpy(lab), torch.from_numpy(tab), torch.from_numpy(ext), t[0], t[1], t[2], t[3], lo, v.shape)


def test_table_functions_on_cpu_tensors():
    v = pic("##...",
            "##..#",
            "....#",
            ".#...")
    v[0, 0], v[4, 2] = -3.0, -0.5
    res = result(v, 0.0, (3, 2))
    assert regions.volume(res).tolist() == [4, 2, 1]
    assert regions.centroid(res).tolist() == [[3.0, 2.0], [6.5, 3.0], [3.5, 4.5]]
    assert regions.bbox(res).tolist() == [[[3, 4], [2, 3]], [[7, 7], [3, 4]], [[4, 4], [5, 5]]]
    val, pos = regions.peak(res, "min")
    assert val.tolist() == [-3.0, -1.0, -1.0] and pos.tolist() == [[3, 2], [7, 3], [4, 5]]
    val, pos = regions.peak(res, "max")
    assert val.tolist() == [-1.0, -0.5, -1.0] and pos.tolist() == [[4, 2], [7, 4], [4, 5]]
    assert regions.select(res, min_cells=2).tolist() == [0, 1]
    assert regions.select(res, touching_box=True).tolist() == [0, 1, 2] and regions.select(res, touching_box=False).tolist() == []
    w = np.ones((5, 5))
    w[2, 2] = w[0, 3] = -1.0
    r2 = result(w, 0.0, (1, 1))
    assert regions.select(r2, touching_box=False).tolist() == [0] and regions.select(r2, touching_box=True).tolist() == [1]
    assert regions.mask(res, 1).T.tolist() == (RR.regions(v, 0.0)[0] == 1).T.tolist() and regions.mask(res, 1).sum() == 2
    assert res.flat.tolist() == RR.regions(v, 0.0)[0].reshape(-1, order="F").tolist()
    with pytest.raises(ValueError):
        regions.peak(res, "mean")
    # follow: the blob with the peak at (3, 2) moved one cell in x and split off a new first region; the last one is gone
    v2 = pic(".##..",
             ".##.#",
             "#...#",
             ".....")
    now = result(v2, 0.0, (3, 2))
    assert RR.regions(v2, 0.0)[3][0] == 3
    assert regions.follow(res, now, "min").tolist() == [-1, 1, -1] and regions.follow(res, now, "max").tolist() == [0, 1, -1]
    short = result(v, 0.0, (3, 2))
    short.count = torch.tensor(2)                              # rows beyond the count mean nothing
    assert regions.follow(short, now, "max").tolist() == [0, 1, -1]
    with pytest.raises(ValueError, match="different boxes"):
        regions.follow(res, result(v2, 0.0, (1, 1)))
    big = regions.largest(res, 4)
    assert big.shape == (4, 15) and big[:, 1].tolist()[:3] == [4.0, 2.0, 1.0] and torch.isnan(big[3]).all() and big[0, 13] == -3.0
    short.tab[2, 1] = 99                                       # a stale row beyond the count must not be picked
    assert regions.largest(short, 2)[:, 1].tolist() == [4.0, 2.0] and torch.isnan(regions.largest(short, 3)[2]).all()


def test_value_is_one_descriptor_for_twopoint_and_regions():
    assert regions.Value is Value and Value("scalar").absval is False and Value("lambda2", absval=True).absval is True

    class Layout:
        slab = None

    class Flow:
        D, N, layout = 2, (10, 9), Layout()

    with pytest.raises(ValueError, match="absval"):
        TwoPoint(Flow(), Value("scalar", absval=True))
    with pytest.raises(ValueError, match="exactly one"):
        regions.Regions(Flow(), Value("scalar"))
    with pytest.raises(ValueError, match="exactly one"):
        regions.Regions(Flow(), Value("scalar"), below=0.0, above=1.0)
    with pytest.raises(ValueError, match="NaN"):
        regions.Regions(Flow(), Value("scalar"), below=float("nan"))
    with pytest.raises(ValueError, match="box"):
        regions.Regions(Flow(), Value("scalar"), below=0.0, box=((1, 1), (10, 4)))
    with pytest.raises(ValueError, match="periodic"):
        regions.Regions(Flow(), Value("scalar"), below=0.0, periodic=(2,))
