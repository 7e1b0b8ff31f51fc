"""What the read-outs share (waterlily_amd/_readout.py, _series.host_parts) without a GPU: the box rule gives one verdict through
the shared function and through every constructor, before anything is allocated; the one Value fills the four ctypes structs
and the flat arguments alike; the structs have the header's layout; a gather() on one rank is a host copy."""
import ctypes as C

import numpy as np
import pytest
import torch

import waterlily_amd
from waterlily_amd import _lib, _series, downsample, hist, iso, regions, render, twopoint
from waterlily_amd import _readout as R
from waterlily_amd import sim as S


class Reached(Exception):
    """a constructor is through with its validation: it asks for the grid, the first thing the device work needs"""


class Layout:
    slab = None

    def grid(self):
        raise Reached


class Flow:
    """no device, no arrays: whatever is allocated or launched fails with something that is no ValueError and no Reached"""

    def __init__(self, N):
        self.D, self.N, self.layout = len(N), N, Layout()


N3, N2 = (10, 11, 14), (10, 9)
GOOD = {N3: [None, ((2, 3, 4), (7, 8, 9)), ((0, 0, 0), (9, 10, 13))],
        N2: [None, ((2, 3), (7, 8)), ((0, 0), (9, 8))]}
BAD = {N3: [((1, 1, 1), (10, 10, 13)),                                   # hi = n
            ((1, 1, 1), (9, 11, 13)),
            ((-1, 1, 1), (5, 5, 5)),                                     # a negative lo
            ((1, 4, 1), (5, 4, 5)),                                      # lo == hi
            ((1, 6, 1), (5, 4, 5)),                                      # lo > hi
            ((1, 1), (5, 5)), ((1, 1, 1), (5, 5)), ((1, 1, 1, 1), (5, 5, 5, 5)),         # a wrong number of entries
            ((1, 1, 1),), ((1, 1, 1), None), (None, (5, 5, 5))],        # only one side usable
       N2: [((1, 1), (10, 8)), ((1, 1), (9, 9)), ((1, -1), (5, 5)), ((4, 1), (4, 5)), ((6, 1), (4, 5)),
            ((1,), (5,)), ((1, 1), (5, 5, 5)), ((1, 1, 1), (5, 5, 5)), ((1, 1),), ((1, 1), None), (None, (5, 5))]}

MAKERS = [lambda f, box: hist.Histogram(f, hist.Axis("scalar", bins=8, range=(0, 1)), box=box),
          lambda f, box: twopoint.TwoPoint(f, R.Value("scalar"), box=box),
          lambda f, box: regions.Regions(f, R.Value("scalar"), below=0.0, box=box)]


@pytest.mark.parametrize("N", [N3, N2])
def test_the_box_rule_gives_one_verdict_everywhere_before_anything_is_allocated(N):
    for box in GOOD[N]:
        (lo, hi), given = R.box_of("X", N, box)
        assert given == (box is not None) and (lo, hi) == (R.inside(N) if box is None else box)
        assert all(isinstance(x, int) for x in lo + hi)
        assert downsample.trim(N, 1, box) == (lo, hi)
        for make in MAKERS:
            with pytest.raises(Reached):
                make(Flow(N), box)
    for box in BAD[N]:
        with pytest.raises(ValueError, match=f"X: a box is .lo, hi. with {len(N)} entries each, 0 <= lo < hi <= n - 1"):
            R.box_of("X", N, box)
        with pytest.raises(ValueError, match="Downsampler"):
            downsample.trim(N, 1, box)
        for make, who in zip(MAKERS, ("Histogram", "TwoPoint", "Regions")):
            with pytest.raises(ValueError, match=f"{who}: a box is"):
                make(Flow(N), box)
    assert R.inside(N3) == ((1, 1, 1), (9, 10, 13))


def test_box_args_and_each_class_keeps_its_own_checks():
    assert R.box_args(None) == (None, None)
    lo, hi = R.box_args(((1, 2), (7, 8)))
    assert list(lo) == [1, 2, 0] and list(hi) == [7, 8, 0] and isinstance(lo, C.c_int32 * 3)
    assert downsample.trim(N3, 4, ((1, 1, 1), (9, 10, 13))) == ((1, 1, 1), (9, 9, 13))       # trimmed, then the rule
    assert downsample.trim((10,), 4, ((1,), (10,))) == ((1,), (9,))                          # (hi = n is trimmed away first, as ever)
    with pytest.raises(ValueError, match="after trimming to multiples of 8"):
        downsample.trim(N2, 8, ((1, 1), (8, 8)))
    with pytest.raises(ValueError, match="inside"):                                          # Regions: a metric's box lies in inside()
        regions.Regions(Flow(N3), R.Value("lambda2"), below=0.0, box=((0, 1, 1), (5, 5, 5)))
    with pytest.raises(ValueError, match="nsep"):                                            # TwoPoint: nsep within the box's extent
        twopoint.TwoPoint(Flow(N3), R.Value("scalar"), axis=1, nsep=6, box=((1, 1, 1), (5, 6, 5)))
    with pytest.raises(ValueError, match=f"longer than {twopoint.MAX_LINE}"):
        twopoint.TwoPoint(Flow((2000, 8)), R.Value("scalar"))


def test_one_value_descriptor_fills_every_struct_and_the_flat_arguments():
    assert waterlily_amd.Value is twopoint.Value is regions.Value is R.Value and issubclass(hist.Axis, R.Value)
    kind = R.R_METRIC + S._METRIC["omega_theta"]
    v = R.Value("omega_theta", i=2, par=(1, 2), par2=(3, 4, 5), absval=True)
    assert (v.kind, v.i, v.par, v.par2, v.absval) == (kind, 2, (1, 2), (3, 4, 5), True)
    plain = R.Value("scalar")
    for s in (_lib.HistAxis(), _lib.TpValue(), _lib.RgValue(), _lib.RsCol().v):
        s.f = 0x1000
        assert v.fill(s) is s
        assert (s.f, s.kind, s.ipar, list(s.par), list(s.par2)) == (0x1000, kind, 2, [1.0, 2.0, 0.0], [3.0, 4.0, 5.0])
        assert not hasattr(s, "absval") or s.absval == 1
        assert hasattr(s, "absval") != isinstance(s, _lib.TpValue)
        plain.fill(s)                                                                        # an absent par: zeros, over what was there
        assert (s.f, s.kind, s.ipar, list(s.par), list(s.par2), getattr(s, "absval", 0)) == (0x1000, 0, 0, [0.0] * 3, [0.0] * 3, 0)
    axis = _lib.HistAxis()
    axis.nbins, axis.hi = 7, 2.5
    v.fill(axis)
    assert (axis.nbins, axis.lo, axis.hi, axis.range_dev, axis.edges_dev) == (7, 0.0, 2.5, None, None)      # only the leading fields
    k, ipar, par, par2 = v.flat()
    assert (k, ipar) == (kind, 2) and isinstance(par, C.c_double * 3) and isinstance(par2, C.c_double * 3)
    assert list(par) == [1.0, 2.0, 0.0] and list(par2) == [3.0, 4.0, 5.0]
    assert plain.flat() == (R.R_SCALAR, 0, None, None)                                       # an absent par: NULL


def test_axis_is_a_value_and_the_names_stay_where_they_were():
    a = hist.Axis("curl", i=1, par=(0, 0, 1), bins=16, range=(-1, 1), abs=True)
    assert a.absval is True and a.abs is True and hist.Axis("scalar").absval is False
    assert (a.kind, a.i, a.par, a.par2, a.bins, a.range, a.edges, a.auto) == (R.R_METRIC + 1, 1, (0, 0, 1), None, 16, (-1.0, 1.0), None, False)
    with pytest.raises(ValueError, match="range or edges"):
        hist.Axis(range=(0, 1), edges=(0, 1))
    for name in ("face", "nothing"):
        with pytest.raises(KeyError):
            R.Value(name)
    assert R.Value("center").kind == R.Value("centre").kind == R.Value(2).kind == R.R_CENTRE
    assert (render.R_SCALAR, render.R_UCOMP, render.R_CENTRE, downsample.R_FACE, render.R_METRIC) == (0, 1, 2, 3, 16)
    assert downsample._KIND["face"] == R.R_FACE and "face" not in R.KIND and downsample._MODE["sample"] == 5 and "sample" not in R.MODE
    assert {k: v - R.R_METRIC for k, v in R.KIND.items() if v >= R.R_METRIC} == S._METRIC
    assert R.code(R.MODE, "absmax") == 2 and R.code(R.MODE, 4) == 4
    assert not hasattr(downsample, "_DevBuf") and callable(render.drain_one)


def test_the_structs_have_the_layout_of_the_header():
    def layout(s):
        return C.sizeof(s), {name: getattr(s, name).offset for name, _ in s._fields_}

    value = {"f": 0, "kind": 8, "ipar": 12, "par": 16, "par2": 40}
    assert layout(_lib.TpValue) == (64, value)
    assert layout(_lib.RgValue) == (72, dict(value, absval=64))
    assert layout(_lib.HistAxis) == (104, dict(value, absval=64, nbins=68, lo=72, hi=80, range_dev=88, edges_dev=96))
    assert layout(_lib.RsCol) == (80, {"v": 0, "power": 72, "moment": 76})


class OneRank:
    size, rank = 1, 0


@pytest.mark.parametrize("slab", [None, OneRank()])
def test_gather_on_one_rank_is_a_host_copy(slab):
    t = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    parts, on_rank0 = _series.host_parts(t, slab)
    assert on_rank0 is True and len(parts) == 1 and isinstance(parts[0], np.ndarray) and np.array_equal(parts[0], t.numpy())
    parts[0][0, 0, 0] = 99.0
    assert t[0, 0, 0] == 0.0                                                                 # a copy, not a view
    a = np.arange(6.0).reshape(2, 3)
    assert _series.host_parts(a, slab)[0][0] is a                                            # a host array passes as it is
    img, cnt = t[0], torch.arange(12, dtype=torch.int64).reshape(3, 4)
    for axis, mode in ((0, "max"), (1, "sum"), (2, "sum"), (2, "absmax"), (2, "slice")):
        assert np.array_equal(render.gather(img, axis, mode, slab), img.numpy())
    assert np.array_equal(downsample.gather(t, slab), t.numpy()) and np.array_equal(downsample.gather(img, slab), img.numpy())
    got = hist.gather(cnt, slab)
    assert got.dtype == np.int64 and np.array_equal(got, cnt.numpy())
    assert np.array_equal(twopoint.gather(img, slab), img.numpy())
    tri, val = torch.rand(5, 3, 3, dtype=torch.float64), torch.rand(5, 3, dtype=torch.float64)
    gt, gv = iso.gather(tri, val, slab)
    assert np.array_equal(gt, tri.numpy()) and np.array_equal(gv, val.numpy())
    gt, gv = iso.gather(tri[:0], None, slab)
    assert gt.shape == (0, 3, 3) and gv is None
