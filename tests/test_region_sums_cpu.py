"""Region sums without a GPU: the yardstick tests/region_sums_ref.py against exact rational sums and against answers known in
closed form (pairs that cancel, ties of the one rounding, the clamp of the scale), regions.combine / finish / mean on CPU tensors
against the yardstick's own finish, and every refusal of wl_region_sums, which comes back WL_E_ARG through the C ABI before the
device is touched (pointers are fake: nothing is dereferenced but the column structs).

The bound the contract states, |sum - sum of the terms| <= cells * 2^(E - 126) + ulp(sum) / 2, is checked in exact arithmetic
(fractions.Fraction) over 200 seeded cases: normal noise times 2^k, k uniform in -100..40; every third case pairs every term with
its negative, every fifth is rounded to Float32 first."""
import ctypes as C
import math
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import region_sums_ref as SR  # noqa: E402

from waterlily_amd import _lib, regions  # noqa: E402
from waterlily_amd.twopoint import Value  # noqa: E402

E = _lib.WL_E_ARG
FAKE = C.c_void_p(0x1000)
R_METRIC, M_OMAG, M_LAMBDA2 = 16, 2, 4
F64 = np.float64


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F64)).view(np.uint64)


# --------------------------------------------------------------------------- the yardstick against exact sums

def case(seed):
    rng = np.random.default_rng(1000 + seed)
    n = (int(rng.integers(8, 40)), int(rng.integers(1, 4)))
    lab = rng.integers(-1, 4, size=n).astype(np.int32)
    v = rng.standard_normal(n) * np.exp2(rng.integers(-100, 41, size=n).astype(F64))
    if seed % 5 == 0:
        v = v.astype(np.float32).astype(F64)
    if seed % 3 == 0:                                          # every term beside its negative, inside the same region
        lab = np.concatenate([lab, lab], axis=0)
        v = np.concatenate([v, -v], axis=0)
    return lab, v


def test_the_restatement_stays_within_the_stated_bound_of_the_exact_sum():
    worst = 0.0
    for seed in range(200):
        lab, v = case(seed)
        acc, val, Es, over = SR.sums(lab, [(v, 1, None), (v, 2, 0)], lo=(3, 2), R=4)
        assert over.tolist() == [0, 0] and (acc[:, :, 4] == 0).all()
        I = np.indices(lab.shape)[0] + 3
        for c, terms in enumerate((v, (v * v) * I.astype(F64))):
            for r in range(4):
                t = terms[lab == r].tolist()
                exact = sum((Fraction(x) for x in t), Fraction(0))
                got = float(val[r, c])
                assert math.isfinite(got)
                bound = len(t) * Fraction(2) ** (int(Es[c]) - 126) + Fraction(math.ulp(got)) / 2
                err = abs(Fraction(got) - exact)
                assert err <= bound, (seed, c, r, float(err), float(bound))
                worst = max(worst, float(err / bound)) if bound else worst
                if seed % 3 == 0 and c == 0:
                    assert got == 0.0 and not math.copysign(1.0, got) < 0      # the pairs cancel exactly: +0
    assert 0.0 < worst <= 1.0


def test_pairs_that_cancel_leave_exactly_the_one_tiny_term():
    big = np.array([3.0e20, 1.7e18, 2.5, 7.0e-3] * 3)
    E0 = SR.scale_of(big.tolist())
    tiny = math.ldexp(5.0, E0 - 126)                           # five units: 2^95 times smaller than the largest term
    v = np.concatenate([big, [tiny], -big]).reshape(-1, 1)
    lab = np.zeros(v.shape, dtype=np.int32)
    acc, val, Es, over = SR.sums(lab, [(v, 1, None)], lo=(1, 1))
    assert Es[0] == E0 == 68 and val[0, 0] == tiny and acc[0, 0].tolist() == [5, 0, 0, 0, 0]
    assert float(np.sum(v)) != tiny                            # what a chain of double additions makes of it
    half = math.ldexp(1.5, E0 - 126)                           # one unit and a half: cut toward zero, in both signs
    for s in (1.0, -1.0):
        v[len(big), 0] = s * half
        assert SR.sums(lab, [(v, 1, None)], lo=(1, 1))[1][0, 0] == s * math.ldexp(1.0, E0 - 126)


def test_the_one_rounding_is_to_nearest_even_in_both_signs():
    for sign in (1, -1):
        for N, want in ((2 ** 60 + 2 ** 7, 2.0 ** 60), (2 ** 60 + 2 ** 8 + 2 ** 7, 2.0 ** 60 + 2.0 ** 9), (2 ** 60 + 2 ** 7 + 1, 2.0 ** 60 + 2.0 ** 8),
                        (2 ** 53 + 1, 2.0 ** 53), (2 ** 53 + 3, 2.0 ** 53 + 4.0), (2 ** 54 - 1, 2.0 ** 54), (2 ** 158 + 2 ** 105, 2.0 ** 158),
                        (2 ** 158 + 2 ** 105 + 1, 2.0 ** 158 + 2.0 ** 106), (1, 1.0), (2 ** 53 - 1, 2.0 ** 53 - 1.0)):
            for f in (SR.finish, regions._round_once):
                assert f(sign * N, 126) == sign * want, (N, sign, f)
                assert f(sign * N, 126 - 40) == sign * want * 2.0 ** -40
    rng = np.random.default_rng(7)
    for _ in range(2000):                                      # Python's int -> float is one rounding to nearest-even too
        N = int.from_bytes(rng.bytes(int(rng.integers(1, 20))), "little") * (1 if rng.random() < 0.5 else -1)
        assert bits(SR.finish(N, 126)) == bits(float(N)) and bits(regions._round_once(N, 126)) == bits(float(N))
    assert SR.finish(2 ** 150, 1023) == math.inf and regions._round_once(-2 ** 150, 1023) == -math.inf
    assert SR.finish((2 ** 54 - 1) << 73, 1023) == math.inf    # rounds up past the largest double
    assert SR.finish((2 ** 53 - 1) << 74, 1023) == sys.float_info.max
    assert SR.finish(1, SR.EMIN) == 2.0 ** -1020 and SR.finish(0, 5) == 0.0


def test_the_scale_is_clamped_at_emin():
    assert SR.EMIN == _lib.WL_RS_EMIN == -894
    assert SR.scale_of([]) == SR.scale_of([0.0, -0.0]) == SR.scale_of([math.nan, math.inf]) == -894
    assert SR.scale_of([2.0 ** -1000, 5e-324]) == -894 and SR.scale_of([2.0 ** -894]) == -894 and SR.scale_of([-2.0 ** -893]) == -893
    assert SR.scale_of([1.0]) == 0 and SR.scale_of([-1.999, 0.5]) == 0 and SR.scale_of([sys.float_info.max, math.inf]) == 1023
    v = np.array([[2.0 ** -1000, 2.0 ** -1019, -(2.0 ** -1021), 5e-324]]).T
    acc, val, Es, over = SR.sums(np.zeros(v.shape, dtype=np.int32), [(v, 1, None)], lo=(1, 1))
    assert Es[0] == -894 and acc[0, 0].tolist() == [2 ** 20 + 2, 0, 0, 0, 0] and val[0, 0] == 2.0 ** -1000 + 2.0 ** -1019
    assert SR.clamp(-5000) == -894 and SR.clamp(5000) == 1023


def test_non_finite_terms_are_counted_and_given_scales_count_overflows():
    v = np.array([[1.0, math.nan, 3.0, math.inf, -5.0, 0.25]]).T
    lab = np.array([[0, 0, 1, 2, 1, -1]], dtype=np.int32).T
    acc, val, Es, over = SR.sums(lab, [(v, 1, None)], lo=(1, 1))
    assert Es[0] == 2 and acc[:, 0, 4].tolist() == [1, 0, 1] and math.isnan(val[0, 0]) and val[1, 0] == -2.0 and math.isnan(val[2, 0])
    acc, val, Es, over = SR.sums(lab, [(v, 1, None)], lo=(1, 1), scale=[0])       # 3 and -5 are at or beyond 2^1
    assert over.tolist() == [2] and val[1, 0] == 0.0 and acc[0, 0].tolist() == [0, 0, 0, 2 ** 30, 1]
    acc, val, Es, over = SR.sums(lab, [(v, 1, None)], lo=(1, 1), cap=2)           # the third region has no row
    assert acc.shape == (2, 1, 5) and Es[0] == 2


# --------------------------------------------------------------------------- regions.combine, finish, mean on CPU tensors

def test_combine_and_finish_equal_the_restatement_bit_for_bit():
    for seed in (1, 2, 3, 5, 6, 10):
        lab, v = case(seed)
        whole = SR.sums(lab, [(v, 1, None), (v, 2, 1)], lo=(1, 1), R=4)
        cut = lab.shape[0] // 2
        halves = []
        for sl, lo in ((slice(0, cut), (1, 1)), (slice(cut, None), (1 + cut, 1))):
            acc, val, Es, over = SR.sums(lab[sl], [(v[sl], 1, None), (v[sl], 2, 1)], lo=lo, R=4, scale=whole[2])
            assert over.tolist() == [0, 0]
            halves.append(regions.Sums(torch.from_numpy(val), torch.from_numpy(acc), torch.from_numpy(Es), torch.from_numpy(over)))
            assert np.array_equal(bits(regions.finish(halves[-1].acc, halves[-1].scale).numpy()), bits(val))
        got = regions.combine(halves[0], halves[1])
        assert got.dtype == torch.float64 and np.array_equal(bits(got.numpy()), bits(whole[1])), seed
        assert np.array_equal((halves[0].acc + halves[1].acc).numpy(), whole[0])
    other = regions.Sums(halves[1].value, halves[1].acc, halves[1].scale + 1, halves[1].over)
    with pytest.raises(ValueError, match="same scale"):
        regions.combine(halves[0], other)
    nan = halves[0].acc.clone()
    nan[1, 0, 4] = 2
    assert torch.isnan(regions.finish(nan, halves[0].scale)[1, 0])


def test_mean_and_the_refusals_of_the_python_layer():
    sm = regions.Sums(torch.tensor([[6.0, -3.0], [1.0, 0.0]], dtype=torch.float64), None, None, None)
    tab = torch.zeros((2, 13), dtype=torch.int64)
    tab[:, 1] = torch.tensor([3, 4])
    res = regions.Result(None, tab, None, torch.tensor(2), None, None, None, (1, 1), (4, 4))
    assert regions.mean(sm, res).tolist() == [[2.0, -1.0], [0.25, 0.0]]
    w = regions.Weight(Value("curl", i=2), power=2, moment=1)
    assert (w.power, w.moment, w.field) == (2, 1, None) and regions._weight(w) is w and regions._weight(Value("ke")).power == 1
    with pytest.raises(ValueError, match="power"):
        regions.Weight(Value("scalar"), power=3)
    with pytest.raises(ValueError, match="moment"):
        regions.Weight(Value("scalar"), moment=3)

    # the arithmetic of weighted_centroid: sum(w J) / sum(w) - 0.5, NaN where sum(w) == 0 (+0 and -0), signs kept
    v = torch.tensor([[4.0, 10.0, 18.0], [0.0, 3.0, 0.0], [-0.0, 0.0, 1.0], [-2.0, -5.0, 1.0], [0.125, 0.125 * 7, 0.125 * 9]], dtype=torch.float64)
    c = regions.centroid_of(v)
    assert c.shape == (5, 2) and c[0].tolist() == [2.0, 4.0] and c[3].tolist() == [2.0, -1.0] and c[4].tolist() == [6.5, 8.5]
    assert torch.isnan(c[1]).all() and torch.isnan(c[2]).all()
    tab5 = torch.zeros((1, 13), dtype=torch.int64)
    tab5[0, 1:4] = torch.tensor([8, 56, 72])                   # a uniform weight gives the table's centroid, bit for bit
    uni = regions.Result(None, tab5, None, torch.tensor(1), None, None, None, (1, 1), (4, 4))
    assert torch.equal(regions.centroid_of(0.125 * tab5[:, 1:4].to(torch.float64)), regions.centroid(uni))
    with pytest.raises(ValueError, match="without a moment"):
        regions.weighted_centroid(None, res, w)

    class Rg:
        capacity, lo, n = 4, (1, 1), (4, 4)

    with pytest.raises(ValueError, match="at least one"):
        regions.sums(Rg(), res, [])
    with pytest.raises(ValueError, match="another box"):
        regions.sums(Rg(), regions.Result(None, tab, None, None, None, None, None, (2, 1), (4, 4)), [w])
    Rg.capacity = 0
    with pytest.raises(ValueError, match="capacity"):
        regions.sums(Rg(), res, [w])


# --------------------------------------------------------------------------- the C ABI

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


def cols(*specs):
    """specs: dicts with kind, ipar, f, absval, power, moment"""
    arr = (_lib.RsCol * max(1, len(specs)))()
    for c, sp in enumerate(specs):
        arr[c].v.f, arr[c].v.kind, arr[c].v.ipar = sp.get("f", 0x1000), sp.get("kind", 0), sp.get("ipar", 0)
        arr[c].power, arr[c].moment = sp.get("power", 1), sp.get("moment", -1)
    return arr


def call(g=None, t=0, lo=None, hi=None, label=FAKE, n=FAKE, cap=4, ncol=None, cs=None, mode=0, scale=FAKE, acc=FAKE, val=FAKE, over=FAKE,
         null_g=False, null_cols=False):
    g = grid() if g is None else g
    cs = cols({}) if cs is None else cs
    ncol = len(cs) if ncol is None else ncol
    return _lib.lib().wl_region_sums(t, None if null_g else C.byref(g), lo, hi, label, n, cap, ncol, None if null_cols else C.cast(cs, C.c_void_p),
                                     mode, scale, acc, val, over)


def refused(word, **kw):
    rc = call(**kw)
    err = _lib.lib().wl_last_error()
    assert rc == E and b"wl_region_sums" in err and word in err, (kw, rc, err)


def test_every_refusal_comes_back_before_the_device_is_touched():
    refused(b"null", null_g=True)
    for name in ("label", "n", "scale", "acc", "val", "over"):
        refused(b"null", **{name: None})
    refused(b"null", null_cols=True)
    refused(b"ncol", ncol=0)
    refused(b"ncol", cs=cols(*[{}] * 9))
    refused(b"ncol", ncol=-1)
    refused(b"capacity", cap=0)
    refused(b"capacity", cap=-3)
    refused(b"power", cs=cols({"power": 0}))
    refused(b"power", cs=cols({}, {"power": 3}))
    refused(b"moment", cs=cols({"moment": -2}))
    refused(b"moment", cs=cols({"moment": 3}))
    refused(b"moment", cs=cols({"moment": 2}), g=grid((10, 9)))                  # an axis a 2-D grid does not have
    refused(b"null field", cs=cols({}, {"f": None}))
    refused(b"kind", cs=cols({"kind": 3}))                                      # WL_R_FACE
    refused(b"kind", cs=cols({"kind": 9}))
    refused(b"kind", cs=cols({"kind": 1, "ipar": 3}))
    refused(b"metric", cs=cols({"kind": R_METRIC + 7}))
    refused(b"metric", cs=cols({"kind": R_METRIC + M_LAMBDA2}), g=grid((10, 9)))
    refused(b"inside()", cs=cols({}, {"kind": R_METRIC + M_OMAG}), lo=i3(0, 1, 1), hi=i3(4, 4, 4))
    refused(b"only one", lo=i3(1, 1, 1))
    refused(b"only one", hi=i3(4, 4, 4))
    refused(b"box", lo=i3(1, 1, 1), hi=i3(10, 4, 4))
    refused(b"box", lo=i3(-1, 1, 1), hi=i3(4, 4, 4))
    refused(b"box", lo=i3(4, 1, 1), hi=i3(4, 4, 4))                             # empty
    refused(b"2^31", g=grid((2050, 1026, 1026)))
    refused(b"aligned", label=C.c_void_p(0x1002))
    refused(b"aligned", scale=C.c_void_p(0x1002))
    for name in ("n", "acc", "val", "over"):
        refused(b"aligned", **{name: C.c_void_p(0x1004)})
    refused(b"dtype", t=7)
    refused(b"scale_mode", mode=2)
    refused(b"scale_mode", mode=-1)
    slab = grid()
    slab.nzg, slab.kz0, slab.own_lo, slab.own_hi = 14, 0, 1, 6                 # a z-slab of a decomposed array
    refused(b"decomposed", g=slab)


def test_what_passes_every_check_reaches_the_device():
    """the mirror of the refusals: the same calls with nothing wrong pass validation, which shows as the device's own refusal (a
    HIP error number) where there is no device -- with one, the call would run on the fake pointers"""
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    eight = cols(*[{"kind": 1, "ipar": c % 3, "power": 1 + c % 2, "moment": c % 4 - 1} for c in range(8)])
    for kw in (dict(), dict(mode=1), dict(cs=eight), dict(cap=1 << 40), dict(lo=i3(0, 0, 0), hi=i3(9, 8, 7)),
               dict(cs=cols({"kind": R_METRIC + M_LAMBDA2}, {"f": 0x2000}), lo=i3(1, 1, 1), hi=i3(9, 8, 7)),
               dict(g=grid((10, 9)), cs=cols({"kind": 2, "ipar": 1, "moment": 1}))):
        rc = call(**kw)
        assert rc != 0 and rc != E, (kw, rc, _lib.lib().wl_last_error())


def test_the_binding_and_the_header_agree():
    assert C.sizeof(_lib.RsCol) == C.sizeof(_lib.RgValue) + 8 and _lib.WL_RS_MAX_COLS == 8 and (_lib.WL_RS_FIND, _lib.WL_RS_GIVEN) == (0, 1)
    src = open(os.path.join(os.path.dirname(_lib.__file__), "..", "include", "wlhip.h")).read()
    assert "WL_RS_MAX_COLS = 8, WL_RS_EMIN = -894" in src and "WL_RS_FIND = 0, WL_RS_GIVEN = 1" in src
    assert _lib.lib().wl_abi_version() == 6
