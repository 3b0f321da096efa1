"""The long-double reference of the k-table contract (tests/ktable_reference.py) against exact rational arithmetic, and the
numpy backend (helios_amd.ktable.numpy_bin, numpy_regrid) against that reference over the edge matrix the device is held to
in tests/test_gpu_ktable_edges.py.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import ktable_reference as kr
from helios_amd import ktable


def test_long_double_is_extended():
    kr.require_extended_precision()
    assert np.finfo(np.longdouble).eps <= 1.1e-19


# ---- the reference against exact arithmetic -----------------------------------------------------------------------------------
def exact_bin(lam, lo, hi, expo, yg):
    """the contract in Fractions: `expo` are the exponents of opacities 10^expo (None: a value that is floored); returns
    log10 k per abscissa and the steepest slope met"""
    lam = [Fraction(float(v)) for v in lam]
    lo, hi, n = Fraction(float(lo)), Fraction(float(hi)), len(lam)
    w = [(lam[min(i + 1, n - 1)] - lam[max(i - 1, 0)]) / 2 for i in range(n)]
    w[0] = (lam[0] - lo) + (lam[1] - lam[0]) / 2
    w[-1] = (hi - lam[-1]) + (lam[-1] - lam[-2]) / 2
    assert sum(w) == hi - lo
    pts = sorted((Fraction(-15 if e is None else e), w[i] / (hi - lo), i) for i, e in enumerate(expo))
    y, acc, prev = [], Fraction(0), Fraction(0)
    for _, wi, _ in pts:
        acc += (prev + wi) / 2
        prev = wi
        y.append(acc)
    out, steepest = [], Fraction(0)
    for v in yg:
        v = Fraction(float(v))
        if v <= y[0]:
            out.append(pts[0][0])
        elif v >= y[-1]:
            out.append(pts[-1][0])
        else:
            i = next(i for i in range(1, n) if y[i] >= v)
            slope = (pts[i][0] - pts[i - 1][0]) / (y[i] - y[i - 1])
            steepest = max(steepest, abs(slope))
            out.append(pts[i - 1][0] + slope * (v - y[i - 1]))
    return out, y, steepest


# lam, lower and upper interface: dyadic, the width a power of two, so that every y_i is a double
LAM4 = [1.0, 2.0, 3.5, 5.5]          # interior weights 1.25 and 1.75 (over the width)
EXACT = [
    # (lam, lo, hi, exponents); the end weights over the width, next to the interior 1.25 and 1.75:
    ("4 points, first lightest, last heaviest", LAM4, 0.75, 8.75, [3, 0, 2, 1]),                  # 0.75 | 4.25
    ("4 points, first in between, last heaviest", LAM4, 0.0, 8.0, [1, 1, 1, 0]),                  # 1.5 | 3.5
    ("4 points, first heaviest, last lightest", LAM4, -2.375, 5.625, [2, 0, 2, 2]),               # 3.875 | 1.125
    ("4 points, first heaviest, last in between", LAM4, -2.0, 6.0, [0, 0, 0, 0]),                 # 3.5 | 1.5
    ("4 points, ties around the heavier end", LAM4, 0.0, 8.0, [0, 5, 0, 0]),
    ("4 points, floored ones tie", LAM4, -2.0, 6.0, [None, 1, None, None]),
    ("3 points, the last heavier", [1.0, 2.0, 3.0], 0.5, 4.5, [1, 1, 0]),
    ("3 points, the first heavier, ties", [1.0, 2.0, 3.0], -0.5, 3.5, [4, 0, 4]),
    ("2 points", [1.0, 2.0], 0.5, 4.5, [2, 0]),
    ("2 points tied, the second lighter", [1.0, 2.0], -1.0, 3.0, [1, 1]),
]


@pytest.mark.parametrize("what,lam,lo,hi,expo", EXACT, ids=[c[0] for c in EXACT])
def test_reference_against_fractions(what, lam, lo, hi, expo):
    """bins of 2, 3 and 4 points whose opacities are powers of ten that fp32 holds exactly (log10 is exact) or values under
    the floor; abscissae below y_0, above y_{n-1}, on every y_i and between them.  Bound: each long-double operation adds
    at most eps relative; a dozen of them on values below 16 in magnitude, the y-dependent ones amplified by the steepest
    slope: (16 |slope|_max + 256) eps_ld."""
    k = np.array([1e-20 if e is None else 10.0 ** e for e in expo], np.float32)
    assert all(e is None or float(k[i]) == 10.0 ** e for i, e in enumerate(expo))
    n = len(lam)
    _, y, _ = exact_bin(lam, lo, hi, expo, [])
    assert all(Fraction(float(v)) == v for v in y), "choose dyadic points: y_i must be doubles"
    yg = [float(y[0]) / 2, float(y[0]), 1 - (1 - float(y[-1])) / 2, float(y[-1])] + [float(v) for v in y[1:-1]]
    yg += [float(a + b) / 2 for a, b in zip(y[:-1], y[1:])] + [float(a + 3 * b) / 4 for a, b in zip(y[:-1], y[1:])]
    want, _, steepest = exact_bin(lam, lo, hi, expo, yg)
    got = kr.reference_bin(np.array(lam), np.array([lo, hi]), 0, 0, n, k, np.array(yg))
    assert got.dtype == np.longdouble
    bound = (16 * float(steepest) + 256) * kr.EPS_LD
    dev = max(abs(float(g - np.longdouble(w.numerator) / np.longdouble(w.denominator))) for g, w in zip(got, want))
    print("%s: deviation %.3e, bound %.3e" % (what, dev, bound))
    assert dev <= bound


def test_reference_orders_ties_by_weight():
    """two tied points swap y when their weights swap: [k, w] = [1, light], [1, heavy], [10, .]"""
    lam, lo, hi = [1.0, 2.0, 3.0], 0.5, 4.5             # w = 1, 1, 2 over 4: the last is the heavier
    y, logk = kr.reference_curve(np.array(lam), np.array([lo, hi]), 0, 0, 3, np.array([10, 1, 10], np.float32))
    assert [float(v) for v in logk] == [0.0, 1.0, 1.0]
    assert [float(v) for v in y] == [0.125, 0.375, 0.75]        # the first point (w 1/4) before the last (w 1/2)


def test_reference_floor():
    k = np.array([np.nan, 0.0, -1.0, 1e-16, kr.F32_FLOOR_DOWN, kr.F32_FLOOR_UP, kr.F32_SUBNORMAL, kr.F32_MAX], np.float32)
    f = kr.reference_floored(k)
    assert [float(v) for v in f] == [1e-15] * 5 + [float(np.float32(1e-15)), 1e-15, float(kr.F32_MAX)]
    assert float(f[5]) > 1e-15
    one = kr.reference_bin(np.array([1.0, 2.0]), np.array([0.5, 1.5]), 0, 0, 1, k[7:], np.array([0.1, 0.9]))
    none = kr.reference_bin(np.array([1.0, 2.0]), np.array([0.1, 0.5]), 0, 0, 0, k, np.array([0.1, 0.9]))
    assert abs(float(one[0]) - np.log10(float(kr.F32_MAX))) < 1e-14 and abs(float(none[1]) + 15) < 1e-15


def test_synthetic_grids_hold_their_sizes():
    for name in kr.GRIDS:
        make, place, _ = kr.GRIDS[name]
        lam, start, end, inter = make(place)
        s, e = ktable.bin_ranges(lam, inter)
        np.testing.assert_array_equal(s[e > s], start[e > s])
        np.testing.assert_array_equal(e - s, end - start)
        if place == kr.ON_POINT:
            full = end > start
            np.testing.assert_array_equal(inter[:-1][full], lam[start[full]])
    assert kr.edge_case("nu0-0.3").lam[-1] == 10000.0 and kr.edge_case("nu0-0.3").end[-1] == len(kr.edge_case("nu0-0.3").lam)
    # the end weights differ from each other and from the interior ones
    c = kr.edge_case("main-0.3")
    w = kr.reference_weights(c.lam, c.inter, 8, int(c.start[8]), int(c.end[8]))
    assert w[0] != w[-1] and w[0] not in w[1:-1] and w[-1] not in w[1:-1]


# ---- the numpy backend against the reference ------------------------------------------------------------------------------------
@pytest.mark.parametrize("gauss", ["ng1", "ng20", "ng1100"])
@pytest.mark.parametrize("grid", kr.REFERENCE_CASES)
def test_numpy_backend_against_the_reference(grid, gauss):
    """every entry of every bin of the edge matrix: |log10 k - reference| <= max(1e-13, 8 eps64_ld) per slab, eps64_ld being
    the reference's own change when every y_i moves by one ulp of a double (neighbours in opposite directions).
    The backend sums y with compensation (ktable._compensated_cumsum): its plain running sum drifted by tens of ulps of y
    over the 70001-point bin and missed this bound by up to 5.7e-9 against 1.8e-10."""
    c = kr.edge_case(grid)
    yg = c.gauss[gauss]
    ref = c.reference(yg)
    eps_ld = np.abs(c.reference(yg, kr.perturbed) - ref).reshape(len(c.slabs), -1).max(axis=1).astype(np.float64)
    dev = c.eps64(ktable.numpy_bin, yg, ref)
    bound = np.maximum(1e-13, 8 * eps_ld)
    for t in range(len(c.slabs)):
        print("numpy %s %s slab %d: deviation %.3e, eps64_ld %.3e, bound %.3e" % (grid, gauss, t, dev[t], eps_ld[t], bound[t]))
    assert np.all(np.isfinite(dev)) and np.all(dev <= bound)


def test_reference_plan():
    left, clamped = kr.reference_plan([200.0, 450.0, 900.0], kr.REGRID_T)
    assert list(left) == [0, 0, 0, 1, 1, 2, 2] and list(clamped) == [1, 1, 0, 0, 0, 1, 1]
    left, clamped = kr.reference_plan([300.0], [100.0, 300.0, 500.0])
    assert list(left) == [0, 0, 0] and list(clamped) == [1, 1, 1]


@pytest.mark.parametrize("temps,press", kr.REGRID_SOURCES, ids=["1x1", "1x3", "3x1", "3x4"])
def test_numpy_regrid_against_the_reference(temps, press):
    """at the project's floor of 1e-13 in log10 k: the blend sums positive terms, and no source interval here is so short
    that the double log10 P costs more"""
    nc = 35
    k = kr.regrid_source(temps, press, nc)
    got = ktable.numpy_regrid(press, temps, k, kr.REGRID_T, kr.REGRID_P, 7, 5).reshape(len(kr.REGRID_T), len(kr.REGRID_P), nc)
    ref = kr.reference_regrid(temps, press, k, kr.REGRID_T, kr.REGRID_P, nc)
    dev = float(np.abs(np.log10(got.astype(np.longdouble)) - np.log10(ref)).max())
    print("numpy regrid %dx%d: deviation %.3e" % (len(temps), len(press), dev))
    assert dev <= 1e-13
    # the plans agree wherever the node is not clamped, and on what is clamped
    for old, new in ((temps, kr.REGRID_T), (press, kr.REGRID_P)):
        left, red = ktable.regrid_plan(old, new)
        rl, rc = kr.reference_plan(old, new)
        np.testing.assert_array_equal(red, rc)
        np.testing.assert_array_equal(left[red == 0], rl[rc == 0])


def test_compensated_sum_is_the_rounded_exact_sum():
    """1e5 positive terms over six decades: every partial sum within one ulp of the long-double sum, where the plain running
    sum is tens of ulps off"""
    a = 10.0 ** np.random.default_rng(8).uniform(-9, -3, 100000)
    exact = np.cumsum(a.astype(np.longdouble))
    ulp = np.spacing(exact.astype(np.float64))
    assert np.abs(ktable._compensated_cumsum(a) - exact).max() <= ulp.max() and \
        np.all(np.abs(ktable._compensated_cumsum(a) - exact) <= ulp)
    assert np.any(np.abs(np.cumsum(a) - exact) > 8 * ulp)
