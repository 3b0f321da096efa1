"""The restatement of tests/lines_reference.py against what is known without it: K against mpmath (tests/golden/lines), S at the
reference temperature, the integral of a line, the Doppler and the Lorentz limit, and the coefficient literals on both sides."""
import importlib.util
import os
import re

import numpy as np
import pytest

import lines_cases as lc
import lines_reference as lr
from helios_amd import lines, lines_data, phys_const

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGION_BOUND = (lc.GOLDEN_BOUND, lc.GOLDEN_BOUND, lc.GOLDEN_BOUND_OUTER, lc.GOLDEN_BOUND_OUTER)
REGION_NAME = ("Weideman", "eight levels", "four levels", "two levels")


def test_the_restated_constants_are_the_modules():
    assert (lr.C, lr.K_B, lr.H, lr.N_A) == (phys_const.C, phys_const.K_B, phys_const.H, phys_const.N_A)
    assert (lr.T_REF, lr.ATM, lr.Y_MIN) == (lines.T_REF, lines.ATM, lines.Y_MIN)
    assert lr.R2 == (lines.R2_WEIDEMAN, lines.R2_EIGHT, lines.R2_FOUR) and lr.LEVELS == lines.LEVELS
    assert lr.constants(np.float64) == (lines.LN2, lines.INV_SQRT_PI)
    assert lines.LN2 == float(np.log(2.0)) and abs(lines.INV_SQRT_PI - 1.0 / np.sqrt(np.pi)) <= 1.2e-16
    assert lr.FIELDS == lines.FIELDS and dict((n, (a, b)) for n, a, b in lr.COLUMNS) == lines._COLUMNS
    assert lr.WEIDEMAN_N == lines_data.WEIDEMAN_N == len(lines_data.WEIDEMAN_A)
    assert lines_data.WEIDEMAN_L == float(np.sqrt(40.0 / np.sqrt(2.0)))


@pytest.mark.parametrize("reg", [0, 1, 2, 3])
def test_k_against_mpmath(reg):
    """both restatements within 1e-6 relative of the goldens in every region, within 1e-9 in the two outer ones.

    The goldens hold both sides of |z| = 6 as well as of the scheme's boundaries 6.5, 15 and 100.  With the first boundary at 6 the
    region of eight levels missed its bound at x = 6.000000000000001, y = 1e-8 (1.417e-6: the continued fraction has no term
    exp(-x^2), and exp(-36) = 2.3e-16 is that share of K = 1.6e-10 there), so the boundary stands at 6.5, where the term is 3.4e-9.
    Measured: Weideman's region 1.2e-7, eight levels 3.4e-9, four levels 7.8e-11, two levels 5.3e-12."""
    g = lc.goldens()
    m = lr.region(g["x"], g["y"]) == reg
    assert m.sum() >= 20
    x, y, k = g["x"][m], g["y"][m], g["k"][m].astype(np.longdouble)
    worst = []
    for T in (np.longdouble, np.float64):
        dev = np.abs(lr.voigt_k(x, y, T).astype(np.longdouble) / k - 1)
        j = int(np.argmax(dev))
        print("%s in %s: worst deviation from mpmath %.3e at x = %.17g, y = %g; bound %g"
              % (REGION_NAME[reg], T.__name__, float(dev[j]), x[j], y[j], REGION_BOUND[reg]))
        worst.append(float(dev[j]))
    assert max(worst) <= REGION_BOUND[reg]


def test_the_goldens_hold_what_the_grid_promises():
    g = lc.goldens()
    assert sorted(g) == ["k", "x", "y"] and len(g["x"]) == len(g["y"]) == len(g["k"]) >= 400
    assert sorted(set(g["y"].tolist())) == [1e-8, 1e-6, 1e-3, 1.0, 1e2, 1e4] and (g["x"] == 0).sum() == 6
    r2 = g["x"] ** 2 + g["y"] ** 2
    for r in (6.0, 6.5, 15.0, 100.0):
        for y in (1e-8, 1e-6, 1e-3, 1.0):
            row = g["y"] == y
            inside = g["x"][row & (r2 <= r * r)].max()
            assert np.nextafter(inside, np.inf) in g["x"][row & (r2 > r * r)]       # one ulp apart across the boundary


def test_module_k_is_the_plain_restatement_to_the_bit():
    g = lc.goldens()
    assert np.array_equal(lines.voigt_k(g["x"], g["y"]), lr.voigt_k(g["x"], g["y"], np.float64))
    assert np.array_equal(lines.region(g["x"], g["y"]), lr.region(g["x"], g["y"]))


def test_s_at_the_reference_temperature_is_s_ref_to_the_bit():
    line = lc.synthetic_lines(200, 1.0, 30000.0, seed=3)
    q = lc.q_table()
    q_ref = lines.partition_value(q, 296.0)
    assert q_ref == lines.partition_value(q, lr.T_REF)
    assert np.array_equal(lines.line_strength(line, 296.0, q_ref, q_ref), line["s_ref"])
    for j in range(200):
        one = dict((k, line[k][j]) for k in lr.FIELDS)
        assert lr.strength(one, 296.0, q_ref, q_ref, np.float64) == line["s_ref"][j]
        assert lr.strength(one, 296.0, q_ref, q_ref, np.longdouble) == np.longdouble(line["s_ref"][j])


def test_the_parsers_numbers():
    line = lc.synthetic_lines(5, 100.0, 200.0, seed=2)
    for j in range(5):
        rec = lc.par_record(line, j)
        v, iso = lr.parse_record(rec)
        assert iso == "1" and len(rec) == 160
        assert v["nu0"] == float("%.6f" % line["nu0"][j]) and v["s_ref"] == float("%.3e" % line["s_ref"][j])
        assert v["n_air"] == float("%.2f" % line["n_air"][j]) and v["delta_air"] == float("%.6f" % line["delta_air"][j])


def test_the_integral_of_one_line():
    """sum kappa_i dnu over the grid equals S N_A / M less the Lorentz wings beyond the cut-off, S (2 / pi) atan(gamma / C).

    The tolerance, relative to S N_A / M, is derived and not fitted.  The line stands on a grid point and C is a whole number
    of steps h, so the sum is the trapezoid rule over [-C, C] plus h f(C) (both end points in full, not halved), f = the profile:
      end points      h f(C) <= h gamma / (pi C^2)
      trapezoid rule  (h^2 / 12) |f'(C) - f'(-C)| = (h^2 / 12) 4 gamma / (pi C^3)   (Euler-Maclaurin's first term; the next, in h^4
                      f''', is smaller by (h / C)^2), and inside the interval 2 exp(-2 pi gamma / h) for a function analytic in the
                      strip of half width gamma
      the wings       the Voigt wing exceeds the Lorentzian by the factor 1 + 3 / (2 x^2) + ..., x = a C: at most
                      2 * 3 / (2 (a C)^2) of the wing's share (2 / pi) gamma / C
      the scheme      K's error against mpmath, 1e-6 of any part (lines_cases.GOLDEN_BOUND), over the whole line: 1e-6
      the sum         8 eps per addition in fp64, n additions: 8 n 2.2e-16"""
    nu0, h, C, temp, press = 1000.0, 0.005, 25.0, 300.0, 1013250.0
    n = int(round(2 * (C + 5.0) / h)) + 1
    nu_first = nu0 - (C + 5.0)
    line = lc.one_line(nu0)
    q = lc.q_table()
    q_t, q_ref = lines.partition_value(q, temp), lines.partition_value(q, 296.0)
    kappa = lr.plain_fp64(line, temp, press, q_t, q_ref, lc.M_H2O, 0.0, C, nu_first, h, n)
    p = lr.params(line, temp, press, q_t, q_ref, lc.M_H2O, 0.0, np.float64)[:, 0]
    a, gamma = p[2], p[3] / p[2]
    assert p[0] == nu0 and (nu_first + np.arange(n) * h == nu0).sum() == 1
    assert int(np.count_nonzero(kappa)) == int(round(2 * C / h)) + 1
    total = float(lr.strength(dict((k, line[k][0]) for k in lr.FIELDS), temp, q_t, q_ref, np.float64)) * lr.N_A / lc.M_H2O
    expected = total * (1.0 - 2.0 / np.pi * np.arctan(gamma / C))
    tol = (h * gamma / (np.pi * C * C) + h * h / 12.0 * 4.0 * gamma / (np.pi * C ** 3) + 2.0 * np.exp(-2.0 * np.pi * gamma / h)
           + 3.0 / (a * C) ** 2 * (2.0 / np.pi) * gamma / C + lc.GOLDEN_BOUND + 8.0 * n * 2.2e-16)
    got = float(np.sum(kappa) * h)
    print("integral %.12e, expected %.12e: relative difference %.3e, tolerance %.3e" % (got, expected, abs(got / expected - 1), tol))
    assert tol < 2e-6 and abs(got - expected) <= tol * total


def test_the_doppler_limit():
    """y at the clamp, the core |x| <= 2: K(x, y) = exp(-x^2) + (2 y / sqrt pi) (2 x F(x) - 1) + O(y^2) with Dawson's F and
    |2 x F(x) - 1| <= 1, so the Gaussian differs from K by at most 1.13e-8 / exp(-4) = 6.2e-7 relative there: inside the
    region's golden bound of 1e-6, to which the restatement is held"""
    x = np.linspace(-2.0, 2.0, 81)
    for T in (np.longdouble, np.float64):
        k = lr.voigt_k(x, np.full(81, lr.Y_MIN), T).astype(np.longdouble)
        dev = np.abs(k / np.exp(-x.astype(np.longdouble) ** 2) - 1)
        print("Doppler limit in %s: %.3e" % (T.__name__, float(dev.max())))
        assert dev.max() <= lc.GOLDEN_BOUND


def test_the_lorentz_limit():
    """y = 1e3: K(x, y) = Re[(i / sqrt pi) / z (1 + 1 / (2 z^2) + ...)], whose first term is the Lorentzian y / (sqrt pi (x^2 + y^2));
    the second is at most 1 / (2 |z|^2) = 5e-7 of it at y = 1e3.  The comparison can hold to the bound the scheme has everywhere,
    1e-6, and not to the 1e-9 of the outer region against mpmath: that much the two functions differ"""
    x = np.concatenate([[0.0], 10.0 ** np.linspace(-2.0, 5.0, 71)])
    y = np.full(len(x), 1e3)
    for T in (np.longdouble, np.float64):
        k = lr.voigt_k(x, y, T).astype(np.longdouble)
        lorentz = y / (np.sqrt(np.longdouble(np.pi)) * (x.astype(np.longdouble) ** 2 + y ** 2))
        dev = np.abs(k / lorentz - 1)
        print("Lorentz limit in %s: %.3e" % (T.__name__, float(dev.max())))
        assert dev.max() <= lc.GOLDEN_BOUND


def test_the_coefficient_literals_are_the_same_numbers_on_both_sides():
    text = open(os.path.join(ROOT, "helios_amd", "csrc", "lines_weideman.h")).read()
    text = re.sub(r"//[^\n]*", "", text)
    assert int(re.search(r"#define LINES_WEIDEMAN_N (\d+)", text).group(1)) == lines_data.WEIDEMAN_N == 40
    device_l = re.search(r"#define LINES_WEIDEMAN_L (\S+)", text).group(1)
    body = text.split("#define LINES_WEIDEMAN_A", 1)[1].replace("\\", " ")
    device_a = [w.strip() for w in body.split(",")]
    assert len(device_a) == 40
    host = open(os.path.join(ROOT, "helios_amd", "lines_data.py")).read()
    host_a = [w.strip() for w in host.split("WEIDEMAN_A = (", 1)[1].split(")", 1)[0].split(",") if w.strip()]
    assert len(host_a) == 40
    for n, (d, h, v) in enumerate(zip(device_a, host_a, lines_data.WEIDEMAN_A)):
        assert float(d) == float(h) == v, (n, d, h)
        assert len(re.sub(r"e.*", "", d).replace("-", "").replace(".", "").lstrip("0")) == 17, d       # 17 significant digits
    assert float(device_l) == lines_data.WEIDEMAN_L


def test_the_literals_are_what_the_generator_computes():
    spec = importlib.util.spec_from_file_location("make_lines_data", os.path.join(ROOT, "tools", "make_lines_data.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    L, a = gen.coefficients()
    assert float(L) == lines_data.WEIDEMAN_L and [float(v) for v in a] == list(lines_data.WEIDEMAN_A)
