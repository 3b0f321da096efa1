"""The restatement of the ExoMol contract (tests/exomol_reference.py) against what does not depend on it: the worked value of the
issue, the integral of one isolated line, and lines.py's restatement on the same list converted to HITRAN-style fields."""
import importlib.util
import os

import numpy as np

import exomol_cases as ec
import exomol_reference as er
import lines_reference as lr
from helios_amd import exomol, phys_const as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_constants_are_the_modules():
    assert (lr.C, lr.K_B, lr.H, lr.N_A) == (pc.C, pc.K_B, pc.H, pc.N_A)
    assert er.BAR == exomol.BAR == 1.0e6 and exomol.DEFAULT_BROADENING == (0.07, 0.5)
    assert float(er.pi(np.float64)) == np.pi and abs(float(er.pi(np.longdouble)) - np.pi) < 1e-15


def test_the_worked_value():
    """g = 3, A = 1, E_up = 1100, E_low = 100, T = 1000, Q = 1000^1.5 give S = 8.31717802424e-23, to 1e-12 relative, in both
    restatements and in the module"""
    want = 8.31717802424e-23
    for T in (np.longdouble, np.float64):
        s = er.strength(3.0, 1.0, 100.0, 1100.0 - 100.0, 1000.0, 1000.0 ** 1.5, T)
        print("S in %s: %.15e" % (T.__name__, float(s)))
        assert abs(float(s) / want - 1) <= 1e-12
    states = {"E": np.array([100.0, 1100.0]), "g": np.array([1.0, 3.0]), "J": np.array([0.0, 1.0]), "jidx": np.array([0, 2], np.int32)}
    trans, skipped = exomol.sort_transitions({"up": [1], "low": [0], "A": [1.0]}, states)
    assert skipped == 0 and trans["nu0"][0] == 1000.0
    assert abs(exomol.strengths(states, trans, 1000.0, 1000.0 ** 1.5)[0] / want - 1) <= 1e-12


def test_the_integral_of_one_line():
    """sum kappa_i dnu over the grid equals S N_A / M less the Lorentz wings beyond the cut-off, S (2 / pi) atan(gamma / C).  The
    tolerance is tests/test_lines_reference.py::test_the_integral_of_one_line's, term by term: the end points h gamma / (pi C^2), the
    trapezoid rule (h^2 / 12) 4 gamma / (pi C^3) and 2 exp(-2 pi gamma / h), the Voigt wing's excess 3 / (a C)^2 of the wings' share,
    K's 1e-6 and 8 n eps of the sum; the line stands on a grid point, C is a whole number of steps, P = 1 bar"""
    import lines_cases as lc
    nu0, h, C, temp, press = 1000.0, 0.005, 25.0, 300.0, 1.0e6
    n = int(round(2 * (C + 5.0) / h)) + 1
    nu_first = nu0 - (C + 5.0)
    case = ec.two_states_case(nu0, cutoff=C, grid=(nu_first, h, n))
    q_t = case.q(temp)
    kappa, p, kept = er.plain_fp64(case.states, case.trans, case.broadening, temp, press, q_t, case.molar_mass, 0.0, C, nu_first, h, n)
    p = p[:, 0]
    a, gamma = p[2], p[3] / p[2]
    assert p[0] == nu0 and (nu_first + np.arange(n) * h == nu0).sum() == 1 and len(kept) == 1
    assert int(np.count_nonzero(kappa)) == int(round(2 * C / h)) + 1
    total = float(er.strengths(case.states, case.trans, temp, q_t, np.float64)[0]) * lr.N_A / case.molar_mass
    expected = total * (1.0 - 2.0 / np.pi * np.arctan(gamma / C))
    tol = (h * gamma / (np.pi * C * C) + h * h / 12.0 * 4.0 * gamma / (np.pi * C ** 3) + 2.0 * np.exp(-2.0 * np.pi * gamma / h)
           + 3.0 / (a * C) ** 2 * (2.0 / np.pi) * gamma / C + lc.GOLDEN_BOUND + 8.0 * n * 2.2e-16)
    got = float(np.sum(kappa) * h)
    print("integral %.12e, expected %.12e: relative difference %.3e, tolerance %.3e" % (got, expected, abs(got / expected - 1), tol))
    assert tol < 2e-6 and abs(got - expected) <= tol * total


def test_against_the_restatement_of_lines_py():
    """one broadener, the list converted to the seven fields (tools/exomol_parity.py): the two long-double restatements agree at
    the project's floor.  The figure is measured by the tool and kept in profiles/exomol_parity.json"""
    spec = importlib.util.spec_from_file_location("exomol_parity", os.path.join(ROOT, "tools", "exomol_parity.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.measure()
    for node in out["nodes"]:
        print("T = %g K, P = %g: kappa %.3e, nu_0, s, a, y %s" % (node["T"], node["P"], node["kappa"], node["line_params"]))
    assert len(out["nodes"]) == 3 and out["largest"] <= ec.lc.FLOOR == out["floor"]


def test_the_plain_fp64_restatement_lies_where_fp64_can():
    """plain_fp64's four numbers per line against long double's on a case with two broadeners: the yardstick itself stays at the
    floor, and both restatements keep the same transitions"""
    case = ec.make("broadeners: 2")
    r = ec.restated(case, 0)
    dev = np.abs(r["params_f64"] / r["params_ld"] - 1).max()
    print("line_params of plain_fp64 against long double: %.3e" % float(dev))
    assert dev < 1e-13
    assert len(r["kept"]) == np.count_nonzero(ec.pattern("alternating", ec.B + 1))
