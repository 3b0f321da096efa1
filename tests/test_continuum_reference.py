"""The long-double restatement of the Rayleigh and continuum contract (tests/continuum_reference.py) against facts that can be
derived by hand.  No GPU, no golden."""
import numpy as np

import continuum_reference as cr
from helios_amd import continuum_data as cd
from helios_amd import phys_const as pc

LD = np.longdouble


def test_long_double_is_extended():
    cr.require_extended_precision()


def test_h_minus_bound_free_vanishes_at_the_threshold_and_outside():
    """0 beyond both limits and AT the photo-detachment threshold 1.6419 micron, where x = 0; at 0.125 micron itself the formula
    applies (the reference tests `< 0.125`), and inside it is positive"""
    for mu in (0.1, np.nextafter(0.125, 0), np.nextafter(1.6419, 2), 1.7, 200.0, 1.6419):
        assert cr.hm_bf_one(mu) == 0, mu
    for mu in (0.125, np.nextafter(1.6419, 0), 0.8):
        assert cr.hm_bf_one(mu) > 0, mu
    # at 0.125 micron by hand: x = 8 - 1/1.6419
    x = LD(8) - 1 / cr.ld(1.6419)
    want = cr.ld(1e-18) * cr.ld(0.125) ** 3 * x ** LD(1.5) * sum(cr.ld(c) * x ** (LD(k) / 2) for k, c in enumerate(cd.HM_BF_C))
    assert abs(cr.hm_bf_one(0.125) * cr.mass("H") / want - 1) < 1e-17


def test_he_minus_at_a_node_is_the_tabulated_number():
    P, m = 1e6, cr.mass("He")
    for theta, row in ((0.5, 10), (1.0, 7), (3.6, 0)):
        for col in (0, 5, 15):
            want = cr.ld(cd.HEM_K[row][col] * 1e-26) * cr.ld(P) / m
            got = cr.he_one(cd.HEM_LAMBDA[col], 5040.0 / theta, P)
            assert abs(got / want - 1) < 1e-16, (theta, col, float(got), float(want))
    # the appended wavelengths, and the 50 K row that repeats the 1400 K row
    want = cr.ld(cd.HEM_LONG[7] * 200.0 ** 2 * 1e-26) * cr.ld(P) / m
    assert abs(cr.he_one(200.0, 5040.0, P) / want - 1) < 1e-16
    assert abs(cr.he_one(cd.HEM_LAMBDA[3], 5040.0 / 100.8, P) / cr.he_one(cd.HEM_LAMBDA[3], 5040.0 / 3.6, P) - 1) < 1e-16
    # outside the table: 1e-30 P / m
    for mu, T in ((0.5, 3000.0), (201.0, 3000.0), (1.0, 49.0), (1.0, 10081.0)):
        assert abs(cr.he_one(mu, T, P) / (LD(10) ** -30 * cr.ld(P) / m) - 1) < 1e-16


def test_thomson_is_constant():
    s = cr.rayleigh("e-", [1e-5, 1e-4, 2e-2])
    assert np.all(s == cr.ld(pc.SIGMA_T)) and pc.SIGMA_T == 6.6524587321000005e-25


def test_hydrogen_tends_to_the_first_term():
    lam = 1.0                                       # 1 cm: (lambda_L / lambda)^2 = 8.3e-11
    r = cr.ld(cd.H_SERIES_LYMAN) / LD(lam)
    lead = cr.ld(cd.H_SERIES_SIGMA_T) * r ** 4 * cr.ld(1.26563)
    assert abs(cr.rayleigh_one("H", lam) / lead - 1) < 4 * float(r ** 2)
    assert cd.H_SERIES[0] == 1.26563


def test_h_minus_free_free_is_linear_in_pressure():
    for mu in (0.2, 0.3645, 1.0, 100.0):
        a, b = cr.hm_ff_one(mu, 2000.0, 1.0), cr.hm_ff_one(mu, 2000.0, 1024.0)
        assert a > 0 and abs(b / a / 1024 - 1) < 1e-18
    assert cr.hm_ff_one(np.nextafter(0.1823, 0), 2000.0, 1.0) == 0


def test_the_molecules_follow_lambda_to_the_minus_four_in_the_infrared():
    """far from the resonances n - 1 and the King factor are constant: sigma lambda^4 changes by less than 1e-3 from 50 to 200
    micron"""
    for name in ("H2", "He", "CO2", "CO", "O2", "N2"):
        a, b = cr.rayleigh_one(name, 50e-4) * LD(50e-4) ** 4, cr.rayleigh_one(name, 200e-4) * LD(200e-4) ** 4
        assert a > 0 and abs(a / b - 1) < 1e-3, name
