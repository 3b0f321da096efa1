"""The contract of helios_amd/chem.py restated one node at a time in np.longdouble (`node`), and the same statements in fp64
(`plain_fp64`); tests/test_chem_reference.py holds the restatement to mpmath at 60 digits.  The bisection here is arithmetic and
runs until the interval collapses; the package's runs on bit patterns.  Nothing is shared with the package but the species'
order and weights.  Also the Gibbs file the tests write from the golden, and the sign changes of the quintic on a grid."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chem", "reference.npz")
KEYS = ("H2", "He", "H2O", "CO", "CH4", "CO2", "C2H2", "mu")
ALL = ("n_CH4",) + KEYS
MAX_HALVINGS = 40000             # a long-double interval from 0 collapses after about 16 500


def golden():
    return np.load(GOLDEN)


def golden_table():
    g = golden()
    return g["gibbs_temperatures"], g["gibbs_dg1"], g["gibbs_dg2"], g["gibbs_dg3"]


def constants(ft, table, temp, press, gas_constant, exp):
    t = [ft(v) for v in table[0]]
    temp, press, gas_constant = ft(temp), ft(press), ft(gas_constant)
    i = 0
    while i < len(t) - 2 and t[i + 1] <= temp:
        i += 1
    u = (temp - t[i]) / (t[i + 1] - t[i])
    g = [ft(dg[i]) + u * (ft(dg[i + 1]) - ft(dg[i])) for dg in table[1:]]
    rt = gas_constant * temp
    return exp(-g[0] / rt) / press / press, exp(-g[1] / rt), exp(-g[2] / rt) / press / press


def coefficients(ft, k1, k2, k3, n_o, n_c):
    d = n_o - n_c
    return [ft(-2) * n_c,
            ft(8) * k1 / k2 * d * d + ft(1) + ft(2) * k1 * d,
            ft(8) * k1 / k2 * d + ft(2) * k3 + k1,
            ft(2) * k1 / k2 * (ft(1) + ft(8) * k3 * d) + ft(2) * k1 * k3,
            ft(8) * k1 * k3 / k2,
            ft(8) * k1 * k3 * k3 / k2]


def horner(a, x):
    return ((((a[5] * x + a[4]) * x + a[3]) * x + a[2]) * x + a[1]) * x + a[0]


def bracket(ft, k3, n_o, n_c, sqrt):
    d = n_o - n_c
    x_min = ft(4) * (-d) / (ft(1) + sqrt(ft(1) + ft(16) * k3 * (-d))) if d < 0 else ft(0)
    return x_min, ft(2) * n_c


def solve(ft, table, temp, press, n_o, n_c, he_to_h, gas_constant, weights, exp, sqrt):
    """{n_CH4, the seven mixing ratios, mu} of one node in the number type ft"""
    n_o, n_c = ft(n_o), ft(n_c)
    k1, k2, k3 = constants(ft, table, temp, press, gas_constant, exp)
    a = coefficients(ft, k1, k2, k3, n_o, n_c)
    lo, hi = bracket(ft, k3, n_o, n_c, sqrt)
    if horner(a, hi) > 0:
        for _ in range(MAX_HALVINGS):
            mid = (lo + hi) / ft(2)
            if mid == lo or mid == hi:
                break
            if horner(a, mid) < 0:
                lo = mid
            else:
                hi = mid
        else:
            raise AssertionError("the interval did not collapse")
    x = hi
    b = ft(1) + k1 * x
    h = ft(4) * n_o / (b + sqrt(b * b + ft(16) * k1 * x * n_o / k2))
    co = k1 * x * h
    co2 = co * h / k2
    c2h2 = k3 * x * x
    n_he = ft(2) * ft(he_to_h)
    s = ft(1) + n_he + h + co + x + co2 + c2h2
    out = {"n_CH4": x, "H2": ft(1) / s, "He": n_he / s, "H2O": h / s, "CO": co / s, "CH4": x / s, "CO2": co2 / s, "C2H2": c2h2 / s}
    mu = ft(0)
    for name, w in zip(KEYS[:7], weights):
        mu = mu + out[name] * ft(w)
    out["mu"] = mu
    return out


def node(table, temp, press, n_o, n_c, he_to_h, gas_constant, weights):
    with np.errstate(all="ignore"):
        return solve(np.longdouble, table, temp, press, n_o, n_c, he_to_h, gas_constant, weights, np.exp, np.sqrt)


def plain_fp64(table, temp, press, n_o, n_c, he_to_h, gas_constant, weights):
    with np.errstate(all="ignore"):
        return solve(np.float64, table, temp, press, n_o, n_c, he_to_h, gas_constant, weights, np.exp, np.sqrt)


def with_mpmath(table, temp, press, n_o, n_c, he_to_h, gas_constant, weights, digits=60):
    import mpmath as mp
    with mp.workdps(digits):
        return solve(mp.mpf, table, temp, press, n_o, n_c, he_to_h, gas_constant, weights, mp.exp, mp.sqrt)


def deviation(got, want):
    """|got - want| / |want| in long double, as a float; 0 where both are 0"""
    got, want = np.longdouble(got), np.longdouble(want)
    if want == 0:
        return 0.0 if got == 0 else np.inf
    return float(abs(got - want) / abs(want))


def sign_changes(table, temp, press, n_o, n_c, gas_constant, samples=400):
    """(sign changes of the long-double quintic over `samples` points spaced geometrically from the bracket's lower end to
    2 n_C, f(x_min) <= 0, f(2 n_C) <= 0 -- all carbon in methane, the root within a rounding of the bracket's end --, the
    coefficients in fp64 from a_0 up)"""
    ft = np.longdouble
    with np.errstate(all="ignore"):
        k1, k2, k3 = constants(ft, table, temp, press, gas_constant, np.exp)
        a = coefficients(ft, k1, k2, k3, ft(n_o), ft(n_c))
        lo, hi = bracket(ft, k3, ft(n_o), ft(n_c), np.sqrt)
        start = lo if lo > 0 else hi * ft(1e-60)
        xs = np.concatenate(([lo], start * (hi / start) ** (np.arange(1, samples + 1, dtype=ft) / ft(samples))))
        xs[-1] = hi
        f = horner(a, xs)
    s = np.sign(f[f != 0])
    return int(np.count_nonzero(s[1:] != s[:-1])), bool(f[0] <= 0), bool(f[-1] <= 0), [float(v) for v in a]
