"""The contract of the Rayleigh file and the continuum containers (helios_amd/continuum.py) restated plainly in np.longdouble:
every formula as the papers write it, one wavelength at a time -- 64 mantissa bits carry the cancellations that the product's
fp64 code avoids by other forms (one exception: 1/mu - 1/mu_0 of H-_bf is taken over a common denominator, since a wavelength a
part in 1e12 below mu_0 leaves long double seven digits otherwise).  Of the project it takes the published numbers
(continuum_data), the constants and the molar weights; no formula, no table construction, no interpolation.

The wavelength in micron is the DOUBLE product lam * 1e4, and every branch is decided on doubles, as the contract says; the
arithmetic behind the branch is long double.
"""
import os

import numpy as np

from helios_amd import continuum_data as cd
from helios_amd import phys_const as pc
from helios_amd.species_data import species_lib

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ktable_continuum", "reference.npz")


def require_extended_precision():
    assert EPS_LD <= 1.1e-19, "np.longdouble has eps %.3e here: no 64-bit mantissa to hold the tables to" % EPS_LD


def ld(v):
    return LD(np.float64(v))            # a double, exactly


PI = LD(2) * np.arccos(LD(0))


# ---- Rayleigh ---------------------------------------------------------------------------------------------------------------------
def rayleigh_one(name, lam64):
    lam = ld(lam64)
    if name == "e-":
        return ld(pc.SIGMA_T)
    if name == "H":
        r = ld(cd.H_SERIES_LYMAN) / lam
        return ld(cd.H_SERIES_SIGMA_T) * r ** 4 * sum(ld(c) * r ** (2 * k) for k, c in enumerate(cd.H_SERIES))
    f = cd.RAYLEIGH[name]
    nu2 = 1 / (lam * lam)
    if f["form"] == "cauchy":
        n = ld(f["scale"]) * (1 + ld(f["b"]) * nu2) + 1
    elif f["form"] == "sellmeier":
        a, b = f["a"], f["b"]
        if "split_nu" in f and not (1.0 / np.float64(lam64) <= f["split_nu"]):        # decided on the double wavenumber
            a, b = f["a_blue"], f["b_blue"]
        n = ld(f["scale"]) * (ld(a) + ld(b) / (ld(f["c"]) - nu2)) + 1
    else:
        n = ld(f["scale"]) * sum(ld(b) / (ld(c) - nu2) for b, c in zip(f["b"], f["c"])) + 1
    k0, k1, k2, k4 = [ld(v) for v in f["king"]]
    king = k0 + k1 / lam + k2 * nu2 + k4 * nu2 * nu2
    return 24 * PI ** 3 / (ld(f["n_ref"]) ** 2 * lam ** 4) * ((n * n - 1) / (n * n + 2)) ** 2 * king


def rayleigh(name, wave):
    require_extended_precision()
    return np.array([rayleigh_one(name, l) for l in np.asarray(wave, np.float64)], LD)


# ---- continuum --------------------------------------------------------------------------------------------------------------------
def mass(name):
    return ld(species_lib[name].weight) * ld(pc.AMU)


def hm_bf_one(mu64):
    if mu64 < cd.HM_BF_LAMBDA_MIN or mu64 > cd.HM_BF_LAMBDA_0:
        return LD(0)
    mu = ld(mu64)
    x = (ld(cd.HM_BF_LAMBDA_0) - mu) / (mu * ld(cd.HM_BF_LAMBDA_0))     # 1/mu - 1/mu_0; the difference of two doubles is exact here
    f = sum(ld(c) * x ** (LD(k) / 2) for k, c in enumerate(cd.HM_BF_C))
    return ld(1e-18) * mu ** 3 * x ** LD(1.5) * f / mass("H")


def hm_ff_one(mu64, T, P):
    if mu64 < cd.HM_FF_LAMBDA_MIN:
        return LD(0)
    s = cd.HM_FF["short" if mu64 < cd.HM_FF_LAMBDA_SPLIT else "long"]
    mu, theta = ld(mu64), ld(cd.THETA_K) / ld(T)
    total = LD(0)
    for n in range(6):
        bracket = (ld(s["A"][n]) * mu ** 2 + ld(s["B"][n]) + ld(s["C"][n]) / mu + ld(s["D"][n]) / mu ** 2 + ld(s["E"][n]) / mu ** 3
                   + ld(s["F"][n]) / mu ** 4)
        total += theta ** (LD(n + 2) / 2) * bracket
    return ld(1e-29) * total * ld(P) / mass("H")


def he_nodes():
    """temperatures (ascending, doubles as 5040 / theta gives them), wavelengths in micron, and k in cm^4 dyne^-1 per node as
    doubles: the table's rows in ascending temperature, the 50 K row a copy of the 1400 K row, six wavelengths appended with
    k = limit * lambda^2"""
    thetas = sorted(cd.HEM_THETA + (cd.HEM_THETA_FLOOR,), reverse=True)
    temps = [cd.THETA_K / th for th in thetas]
    assert temps == sorted(temps)
    lams = list(cd.HEM_LAMBDA) + list(cd.HEM_LAMBDA_LONG)
    rows = []
    for th in thetas:
        r = 0 if th == cd.HEM_THETA_FLOOR else cd.HEM_THETA.index(th)
        rows.append([k * cd.HEM_UNIT for k in cd.HEM_K[r]] + [cd.HEM_LONG[r] * l ** 2 * cd.HEM_UNIT for l in cd.HEM_LAMBDA_LONG])
    return temps, lams, rows


_HE = []


def he_one(mu64, T, P):
    if not _HE:                         # the nodes and their logarithms, once
        temps, lams, rows = he_nodes()
        _HE.extend((temps, lams, [np.log10(ld(l)) for l in lams], [[np.log10(ld(k)) for k in r] for r in rows]))
    temps, lams, xs, logk = _HE
    x64 = np.log10(np.float64(mu64))
    inside = temps[0] <= T <= temps[-1] and np.log10(np.float64(lams[0])) <= x64 <= np.log10(np.float64(lams[-1]))
    v = ld(cd.HEM_FILL_LOG10)
    if inside:
        i = max(k for k in range(len(temps) - 1) if temps[k] <= T or k == 0)
        x = np.log10(ld(mu64))
        j = max(k for k in range(len(lams) - 1) if np.log10(np.float64(lams[k])) <= x64 or k == 0)
        ft = (ld(T) - ld(temps[i])) / (ld(temps[i + 1]) - ld(temps[i]))
        fx = (x - xs[j]) / (xs[j + 1] - xs[j])
        z = lambda a, b: logk[a][b]
        v = (1 - ft) * (1 - fx) * z(i, j) + ft * (1 - fx) * z(i + 1, j) + (1 - ft) * fx * z(i, j + 1) + ft * fx * z(i + 1, j + 1)
    return LD(10) ** v * ld(P) / mass("He")


def continuum(name, wave, temp, press):
    """k[t][p][x] in long double"""
    require_extended_precision()
    mu = np.asarray(wave, np.float64) * 1e4
    out = np.empty((len(temp), len(press), len(mu)), LD)
    for t, T in enumerate(np.asarray(temp, np.float64)):
        for p, P in enumerate(np.asarray(press, np.float64)):
            for x, m in enumerate(mu):
                out[t, p, x] = (hm_bf_one(m) if name == "H-_bf" else hm_ff_one(m, T, P) if name == "H-_ff"
                                else he_one(m, T, P))
    return out


# ---- the tolerance rule --------------------------------------------------------------------------------------------------------------
def relative(a, ref):
    """|a - ref| / |ref| per entry in long double; 0 where both are 0, inf where only the restatement is"""
    a, ref = np.asarray(a).astype(LD), np.asarray(ref, LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(a - ref) / np.abs(ref)
    r = np.where((a == 0) & (ref == 0), LD(0), r)
    return np.where((ref == 0) & (a != 0), LD(np.inf), r)


def check(got, other, exact, what):
    """`got` against `other` entry by entry at max(1e-13, 8 eps), eps = |other - exact| / |exact| at that entry; zeros of `other`
    are zeros of `got`.  Prints before it asserts; returns the record."""
    got, other = np.asarray(got, np.float64).reshape(-1), np.asarray(other, np.float64).reshape(-1)
    exact = np.asarray(exact, LD).reshape(-1)
    assert got.shape == other.shape == exact.shape, (what, got.shape, other.shape, exact.shape)
    zero = other == 0
    eps = relative(other, exact).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        dev = np.where(zero, 0.0, np.abs(got.astype(LD) - other.astype(LD)) / np.abs(other.astype(LD))).astype(np.float64)
    bound = np.maximum(1e-13, 8 * eps)
    worst = int(np.argmax(dev / bound))
    rec = {"max_deviation": float(dev.max()), "max_eps": float(eps[~zero].max()) if (~zero).any() else 0.0,
           "worst_ratio_to_bound": float(dev[worst] / bound[worst]), "zeros": int(zero.sum()), "entries": int(len(got)),
           "own_max_deviation_from_long_double": float(relative(got, exact)[~zero].max()) if (~zero).any() else 0.0}
    print("%s: deviation %.3e (eps up to %.3e), worst deviation / bound %.3f, own deviation from long double %.3e, %d zeros of %d"
          % (what, rec["max_deviation"], rec["max_eps"], rec["worst_ratio_to_bound"], rec["own_max_deviation_from_long_double"],
             rec["zeros"], rec["entries"]))
    assert np.all(got[zero] == 0), "%s: %d entries are 0 on one side only" % (what, int((got[zero] != 0).sum()))
    assert np.all(np.isfinite(dev)) and np.all(dev <= bound), "%s: entry %d deviates by %.3e, bound %.3e" % (
        what, worst, dev[worst], bound[worst])
    return rec


def check_exact(got, fp64, exact, what):
    """`got` against the restatement `exact` entry by entry at max(1e-13, 8 eps64), eps64 = |fp64 - exact| / |exact| at that entry
    with `fp64` the numpy backend's values; zeros of the restatement are zeros of both.  Prints before it asserts."""
    got, fp64 = np.asarray(got, np.float64).reshape(-1), np.asarray(fp64, np.float64).reshape(-1)
    exact = np.asarray(exact, LD).reshape(-1)
    assert got.shape == fp64.shape == exact.shape, (what, got.shape, fp64.shape, exact.shape)
    zero = exact == 0
    eps = np.where(zero, 0.0, relative(fp64, exact).astype(np.float64))
    dev = np.where(zero, 0.0, relative(got, exact).astype(np.float64))
    bound = np.maximum(1e-13, 8 * eps)
    worst = int(np.argmax(dev / bound))
    rec = {"max_deviation": float(dev.max()), "max_eps64": float(eps.max()), "worst_ratio_to_bound": float(dev[worst] / bound[worst]),
           "zeros": int(zero.sum()), "entries": int(len(got))}
    print("%s: deviation from long double %.3e (eps64 up to %.3e), worst deviation / bound %.3f, %d zeros of %d"
          % (what, rec["max_deviation"], rec["max_eps64"], rec["worst_ratio_to_bound"], rec["zeros"], rec["entries"]))
    assert np.all(got[zero] == 0) and np.all(fp64[zero] == 0), "%s: entries that are 0 in the restatement are not 0" % what
    assert np.all(got[~zero] != 0), "%s: zeros where the restatement has none" % what
    assert np.all(np.isfinite(dev)) and np.all(dev <= bound), "%s: entry %d deviates by %.3e, bound %.3e" % (
        what, worst, dev[worst], bound[worst])
    return rec


# ---- shapes of the device tests ------------------------------------------------------------------------------------------------------
def branch_wavelengths(n):
    """n wavelengths in cm, ascending: the golden's branch-straddling set, thinned or padded log-uniformly to n"""
    base = np.load(GOLDEN)["wavelengths"]
    if n <= len(base):
        keep = np.unique(np.round(np.linspace(0, len(base) - 1, n)).astype(int))
        assert len(keep) == n
        return base[keep]
    extra = 10 ** np.linspace(np.log10(0.11e-4), np.log10(230e-4), n - len(base))
    out = np.unique(np.concatenate((base, extra)))
    assert len(out) == n
    return out
