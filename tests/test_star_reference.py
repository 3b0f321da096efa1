"""The long-double restatement of the star tool (tests/star_reference.py) against exact arithmetic on small cases: rational
numbers for the blend and the re-binning, 60-digit decimals for the Planck series and a secant step (exp is not rational)."""
from decimal import Decimal, getcontext
from fractions import Fraction

import numpy as np

import star_reference as sr
from helios_amd import phys_const as pc

F = Fraction


def _fr(a):
    return [F(float(v)) for v in a]


def _close(value, exact, ulps=4):
    """a long double against an exact rational or decimal: within a few ulps of long double"""
    v = F(*[int(x) for x in np.longdouble(value).as_integer_ratio()]) if not isinstance(value, F) else value
    e = F(exact) if not isinstance(exact, Decimal) else F(str(exact))
    assert abs(v - e) <= ulps * F(sr.EPS_LD) * abs(e), (float(v), float(e))


def test_blend_in_rationals():
    rng = np.random.default_rng(1)
    spectra = {}

    def corner(t, g, m):
        return spectra.setdefault((t, g, m), (1e14 * (1 + rng.random(5))).astype(np.float32))
    for teff, log_g, metal in ((3026, 4.944, 0.39), (3000, 4.944, 0.39), (3026, 5.0, 0.5), (7100, 4.2, -0.3), (3000, 5.0, 0.5)):
        out = sr.reference_blend(corner, teff, log_g, metal)
        td, tu, gd, gu, md, mu = sr.reference_nodes(teff, log_g, metal)
        exact = [F(0)] * 5
        for t, wt in ([(tu, F(1))] if tu == td else [(tu, (F(teff) - td) / (tu - td)), (td, (tu - F(teff)) / (tu - td))]):
            for g, wg in ([(gu, F(1))] if gu == gd else [(gu, (F(log_g) - F(gd)) / (F(gu) - F(gd))), (gd, (F(gu) - F(log_g)) / (F(gu) - F(gd)))]):
                for m, wm in ([(mu, F(1))] if mu == md else [(mu, (F(metal) - F(md)) / (F(mu) - F(md))), (md, (F(mu) - F(metal)) / (F(mu) - F(md)))]):
                    exact = [e + F(float(v)) * wt * wg * wm for e, v in zip(exact, corner(t, g, m))]
        for v, e in zip(out, exact):
            _close(v, e, ulps=16)


def test_rebinning_in_rationals():
    lam = np.array([1.0, 1.5, 2.0, 2.25, 2.5, 3.0, 3.5, 4.0])
    flux = np.array([3.0, 4.0, 2.5, 2.0, 6.0, 0.0, 5.0, 7.0])
    inter = np.array([0.5, 1.0, 1.2, 1.4, 2.0, 2.6, 3.0, 3.2, 3.3, 4.0, 5.0])
    ext = np.arange(10) + 100.0
    out = sr.reference_rebin(lam, flux, inter, ext)
    l, f = _fr(lam), _fr(flux)

    def at(x):
        x = F(float(x))
        if x < l[0] or x > l[-1]:
            return F(0)
        p = sum(1 for v in l if v < x) - 1          # -1 on the first point: Python's index, the last point
        return (f[p] * (l[p + 1] - x) + f[p + 1] * (x - l[p])) / (l[p + 1] - l[p])
    for i in range(10):
        a, b = F(float(inter[i])), F(float(inter[i + 1]))
        Fa, Fb = at(inter[i]), at(inter[i + 1])
        if Fa == 0 or Fb == 0:
            exact = F(float(ext[i]))
        else:
            nodes = [(a, Fa)] + [(x, y) for x, y in zip(l, f) if a <= x < b] + [(b, Fb)]
            exact = (Fa + Fb) / 2 if len(nodes) == 2 else \
                sum((y0 + y1) / 2 * (x1 - x0) for (x0, y0), (x1, y1) in zip(nodes[:-1], nodes[1:])) / (b - a)
        _close(out[i], exact, ulps=16)
    assert out[0] == 100 and out[5] == 105 and out[6] == 106 and out[9] == 109      # outside, the tabulated 0, outside
    assert float(sr.reference_interface(lam, flux, 1.0)) == 3.0                     # on the first point: flux[0] (wrap)


def _planck_decimal(temp, lo, hi):
    getcontext().prec = 60
    D = Decimal
    kb, h, c, T, lo, hi = D(pc.K_B), D(pc.H), D(pc.C), D(float(temp)), D(float(lo)), D(float(hi))
    d = 2 * (kb / h) ** 3 * kb * T ** 4 / c ** 2
    yt, yb = h * c / (hi * kb * T), h * c / (lo * kb * T)
    tot = D(0)
    for n in range(1, 200):
        tot += (-n * yt).exp() * (yt ** 3 / n + 3 * yt ** 2 / n ** 2 + 6 * yt / n ** 3 + D(6) / n ** 4) \
            - (-n * yb).exp() * (yb ** 3 / n + 3 * yb ** 2 / n ** 2 + 6 * yb / n ** 3 + D(6) / n ** 4)
    return D("3.14159265358979323846264338327950288419716939937510582") * tot * d / (hi - lo)


def test_planck_series_in_60_digits():
    """good to a few hundred ulps of long double everywhere: at 200 micron and 12000 K too, where the closed forms at the two
    limits agree to ten digits and the restatement takes the terms from the power series of the lower limit's integral"""
    for temp, lo, hi, tol in ((2300.0, 0.3e-4, 0.306e-4, 1e-17), (5772.0, 1e-4, 1.02e-4, 1e-16), (12000.0, 196e-4, 200e-4, 1e-16)):
        v = sr.reference_planck(temp, np.array([lo]), np.array([hi]))[0]
        e = _planck_decimal(temp, lo, hi)
        rel = abs(F(*[int(x) for x in v.as_integer_ratio()]) / F(str(e)) - 1)
        assert rel < F(tol), (temp, lo, float(rel))


def test_secant_steps_meet_the_flux():
    inter = np.array([1.0e-4, 1.02e-4, 1.0404e-4, 1.061208e-4])
    target = float(_planck_decimal(4321.0, inter[1], inter[2]))
    t = sr.reference_secant(inter, 1, target, 4000.0)
    assert abs(t / 4321.0 - 1) < 1e-12
    assert sr.reference_fit_index(inter, 1.03e-4) == 0 and sr.reference_fit_index(inter, 2e-4) is None
    assert sr.reference_fit_index(inter, 0.5e-4) == -2       # Python's index arithmetic: counted from the end
