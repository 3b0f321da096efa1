"""The star tool's contract (helios_amd/star.py, include/helios_hip.h section 8) restated plainly in np.longdouble: the blend
of the corner spectra, the re-binning one interface and one bin at a time, the 199-term Planck integral and the secant steps.
Of the project it takes the physical constants, nothing else: no plan, no index array, no vectorised sum.  Checked against
exact rational and 60-digit decimal arithmetic in tests/test_star_reference.py; the CPU and GPU tests hold both backends to
it."""
import numpy as np

from helios_amd import phys_const as pc

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
_PI = LD("3.14159265358979323846264338327950288")


def require_extended_precision():
    """the reference is worth nothing in a long double that is a double: fail, do not skip"""
    assert EPS_LD <= 1.1e-19, "np.longdouble has eps %.3e here: no 64-bit mantissa to hold the kernels to" % EPS_LD


def ld(a):
    """double -> long double is exact"""
    return np.asarray(a, np.float64).astype(LD)


# ---- the blend ------------------------------------------------------------------------------------------------------------
def reference_nodes(teff, log_g, metal):
    step = 100 if teff < 7000 else 200
    tdown, tup = step * int(np.floor(teff / step)), step * int(np.ceil(teff / step))
    gdown, gup = 0.5 * np.floor(log_g / 0.5), 0.5 * np.ceil(log_g / 0.5)
    mdown, mup = 0.5 * np.floor(metal / 0.5), 0.5 * np.ceil(metal / 0.5)
    return tdown, tup, float(gdown), float(gup), float(mdown), float(mup)


def reference_blend(corner, teff, log_g, metal):
    """`corner(t, g, m)` gives the fp32 spectrum at a node.  Trilinear in the axes that are off a node, the value itself on
    the others; long double throughout, rounded nowhere"""
    require_extended_precision()
    tdown, tup, gdown, gup, mdown, mup = reference_nodes(teff, log_g, metal)
    axes = []
    for x, down, up in ((teff, tdown, tup), (log_g, gdown, gup), (metal, mdown, mup)):
        if up == down:
            axes.append([(up, LD(1))])
        else:
            axes.append([(up, (LD(x) - LD(down)) / (LD(up) - LD(down))), (down, (LD(up) - LD(x)) / (LD(up) - LD(down)))])
    total = None
    for t, wt in axes[0]:
        for g, wg in axes[1]:
            for m, wm in axes[2]:
                term = np.asarray(corner(t, g, m), np.float32).astype(LD) * (wt * wg * wm)
                total = term if total is None else total + term
    return total


# ---- the re-binning -------------------------------------------------------------------------------------------------------
def reference_interface(lam, flux, x):
    """0 outside the table; else the linear interpolant between the points around x, found by counting the tabulated
    wavelengths below x -- on the first one the count is 0 and the index -1 is the LAST point, as in the reference"""
    lam64 = np.asarray(lam, np.float64)
    if x < lam64[0] or x > lam64[-1]:
        return LD(0)
    p = int(np.sum(lam64 < x)) - 1
    l, f, x = ld(lam), ld(flux), LD(np.float64(x))
    v = f[p] * (l[p + 1] - x) + f[p + 1] * (x - l[p])
    return v / (l[p + 1] - l[p])


def reference_rebin(lam, flux, inter, extrapol):
    """every bin: the extrapolation value when an interface value is 0, the mean of the interface values when no tabulated
    point lies inside, else the trapezoids from interface to interface over the points inside, divided by the width"""
    require_extended_precision()
    lam64, inter64 = np.asarray(lam, np.float64), np.asarray(inter, np.float64)
    l, f = ld(lam), ld(flux)
    # an interface value that rounds to 0 in fp64 counts as 0: the comparison is the fp64 code's
    F = [reference_interface(lam, flux, x) for x in inter64]
    out = np.zeros(len(inter64) - 1, LD)
    for i in range(len(out)):
        if float(F[i]) == 0 or float(F[i + 1]) == 0:
            out[i] = LD(extrapol[i])
            continue
        inside = np.nonzero((lam64 >= inter64[i]) & (lam64 < inter64[i + 1]))[0]
        xi, xj = LD(inter64[i]), LD(inter64[i + 1])
        if len(inside) == 0:
            out[i] = (F[i] + F[i + 1]) / 2
            continue
        ln = np.concatenate(([xi], l[inside], [xj]))
        fn = np.concatenate(([F[i]], f[inside], [F[i + 1]]))
        out[i] = np.sum((fn[:-1] + fn[1:]) / 2 * (ln[1:] - ln[:-1]), dtype=LD) / (xj - xi)
    return out


# ---- the black body -------------------------------------------------------------------------------------------------------
def _lower_gamma4(x):
    """int_0^x t^3 e^-t dt by its power series, 60 terms (x <= 2)"""
    total, term = LD(0), x ** 4 / 4
    for k in range(60):
        total = total + term
        term = term * (-x) / (k + 1) * LD(k + 4) / LD(k + 5)      # (-x)^(k+1) / (k+1)! / (k+5)
    return total


def reference_planck(temp, lo, hi):
    """pi x the 199-term series of the Planck integral between lo and hi (cm), divided by the width.  Term n is
    int t^3 e^-t dt between n y_top and n y_bot, over n^4: its closed form e^-x (x^3 + 3 x^2 + 6 x + 6) at both limits, or --
    both limits below 2, where the two closed forms are 6 less a little and their difference would keep few of the long
    double's digits -- the difference of the alternating power series of int_0^x"""
    require_extended_precision()
    if temp == 0:
        return np.zeros(np.shape(lo), LD)
    T, lo, hi = LD(np.float64(temp)), np.atleast_1d(ld(lo)), np.atleast_1d(ld(hi))
    kb, h, c = LD(pc.K_B), LD(pc.H), LD(pc.C)
    d = 2 * (kb / h) ** 3 * kb * T ** 4 / c ** 2
    yt, yb = h * c / (hi * kb * T), h * c / (lo * kb * T)
    closed = lambda x: np.exp(-x) * (x ** 3 + 3 * x ** 2 + 6 * x + 6)
    result = np.zeros(np.shape(lo), LD)
    for n in range(1, 200):
        a, b = n * yt, n * yb
        term = closed(a) - closed(b)
        small = (a < 2) & (b < 2)
        if small.any():
            term[small] = _lower_gamma4(b[small]) - _lower_gamma4(a[small])
        result = result + term / LD(n) ** 4
    return _PI * (result * (d / (hi - lo)))


def reference_fit_index(inter, last_tabulated):
    for i, x in enumerate(np.asarray(inter, np.float64)):
        if x > last_tabulated:
            return i - 2
    return None


def reference_secant(inter, index, bin_flux, start_temp, steps=10):
    """the temperatures of the secant steps, kept in fp64 between steps as the code keeps them; the arithmetic of a step in
    long double"""
    inter = list(np.asarray(inter, np.float64))
    lo, hi = np.array([inter[index]]), np.array([inter[index + 1]])
    before, now = np.float64(start_temp) - 100, np.float64(start_temp)
    for n in range(steps):
        vb, vn = reference_planck(before, lo, hi)[0], reference_planck(now, lo, hi)[0]
        if float(vb) != float(vn):
            new = np.float64(LD(now) - (vn - LD(np.float64(bin_flux))) / (vn - vb) * (LD(now) - LD(before)))
        else:
            new = now
        before, now = now, new
    return float(now)


def rel_dev(value, reference):
    """|value - reference| / |reference| per entry in long double; 0 where both are 0, inf where only the reference is"""
    v, r = np.asarray(value).astype(LD), np.asarray(reference).astype(LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(v - r) / np.abs(r)
    d = np.where((r == 0) & (v == 0), LD(0), d)
    return np.where((r == 0) & (v != 0), LD(np.inf), d).astype(np.float64)
