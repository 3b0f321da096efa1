"""The line-by-line contract of helios_amd/lines.py, restated in plain statements, one line at a time and elementwise over the
spectral points it is asked for: `long_double(...)` in np.longdouble (the checker of both backends), `plain_fp64(...)` the same
statements in fp64 (the yardstick of what fp64 can hold).  The constants are restated; tests/test_lines_reference.py holds them
to the module's.

The contract is one of fp64 numbers, so what it DECIDES -- whether a point lies within the cut-off of a line, and the region of
|z| that K is taken from -- is decided on the fp64 values in both restatements; what it COMPUTES is computed in the number format
asked for.  (A pair one ulp beyond the cut-off is out, whatever a longer format would say.)

Per node (T, P) and line, every statement left to right:
    S      = S_ref * (Q(296) / Q(T)) * exp(-c2 * E'' * (1/T - 1/296)) * (expm1(-c2 * nu_0 / T) / expm1(-c2 * nu_0 / 296))
    nu_0'  = nu_0 + delta_air * P_atm                    P_atm = P / 1013250,  c2 = H C / K_B
    gamma  = (296 / T)^n_air * P_atm * (gamma_air * (1 - x_self) + gamma_self * x_self)
    alpha  = (nu_0' / C) * sqrt(2 * ln 2 * N_A * K_B * T / M)
    a      = sqrt(ln 2) / alpha,   y = max(a * gamma, 1e-8),   s = S * a * (1 / sqrt pi)
per point nu_i = nu_first + i * dnu:  sigma = sum, in the order of the list, over |nu_i - nu_0'| <= cutoff of s * K(a * (nu_i - nu_0'), y),
kappa = sigma * N_A / M.  K(x, y) = Re w(x + i y) from Weideman's approximation (N = 40) for x^2 + y^2 <= 42.25 (|z| <= 6.5), and
from 8, 4 or 2 levels of Laplace's continued fraction beyond 42.25, 225 and 1e4.
"""
import numpy as np

# helios_amd/phys_const.py
C = 2.99792458e10
K_B = 1.380649e-16
H = 6.62607015e-27
N_A = 6.02214076e23
T_REF = 296.0
ATM = 1013250.0
Y_MIN = 1e-8
R2 = (42.25, 225.0, 1.0e4)
LEVELS = (8, 4, 2)
WEIDEMAN_N = 40
COLUMNS = (("nu0", 3, 15), ("s_ref", 15, 25), ("gamma_air", 35, 40), ("gamma_self", 40, 45), ("e_low", 45, 55), ("n_air", 55, 59),
           ("delta_air", 59, 67))
FIELDS = tuple(c[0] for c in COLUMNS)


def weideman():
    """(L, coefficients of Z^39 ... Z^0): the literals of helios_amd/lines_data.py, which are part of the contract"""
    from helios_amd import lines_data
    return lines_data.WEIDEMAN_L, lines_data.WEIDEMAN_A


def constants(T):
    """ln 2 and 1 / sqrt pi in the number format: fp64 takes the literals of the module, long double its own"""
    if T is np.float64:
        return np.float64(0.6931471805599453), np.float64(0.5641895835477563)
    return np.log(T(2.0)), T(1.0) / np.sqrt(T(4.0) * np.arctan(T(1.0)))


def parse_record(rec):
    """the seven numbers of one `.par` record, and its isotopologue character"""
    return dict((name, float(rec[lo:hi])) for name, lo, hi in COLUMNS), rec[2:3]


def region(x, y):
    """0 ... 3 on the fp64 values"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    r2 = x * x + y * y
    return (r2 > R2[0]).astype(np.int64) + (r2 > R2[1]) + (r2 > R2[2])


def k_weideman(x, y, T):
    L, A = weideman()
    L = T(L)
    lr, li = L + y, -x
    nr, ni = L - y, x
    d = lr * lr + li * li
    zr, zi = (nr * lr + ni * li) / d, (ni * lr - nr * li) / d
    pr, pi = T(A[0]) + T(0.0) * x, T(0.0) * x
    for a in A[1:]:
        pr, pi = pr * zr - pi * zi + T(a), pr * zi + pi * zr
    l2r, l2i = lr * lr - li * li, T(2.0) * lr * li
    d2 = l2r * l2r + l2i * l2i
    return (T(2.0) * pr * l2r + T(2.0) * pi * l2i) / d2 + constants(T)[1] * lr / d


def k_fraction(x, y, levels, T):
    tr, ti = x, y
    for k in range(levels, 0, -1):
        c = T(0.5) * T(k)
        d = tr * tr + ti * ti
        tr, ti = x - c * tr / d, y + c * ti / d
    return constants(T)[1] * ti / (tr * tr + ti * ti)


def voigt_k(x, y, T):
    """K at arrays of one length (fp64 values), computed in T; the region is the fp64 one"""
    x64, y64 = np.asarray(x, np.float64).reshape(-1), np.asarray(y, np.float64).reshape(-1)
    reg = region(x64, y64)
    xt, yt = x64.astype(T), y64.astype(T)
    return _k_by_region(xt, yt, reg, T)


def _k_by_region(xt, yt, reg, T):
    out = np.empty(len(xt), T)
    for r in range(4):
        m = reg == r
        if m.any():
            with np.errstate(over="ignore", invalid="ignore"):
                out[m] = k_weideman(xt[m], yt[m], T) if r == 0 else k_fraction(xt[m], yt[m], LEVELS[r - 1], T)
    return out


def strength(line, temp, q_t, q_ref, T):
    """S(T) of one line in T"""
    v = dict((k, T(line[k])) for k in FIELDS)
    temp, q_t, q_ref, one = T(temp), T(q_t), T(q_ref), T(1.0)
    c2 = T(H) * T(C) / T(K_B)
    return v["s_ref"] * (q_ref / q_t) * np.exp(-c2 * v["e_low"] * (one / temp - one / T(T_REF))) \
        * (np.expm1(-c2 * v["nu0"] / temp) / np.expm1(-c2 * v["nu0"] / T(T_REF)))


def line_numbers(line, temp, press, q_t, q_ref, molar_mass, x_self, T):
    """(nu_0', s, a, y) of one line (a dict of the seven numbers) in T"""
    ln2, inv_sqrt_pi = constants(T)
    v = dict((k, T(line[k])) for k in FIELDS)
    s = strength(line, temp, q_t, q_ref, T)
    temp, press, molar_mass, x_self = T(temp), T(press), T(molar_mass), T(x_self)
    patm = press / T(ATM)
    one = T(1.0)
    nu0p = v["nu0"] + v["delta_air"] * patm
    gamma = (T(T_REF) / temp) ** v["n_air"] * patm * (v["gamma_air"] * (one - x_self) + v["gamma_self"] * x_self)
    alpha = (nu0p / T(C)) * np.sqrt(T(2.0) * ln2 * T(N_A) * T(K_B) * temp / molar_mass)
    a = np.sqrt(ln2) / alpha
    y = max(a * gamma, T(Y_MIN))
    return nu0p, s * a * inv_sqrt_pi, a, y


def params(lines, temp, press, q_t, q_ref, molar_mass, x_self, T):
    """[4][lines] in T; `lines`: the seven arrays, sorted"""
    n = len(lines["nu0"])
    out = np.empty((4, n), T)
    for j in range(n):
        out[:, j] = line_numbers(dict((k, lines[k][j]) for k in FIELDS), temp, press, q_t, q_ref, molar_mass, x_self, T)
    return out


def opacity(lines, temp, press, q_t, q_ref, molar_mass, x_self, cutoff, nu_first, dnu, n_points, T, points=None):
    """kappa in T at the points `points` (indices; None: all) of the grid: the lines in the order of the list"""
    idx = np.arange(n_points) if points is None else np.asarray(points, np.int64)
    p64 = params(lines, temp, press, q_t, q_ref, molar_mass, x_self, np.float64)
    pt = p64 if T is np.float64 else params(lines, temp, press, q_t, q_ref, molar_mass, x_self, T)
    nu64 = np.float64(nu_first) + idx.astype(np.float64) * np.float64(dnu)
    nut = T(nu_first) + idx.astype(T) * T(dnu)
    sigma = np.zeros(len(idx), T)
    for j in range(p64.shape[1]):
        d64 = nu64 - p64[0, j]
        inside = np.abs(d64) <= cutoff                       # the decision: fp64
        if not inside.any():
            continue
        reg = region(p64[2, j] * d64[inside], p64[3, j])
        x = pt[2, j] * (nut[inside] - pt[0, j])
        k = _k_by_region(x, np.full(len(x), pt[3, j], T), reg, T)
        sigma[inside] = sigma[inside] + pt[1, j] * k
    return sigma * T(N_A) / T(molar_mass)


def long_double(lines, temp, press, q_t, q_ref, molar_mass, x_self, cutoff, nu_first, dnu, n_points, points=None):
    return opacity(lines, temp, press, q_t, q_ref, molar_mass, x_self, cutoff, nu_first, dnu, n_points, np.longdouble, points)


def plain_fp64(lines, temp, press, q_t, q_ref, molar_mass, x_self, cutoff, nu_first, dnu, n_points, points=None):
    return opacity(lines, temp, press, q_t, q_ref, molar_mass, x_self, cutoff, nu_first, dnu, n_points, np.float64, points)
