"""The ExoMol contract of helios_amd/exomol.py, restated in plain statements, one transition at a time and elementwise over the
spectral points it is asked for: `long_double(...)` in np.longdouble (the checker of both backends), `plain_fp64(...)` the same
statements in fp64 (the yardstick of what fp64 can hold).  The constants, K and its regions are tests/lines_reference.py's.

The inputs are fp64 numbers, nu_0 = E[up] - E[low] among them (one fp64 subtraction, done before any restatement).  What the
contract DECIDES on a point -- whether it lies within the cut-off of a line, and the region of |z| -- is decided on the fp64 values
in both restatements, as in lines_reference.  The strength cut is decided by each restatement on its own S; the cases keep every
S a relative 1e-9 away from S_min (exomol_cases.assert_clear_of_the_cut), so the kept set is one set.

Per transition and node, every statement left to right, c2 = H C / K_B, P_bar = P / 1e6:
    pre    = g[up] * A / (8 * pi * C * nu_0 * nu_0)
    S      = pre * exp(-c2 * E[low] / T) * (-expm1(-c2 * nu_0 / T)) / Q(T)
    gamma  = P_bar * sum_b x_b * gamma_b[jidx[low]] * (296 / T)^n_b[jidx[low]]          the sum starts from 0, b in the order given
    alpha  = (nu_0 / C) * sqrt(2 * ln 2 * N_A * K_B * T / M),  a = sqrt(ln 2) / alpha,  y = max(a * gamma, 1e-8),  s = S * a / sqrt pi
kept iff S >= S_min; the sum over the kept transitions in list order is lines_reference's.
"""
import numpy as np

import lines_reference as lr

BAR = 1.0e6


def pi(T):
    return np.float64(np.pi) if T is np.float64 else T(4.0) * np.arctan(T(1.0))


def strength(g_up, a_coef, e_low, nu0, temp, q_t, T):
    """S(T) of one transition in T"""
    c2 = T(lr.H) * T(lr.C) / T(lr.K_B)
    g_up, a_coef, e_low, nu0, temp, q_t = T(g_up), T(a_coef), T(e_low), T(nu0), T(temp), T(q_t)
    pre = g_up * a_coef / (T(8.0) * pi(T) * T(lr.C) * nu0 * nu0)
    with np.errstate(under="ignore"):
        return pre * np.exp(-c2 * e_low / temp) * (-np.expm1(-c2 * nu0 / temp)) / q_t


def strengths(states, trans, temp, q_t, T):
    """S per transition of the sorted list, in T"""
    n = len(trans["nu0"])
    out = np.empty(n, T)
    for j in range(n):
        up, low = int(trans["up"][j]), int(trans["low"][j])
        out[j] = strength(states["g"][up], trans["A"][j], states["E"][low], trans["nu0"][j], temp, q_t, T)
    return out


def transition_numbers(s, nu0, jx, broadening, temp, press, molar_mass, T):
    """(nu_0, s, a, y) of one transition of strength `s` (in T) and lower-state index jx"""
    ln2, inv_sqrt_pi = lr.constants(T)
    x, table = broadening
    nu0, temp, molar_mass = T(nu0), T(temp), T(molar_mass)
    pbar = T(press) / T(BAR)
    total = T(0.0)
    for b in range(len(x)):
        total = total + T(x[b]) * T(table[b, jx, 0]) * (T(lr.T_REF) / temp) ** T(table[b, jx, 1])
    gamma = pbar * total
    alpha = (nu0 / T(lr.C)) * np.sqrt(T(2.0) * ln2 * T(lr.N_A) * T(lr.K_B) * temp / molar_mass)
    a = np.sqrt(ln2) / alpha
    y = max(a * gamma, T(lr.Y_MIN))
    return nu0, s * a * inv_sqrt_pi, a, y


def params(states, trans, broadening, temp, press, q_t, molar_mass, s_min, T):
    """([4][kept] in T, the kept transitions' indices in the list, S of every transition in T)"""
    s_all = strengths(states, trans, temp, q_t, T)
    kept = np.nonzero(s_all >= T(s_min))[0]
    out = np.empty((4, len(kept)), T)
    for k, j in enumerate(kept):
        jx = int(states["jidx"][int(trans["low"][j])])
        out[:, k] = transition_numbers(s_all[j], trans["nu0"][j], jx, broadening, temp, press, molar_mass, T)
    return out, kept, s_all


def sum_over(p64, pt, cutoff, nu_first, dnu, n_points, molar_mass, T, points=None):
    """lines_reference.opacity's sum over prepared numbers: `p64` decides, `pt` computes"""
    idx = np.arange(n_points) if points is None else np.asarray(points, np.int64)
    nu64 = np.float64(nu_first) + idx.astype(np.float64) * np.float64(dnu)
    nut = T(nu_first) + idx.astype(T) * T(dnu)
    sigma = np.zeros(len(idx), T)
    for j in range(p64.shape[1]):
        d64 = nu64 - p64[0, j]
        inside = np.abs(d64) <= cutoff
        if not inside.any():
            continue
        reg = lr.region(p64[2, j] * d64[inside], p64[3, j])
        x = pt[2, j] * (nut[inside] - pt[0, j])
        k = lr._k_by_region(x, np.full(len(x), pt[3, j], T), reg, T)
        sigma[inside] = sigma[inside] + pt[1, j] * k
    return sigma * T(lr.N_A) / T(molar_mass)


def opacity(states, trans, broadening, temp, press, q_t, molar_mass, s_min, cutoff, nu_first, dnu, n_points, T, points=None):
    """(kappa in T, params [4][kept] in T, kept indices)"""
    p64, kept64, _ = params(states, trans, broadening, temp, press, q_t, molar_mass, s_min, np.float64)
    if T is np.float64:
        pt, kept = p64, kept64
    else:
        pt, kept, _ = params(states, trans, broadening, temp, press, q_t, molar_mass, s_min, T)
        assert np.array_equal(kept, kept64), "the cases keep S clear of S_min: one kept set"
    return sum_over(p64, pt, cutoff, nu_first, dnu, n_points, molar_mass, T, points), pt, kept


def long_double(*args, **kw):
    return opacity(*args, T=np.longdouble, **kw)


def plain_fp64(*args, **kw):
    return opacity(*args, T=np.float64, **kw)
