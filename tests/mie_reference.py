"""The Lorenz-Mie contract of helios_amd/mie.py, restated one pair at a time in plain statements: `long_double(...)` in
np.longdouble (the checker of both backends), `plain_fp64(...)` the same statements in fp64 (the yardstick of what fp64 can
hold).  No vectorisation, no tricks; the constants are restated, and tests/test_mie.py holds them to the module's.

Per pair (x, m = m_re + i m_im), with z = m x and N = floor(x + 4.05 x^(1/3) + 2):
  D_N(z)      the logarithmic derivative of psi_N, from Lentz's continued fraction of J_{N-1/2}(z) / J_{N+1/2}(z)
  D_{n-1}     = n/z - 1 / (D_n + n/z), downward
  psi, chi    upward from sin x, cos x; for x < X_SMALL every psi_n (n >= 1) comes from its ascending series instead, which has
              no cancellation (the recurrence loses 3 eps / x^2 of psi_1: it is the difference of two numbers near 1)
  a_n, b_n    Bohren & Huffman (4.88), and the three sums of the contract; the term of g that needs a_{N+1} is dropped
Complex arithmetic is written out on pairs of reals; no function of the complex z is taken.
"""
import math
import sys

import numpy as np

X_SMALL = 0.5            # below it: psi_n by series
SERIES_TERMS = 10        # x^20 / (2^10 10! 23!!) relative: < 1e-23 at x = 0.5
LENTZ_TOL_EPS = 16       # the continued fraction stops when |C D - 1| (1-norm) < 16 eps of the number format
TINY = 1e-30


def n_terms(x):
    return int(math.floor(x + 4.05 * x ** (1.0 / 3.0) + 2.0))


def lentz_cap(m_re, m_im, x):
    zabs = math.sqrt(m_re * m_re + m_im * m_im) * x
    return int(zabs + 4.05 * zabs ** (1.0 / 3.0)) + 100


def _crec(br, bi):
    d = br * br + bi * bi
    return br / d, -bi / d


def _cmul(ar, ai, br, bi):
    return ar * br - ai * bi, ar * bi + ai * br


def _cdiv(ar, ai, br, bi):
    d = br * br + bi * bi
    return (ar * br + ai * bi) / d, (ai * br - ar * bi) / d


def psi_series(n, x, T):
    s = T(1.0)
    x2 = x * x
    for k in range(SERIES_TERMS, 0, -1):
        s = T(1.0) - x2 / T(2 * k * (2 * n + 2 * k + 1)) * s
    pref = x
    for j in range(1, n + 1):
        pref = pref * x / T(2 * j + 1)
    return pref * s


def d_start(N, zinv_r, zinv_i, cap, T, eps):
    """D_N(z) by the modified Lentz algorithm: J_{nu-1}(z) / J_nu(z) = a_1 + 1 / (a_2 + 1 / (a_3 + ...)) with nu = N + 1/2 and
    a_k = (-1)^(k+1) (2 N + 2 k - 1) / z"""
    tol = T(LENTZ_TOL_EPS) * eps
    tiny = T(TINY)
    one, zero = T(1.0), T(0.0)
    c = T(2 * N + 1)
    fr, fi = c * zinv_r, c * zinv_i
    if fr == zero and fi == zero:
        fr = tiny
    Cr, Ci, Dr, Di = fr, fi, zero, zero
    k, sign = 2, -1
    while True:
        c = T(sign * (2 * N + 2 * k - 1))
        ar, ai = c * zinv_r, c * zinv_i
        Dr, Di = ar + Dr, ai + Di
        if Dr == zero and Di == zero:
            Dr = tiny
        Dr, Di = _crec(Dr, Di)
        tr, ti = _crec(Cr, Ci)
        Cr, Ci = ar + tr, ai + ti
        if Cr == zero and Ci == zero:
            Cr = tiny
        dr, di = _cmul(Cr, Ci, Dr, Di)
        fr, fi = _cmul(fr, fi, dr, di)
        if abs(dr - one) + abs(di) < tol or k >= cap:
            break
        k, sign = k + 1, -sign
    c = T(N)
    return fr - c * zinv_r, fi - c * zinv_i


def mie_pair(m_re, m_im, x, T, eps, sin, cos):
    """(Q_ext, Q_sca, g) of one pair in the number format T"""
    x, mr, mi = T(x), T(m_re), T(m_im)
    N = n_terms(float(x))
    zr, zi = mr * x, mi * x
    zinv_r, zinv_i = _crec(zr, zi)
    minv_r, minv_i = _crec(mr, mi)
    D = [None] * (N + 1)
    D[N] = d_start(N, zinv_r, zinv_i, lentz_cap(float(m_re), float(m_im), float(x)), T, eps)
    for n in range(N, 1, -1):
        c = T(n)
        tr, ti = c * zinv_r, c * zinv_i
        ir, ii = _crec(D[n][0] + tr, D[n][1] + ti)
        D[n - 1] = (tr - ir, ti - ii)
    small = float(x) < X_SMALL
    sx, cx = sin(x), cos(x)
    psi0, chi0 = sx, cx
    psi1 = psi_series(1, x, T) if small else sx / x - cx
    chi1 = cx / x + sx
    s_ext = s_sca = s_g = T(0.0)
    a_pr = a_pi = b_pr = b_pi = T(0.0)
    for n in range(1, N + 1):
        if n >= 2:
            c = T(2 * n - 1) / x
            psi = psi_series(n, x, T) if small else c * psi1 - psi0
            chi = c * chi1 - chi0
            psi0, psi1, chi0, chi1 = psi1, psi, chi1, chi
        nx = T(n) / x
        dr, di = D[n]
        ur, ui = _cmul(dr, di, minv_r, minv_i)          # D / m + n / x
        ur = ur + nx
        ar, ai = _cdiv(ur * psi1 - psi0, ui * psi1, ur * psi1 + ui * chi1 - psi0, ui * psi1 - ur * chi1 + chi0)
        ur, ui = _cmul(mr, mi, dr, di)                  # m D + n / x
        ur = ur + nx
        br, bi = _cdiv(ur * psi1 - psi0, ui * psi1, ur * psi1 + ui * chi1 - psi0, ui * psi1 - ur * chi1 + chi0)
        f = T(2 * n + 1)
        s_ext = s_ext + f * (ar + br)
        s_sca = s_sca + f * ((ar * ar + ai * ai) + (br * br + bi * bi))
        if n >= 2:
            s_g = s_g + T((n - 1) * (n + 1)) / T(n) * ((a_pr * ar + a_pi * ai) + (b_pr * br + b_pi * bi))
        s_g = s_g + f / T(n * (n + 1)) * (ar * br + ai * bi)
        a_pr, a_pi, b_pr, b_pi = ar, ai, br, bi
    two = T(2.0)
    q = two / (x * x)
    return q * s_ext, q * s_sca, two * s_g / s_sca


def long_double(m_re, m_im, x):
    return mie_pair(m_re, m_im, x, np.longdouble, np.finfo(np.longdouble).eps, np.sin, np.cos)


def plain_fp64(m_re, m_im, x):
    return mie_pair(m_re, m_im, x, float, sys.float_info.epsilon, math.sin, math.cos)
