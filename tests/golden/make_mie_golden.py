"""Writes tests/golden/mie/reference.npz: Q_ext, Q_sca and g of the truncated Lorenz-Mie series of helios_amd/mie.py's contract,
evaluated with mpmath at 120 digits and rounded to doubles.  Run by hand where mpmath is installed; no test imports it.

    python tests/golden/make_mie_golden.py

The algorithm is not the fp64 one: D_n(z) comes from the downward recurrence started at 0 far above max(N, |z|) (the fp64 code
starts at N from Lentz's continued fraction), psi_n and chi_n from the upward recurrences at 120 digits (which lose some
twenty of them at most) with no small-x branch.  Before anything is written the recurrences are held to mpmath.besselj and
mpmath.bessely at small orders, and D_n(z) to the ratio of two besselj.
"""
import math
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 120
X_SMALL = 0.5
XS = [1e-6, 1e-4, 3e-4, 1e-2, X_SMALL * (1 - 1e-9), X_SMALL, X_SMALL * (1 + 1e-9), 0.055, 1.0, 10.0, 100.0, 1000.0, 3000.0,
      20944.0]
MS = [(1.5, 0.0), (1.33, 1e-5), (1.7, 1e-8), (1.5, 1.0), (0.75, 0.0), (10.0, 10.0)]
X_TOP = {(10.0, 10.0): 1000.0}


def n_terms(x):
    return int(math.floor(x + 4.05 * x ** (1.0 / 3.0) + 2.0))


def log_derivatives(z, N):
    start = int(1.2 * max(N, float(abs(z)))) + 300
    d = mp.mpc(0)
    out = [None] * (N + 1)
    for n in range(start, 0, -1):
        d = n / z - 1 / (d + n / z)
        if n - 1 <= N:
            out[n - 1] = d
    return out


def riccati(x, N):
    psi, chi = [mp.sin(x), mp.sin(x) / x - mp.cos(x)], [mp.cos(x), mp.cos(x) / x + mp.sin(x)]
    for n in range(2, N + 1):
        psi.append((2 * n - 1) / x * psi[n - 1] - psi[n - 2])
        chi.append((2 * n - 1) / x * chi[n - 1] - chi[n - 2])
    return psi, chi


def series(m_re, m_im, x):
    """the doubles are taken as they are: x and m are the exact values of the fp64 inputs"""
    x, m = mp.mpf(x), mp.mpc(mp.mpf(m_re), mp.mpf(m_im))
    N = n_terms(float(x))
    D = log_derivatives(m * x, N)
    psi, chi = riccati(x, N)
    a, b = [None], [None]
    for n in range(1, N + 1):
        xi_n, xi_p = mp.mpc(psi[n], -chi[n]), mp.mpc(psi[n - 1], -chi[n - 1])
        u = D[n] / m + n / x
        a.append((u * psi[n] - psi[n - 1]) / (u * xi_n - xi_p))
        u = m * D[n] + n / x
        b.append((u * psi[n] - psi[n - 1]) / (u * xi_n - xi_p))
    a.append(mp.mpc(0))
    b.append(mp.mpc(0))
    s_ext = sum((2 * n + 1) * (a[n] + b[n]).real for n in range(1, N + 1))
    s_sca = sum((2 * n + 1) * (abs(a[n]) ** 2 + abs(b[n]) ** 2) for n in range(1, N + 1))
    s_g = sum(mp.mpf(n * (n + 2)) / (n + 1) * (a[n] * mp.conj(a[n + 1]) + b[n] * mp.conj(b[n + 1])).real
              + mp.mpf(2 * n + 1) / (n * (n + 1)) * (a[n] * mp.conj(b[n])).real for n in range(1, N + 1))
    q_ext, q_sca = 2 / x ** 2 * s_ext, 2 / x ** 2 * s_sca
    return N, float(q_ext), float(q_sca), float(4 / (x ** 2 * q_sca) * s_g)


def cross_check():
    """psi_n = sqrt(pi x / 2) J_{n + 1/2}(x), chi_n = -sqrt(pi x / 2) Y_{n + 1/2}(x), D_n(z) = J_{n - 1/2}(z) / J_{n + 1/2}(z) - n / z"""
    worst = mp.mpf(0)
    for x in (mp.mpf("1e-4"), mp.mpf("0.1"), mp.mpf(1), mp.mpf("7.5"), mp.mpf(40)):
        top = min(6, n_terms(float(x)))            # the orders the series uses at this x
        psi, chi = riccati(x, top)
        for n in range(0, top + 1):
            f = mp.sqrt(mp.pi * x / 2)
            worst = max(worst, abs(psi[n] / (f * mp.besselj(n + 0.5, x)) - 1), abs(chi[n] / (-f * mp.bessely(n + 0.5, x)) - 1))
    for z in (mp.mpc("1.5e-4", 0), mp.mpc(1.5, 1), mp.mpc(13.3, 1e-4), mp.mpc(30, 30), mp.mpc(7.5, 0)):
        D = log_derivatives(z, 6)
        for n in range(1, 7):
            ref = mp.besselj(n - 0.5, z) / mp.besselj(n + 0.5, z) - n / z
            worst = max(worst, abs(D[n] / ref - 1))
    assert worst < mp.mpf(10) ** -80, worst
    return worst


def main():
    print("cross-check against besselj / bessely: worst relative deviation %s" % mp.nstr(cross_check(), 3))
    rows = []
    for m_re, m_im in MS:
        for x in XS:
            if x > X_TOP.get((m_re, m_im), 1e99):
                continue
            N, q_ext, q_sca, g = series(m_re, m_im, x)
            rows.append((m_re, m_im, x, N, q_ext, q_sca, g))
            print("m = %g + %g i  x = %.17g  N = %d  Q_ext = %.17g  Q_sca = %.17g  g = %.17g" % rows[-1])
    rows = np.array(rows, np.float64)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mie")
    os.makedirs(out, exist_ok=True)
    np.savez(os.path.join(out, "reference.npz"), m_re=rows[:, 0], m_im=rows[:, 1], x=rows[:, 2], n_terms=rows[:, 3].astype(np.int32),
             q_ext=rows[:, 4], q_sca=rows[:, 5], g=rows[:, 6])


if __name__ == "__main__":
    main()
