#!/usr/bin/env python3
"""Writes the 40 coefficients of Weideman's rational approximation of w(z) (N = 40, L = sqrt(40 / sqrt 2)) as literals of 17
significant digits, once for the host and once for the device:

    helios_amd/lines_data.py            WEIDEMAN_N, WEIDEMAN_L, WEIDEMAN_A (highest power first, as Horner takes them)
    helios_amd/csrc/lines_weideman.h    the same numbers for csrc/lines.hip

J. A. C. Weideman, SIAM J. Numer. Anal. 31 (1994) 1497: with M = 2 N nodes theta_k = k pi / M, k = -M + 1 ... M - 1,
t_k = L tan(theta_k / 2) and f_k = exp(-t_k^2) (L^2 + t_k^2), the coefficient of Z^(n-1), n = 1 ... N, is
    a_n = 1 / (2 M) sum_k f_k cos(n theta_k),
which is the real part of the FFT in Weideman's listing.  Here the sum is taken as it stands, in mpmath at 60 digits, so the
literals are the correctly rounded doubles.  tests/test_lines_reference.py compares the two files number by number.

    python tools/make_lines_data.py
"""
import os

import mpmath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 40


def coefficients(n_terms=N, digits=60):
    """(L, [a_N ... a_1]) as mpmath numbers"""
    mpmath.mp.dps = digits
    M = 2 * n_terms
    L = mpmath.sqrt(n_terms / mpmath.sqrt(2))
    theta = [k * mpmath.pi / M for k in range(-M + 1, M)]
    f = []
    for th in theta:
        t = L * mpmath.tan(th / 2)
        f.append(mpmath.exp(-t * t) * (L * L + t * t))
    a = [mpmath.fsum(fk * mpmath.cos(n * th) for fk, th in zip(f, theta)) / (2 * M) for n in range(1, n_terms + 1)]
    return L, a[::-1]


def literal(v):
    return "%.16e" % float(v)


def main():
    L, a = coefficients()
    lit = [literal(v) for v in a]
    assert all(float(s) == float(v) for s, v in zip(lit, a))
    note = "made by tools/make_lines_data.py; do not edit"
    with open(os.path.join(ROOT, "helios_amd", "lines_data.py"), "w") as f:
        f.write('"""Weideman\'s rational approximation of w(z), N = 40: the coefficients of Z^39 ... Z^0 (%s)."""\n' % note)
        f.write("WEIDEMAN_N = %d\n" % N)
        f.write("WEIDEMAN_L = %s\n" % literal(L))
        f.write("WEIDEMAN_A = (\n")
        for s in lit:
            f.write("    %s,\n" % s)
        f.write(")\n")
    with open(os.path.join(ROOT, "helios_amd", "csrc", "lines_weideman.h"), "w") as f:
        f.write("// Weideman's rational approximation of w(z), N = 40: the coefficients of Z^39 ... Z^0 (%s)\n" % note)
        f.write("#pragma once\n")
        f.write("#define LINES_WEIDEMAN_N %d\n" % N)
        f.write("#define LINES_WEIDEMAN_L %s\n" % literal(L))
        f.write("#define LINES_WEIDEMAN_A \\\n")
        f.write(", \\\n".join("    %s" % s for s in lit) + "\n")


if __name__ == "__main__":
    main()
