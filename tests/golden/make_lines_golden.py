#!/usr/bin/env python3
"""Writes tests/golden/lines/voigt.npz: K(x, y) = Re w(x + i y), w(z) = exp(-z^2) erfc(-i z), from mpmath at 60 digits, rounded
to fp64.  The file holds the arrays x, y, k and nothing else.

The grid, per y in 1e-8, 1e-6, 1e-3, 1, 1e2, 1e4:
    x = 0 and 60 values evenly spaced in log x from 1e-3 to 1e6 (the sweep the scheme of helios_amd/lines.py was measured on, thinned);
    on both sides of |z| = 6, 6.5, 15 and 100 (6.5, 15 and 100 bound the regions of the scheme; at 6 the continued fraction would
    miss 1e-6, which is why the scheme's first boundary is not there) where y lies below it: the largest x whose fp64 x * x + y * y is still <= |z|^2, the next
    double above it (one ulp apart), and 3 per cent below and above.

    python tests/golden/make_lines_golden.py
"""
import os

import mpmath
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
Y_VALUES = (1e-8, 1e-6, 1e-3, 1.0, 1e2, 1e4)
BOUNDARIES = (6.0, 6.5, 15.0, 100.0)


def last_inside(r, y):
    """the largest double x with x * x + y * y <= r * r in fp64"""
    x = np.sqrt(r * r - y * y)
    while x * x + y * y > r * r:
        x = np.nextafter(x, 0.0)
    while np.nextafter(x, np.inf) ** 2 + y * y <= r * r:
        x = np.nextafter(x, np.inf)
    return float(x)


def grid():
    xs, ys = [], []
    sweep = [0.0] + (10.0 ** np.linspace(-3.0, 6.0, 60)).tolist()
    for y in Y_VALUES:
        row = list(sweep)
        for r in BOUNDARIES:
            if y < r:
                xb = last_inside(r, y)
                row += [xb, float(np.nextafter(xb, np.inf)), 0.97 * xb, 1.03 * xb]
        xs += row
        ys += [y] * len(row)
    return np.array(xs), np.array(ys)


def faddeeva_re(x, y):
    z = mpmath.mpc(mpmath.mpf(float(x)), mpmath.mpf(float(y)))
    return float(mpmath.re(mpmath.exp(-z * z) * mpmath.erfc(-1j * z)))


def main():
    mpmath.mp.dps = 60
    x, y = grid()
    k = np.array([faddeeva_re(a, b) for a, b in zip(x, y)])
    assert np.all(np.isfinite(k)) and np.all(k > 0)
    os.makedirs(os.path.join(HERE, "lines"), exist_ok=True)
    np.savez(os.path.join(HERE, "lines", "voigt.npz"), x=x, y=y, k=k)
    print("%d pairs -> tests/golden/lines/voigt.npz" % len(x))


if __name__ == "__main__":
    main()
