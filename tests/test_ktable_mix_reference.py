"""The long-double restatement of the mixing stage (tests/ktable_mix_reference.py) against exact rational arithmetic at a
handful of entries, as tests/test_ktable_reference.py does for the k-table contract: the weighted sum with its mass mixing
ratios, and the water formula, which is + - * / only.  No GPU."""
import numpy as np

import ktable_mix_reference as kr
from helios_amd import ktable_mix


def test_restatement_against_fractions():
    from fractions import Fraction as F
    rng = np.random.default_rng(2)
    nodes, nc, ns = 2, 3, 3
    tables = [10.0 ** rng.uniform(-15, 3, nodes * nc) for _ in range(ns)]
    x, x2, mu = rng.uniform(1e-6, 1, (ns, nodes)), rng.uniform(0.1, 1, (ns, nodes)), rng.uniform(2, 3, nodes)
    w = [18.0153, 44.01, 2.01588]
    mmr = [x[s].astype(kr.LD) * x2[s].astype(kr.LD) * kr.LD(np.float64(w[s])) / mu.astype(kr.LD) for s in range(ns)]
    got = kr.reference_sum(tables, mmr, nodes, nc)
    for node in range(nodes):
        for e in range(nc):
            exact = sum(F(float(x[s, node])) * F(float(x2[s, node])) * F(w[s]) / F(float(mu[node]))
                        * F(float(tables[s][node * nc + e])) for s in range(ns))
            assert abs(F(float(got[node * nc + e])) - exact) <= abs(exact) * F(3, 2 ** 54)       # rounded once (and a bit)
    # the water formula: only + - * /, so the rationals are exact
    wave, temp, press, f = [1.1e-4, 2.5e-4], [300.0, 2000.0], [1e3, 1e7], [1e-12, 1e-3, 0.5, 1.0]
    sig = kr.reference_h2o(wave, temp, press, np.array(f, kr.LD))
    a = [F(float(v)) for v in kr.H2O_A]
    for node in range(4):
        T, P, fr = F(temp[node // 2]), F(press[node % 2]), F(f[node])
        kt = F(ktable_mix.pc.K_B) * T
        delta = fr * P * F(18.0153) * F(ktable_mix.pc.AMU) / kt
        n_ref = fr * P / kt
        for i, lam in enumerate(wave):
            L2 = (F(lam) / F(0.589e-4)) ** 2
            A = delta * (a[0] + a[1] * delta + a[2] * T / F(273.15) + a[3] * L2 * T / F(273.15) + a[4] / L2
                         + a[5] / (L2 - F(0.229202) ** 2) + a[6] / (L2 - F(5.432937) ** 2) + a[7] * delta ** 2)
            exact = 24 * F(float(kr.LD(np.pi))) ** 3 / (n_ref ** 2 * F(lam) ** 4) * A ** 2 * (6 + 3 * F(3e-4)) / (6 - 7 * F(3e-4))
            assert abs(F(float(sig[node, i])) - exact) <= abs(exact) * F(1, 2 ** 50)
    assert np.all(kr.reference_h2o([2.6e-4], temp, press, np.array(f, kr.LD)) == 0)
