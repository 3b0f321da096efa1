"""The long-double restatement tests/mie_reference.py against the arbitrary-precision goldens (tests/golden/mie/reference.npz,
made by tests/golden/make_mie_golden.py with mpmath at 120 digits by another algorithm).  CPU only; mpmath is not imported.

The bound is measured: tools/mie_parity.py writes the restatement's largest deviation per quantity into profiles/mie_parity.json
(`largest.restatement_vs_golden`): 1.36e-16 for Q_ext, 1.05e-16 for Q_sca (relative), 6.62e-17 for g (absolute).  Up to
2^-53 = 1.11e-16 of that is the goldens' own rounding to doubles; the rest, at most 2.5e-17, is the restatement's.  Asserted
is 8 x the measured figure, with a floor of 1e-17.  Long double with the series for psi_n below X_SMALL = 0.5 reaches 1e-15
in every case, the small-x ones included (x = 1e-6 ... 0.5: at most 1.1e-16), so no case has to be excused.
"""
import numpy as np

import mie_cases as mc
import mie_reference

MEASURED = {"q_ext": 1.3600160255428798e-16, "q_sca": 1.0462915501368288e-16, "g": 6.619054263024005e-17}


def test_the_restatement_reaches_every_golden():
    g = mc.goldens()
    ld, _ = mc.restated(g["m_re"], g["m_im"], g["x"])
    dev = mc.deviations(ld, [g["q_ext"], g["q_sca"], g["g"]])
    for q, name in enumerate(mc.NAMES):
        worst = float(dev[q].max())
        print("%s: worst deviation %.3e (x = %g), measured %.3e" % (name, worst, g["x"][int(np.argmax(dev[q]))], MEASURED[name]))
        assert worst <= max(8.0 * MEASURED[name], 1e-17), (name, worst)
        assert worst < 1e-15


def test_the_bound_is_the_one_on_record():
    import json
    import os
    with open(os.path.join(os.path.dirname(mc.HERE), "profiles", "mie_parity.json")) as f:
        rec = json.load(f)
    for name in mc.NAMES:
        assert rec["largest"]["restatement_vs_golden"][name] == MEASURED[name]
        assert rec["asserted_for_the_restatement"][name] == max(8.0 * MEASURED[name], 1e-17)
    assert rec["x_small"] == mie_reference.X_SMALL


def test_the_goldens_hold_the_cases_the_contract_names():
    g = mc.goldens()
    xs = mie_reference.X_SMALL
    wanted = [1e-6, 1e-4, 3e-4, 1e-2, xs * (1 - 1e-9), xs, xs * (1 + 1e-9), 0.055, 1.0, 10.0, 100.0, 1000.0, 3000.0]
    for m in ((1.5, 0.0), (1.33, 1e-5), (1.7, 1e-8), (1.5, 1.0), (0.75, 0.0), (10.0, 10.0)):
        have = g["x"][(g["m_re"] == m[0]) & (g["m_im"] == m[1])]
        top = 1000.0 if m == (10.0, 10.0) else 3000.0
        assert set(x for x in wanted if x <= top) <= set(have.tolist()), m
        assert m == (10.0, 10.0) or have.max() >= 2e4
    # N = floor(x + 4.05 x^(1/3) + 2) is at least 2 for every x > 0: the shortest series there is has two terms
    assert {2, 3} <= set(g["n_terms"].tolist()) and g["n_terms"].min() == 2
    assert [mie_reference.n_terms(float(x)) for x in g["x"]] == g["n_terms"].tolist()


def test_plain_fp64_shows_what_the_series_for_psi_is_for():
    """the recurrences started from sin x and cos x, in fp64, at x = 1e-4 and m = 1.5 + i: Q_sca off by some 1e-8, g of the order
    of -1e-8 where it is 1.6e-9; the series holds both to a few ulps"""
    g = mc.goldens()
    p = int(np.nonzero((g["m_re"] == 1.5) & (g["m_im"] == 1.0) & (g["x"] == 1e-4))[0][0])
    keep = mie_reference.X_SMALL
    try:
        mie_reference.X_SMALL = 0.0
        lossy = mie_reference.plain_fp64(1.5, 1.0, 1e-4)
    finally:
        mie_reference.X_SMALL = keep
    good = mie_reference.plain_fp64(1.5, 1.0, 1e-4)
    print("x = 1e-4, m = 1.5 + i: recurrences Q_sca off by %.2e, g = %.3e; series Q_sca off by %.2e, g = %.3e; golden g = %.3e"
          % (lossy[1] / g["q_sca"][p] - 1, lossy[2], good[1] / g["q_sca"][p] - 1, good[2], g["g"][p]))
    assert abs(lossy[1] / g["q_sca"][p] - 1) > 1e-10
    assert abs(good[1] / g["q_sca"][p] - 1) < 1e-14 and abs(good[2] - g["g"][p]) < 1e-15
