"""What the Mie tests share: the goldens of tests/golden/mie/reference.npz, the long-double restatement and `plain_fp64` over a
table of pairs (computed once per process and kept), and the tolerance rule of the backends.

The rule.  Within one test's table, eps_q is the largest deviation of `plain_fp64` from the long-double restatement for quantity
q over that table.  Every entry of the backend under test lies within max(1e-13, 8 eps_q) of the restatement: relative for Q_ext
and Q_sca, absolute for g.  In the small-x cases (x <= X_SMALL (1 + 1e-9)) the backend is held to the goldens directly, with
1 ulp of the golden in place of plain_fp64's deviation.  The margin of 8 covers a different but equally long order of the same
rounded operations.
"""
import os

import numpy as np

import mie_reference

HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 1e-13
MARGIN = 8.0
NAMES = ("q_ext", "q_sca", "g")
_kept = {}


def goldens():
    if "golden" not in _kept:
        with np.load(os.path.join(HERE, "golden", "mie", "reference.npz")) as f:
            _kept["golden"] = {k: f[k] for k in f.files}
    return _kept["golden"]


def small_x(x):
    return np.asarray(x) <= mie_reference.X_SMALL * (1 + 1e-9)


def restated(m_re, m_im, x):
    """(long double [3][P] as np.longdouble, plain_fp64 [3][P]) of the pairs; a pair is computed once per process"""
    ld = np.empty((3, len(x)), np.longdouble)
    f64 = np.empty((3, len(x)), np.float64)
    for p, key in enumerate(zip(np.asarray(m_re, np.float64).tolist(), np.asarray(m_im, np.float64).tolist(),
                                np.asarray(x, np.float64).tolist())):
        if key not in _kept:
            _kept[key] = (mie_reference.long_double(*key), mie_reference.plain_fp64(*key))
        ld[:, p], f64[:, p] = _kept[key]
    return ld, f64


def deviations(values, reference):
    """[3][P] in long double: relative for Q_ext and Q_sca, absolute for g"""
    v = np.asarray(values, np.longdouble).reshape(3, -1)
    r = np.asarray(reference, np.longdouble).reshape(3, -1)
    d = np.abs(v - r)
    d[:2] = d[:2] / np.abs(r[:2])
    return d


def bounds(ld, f64):
    """max(1e-13, 8 eps_q) per quantity for one table"""
    eps = deviations(f64, ld).max(axis=1)
    return np.maximum(FLOOR, MARGIN * eps.astype(np.float64)), eps.astype(np.float64)


def check_backend(values, m_re, m_im, x, golden=None, label="", report=None):
    """holds `values` = (q_ext, q_sca, g) of a backend to the rule; `golden`: (q_ext, q_sca, g) for the table's small-x cases
    (those pairs are then held to them instead of the restatement).  Prints each figure before it asserts"""
    x = np.asarray(x, np.float64)
    ld, f64 = restated(m_re, m_im, x)
    bound, eps = bounds(ld, f64)
    dev = deviations(values, ld)
    if golden is not None:
        sm = small_x(x)
        if sm.any():
            gd = deviations(np.asarray(values).reshape(3, -1)[:, sm], np.asarray(golden, np.float64).reshape(3, -1)[:, sm])
            dev[:, sm] = gd
            ulp = np.spacing(np.abs(np.asarray(golden, np.float64).reshape(3, -1)[:, sm]))
            ulp[:2] = ulp[:2] / np.abs(np.asarray(golden, np.float64).reshape(3, -1)[:2, sm])
            assert MARGIN * ulp.max() <= FLOOR           # the small-x bound is the floor
    worst = dev.max(axis=1).astype(np.float64)
    for q in range(3):
        print("%s %s: worst deviation %.3e at pair %d, plain_fp64's %.3e, bound %.3e"
              % (label, NAMES[q], worst[q], int(np.argmax(dev[q])), eps[q], bound[q]))
    if report is not None:
        report.update({NAMES[q]: {"worst": worst[q], "plain_fp64": eps[q], "bound": bound[q]} for q in range(3)})
    assert np.all(np.isfinite(np.asarray(values, np.float64)))
    for q in range(3):
        limit = np.full(len(x), bound[q])
        if golden is not None:
            limit[small_x(x)] = FLOOR
        bad = np.nonzero(~(dev[q] <= limit))[0]
        assert len(bad) == 0, (label, NAMES[q], [(float(x[p]), float(dev[q][p]), float(limit[p])) for p in bad[:5]])
    return worst


def smooth_material(lam_um):
    """a smooth synthetic n(lambda), k(lambda): a silicate-like band near 10 micron on a slowly falling index"""
    l = np.asarray(lam_um, np.float64)
    n = 1.6 - 0.1 * np.log10(l) + 0.4 * np.exp(-0.5 * (np.log10(l / 12.0) / 0.15) ** 2)
    k = 1e-3 + 0.8 * np.exp(-0.5 * (np.log10(l / 10.0) / 0.12) ** 2) + 0.05 * (l / 250.0)
    return n, k


def write_nk_file(path, lam, n, k, header=()):
    with open(path, "w") as f:
        for h in header:
            f.write(h + "\n")
        f.write("# wavelength[micron] n k\n")
        for row in zip(lam, n, k):
            f.write("%.17g %.17g %.17g\n" % row)
