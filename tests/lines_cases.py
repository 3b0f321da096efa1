"""What the tests of lines.py share: the goldens of tests/golden/lines/voigt.npz, synthetic line lists and their `.par` records, a
partition function, the two restatements of a node (computed once per process and kept), and the tolerance rule.

The rule.  Every entry of the backend under test lies within max(1e-13, 8 eps) relative of the long-double restatement, where
eps is `plain_fp64`'s own relative deviation from it at that entry.  Where the restatement is 0 (no line in reach) the entry is 0.
"""
import os

import numpy as np

import lines_reference as lr

HERE = os.path.dirname(os.path.abspath(__file__))
FLOOR = 1e-13
MARGIN = 8.0
GOLDEN_BOUND = 1e-6               # the restatement and the kernel against mpmath, everywhere
GOLDEN_BOUND_OUTER = 1e-9         # in the two outer regions
M_H2O = 18.0153
_kept = {}


def goldens():
    if "golden" not in _kept:
        with np.load(os.path.join(HERE, "golden", "lines", "voigt.npz")) as f:
            _kept["golden"] = {k: f[k] for k in f.files}
    return _kept["golden"]


def q_table():
    """Q(T) = T^1.5 on 50, 100, ... 3000 K: 296 K lies between two rows"""
    t = np.arange(50.0, 3001.0, 50.0)
    return t, t ** 1.5


def write_q_file(path, table=None):
    t, q = q_table() if table is None else table
    with open(path, "w") as f:
        f.write("# T [K]  Q(T)\n")
        for row in zip(t, q):
            f.write("%.17g %.17g\n" % row)


def synthetic_lines(n, lo, hi, seed=1, delta=0.01):
    """n lines with nu_0 drawn evenly from lo ... hi, as the seven sorted arrays"""
    rng = np.random.default_rng(seed)
    return dict(nu0=np.sort(rng.uniform(lo, hi, n)), s_ref=10.0 ** rng.uniform(-26.0, -20.0, n), gamma_air=rng.uniform(0.01, 0.1, n),
                gamma_self=rng.uniform(0.1, 0.5, n), e_low=rng.uniform(0.0, 3000.0, n), n_air=rng.uniform(0.4, 0.8, n),
                delta_air=rng.uniform(-delta, delta, n))


def one_line(nu0, s_ref=1e-20, gamma_air=0.07, gamma_self=0.35, e_low=500.0, n_air=0.7, delta_air=0.0):
    return dict(nu0=np.array([nu0]), s_ref=np.array([s_ref]), gamma_air=np.array([gamma_air]), gamma_self=np.array([gamma_self]),
                e_low=np.array([e_low]), n_air=np.array([n_air]), delta_air=np.array([delta_air]))


def join(*lists):
    """several lists as one, sorted by (nu_0, position)"""
    arr = dict((k, np.concatenate([l[k] for l in lists])) for k in lr.FIELDS)
    order = np.argsort(arr["nu0"], kind="stable")
    return dict((k, arr[k][order]) for k in lr.FIELDS)


def parent_bit_cases():
    """the cases of tests/golden/lines/parent_bits.npz, data only: per case the list, the nodes (T, P), x_self, the cut-off,
    the grid, what the handle holds beyond the list and the grid, and the nodes per launch.  Case 4 is a call of
    lines.line_opacity and brings `temps` and `press` in place of nodes"""
    from helios_amd.lines import ATM, LDS_BLOCK, TILE_POINTS
    nu0, dnu = 1000.0, 0.25
    n2 = TILE_POINTS + 1
    spread = synthetic_lines(LDS_BLOCK + 1, nu0 + 0.02 * TILE_POINTS * dnu, nu0 + 0.98 * TILE_POINTS * dnu, seed=n2)
    last = nu0 + TILE_POINTS * dnu
    far = one_line(last + 25.0 + 5.0, s_ref=1e-19, delta_air=-0.01)
    return [
        dict(name="case1", line=one_line(100.0), nodes=[(300.0, 1e5)], x_self=0.0, cutoff=25.0, grid=(100.0, 0.25, 1),
             more_lines=0, more_points=0, per_launch=1),
        dict(name="case2", line=join(spread, synthetic_lines(40, nu0, nu0 + n2 * dnu, seed=5)),
             nodes=[(300.0, 1e3), (900.0, 1e6), (1500.0, 1e3)], x_self=0.25, cutoff=2.0, grid=(nu0, dnu, n2),
             more_lines=5, more_points=3, per_launch=2),
        dict(name="case3", line=join(synthetic_lines(LDS_BLOCK + 30, nu0, last - 60.0, seed=12), far),
             nodes=[(300.0, 1e-4), (300.0, 1e3 * ATM), (1200.0, 1e5)], x_self=0.1, cutoff=25.0, grid=(nu0, dnu, n2),
             more_lines=0, more_points=0, per_launch=3),
        dict(name="case4", line=synthetic_lines(60, 995.0, 1030.0, seed=15), temps=[300.0, 1200.0], press=[1e2, 1e7], x_self=0.1,
             cutoff=5.0, grid=(1000.0, 0.05, 500)),
    ]


def parent_bits():
    if "parent_bits" not in _kept:
        with np.load(os.path.join(HERE, "golden", "lines", "parent_bits.npz")) as f:
            _kept["parent_bits"] = {k: f[k] for k in f.files}
    return _kept["parent_bits"]


def _fit(fmt, width, v):
    s = fmt % v
    if len(s) > width and s.startswith("0."):
        s = s[1:]
    elif len(s) > width and s.startswith("-0."):
        s = "-" + s[2:]
    assert len(s) <= width, (fmt, width, v, s)
    return s.rjust(width)


def par_record(line, j, molecule=1, isotopologue=1):
    """line j as a 160-character HITRAN record"""
    rec = "%2d%1s" % (molecule, isotopologue)
    rec += _fit("%.6f", 12, line["nu0"][j]) + _fit("%.3e", 10, line["s_ref"][j]) + _fit("%.3e", 10, 1.0)
    rec += _fit("%.4f", 5, line["gamma_air"][j]) + _fit("%.3f", 5, line["gamma_self"][j]) + _fit("%.4f", 10, line["e_low"][j])
    rec += _fit("%.2f", 4, line["n_air"][j]) + _fit("%.6f", 8, line["delta_air"][j])
    assert len(rec) == 67
    return rec.ljust(160)


def write_par_file(path, line, isotopologues=None):
    with open(path, "w") as f:
        for j in range(len(line["nu0"])):
            f.write(par_record(line, j, isotopologue=1 if isotopologues is None else isotopologues[j]) + "\n")


def restated(lines, temp, press, x_self, cutoff, nu_first, dnu, n_points, molar_mass=M_H2O, points=None):
    """(long double, plain_fp64) kappa of one node under q_table(); a node is computed once per process"""
    key = (tuple(np.concatenate([lines[k] for k in lr.FIELDS]).tolist()), temp, press, x_self, cutoff, nu_first, dnu, n_points,
           molar_mass, None if points is None else tuple(points))
    if key not in _kept:
        from helios_amd.lines import partition_value
        q_t, q_ref = partition_value(q_table(), temp), partition_value(q_table(), lr.T_REF)
        args = (lines, temp, press, q_t, q_ref, molar_mass, x_self, cutoff, nu_first, dnu, n_points)
        _kept[key] = (lr.long_double(*args, points=points), lr.plain_fp64(*args, points=points))
    return _kept[key]


def restated_params(lines, temp, press, x_self, molar_mass=M_H2O):
    from helios_amd.lines import partition_value
    q_t, q_ref = partition_value(q_table(), temp), partition_value(q_table(), lr.T_REF)
    return (lr.params(lines, temp, press, q_t, q_ref, molar_mass, x_self, np.longdouble),
            lr.params(lines, temp, press, q_t, q_ref, molar_mass, x_self, np.float64))


def check_rule(values, ld, f64, label=""):
    """holds `values` to the rule against the restatements `ld`, `f64`; prints the figures before it asserts"""
    v = np.asarray(values, np.float64).reshape(-1)
    ld = np.asarray(ld, np.longdouble).reshape(-1)
    f64 = np.asarray(f64, np.float64).reshape(-1)
    assert v.shape == ld.shape == f64.shape
    assert np.all(np.isfinite(v)), label
    zero = ld == 0
    assert np.all(v[zero] == 0.0), (label, "entries without a line in reach are 0")
    scale = np.where(zero, 1.0, np.abs(ld))
    dev = (np.abs(v - ld) / scale).astype(np.float64)
    eps = (np.abs(f64 - ld) / scale).astype(np.float64)
    bound = np.maximum(FLOOR, MARGIN * eps)
    worst = int(np.argmax(dev / bound)) if len(dev) else 0
    print("%s: %d entries, worst deviation %.3e (largest of all %.3e), plain_fp64's there %.3e (largest %.3e), bound there %.3e"
          % (label, len(v), dev[worst], dev.max(), eps[worst], eps.max(), bound[worst]))
    bad = np.nonzero(~(dev <= bound))[0]
    assert len(bad) == 0, (label, len(bad), [(int(p), float(dev[p]), float(bound[p])) for p in bad[:5]])
    return float(dev.max())
