"""What the tests of exomol.py share: writers for `.states`, `.trans`, `.broad` and `.pf` files, synthetic lists built so that the
strength cut keeps a chosen pattern, the case lists, and the two restatements of a node (computed once per process and kept).

The rule is lines_cases.check_rule as it is: every entry lies within max(1e-13, 8 eps) relative of the long-double restatement,
eps being plain_fp64's own deviation at that entry, and zeros are zeros.

A condition on the inputs, asserted by `build`: for no transition of a case with S_min > 0 does the long-double S lie within a
relative 1e-9 of S_min, at any node of the case.  The kept set is then the same in long double, plain fp64, numpy and on the
device, and the tests require it to be identical.

How a pattern is made.  Transition i of the sorted list has a lower state of its own: E'' in 0 ... 500 cm^-1 where it is to be kept,
in 20000 ... 20500 cm^-1 where it is to be culled; at 700 K the Boltzmann factors are 0.36 ... 1 and below 1.5e-18, the strengths
above 5e-25 and below 1e-36, and S_min = 1e-34 stands between.  (At 1500 K a `culled` transition has S above 1e-33 and is kept:
the nodes of one case may keep different sets.)  The lower states come first in the table and the upper states after them, so the
last transition's upper state is the table's last state.
"""
import bz2
import os

import numpy as np

import exomol_reference as er
import lines_cases as lc
from helios_amd import exomol, lines

check_rule = lc.check_rule
M_H2O = lc.M_H2O
q_table = lc.q_table
write_q_file = lc.write_q_file
TILE, BLOCK, B, WAVE = exomol.TILE_POINTS, exomol.LDS_BLOCK, exomol.COMPACT_BLOCK, exomol.WAVEFRONT
DNU, CUTOFF = 0.25, 2.0                       # a tile is TILE / 4 cm^-1 wide, a line reaches 17 points
GRID = (1000.0, DNU, TILE + 1)
S_MIN = 1e-34
CLEAR = 1e-9
J_TOP = 15.5                                  # the largest J of every table: jidx 31 is the broadening table's last row
J_FILE = 9.0                                  # the `.broad` rows end here: J'' beyond takes the broadener's defaults
NODE = (700.0, 1e5)
_kept = {}


# ---- files ---------------------------------------------------------------------------------------------------------------
def _opener(path):
    return (lambda p: bz2.open(p, "wt")) if str(path).endswith(".bz2") else (lambda p: open(p, "w"))


def write_states(path, states, extra_columns=True):
    with _opener(path)(path) as f:
        for k in range(len(states["E"])):
            f.write("%12d %.17g %d %.17g%s\n" % (k + 1, states["E"][k], int(states["g"][k]), states["J"][k],
                                                 "  +  e  A1  %d 0 0" % (k % 7) if extra_columns else ""))
    return path


def write_trans(path, up, low, a, fourth_column=False):
    """ids 0-based here, 1-based in the file"""
    with _opener(path)(path) as f:
        for u, l, v in zip(up, low, a):
            f.write("%12d %12d %.17g%s\n" % (u + 1, l + 1, v, " 1234.567890" if fourth_column else ""))
    return path


def write_broad(path, rows, other_codes=0):
    """rows {jidx: (gamma, n)} as `a0 gamma n J''`; `other_codes` rows of the code a1 in between"""
    with open(path, "w") as f:
        for k, j in enumerate(sorted(rows)):
            if k < other_codes:
                f.write("a1 0.0500 0.300 %7.1f %7.1f\n" % (0.5 * j, 0.5 * j + 1))
            f.write("a0 %.17g %.17g %7.1f\n" % (rows[j][0], rows[j][1], 0.5 * j))
    return path


# ---- cases ---------------------------------------------------------------------------------------------------------------
class Case(object):
    """states, transitions in file order (`raw`: up, low, A, 0-based), broadeners, nodes [(T, P)], S_min, the grid and the cut-off"""

    def __init__(self, label, states, raw, broadeners, nodes, s_min, grid, cutoff, molar_mass=M_H2O):
        self.label, self.states, self.raw, self.broadeners = label, states, raw, broadeners
        self.nodes, self.s_min, self.grid, self.cutoff, self.molar_mass = list(nodes), float(s_min), grid, cutoff, molar_mass
        self.trans, self.skipped = exomol.sort_transitions({"up": raw[0], "low": raw[1], "A": raw[2]}, states)
        self.broadening = exomol.broadening_table(broadeners, int(states["jidx"].max()))
        assert_clear_of_the_cut(self)

    def q(self, temp):
        return lines.partition_value(q_table(), temp)

    def with_s_min(self, s_min):
        return Case(self.label + ", S_min %g" % s_min, self.states, self.raw, self.broadeners, self.nodes, s_min, self.grid, self.cutoff,
                    self.molar_mass)


def assert_clear_of_the_cut(case):
    if case.s_min > 0:
        for temp in sorted(set(n[0] for n in case.nodes)):
            s = er.strengths(case.states, case.trans, temp, case.q(temp), np.longdouble)
            gap = np.abs(s / np.longdouble(case.s_min) - 1)
            assert gap.min() > CLEAR, (case.label, temp, float(gap.min()))


def broad_rows(seed, n_exponent):
    """{jidx: (gamma, n)} for J'' = 0, 1/2, ... J_FILE"""
    rng = np.random.default_rng(seed)
    return dict((j, (float(rng.uniform(0.02, 0.12)), float(n_exponent + rng.uniform(-0.05, 0.05)))) for j in range(int(2 * J_FILE) + 1))


def broadeners(n):
    """n broadeners with different temperature exponents; the first without defaults of its own"""
    all_three = [("H2", 0.85, broad_rows(31, 0.45), 0.07, 0.5), ("He", 0.15, broad_rows(32, 0.25), 0.03, 0.3),
                 ("N2", 0.05, broad_rows(33, 0.7), 0.09, 0.75)]
    return all_three[:n]


def build(label, keep, grid=GRID, cutoff=CUTOFF, seed=1, n_broadeners=1, nodes=(NODE,), s_min=S_MIN, shuffle=True, broadener_list=None,
          log_a=(-2.0, 2.0)):
    """a list of len(keep) transitions; keep[i]: whether transition i of the sorted list is kept at 700 K under S_MIN; A is drawn
    from 10^log_a"""
    keep = np.asarray(keep, bool)
    n = len(keep)
    rng = np.random.default_rng(seed)
    nu_first, dnu, n_points = grid
    nu = np.sort(rng.uniform(nu_first - 1.5 * cutoff, nu_first + (n_points - 1) * dnu + 1.5 * cutoff, n))
    e_low = np.where(keep, rng.uniform(0.0, 500.0, n), rng.uniform(20000.0, 20500.0, n))
    e_up = e_low + nu
    j_low = rng.integers(0, int(2 * J_TOP), n) * 0.5             # whole and half J, some beyond J_FILE
    j_low[rng.integers(0, n)] = J_TOP
    j_up = j_low + 1.0
    states = {"E": np.concatenate([e_low, e_up]), "J": np.concatenate([j_low, j_up]),
              "g": np.concatenate([2 * j_low + 1, 2 * j_up + 1]).round()}
    states["jidx"] = np.round(2 * states["J"]).astype(np.int32)
    states["jidx"][n:] = np.minimum(states["jidx"][n:], int(2 * J_TOP))      # the table's last row is a LOWER state's
    states["J"] = 0.5 * states["jidx"]
    order = rng.permutation(n) if shuffle else np.arange(n)
    raw = ((n + np.arange(n))[order], np.arange(n)[order], (10.0 ** rng.uniform(log_a[0], log_a[1], n))[order])
    case = Case(label, states, raw, broadener_list or broadeners(n_broadeners), nodes, s_min, grid, cutoff)
    assert len(case.trans["nu0"]) == n and int(case.trans["up"][-1]) == 2 * n - 1 and int(states["jidx"].max()) == int(2 * J_TOP)
    return case


def pattern(name, n):
    i = np.arange(n)
    if name == "all":
        return np.ones(n, bool)
    if name == "none":
        return np.zeros(n, bool)
    if name == "first":
        return i == 0
    if name == "last":
        return i == n - 1
    if name == "alternating":
        return i % 2 == 0
    if name == "run across a block boundary":
        return (i >= B - 10) & (i < B + 10)
    if name == "a kept block beside a culled block":
        return (i < B) | (i >= 2 * B)
    raise KeyError(name)


COUNTS = [1, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, 1100]
PATTERNS = ["none", "first", "last", "all", "alternating", "run across a block boundary", "a kept block beside a culled block"]
POINTS = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 37]


def make(label):
    """the case of a label of case_labels(), built once per process"""
    if label not in _kept:
        kind, _, what = label.partition(": ")
        if kind == "count":
            n = int(what)
            _kept[label] = build(label, pattern("alternating" if n > 1 else "all", n), seed=100 + n)
        elif kind == "pattern":
            _kept[label] = build(label, pattern(what, 2 * B + 1), seed=200 + PATTERNS.index(what))
        elif kind == "points":
            n_points = int(what)
            _kept[label] = build(label, pattern("alternating", B + 1), grid=(1000.0, DNU, n_points), seed=300 + n_points)
        elif kind == "broadeners":
            _kept[label] = build(label, pattern("alternating", B + 1), n_broadeners=int(what), seed=400 + int(what),
                                 nodes=[(700.0, 1e5), (1500.0, 1e7)])
        else:
            raise KeyError(label)
    return _kept[label]


def case_labels():
    return (["count: %d" % n for n in COUNTS] + ["pattern: %s" % p for p in PATTERNS] + ["points: %d" % n for n in POINTS]
            + ["broadeners: 2", "broadeners: 3"])


def two_states_case(e_up, cutoff=25.0, grid=(0.0, 0.25, 801)):
    """one transition from E'' = 0 to `e_up`, so nu_0 = e_up to the bit; every transition kept"""
    states = {"E": np.array([0.0, e_up]), "g": np.array([1.0, 3.0]), "J": np.array([0.0, 1.0]), "jidx": np.array([0, 2], np.int32)}
    return Case("nu_0 = %.17g" % e_up, states, (np.array([1]), np.array([0]), np.array([50.0])), broadeners(1), [(300.0, 1e5)], 0.0,
                grid, cutoff)


def tie_case(first_file_first):
    """two pairs of transitions with equal nu_0 from different states, in two `.trans` files; the order of the files decides the
    order of each pair.  Returns the case and the two files' (up, low, A)"""
    e = np.array([100.0, 300.0, 40.0, 1100.0, 1300.0, 1075.0, 1275.0])     # 3 - 0 and 4 - 1: 1000; 5 - 0 and 6 - 1 ... 975
    states = {"E": e, "g": np.array([1.0, 3.0, 5.0, 3.0, 5.0, 3.0, 5.0]), "J": np.array([0.0, 1.0, 2.0, 1.0, 2.0, 1.0, 2.0])}
    states["jidx"] = np.round(2 * states["J"]).astype(np.int32)
    file_a = (np.array([3, 5, 3]), np.array([0, 0, 2]), np.array([2.0, 0.7, 1.1]))
    file_b = (np.array([4, 6]), np.array([1, 1]), np.array([90.0, 35.0]))
    parts = (file_a, file_b) if first_file_first else (file_b, file_a)
    raw = tuple(np.concatenate([p[k] for p in parts]) for k in range(3))
    case = Case("ties, file %s first" % ("a" if first_file_first else "b"), states, raw, broadeners(2), [(500.0, 1e6)], 0.0,
                (950.0, 0.05, TILE + 300), 5.0)
    return case, parts


# ---- the restatements ------------------------------------------------------------------------------------------------------
def restated(case, node):
    """{"ld", "f64": kappa; "params_ld", "params_f64": [4][kept]; "kept": indices in the list} of node `node` of the case, computed
    once per process"""
    key = (id(case), node)
    if key not in _kept:
        temp, press = case.nodes[node]
        args = (case.states, case.trans, case.broadening, temp, press, case.q(temp), case.molar_mass, case.s_min, case.cutoff) + case.grid
        ld, pld, kept = er.long_double(*args)
        f64, pf64, kept64 = er.plain_fp64(*args)
        assert np.array_equal(kept, kept64)
        _kept[key] = {"case": case, "ld": ld, "f64": f64, "params_ld": pld, "params_f64": pf64, "kept": kept}
    return _kept[key]


def write_files(wd, case, name="list"):
    """the case as files; returns (states, trans, [broadener entries as -broadeners takes them], pf)"""
    os.makedirs(wd, exist_ok=True)
    st = write_states(os.path.join(wd, name + ".states"), case.states)
    tr = write_trans(os.path.join(wd, name + ".trans"), *case.raw)
    entries = []
    for b_name, fraction, rows, gamma_d, n_d in case.broadeners:
        path = write_broad(os.path.join(wd, "%s_%s.broad" % (name, b_name)), rows)
        entries.append("%s:%.17g:%s:%.17g:%.17g" % (b_name, fraction, path, gamma_d, n_d))
    pf = os.path.join(wd, name + ".pf")
    write_q_file(pf)
    return st, tr, entries, pf
