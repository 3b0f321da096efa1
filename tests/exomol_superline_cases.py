"""What the super-line tests of exomol.py share: lists laid out cell by cell with a chosen class per transition, and the two
restatements of a node (tests/exomol_superline_reference.py), computed once per process and kept.  The rule is
exomol_cases.check_rule: within max(1e-13, 8 eps) of the long-double restatement, eps plain_fp64's own deviation; zeros are zeros.

A layout is a list of (cell, classes): `cell` the whole number floor(nu_0 / d) of the transitions, `classes` one letter per
transition in list order.  At 700 K, with S_MIN = 1e-34 and S_SL = 1e-23:
    s  strong   E'' in 0 ... 500 cm^-1, A in 10 ... 100 s^-1:        S above 1e-22
    w  weak     E'' in 0 ... 500 cm^-1, A in 1e-4 ... 1e-3 s^-1:     S between 1e-28 and 1e-24
    d  dropped  E'' in 20000 ... 20500 cm^-1:                       S below 1e-36 (above 1e-33 at 1500 K, where it is weak)
    z  zero     E'' = 6e6 cm^-1: exp underflows to 0 in fp64 and in long double; kept, and weak, only under S_min = 0
    m  moving   E'' in 8000 ... 9000 cm^-1, A such that S is S_SL / 100 or less at 700 K and 100 S_SL or more at 2500 K: weak in the
                cold node and strong in the hot one
nu_0 lies at (cell + u) d with u ascending inside 0.1 ... 0.9, so no nu_0 / d comes near a whole number; `centred` puts every
transition on its cell's centre with whole-numbered E'', so that nu_0 = (cell + 0.5) d to the bit for d = 0.25.
"""
import numpy as np

import exomol_cases as ec
import exomol_superline_reference as sr
from helios_amd import exomol

TILE, B, WAVE = ec.TILE, ec.B, ec.WAVE
STEP, DNU, CUTOFF = 0.25, ec.DNU, ec.CUTOFF
S_MIN, S_SL = ec.S_MIN, 1e-23
NODE = ec.NODE
FIRST_CELL = 4000                               # 1000 cm^-1, point 0 of ec.GRID
_kept = {}


class Case(ec.Case):
    def __init__(self, label, states, raw, broadeners, nodes, s_min, grid, cutoff, s_sl, step, on_purpose=()):
        ec.Case.__init__(self, label, states, raw, broadeners, nodes, s_min, grid, cutoff)
        self.s_sl, self.step = float(s_sl), float(step)
        sr.assert_clear(self.states, self.trans, self.nodes, self.q, self.s_min, self.s_sl, self.step, on_purpose)

    def with_levels(self, s_min=None, s_sl=None):
        return Case(self.label + ", other levels", self.states, self.raw, self.broadeners, self.nodes,
                    self.s_min if s_min is None else s_min, self.grid, self.cutoff, self.s_sl if s_sl is None else s_sl, self.step)


def layout(label, cells, grid=ec.GRID, cutoff=CUTOFF, seed=1, n_broadeners=1, nodes=(NODE,), s_min=S_MIN, s_sl=S_SL, step=STEP,
           centred=False):
    rng = np.random.default_rng(seed)
    assert [c for c, _ in cells] == sorted(set(c for c, _ in cells)), "cells ascend and occur once"
    kinds = "".join(k for _, k in cells)
    n = len(kinds)
    nu = np.concatenate([(c + (np.full(len(k), 0.5) if centred else np.sort(rng.uniform(0.1, 0.9, len(k))))) * step for c, k in cells])
    e_low, a_coef = np.empty(n), np.empty(n)
    for i, kind in enumerate(kinds):
        low, high, la, ha = {"s": (0.0, 500.0, 1.0, 2.0), "w": (0.0, 500.0, -4.0, -3.0), "d": (20000.0, 20500.0, -2.0, 2.0),
                             "z": (6e6, 6e6, 0.0, 0.0), "m": (8000.0, 9000.0, 0.0, 0.0)}[kind]
        e_low[i] = np.floor(rng.uniform(low, high)) if centred else rng.uniform(low, high)
        a_coef[i] = 10.0 ** rng.uniform(la, ha)
    e_up = e_low + nu
    j_low = rng.integers(0, int(2 * ec.J_TOP), n) * 0.5
    j_low[rng.integers(0, n)] = ec.J_TOP
    states = {"E": np.concatenate([e_low, e_up]), "J": np.concatenate([j_low, j_low + 1.0])}
    states["jidx"] = np.minimum(np.round(2 * states["J"]).astype(np.int32), int(2 * ec.J_TOP))
    states["J"] = 0.5 * states["jidx"]
    states["g"] = (states["jidx"] + 1).astype(np.float64)
    moving = np.array([k == "m" for k in kinds])
    if moving.any():                                            # A from the strengths A = 1 gives in the coldest and hottest node
        unit = {"up": n + np.arange(n), "low": np.arange(n), "A": np.ones(n), "nu0": e_up - e_low}
        q = lambda t: exomol.partition_value(ec.q_table(), t)
        temps = sorted(nd[0] for nd in nodes)
        cold, hot = (exomol.strengths(states, unit, t, q(t))[moving] for t in (temps[0], temps[-1]))
        assert np.all(hot > 1e4 * cold)
        a_coef[moving] = s_sl / np.sqrt(cold * hot)
    order = rng.permutation(n)
    raw = ((n + np.arange(n))[order], np.arange(n)[order], a_coef[order])
    case = Case(label, states, raw, ec.broadeners(n_broadeners), nodes, s_min, grid, cutoff, s_sl, step,
                on_purpose=tuple(nu.tolist()) if centred else ())
    assert len(case.trans["nu0"]) == n and np.array_equal(sr.cells_of(case.trans["nu0"], step), np.repeat([c for c, _ in cells],
                                                                                                          [len(k) for _, k in cells]))
    return case


def classes_at(case, node=0):
    """one letter per transition: s, w or d by the fp64 strengths at the node"""
    temp = case.nodes[node][0]
    s = exomol.strengths(case.states, case.trans, temp, case.q(temp))
    return "".join("d" if v < case.s_min else "s" if v >= case.s_sl else "w" for v in s)


def restated(case, node):
    """{"ld", "f64": kappa; "list_ld", "list_f64": exomol_superline_reference.node_list's} of the node, once per process"""
    key = ("superlines", id(case), node)
    if key not in _kept:
        temp, press = case.nodes[node]
        args = (case.states, case.trans, case.broadening, temp, press, case.q(temp), case.molar_mass, case.s_min, case.s_sl, case.step,
                case.cutoff) + tuple(case.grid)
        ld, list_ld = sr.long_double(*args)
        f64, list_f64 = sr.plain_fp64(*args)
        _kept[key] = {"case": case, "ld": ld, "f64": f64, "list_ld": list_ld, "list_f64": list_f64}
    return _kept[key]


def check_list(params, counts, case, node, label):
    """the four numbers of every entry under the rule, nu to the bit, and the three counts"""
    r = restated(case, node)
    want = r["list_f64"]
    assert tuple(int(c) for c in counts) == (len(want["strong"]), len(want["weak"]), len(want["cells"])), (label, counts)
    assert params.shape == want["params"].shape, (label, params.shape, want["params"].shape)
    assert np.array_equal(params[0], want["params"][0]), (label, "nu in the list's order")
    if params.shape[1]:
        ec.check_rule(params, r["list_ld"]["params"], want["params"], label + ", the list")
    return r


def check_ranges(ranges, nu_list, case, label):
    """a tile's range holds every entry that the per-point test passes for one of its points, and none beyond the reach widened by
    RANGE_WIDEN and the step"""
    nu_first, dnu, n_points = case.grid
    nu = nu_first + np.arange(n_points, dtype=np.float64) * dnu
    widen = case.cutoff * (1.0 + exomol.RANGE_WIDEN[0]) + exomol.RANGE_WIDEN[1] + case.step
    assert ranges.shape == (-(-n_points // TILE), 2), label
    for t, (lo, hi) in enumerate(ranges):
        pts = nu[t * TILE:(t + 1) * TILE]
        assert 0 <= lo <= hi <= len(nu_list), (label, t, lo, hi)
        reached = np.nonzero((np.abs(pts[:, None] - nu_list[None, :]) <= case.cutoff).any(axis=0))[0]
        assert np.all((reached >= lo) & (reached < hi)), (label, t, lo, hi, reached[:3], reached[-3:])
        inside = nu_list[lo:hi]
        assert np.all((inside >= pts[0] - widen) & (inside <= pts[-1] + widen)), (label, t, lo, hi)


# ---- the layouts ---------------------------------------------------------------------------------------------------------------
def spread(kinds, first=FIRST_CELL + 8, gap=9):
    """a layout with the cells `gap` apart"""
    return [(first + gap * i, k) for i, k in enumerate(kinds)]


def interleaved(n, seed=5):
    rng = np.random.default_rng(seed)
    return "".join(rng.choice(list("swd"), n))


SIZES = [1, WAVE - 1, WAVE, WAVE + 1, B - 1, B, B + 1, 700]


def sizes_layout():
    """weak cells of every size of SIZES; the cell of 700 starts at the last lane of a compaction block and crosses three block
    boundaries: the cells before it hold B - 1 transitions.  Then a cell of strong transitions only, one of dropped ones only, one
    with the classes interleaved, and a weak first and last transition of the list"""
    before = [1, WAVE - 1, WAVE, WAVE + 1]
    pad = B - 1 - sum(before)
    assert pad > 0
    kinds = ["w" * k for k in before] + ["s" * pad, "w" * 700, "w" * (B - 1), "w" * B, "w" * (B + 1), "s" * 5, "d" * 7,
                                         interleaved(90), "sw"]
    return spread(kinds)
