"""Opacities of one species from an ExoMol line list, on the device (include/helios_hip.h section 13, csrc/exomol.hip).

`lines.py` reads HITRAN `.par` records, a room-temperature data base.  The hot lists are ExoMol's: a `.states` table, one or more
`.trans` files and `.broad` files per broadener.  This tool makes from them what `lines.py` makes from a `.par` file: the files
`Out_<name>_<numin>_<numax>_<T>_<pcode>.bin` that `ktable.py` reads, or with `-ktable yes` the species' k-table itself.

States.  Whitespace-separated: id, E [cm^-1], g, J; everything after J is ignored.  The ids are 1, 2, ... n in file order, anything
else is refused with the line.  J >= 0 and 2 J is an integer to within 1e-9; jidx = round(2 J).

Transitions.  Whitespace-separated: upper id, lower id, A [s^-1]; a fourth column is ignored.  Several files are concatenated in
the order given.  The wavenumber is always nu_0 = E[up] - E[low] from the states, one fp64 subtraction.  A transition with
nu_0 <= 0 is skipped and counted.  Refused, with file and line: an id outside 1 ... n, a field that is not a finite number, A < 0;
and a list of which no transition is left.

Partition function.  lines.read_partition_function and lines.partition_value; nothing here is referred to 296 K, so 296 K need not
be inside the file.

Broadeners.  `name:fraction:file[:gamma_default:n_default]` each.  Of a `.broad` file only the rows `a0 gamma n J''` are used
(gamma in cm^-1 bar^-1 at 296 K); rows of other codes are skipped and counted; two `a0` rows for one J'' are refused with both
line numbers; a J'' the file does not hold takes the broadener's defaults (`-default_broadening`, 0.07 and 0.5, unless the entry
gives its own).  Fractions are > 0 and used as given.  Without `-broadeners` there is one broadener of fraction 1 with the
defaults.  The host makes the table [broadener][jidx][gamma, n] up to the states' largest jidx; the device never sees a file.

The contract.  All arithmetic is fp64 and nothing is contracted; H, C, K_B, N_A are phys_const's; every statement is evaluated
left to right.  With c2 = H C / K_B and P_bar = P / 1e6 dyne cm^-2 (ExoMol's reference pressure is 1 bar), per transition and node:
    pre    = g[up] * A / (8 * pi * C * nu_0 * nu_0)
    S      = pre * exp(-c2 * E[low] / T) * (-expm1(-c2 * nu_0 / T)) / Q(T)                          [cm / molecule]
    gamma  = P_bar * sum over the broadeners b, in the order given, of x_b * gamma_b[jidx[low]] * (296 / T)^n_b[jidx[low]]
    alpha  = (nu_0 / C) * sqrt(2 * ln 2 * N_A * K_B * T / M),   a = sqrt(ln 2) / alpha,   y = max(a * gamma, 1e-8),
    s      = S * a * (1 / sqrt pi)
There is no pressure shift: nu_0' = nu_0.  The sum over the broadeners starts from 0.
The transitions are sorted by (nu_0, position in the concatenated files), by a stable sort on the host, and every spectral point
adds its terms in ascending order of that index.
The strength cut.  At a node a transition is kept iff S >= S_min (`-strength_cutoff`), S the fp64 number above.  With S_min = 0
every transition is kept, those whose S underflowed to 0 included.  The node's list is the kept transitions in list order.
The sum is lines.py's, unchanged, over the node's list: the inclusive cut-off |nu_i - nu_0| <= C, K(x, y) in its four regions,
kappa = sigma N_A / M rounded once to fp32 when written; lines_k and lines_sum_tile on the device, lines.voigt_k and
lines.numpy_node on the host.  The tool prints per node how many transitions were kept.

Super-lines (`-superline_threshold S_sl`, `-superline_step d`; off unless given).  The strength cut buys time by deleting opacity;
super-lines keep it: strong transitions keep their own profile, the weak ones are added up per small wavenumber cell at the
node's temperature and each cell gets one profile.  fp64, nothing contracted, every statement left to right, as above.  S_sl
[cm / molecule] and the cell width d [cm^-1] are shared by all nodes of a call.  Per node, S, gamma, a as above:
    classes     dropped iff S < S_min (unchanged); strong iff S >= S_min and S >= S_sl; weak otherwise: S_min <= S < S_sl.
    cell        c = floor(nu_0 / d), an integer from one fp64 division.  The cell grid starts at 0 cm^-1 whatever -numin or the
                chunk is, so a chunked run forms the super-lines of a one-chunk run.  The list is sorted by nu_0: a cell is a
                contiguous run of it, and cells do not depend on T (the device receives the occupied cells once per list).
    super-line  one per node and cell that holds at least one weak transition at that node:
                S_c = sum S_j and G_c = sum S_j * gamma_j over the cell's weak transitions in list order,
                gamma_c = G_c / S_c if S_c > 0, else 0;  nu_c = (c + 0.5) * d;  alpha, a by the statements above from nu_c;
                y = max(a * gamma_c, 1e-8);  s = S_c * a * (1 / sqrt pi).
    the list    the strong transitions plus the super-lines, ordered by the integer key (cell, kind, position in the list), the
                super-line (kind 0) before its cell's strong transitions (kind 1).  Every spectral point adds its terms in
                ascending order of that list; the sum, the inclusive cut-off, K's regions and the fp32 rounding are unchanged.
In this list nu ascends only from cell to cell: inside a cell nu_c may lie above a strong nu_0, by less than d.  The tile ranges
are therefore widened by d on top of RANGE_WIDEN; a bisection over a list whose disorder is confined to a cell then still returns
a superset of what the per-point test passes, and that test decides every term, as before.  (lines.numpy_node and count_pairs
take each line's window from its own nu and assume no order.)  On the device the sums S_c, G_c are added lane-strided and by a
butterfly, not one after the other: the super-lines' numbers are held to the tolerance of the tests, not to bits; they are the
same bits in every run and in every launch.  With S_sl <= S_min no transition is weak and the result is the plain one bit for
bit; S_sl = +inf makes every kept transition weak.  Refused, with the value: S_sl that is NaN or < 0; d that is not a finite
number > 0; d greater than the cut-off; nu_0,max / d at or above 2^31; `-superline_step` without `-superline_threshold`.  The tool
prints per node the strong, the weak and the super-lines next to the kept transitions.

Not modelled: `.broad` codes other than `a0`, a pressure shift, a cut relative to the strongest line, several
isotopologues per call; and what lines.py does not model either (no renormalisation for the cut wings, no sub-Lorentzian factor).

`backend="device"`: per launch of up to `-nodes_per_launch` nodes, the node a grid dimension: k_exomol_count flags S >= S_min and
counts per workgroup of COMPACT_BLOCK transitions, k_exomol_scan turns the counts into offsets, k_exomol_prepare writes nu_0, s, a,
y of the kept transitions to their positions, k_exomol_ranges finds per tile of TILE_POINTS points the kept transitions within the
cut-off by bisection in the compacted nu_0, k_exomol_sum is lines_sum_tile.  With super-lines k_exomol_classify (S once per
transition, strong and weak counts), k_exomol_cells (a wavefront per occupied cell), two scans and k_exomol_merge take the place
of count, scan and prepare.  `backend="numpy"` computes the same contract on the
CPU: gather, strengths, cut, lines.numpy_node; the checker of the device path, and what a machine without a GPU gets.

`-ktable yes`: as `lines.py -ktable yes`, word for word.  One chunk 0 ... numax; the kernel steps with the `-dnu` given and the
k-table's axis with numax / points; the nodes sorted ascending and de-duplicated (node = p + np t); ktable.check_empty_bins and the
limit of 2^28 points stand before the first launch; the fp32 slabs stay on the device for k_ktable_bins.  The containers are the
ones `exomol.py` followed by `ktable.py` writes, to the bit.  Refused with `-ktable yes`: `-numin` other than 0, `-chunk_width`,
`-output_format text`, `-output_directory`.

The frame around the readers and the contract is _nodes.py's, shared with lines.py and cia.py.
"""
import argparse
import bz2
import time
import warnings

import numpy as np

from . import _nodes
from . import phys_const as pc
from ._tool import DeviceObject, dp, ip
from .lines import (DEFAULT_CUTOFF, INV_SQRT_PI, LDS_BLOCK, LN2, TILE_POINTS, T_REF, WAVEFRONT, Y_MIN, count_pairs, numpy_node,
                    partition_value, read_partition_function)

BAR = 1.0e6                           # dyne cm^-2
DEFAULT_BROADENING = (0.07, 0.5)      # gamma [cm^-1 bar^-1 at 296 K], n
COMPACT_BLOCK = 256                   # csrc/exomol.hip: EXO_B, the count kernel's block (tests/test_gpu_exomol.py derives its sizes)
JIDX_MAX = 1 << 20
RANGE_WIDEN = (1e-12, 1e-9)           # lines_tile_ranges: reach * (1 + 1e-12) + 1e-9 (super-lines: + d)
CELL_LIMIT = 2.0 ** 31                # cells are numbered by an int
GRID_TOOL = "lines"                   # the refusals of the grid and of the node lists came from lines.py with its word, and keep it


# ---- the inputs --------------------------------------------------------------------------------------------------------
def _open(path):
    return bz2.open(path, "rt") if str(path).endswith(".bz2") else open(path)


def _number(word):
    try:
        v = float(word)
    except ValueError:
        return np.nan
    return v if np.isfinite(v) else np.nan


def read_states(path):
    """{"E", "g", "J", "jidx"} of a `.states` file, in the order of the ids 1 ... n"""
    e, g, jj, jidx = [], [], [], []
    with _open(path) as f:
        for nr, line in enumerate(f, 1):
            if not line.strip():
                continue
            where = "line %d of %s (%r)" % (nr, path, line.rstrip("\r\n")[:60])
            col = line.split()
            if len(col) < 4:
                raise IOError("exomol: %s holds %d columns, a state needs id, E, g and J" % (where, len(col)))
            v = [_number(c) for c in col[:4]]
            for name, x, c in zip(("id", "E", "g", "J"), v, col):
                if np.isnan(x):
                    raise IOError("exomol: %s: %s = %r is not a finite number" % (where, name, c))
            if v[0] != len(e) + 1:
                raise IOError("exomol: %s: id %s where %d is expected; the ids are 1, 2, ... in file order" % (where, col[0], len(e) + 1))
            if v[2] < 0:
                raise IOError("exomol: %s: g = %r is negative" % (where, v[2]))
            two_j = 2.0 * v[3]
            if v[3] < 0 or abs(two_j - round(two_j)) > 1e-9 or round(two_j) > JIDX_MAX:
                raise IOError("exomol: %s: J = %s; J is >= 0 and 2 J a whole number up to %d" % (where, col[3], JIDX_MAX))
            e.append(v[1]); g.append(v[2]); jj.append(v[3]); jidx.append(int(round(two_j)))
    if not e:
        raise IOError("exomol: %s holds no state" % (path,))
    return {"E": np.array(e), "g": np.array(g), "J": np.array(jj), "jidx": np.array(jidx, np.int32)}


def _transition_columns(path, n_states):
    """[rows][upper id, lower id, A] of a file whose every row passes the checks of read_transitions, by numpy's reader; None where
    a row does not, and the caller reads the file line by line to name it"""
    with _open(path) as f:
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                v = np.loadtxt(f, dtype=np.float64, usecols=(0, 1, 2), ndmin=2, comments=None)
        except (ValueError, IndexError):
            return None
    ids = v[:, :2]
    if not (np.all(np.isfinite(v)) and np.all(ids == np.floor(ids)) and np.all((ids >= 1) & (ids <= n_states)) and np.all(v[:, 2] >= 0)):
        return None
    return v


def read_transitions(paths, states):
    """({"up", "low" (0-based int32), "A", "nu0"} sorted by (nu_0, position in the concatenated files), skipped) of `.trans` files"""
    if isinstance(paths, str):
        paths = [paths]
    n = len(states["E"])
    up, low, a = [], [], []
    for path in paths:
        v = _transition_columns(path, n)
        if v is not None:
            up.append(v[:, 0].astype(np.int64) - 1); low.append(v[:, 1].astype(np.int64) - 1); a.append(v[:, 2].copy())
            continue
        rows = ([], [], [])
        with _open(path) as f:
            for nr, line in enumerate(f, 1):
                if not line.strip():
                    continue
                col = line.split()
                where = "line %d of %s (%r)" % (nr, path, line.rstrip("\r\n")[:60])
                if len(col) < 3:
                    raise IOError("exomol: %s holds %d columns, a transition needs upper id, lower id and A" % (where, len(col)))
                v = [_number(c) for c in col[:3]]
                for name, x, c in zip(("upper id", "lower id", "A"), v, col):
                    if np.isnan(x):
                        raise IOError("exomol: %s: %s = %r is not a finite number" % (where, name, c))
                for name, x, c in zip(("upper id", "lower id"), v, col):
                    if x != int(x) or not 1 <= x <= n:
                        raise IOError("exomol: %s: %s = %s lies outside the states' 1 ... %d" % (where, name, c, n))
                if v[2] < 0:
                    raise IOError("exomol: %s: A = %r is negative" % (where, v[2]))
                rows[0].append(int(v[0]) - 1); rows[1].append(int(v[1]) - 1); rows[2].append(v[2])
        up.append(np.array(rows[0], np.int64)); low.append(np.array(rows[1], np.int64)); a.append(np.array(rows[2], np.float64))
    return sort_transitions({"up": np.concatenate(up), "low": np.concatenate(low), "A": np.concatenate(a)}, states,
                            ", ".join(str(p) for p in paths))


def sort_transitions(trans, states, origin="the list"):
    """(the arrays with nu_0 = E[up] - E[low], without the transitions of nu_0 <= 0, sorted by (nu_0, position); skipped)"""
    up = np.asarray(trans["up"], np.int64).reshape(-1)
    low = np.asarray(trans["low"], np.int64).reshape(-1)
    a = np.asarray(trans["A"], np.float64).reshape(-1)
    n = len(states["E"])
    if not (len(up) == len(low) == len(a)):
        raise ValueError("exomol: the three per-transition arrays have one length")
    for name, v in (("upper", up), ("lower", low)):
        bad = (v < 0) | (v >= n)
        if bad.any():
            j = int(np.argmax(bad))
            raise ValueError("exomol: transition %d: %s state %d (0-based) lies outside the states' 0 ... %d" % (j, name, v[j], n - 1))
    bad = ~np.isfinite(a) | (a < 0)
    if bad.any():
        j = int(np.argmax(bad))
        raise ValueError("exomol: transition %d: A = %r is not a finite number >= 0" % (j, float(a[j])))
    energy = np.asarray(states["E"], np.float64)
    nu0 = energy[up] - energy[low]
    keep = nu0 > 0
    skipped = int(len(nu0) - np.count_nonzero(keep))
    if not keep.any():
        raise IOError("exomol: no transition is left of %s (%d with nu_0 <= 0 skipped)" % (origin, skipped))
    up, low, a, nu0 = up[keep], low[keep], a[keep], nu0[keep]
    order = np.argsort(nu0, kind="stable")
    return {"up": np.ascontiguousarray(up[order], np.int32), "low": np.ascontiguousarray(low[order], np.int32),
            "A": np.ascontiguousarray(a[order]), "nu0": np.ascontiguousarray(nu0[order])}, skipped


def read_broad(path):
    """({jidx: (gamma, n)} of the `a0` rows, rows of other codes skipped) of a `.broad` file"""
    rows, lines_of, skipped = {}, {}, 0
    with _open(path) as f:
        for nr, line in enumerate(f, 1):
            col = line.split()
            if not col:
                continue
            if col[0] != "a0":
                skipped += 1
                continue
            where = "line %d of %s (%r)" % (nr, path, line.rstrip("\r\n")[:60])
            if len(col) < 4:
                raise IOError("exomol: %s holds %d columns, an a0 row needs gamma, n and J''" % (where, len(col)))
            v = [_number(c) for c in col[1:4]]
            for name, x, c in zip(("gamma", "n", "J''"), v, col[1:4]):
                if np.isnan(x):
                    raise IOError("exomol: %s: %s = %r is not a finite number" % (where, name, c))
            two_j = 2.0 * v[2]
            if v[0] < 0 or v[2] < 0 or abs(two_j - round(two_j)) > 1e-9:
                raise IOError("exomol: %s: gamma is >= 0, J'' is >= 0 and 2 J'' a whole number" % (where,))
            j = int(round(two_j))
            if j in rows:
                raise IOError("exomol: %s: a second a0 row for J'' = %s; the first is line %d" % (where, col[3], lines_of[j]))
            rows[j], lines_of[j] = (v[0], v[1]), nr
    return rows, skipped


def parse_default_broadening(text):
    word = str(text).split()
    v = [_number(w) for w in word]
    if len(v) != 2 or np.isnan(v).any() or v[0] < 0:
        raise IOError("exomol: -default_broadening %r: gamma >= 0 and n, separated by a blank" % (text,))
    return v[0], v[1]


def parse_broadeners(text, default=DEFAULT_BROADENING):
    """[(name, fraction, file or None, gamma_default, n_default)] of `name:fraction:file[:gamma_default:n_default] ...`"""
    if text is None or not str(text).split():
        return [("default", 1.0, None, float(default[0]), float(default[1]))]
    out = []
    for entry in str(text).split():
        part = entry.split(":")
        if len(part) not in (3, 5) or not part[0] or not part[2]:
            raise IOError("exomol: -broadeners entry %r is not name:fraction:file[:gamma_default:n_default]" % (entry,))
        v = [_number(w) for w in [part[1]] + part[3:]]
        if np.isnan(v).any():
            raise IOError("exomol: -broadeners entry %r: fraction and defaults are finite numbers" % (entry,))
        if not v[0] > 0:
            raise IOError("exomol: -broadeners entry %r: the fraction %s is not > 0" % (entry, part[1]))
        if len(v) == 3 and v[1] < 0:
            raise IOError("exomol: -broadeners entry %r: the default gamma %s is negative" % (entry, part[3]))
        out.append((part[0], v[0], part[2]) + ((v[1], v[2]) if len(v) == 3 else (float(default[0]), float(default[1]))))
    return out


def broadening_table(broadeners, max_jidx, report=None):
    """(fractions [b], table [b][jidx 0 ... max_jidx][gamma, n]); `broadeners`: parse_broadeners' entries, the file of an entry
    may be a dict {jidx: (gamma, n)} in place of a path.  `report` receives a line per broadener"""
    x = np.array([b[1] for b in broadeners], np.float64)
    table = np.empty((len(broadeners), int(max_jidx) + 1, 2))
    for k, (name, fraction, source, gamma_d, n_d) in enumerate(broadeners):
        table[k, :, 0], table[k, :, 1] = gamma_d, n_d
        rows, skipped = ({}, 0) if source is None else (source, 0) if isinstance(source, dict) else read_broad(source)
        for j, (gamma, n) in rows.items():
            if j <= max_jidx:
                table[k, j] = gamma, n
        if report is not None:
            held = sum(1 for j in rows if j <= max_jidx)
            report("exomol: broadener %s, fraction %g: %d of the %d values of 2 J'' from %s, the others gamma = %g, n = %g; "
                   "%d rows of other codes than a0 skipped" % (name, fraction, held, int(max_jidx) + 1,
                                                               "a table" if isinstance(source, dict) else source, gamma_d, n_d, skipped))
    if report is not None:
        report("exomol: the fractions of the %d broadeners sum to %.12g" % (len(x), float(np.sum(x))))
    return x, table


# ---- the contract in numpy ---------------------------------------------------------------------------------------------
def strengths(states, trans, temp, q_t):
    """S(T) per transition [cm / molecule]"""
    c2 = pc.H * pc.C / pc.K_B
    nu0 = trans["nu0"]
    pre = states["g"][trans["up"]] * trans["A"] / (8.0 * np.pi * pc.C * nu0 * nu0)
    with np.errstate(under="ignore"):
        return pre * np.exp(-c2 * states["E"][trans["low"]] / temp) * (-np.expm1(-c2 * nu0 / temp)) / q_t


def node_params(states, trans, broadening, temp, press, q_t, molar_mass, s_min=0.0, superline_threshold=None, superline_step=None):
    """([4][kept]: nu_0, s = S a / sqrt pi, a, y of the node's kept transitions in list order; their indices in the list).  With
    super-lines the four numbers are those of the node's list (superline_node), the indices still those of the kept transitions"""
    if superline_threshold is not None or superline_step is not None:
        sl = check_superlines(superline_threshold, superline_step, np.inf, trans["nu0"][-1])
        node = superline_node(states, trans, broadening, temp, press, q_t, molar_mass, s_min, sl[0], sl[1])
        return node["params"], node["kept"]
    strength = strengths(states, trans, temp, q_t)
    kept = np.nonzero(strength >= s_min)[0]
    nu0, gamma = trans["nu0"][kept], _gamma(states, trans, broadening, kept, temp, press)
    alpha = (nu0 / pc.C) * np.sqrt(2.0 * LN2 * pc.N_A * pc.K_B * temp / molar_mass)
    a = np.sqrt(LN2) / alpha
    y = np.maximum(a * gamma, Y_MIN)
    return np.stack([nu0, strength[kept] * a * INV_SQRT_PI, a, y]), kept


# ---- super-lines ---------------------------------------------------------------------------------------------------------
def check_superlines(superline_threshold, superline_step, cutoff, nu0_max, default_step=None):
    """(S_sl, d) as floats, or None where super-lines are off (both arguments None); every refusal names the value"""
    if superline_threshold is None:
        if superline_step is not None:
            raise ValueError("exomol: a super-line step (%r) without a super-line threshold" % (superline_step,))
        return None
    s_sl = float(superline_threshold)
    if superline_step is None and default_step is None:
        raise ValueError("exomol: the super-line threshold %r without a super-line step" % (s_sl,))
    step = float(default_step if superline_step is None else superline_step)
    if np.isnan(s_sl) or s_sl < 0:
        raise ValueError("exomol: the super-line threshold %r is not a number >= 0 cm / molecule" % (s_sl,))
    if not (np.isfinite(step) and step > 0):
        raise ValueError("exomol: the super-line step %r is not a finite number > 0 cm^-1" % (step,))
    if step > cutoff:
        raise ValueError("exomol: the super-line step %r is greater than the cut-off %r cm^-1" % (step, float(cutoff)))
    if not float(nu0_max) / step < CELL_LIMIT:
        raise ValueError("exomol: the super-line step %r puts the largest nu_0 = %r into cell %r, cells are numbered below 2^31"
                         % (step, float(nu0_max), float(np.floor(float(nu0_max) / step))))
    return s_sl, step


def _gamma(states, trans, broadening, index, temp, press):
    x, table = broadening
    jx = states["jidx"][trans["low"][index]]
    total = np.zeros(len(index))
    for b in range(len(x)):
        total = total + x[b] * table[b, jx, 0] * (T_REF / temp) ** table[b, jx, 1]
    return (press / BAR) * total


def superline_node(states, trans, broadening, temp, press, q_t, molar_mass, s_min, s_sl, step):
    """the node's list with super-lines, by the contract: {"params": [4][strong + super-lines] in the list's order; "kept",
    "strong", "weak": indices in the transition list; "cells": the cell numbers of the super-lines, ascending; "S_c", "G_c":
    their sums; "keys": [entries][cell, kind, position] of the list, kind 0 a super-line (position: its cell's first transition)
    and 1 a strong transition"""
    strength = strengths(states, trans, temp, q_t)
    keep = strength >= s_min
    is_strong = keep & (strength >= s_sl)
    strong, weak = np.nonzero(is_strong)[0], np.nonzero(keep & ~is_strong)[0]
    nu0 = trans["nu0"]
    cell = np.floor(nu0 / step).astype(np.int64)
    cells, slot = np.unique(cell[weak], return_inverse=True)
    s_c = np.bincount(slot, weights=strength[weak], minlength=len(cells))            # one after the other, in list order
    g_c = np.bincount(slot, weights=strength[weak] * _gamma(states, trans, broadening, weak, temp, press), minlength=len(cells))
    with np.errstate(invalid="ignore", divide="ignore"):
        gamma_c = np.where(s_c > 0, g_c / np.where(s_c > 0, s_c, 1.0), 0.0)
    nu_c = (cells.astype(np.float64) + 0.5) * step
    first_of = np.searchsorted(cell, cells, side="left")
    nu = np.concatenate([nu_c, nu0[strong]])
    s = np.concatenate([s_c, strength[strong]])
    gamma = np.concatenate([gamma_c, _gamma(states, trans, broadening, strong, temp, press)])
    kind = np.concatenate([np.zeros(len(cells), np.int64), np.ones(len(strong), np.int64)])
    keys = np.stack([np.concatenate([cells, cell[strong]]), kind, np.concatenate([first_of, strong])], axis=1)
    order = np.lexsort((keys[:, 2], keys[:, 1], keys[:, 0]))
    nu, s, gamma, keys = nu[order], s[order], gamma[order], keys[order]
    alpha = (nu / pc.C) * np.sqrt(2.0 * LN2 * pc.N_A * pc.K_B * temp / molar_mass)
    a = np.sqrt(LN2) / alpha
    y = np.maximum(a * gamma, Y_MIN)
    return {"params": np.stack([nu, s * a * INV_SQRT_PI, a, y]), "kept": np.nonzero(keep)[0], "strong": strong, "weak": weak,
            "cells": cells, "S_c": s_c, "G_c": g_c, "keys": keys}


def tile_ranges(nu, nu_first, dnu, n_points, cutoff, step=0.0):
    """[tiles][first, one past the last] entry of the node's list a tile of TILE_POINTS points walks, as k_exomol_ranges finds them:
    two bisections per tile with the reach cutoff * (1 + 1e-12) + 1e-9 + step.  With super-lines `nu` ascends only from cell to
    cell, and `step` = d makes the result hold every entry within the cut-off of one of the tile's points all the same"""
    nu = np.asarray(nu, np.float64)
    widen = cutoff * (1.0 + RANGE_WIDEN[0]) + RANGE_WIDEN[1] + step
    out = np.empty((-(-n_points // TILE_POINTS), 2), np.int32)
    for t in range(len(out)):
        first, last = t * TILE_POINTS, min((t + 1) * TILE_POINTS, n_points) - 1
        lo, hi = nu_first + float(first) * dnu - widen, nu_first + float(last) * dnu + widen
        a, b = 0, len(nu)
        while a < b:                                             # the first index with nu >= lo
            mid = a + (b - a) // 2
            if nu[mid] < lo:
                a = mid + 1
            else:
                b = mid
        c, d = a, len(nu)
        while c < d:                                             # the first index with nu > hi
            mid = c + (d - c) // 2
            if nu[mid] <= hi:
                c = mid + 1
            else:
                d = mid
        out[t] = a, c
    return out


# ---- device ------------------------------------------------------------------------------------------------------------
class ExomolOpacity(_nodes.NodeOpacity):
    """hx_exomol: resident states, broadening table and sorted transitions; nodes of up to n_points_max spectral points,
    nodes_per_launch per launch into fp32 slabs that stay on the device; `with_fp64`: the rows before rounding as well"""

    PREFIX = "hx_exomol"

    def __init__(self, ctx, n_states_max, n_trans_max, n_broadeners_max, n_points_max, nodes_per_launch, n_nodes_max, with_fp64=False):
        self.n_points_max, self.nodes_per_launch, self.n_nodes_max = int(n_points_max), int(nodes_per_launch), int(n_nodes_max)
        self.with_fp64 = bool(with_fp64)
        self.n_nodes = self.n_points = self.rows_run = self._params_len = 0
        self.superlines = None
        self._create(ctx, int(n_states_max), int(n_trans_max), int(n_broadeners_max), self.n_points_max, self.nodes_per_launch,
                     self.n_nodes_max, int(self.with_fp64))

    @classmethod
    def of(cls, ctx, states, trans, broadening, n_points_max, nodes_per_launch, n_nodes_max, with_fp64=False):
        """a handle that holds the three inputs"""
        h = cls(ctx, len(states["E"]), len(trans["nu0"]), len(broadening[0]), n_points_max, nodes_per_launch, n_nodes_max, with_fp64)
        try:
            h.set_states(states)
            h.set_broadening(*broadening)
            h.set_transitions(trans)
        except Exception:
            h.close()
            raise
        return h

    def set_states(self, states):
        e, g = (np.ascontiguousarray(states[k], np.float64).reshape(-1) for k in ("E", "g"))
        jidx = np.ascontiguousarray(states["jidx"], np.int32).reshape(-1)
        assert len(e) == len(g) == len(jidx)
        self._reset_nodes()
        self._call("set_states", len(e), dp(e), dp(g), ip(jidx))

    def set_broadening(self, fractions, table):
        x = np.ascontiguousarray(fractions, np.float64).reshape(-1)
        t = np.ascontiguousarray(table, np.float64)
        assert t.ndim == 3 and t.shape[0] == len(x) and t.shape[2] == 2
        self._reset_nodes()
        self._call("set_broadening", len(x), t.shape[1], dp(x), dp(t.reshape(-1)))

    def set_transitions(self, trans):
        up, low = (np.ascontiguousarray(trans[k], np.int32).reshape(-1) for k in ("up", "low"))
        a = np.ascontiguousarray(trans["A"], np.float64).reshape(-1)
        assert len(up) == len(low) == len(a)
        self._reset_nodes()
        self.superlines = None                               # the library drops them with the list
        self._call("set_transitions", len(a), ip(up), ip(low), dp(a))

    def set_superlines(self, threshold, step):
        """S_sl and d for the list the handle holds; step = 0 (or None) turns super-lines off.  The nodes are set after it"""
        step = 0.0 if step is None else float(step)
        threshold = 0.0 if threshold is None else float(threshold)
        self._reset_nodes()
        self.superlines = None
        self._call("set_superlines", threshold, step)
        self.superlines = (threshold, step) if step > 0 else None

    def set_nodes(self, temps, pressures, q_t, molar_mass, cutoff, s_min, nu_first, dnu, n_points):
        """T, P and Q(T) per node, and what the nodes share"""
        arr = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (temps, pressures, q_t)]
        assert len(arr[0]) == len(arr[1]) == len(arr[2])
        self._reset_nodes()
        self._call("set_nodes", len(arr[0]), dp(arr[0]), dp(arr[1]), dp(arr[2]), float(molar_mass), float(cutoff), float(s_min),
                   float(nu_first), float(dnu), int(n_points))
        self.n_nodes, self.n_points = len(arr[0]), int(n_points)

    def get(self, name):
        """"line_params": a list of [4][kept[row]] per row of the last launch; with super-lines [4][strong + super-lines]"""
        if name != "line_params":
            return DeviceObject.get(self, name)
        if self.superlines is None:
            kept = DeviceObject.get(self, "kept")
        else:
            kept = DeviceObject.get(self, "superline_counts")[:, [0, 2]].sum(axis=1).astype(np.int32)
        self._params_len = 4 * int(kept.sum())
        flat = DeviceObject.get(self, name)
        at = np.concatenate([[0], np.cumsum(4 * kept.astype(np.int64))])
        return [flat[at[r]:at[r + 1]].reshape(4, int(kept[r])) for r in range(len(kept))]

    def _results(self):
        tiles = -(-self.n_points // TILE_POINTS)
        return {"slabs32": ((self.rows_run, self.n_points), np.float32), "kappa64": (self.rows_run, self.n_points),
                "kept": ((self.rows_run,), np.int32), "superline_counts": ((self.rows_run, 3), np.int32),
                "tile_ranges": ((self.rows_run, tiles, 2), np.int32),
                "line_params": self._params_len, "timing_ms": 2}


# ---- the library functions -----------------------------------------------------------------------------------------------
def _check_node_inputs(temps, pressures, nu_grid, molar_mass, cutoff, s_min):
    out = _nodes.check_node_inputs("exomol", temps, pressures, nu_grid, molar_mass)
    if not (np.isfinite(cutoff) and cutoff > 0):
        raise ValueError("exomol: the cut-off %r is not > 0 cm^-1" % (cutoff,))
    if not (np.isfinite(s_min) and s_min >= 0):
        raise ValueError("exomol: the strength cut-off %r is not a finite number >= 0 cm / molecule" % (s_min,))
    return out


def exomol_opacity(states, trans, broadening, q_table, temps, pressures_cgs, nu_grid, molar_mass=None, cutoff=DEFAULT_CUTOFF,
                   strength_cutoff=0.0, backend="device", ctx=None, nodes_per_launch=4, handle=None, timing=None,
                   superline_threshold=None, superline_step=None):
    """kappa [T][P][nu] in cm^2 g^-1, fp64.  `states`: read_states' arrays; `trans`: sort_transitions' arrays; `broadening`:
    broadening_table's pair; `q_table`: (T, Q); `nu_grid`: (nu of point 0, dnu, points); `handle`: an ExomolOpacity with fp64 rows
    that already holds the three inputs.  `timing` receives prepare_ms, sum_ms and pairs, summed over the nodes, and `kept`, the
    number of transitions kept per node [T][P].  `superline_threshold`, `superline_step`: S_sl and d (d defaults to dnu); `timing`
    then also receives `strong`, `weak` and `superlines` per node [T][P], and a `handle` given is set to them"""
    _nodes.check_backend("exomol", backend)
    s_min = float(strength_cutoff)
    temps, pressures, (nu_first, dnu, n_points) = _check_node_inputs(temps, pressures_cgs, nu_grid, molar_mass, cutoff, s_min)
    sl = check_superlines(superline_threshold, superline_step, cutoff, trans["nu0"][-1], dnu)
    counts = np.zeros((len(temps), len(pressures), 3), np.int64)
    q_t = [partition_value(q_table, t) for t in temps]
    out = np.empty((len(temps), len(pressures), n_points))
    kept = np.zeros((len(temps), len(pressures)), np.int64)
    pairs, ms = 0, np.zeros(2)
    if backend == "numpy":
        for it, t in enumerate(temps):
            for jp, p in enumerate(pressures):
                if sl is None:
                    prm, idx = node_params(states, trans, broadening, t, p, q_t[it], molar_mass, s_min)
                else:
                    node = superline_node(states, trans, broadening, t, p, q_t[it], molar_mass, s_min, sl[0], sl[1])
                    prm, idx = node["params"], node["kept"]
                    counts[it, jp] = len(node["strong"]), len(node["weak"]), len(node["cells"])
                kept[it, jp] = len(idx)
                out[it, jp] = numpy_node(prm, nu_first, dnu, n_points, cutoff, molar_mass)
                if timing is not None:
                    pairs += count_pairs(prm[0], nu_first, dnu, n_points, cutoff)
    else:
        nodes = [(t, p, q_t[it]) for it, t in enumerate(temps) for p in pressures]
        flat, flat_kept, flat_counts = out.reshape(len(nodes), n_points), kept.reshape(-1), counts.reshape(-1, 3)

        def set_nodes(h, part):
            if h.superlines != sl:                                           # a plain handle in a plain call stays untouched
                h.set_superlines(*(sl or (0.0, 0.0)))
            h.set_nodes([n[0] for n in part], [n[1] for n in part], [n[2] for n in part], molar_mass, cutoff, s_min, nu_first, dnu,
                        n_points)

        def collect(h, rows):
            nonlocal pairs
            flat[rows], flat_kept[rows] = h.get("kappa64"), h.get("kept")
            if sl is not None:
                flat_counts[rows] = h.get("superline_counts")
            if timing is not None:
                pairs += sum(count_pairs(prm[0], nu_first, dnu, n_points, cutoff) for prm in h.get("line_params"))
        ms = _nodes.nodes_in_turns(
            ctx, handle, lambda c: ExomolOpacity.of(c, states, trans, broadening, n_points, max(1, min(int(nodes_per_launch), len(nodes))),
                                                    len(nodes), True), nodes, set_nodes, collect)
    if timing is not None:
        timing["prepare_ms"] = timing.get("prepare_ms", 0.0) + float(ms[0])
        timing["sum_ms"] = timing.get("sum_ms", 0.0) + float(ms[1])
        timing["pairs"] = timing.get("pairs", 0) + pairs
        timing["kept"] = kept
        if sl is not None:
            timing["strong"], timing["weak"], timing["superlines"] = counts[..., 0], counts[..., 1], counts[..., 2]
    return out


# ---- from the line list to the k-table -----------------------------------------------------------------------------------
class ExomolSlabs(_nodes.NodeSlabs):
    """ktable.build_table's slabs from an ExoMol list (_nodes.NodeSlabs); `ms` holds the kernel times and `kept` the transitions
    kept per node once the table is built"""

    TOOL = "exomol"

    def __init__(self, states, trans, broadening, q_table, temps, pressures, numax, dnu, n_points, molar_mass, cutoff, s_min,
                 nodes_per_launch=4, superline_threshold=None, superline_step=None):
        self.superlines = check_superlines(superline_threshold, superline_step, cutoff, trans["nu0"][-1], dnu)
        self.counts = []                                             # per node (strong, weak, super-lines), with super-lines
        _nodes.NodeSlabs.__init__(self, temps, pressures, numax, dnu, n_points, nodes_per_launch)
        self.states, self.trans, self.broadening = states, trans, broadening
        self.molar_mass, self.cutoff, self.s_min = molar_mass, cutoff, float(s_min)
        self.q_t = [partition_value(q_table, t) for t in self.temps]
        self.kept = []

    def host_slab(self, it, t, p):
        if self.superlines is None:
            prm, idx = node_params(self.states, self.trans, self.broadening, t, p, self.q_t[it], self.molar_mass, self.s_min)
        else:
            node = superline_node(self.states, self.trans, self.broadening, t, p, self.q_t[it], self.molar_mass, self.s_min,
                                  *self.superlines)
            prm, idx = node["params"], node["kept"]
            self.counts.append((len(node["strong"]), len(node["weak"]), len(node["cells"])))
        self.kept.append(len(idx))
        return numpy_node(prm, 0.0, self.dnu, self.n_points, self.cutoff, self.molar_mass)

    def open_handle(self, ctx, per, nodes):
        self.handle = h = ExomolOpacity.of(ctx, self.states, self.trans, self.broadening, self.n_points, per, len(nodes))
        if self.superlines is not None:
            h.set_superlines(*self.superlines)
        h.set_nodes([n[1] for n in nodes], [n[2] for n in nodes], [self.q_t[n[0]] for n in nodes], self.molar_mass, self.cutoff,
                    self.s_min, 0.0, self.dnu, self.n_points)

    def after_launch(self, h):
        self.kept.extend(int(k) for k in h.get("kept"))            # after the launch's sort is queued: the counts are the tool's report
        if self.superlines is not None:
            self.counts.extend(tuple(int(v) for v in row) for row in h.get("superline_counts"))


def exomol_ktable(states, trans, broadening, q_table, temps, pressure_codes, numax, dnu, inter, n_gauss, molar_mass=None,
                  cutoff=DEFAULT_CUTOFF, strength_cutoff=0.0, target=None, backend="device", ctx=None, nodes_per_launch=4,
                  lds_points=None, timing=None, superline_threshold=None, superline_step=None):
    """the data sets of `<name>_opac_kdistr` and, with `target` = (temperatures, pressures), of `<name>_opac_ip_kdistr`, as
    ktable.build_species returns them for the directory exomol.py would write for the same arguments -- to the bit -- without the
    files.  `temps`: integers in K; `pressure_codes`: keys of ktable.pressure_table(); the range is 0 ... numax in one chunk.
    `timing` receives prepare_ms, sum_ms, kept (per node, node = p + np t) and build_table's entries; with super-lines
    (`superline_threshold`, `superline_step`, which defaults to dnu) also strong, weak and superlines per node"""
    out, source = _nodes.node_ktable(
        "exomol", backend, temps, pressure_codes, numax, dnu,
        lambda t, p, nu_grid: _check_node_inputs(t, p, nu_grid, molar_mass, cutoff, float(strength_cutoff)),
        lambda t, p, n_points: ExomolSlabs(states, trans, broadening, q_table, t, p, numax, dnu, n_points, molar_mass, cutoff,
                                           strength_cutoff, nodes_per_launch, superline_threshold, superline_step),
        inter, n_gauss, target, ctx, lds_points, timing, GRID_TOOL)
    if timing is not None:
        timing["prepare_ms"], timing["sum_ms"], timing["kept"] = float(source.ms[0]), float(source.ms[1]), list(source.kept)
        if source.superlines is not None:
            timing["strong"], timing["weak"], timing["superlines"] = ([c[k] for c in source.counts] for k in range(3))
    return out


# ---- the tool ----------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="exomol.py", description="line-by-line opacities of a species from an ExoMol line list")
    p.add_argument("-name", required=True)
    p.add_argument("-states", required=True, help="the .states file (.bz2 is read too)")
    p.add_argument("-trans", required=True, help="one or more .trans files separated by blanks, concatenated in this order")
    p.add_argument("-partition_function", required=True)
    p.add_argument("-broadeners", default=None, help="name:fraction:file[:gamma_default:n_default], separated by blanks")
    p.add_argument("-default_broadening", default="%g %g" % DEFAULT_BROADENING, help="gamma [cm^-1 / bar at 296 K] and n")
    p.add_argument("-strength_cutoff", type=float, default=0.0, help="S_min in cm / molecule: per node, transitions below it are left out")
    p.add_argument("-superline_threshold", type=float, default=None,
                   help="S_sl in cm / molecule: per node, kept transitions below it are merged per cell into super-lines")
    p.add_argument("-superline_step", type=float, default=None, help="the cell width d in cm^-1; -dnu unless given")
    _nodes.add_node_options(p)
    p.add_argument("-molar_mass", type=float, default=None)
    p.add_argument("-cutoff", type=float, default=DEFAULT_CUTOFF)
    _nodes.add_ktable_options(p)
    return _nodes.parse_node_args(p, argv)


def _print_kept(kept, nodes, n_trans, timing=None):
    """`timing` with super-lines: the three counts next to kept"""
    classes = None
    if timing is not None and "strong" in timing:
        classes = [np.asarray(timing[k]).reshape(-1) for k in ("strong", "weak", "superlines")]
    for i, ((t, code), k) in enumerate(zip(nodes, kept)):
        more = "" if classes is None else ": %d strong, %d weak in %d super-lines" % tuple(int(c[i]) for c in classes)
        print("exomol: %d K, %s: %d of %d transitions kept%s" % (t, code, int(k), n_trans, more))


def main(argv=None):
    """exomol.py: the directory of one species, or with -ktable yes its k-table; returns the paths written"""
    opt = parse_args(argv)
    t0 = time.time()
    temps = _nodes.parse_temperatures(GRID_TOOL, opt.temperatures)
    codes, pressures = _nodes.parse_pressure_codes(GRID_TOOL, opt.pressure_codes)
    if opt.ktable == "yes":
        _nodes.refuse_with_ktable("exomol", opt)
    chunks = _nodes.chunk_limits(GRID_TOOL, opt.numin, opt.numax, opt.dnu, opt.chunk_width)
    if not (np.isfinite(opt.strength_cutoff) and opt.strength_cutoff >= 0):
        raise IOError("exomol: -strength_cutoff %r is not a finite number >= 0 cm / molecule" % (opt.strength_cutoff,))
    if not (np.isfinite(opt.cutoff) and opt.cutoff > 0):
        raise IOError("exomol: -cutoff %r is not > 0 cm^-1" % (opt.cutoff,))
    if opt.superline_step is not None and opt.superline_threshold is None:
        raise IOError("exomol: -superline_step %r without -superline_threshold" % (opt.superline_step,))
    try:                                                 # before the files are read; the largest nu_0 is checked with the list
        check_superlines(opt.superline_threshold, opt.superline_step, opt.cutoff, 0.0, opt.dnu)
    except ValueError as e:
        raise IOError(str(e))
    molar_mass = _nodes.mass_of("exomol", opt.name, opt.molar_mass)
    entries = parse_broadeners(opt.broadeners, parse_default_broadening(opt.default_broadening))
    q_table = read_partition_function(opt.partition_function)
    try:
        for t in temps:
            partition_value(q_table, t, "exomol")
    except ValueError as e:
        raise IOError(str(e))
    states = read_states(opt.states)
    t_parsed = time.time()
    trans, skipped = read_transitions(opt.trans.split(), states)
    n_trans = len(trans["nu0"])
    print("exomol: %d states of %s (largest J %.17g), %d transitions of %s, %d with nu_0 <= 0 skipped, read and sorted in %.2f s"
          % (len(states["E"]), opt.states, float(states["J"].max()), n_trans, opt.trans, skipped, time.time() - t_parsed))
    broadening = broadening_table(entries, int(states["jidx"].max()), print)
    try:
        check_superlines(opt.superline_threshold, opt.superline_step, opt.cutoff, trans["nu0"][-1], opt.dnu)
    except ValueError as e:
        raise IOError(str(e))
    if opt.ktable == "yes":
        def build(inter, target, timing):
            out = exomol_ktable(states, trans, broadening, q_table, temps, codes, opt.numax, opt.dnu, inter, opt.number_of_gaussian_points,
                                molar_mass, opt.cutoff, opt.strength_cutoff, target, opt.backend, None, opt.nodes_per_launch, None, timing,
                                opt.superline_threshold, opt.superline_step)
            by_pressure = sorted(set(codes), key=lambda c: pressures[codes.index(c)])
            _print_kept(timing["kept"], [(t, c) for t in sorted(set(temps)) for c in by_pressure], n_trans, timing)
            return out
        return _nodes.main_ktable(
            "exomol", opt, build, lambda timing: "count to ranges %.1f ms, k_exomol_sum %.1f ms, k_ktable_bins %.1f ms" % (
                timing["prepare_ms"], timing["sum_ms"], timing["device_ms"][0]), t0)
    n_nodes = len(temps) * len(codes)

    def opacity(nu_grid, ctx, handle, timing):
        kappa = exomol_opacity(states, trans, broadening, q_table, temps, pressures, nu_grid, molar_mass, opt.cutoff, opt.strength_cutoff,
                               opt.backend, ctx, opt.nodes_per_launch, handle, timing, opt.superline_threshold,
                               None if opt.superline_threshold is None else opt.dnu if opt.superline_step is None else opt.superline_step)
        if nu_grid[0] == chunks[0][0]:                  # neither the cut nor the cells depend on the chunk
            _print_kept(timing["kept"].reshape(-1), [(t, c) for t in temps for c in codes], n_trans, timing)
        return kappa
    return _nodes.main_files(
        "exomol", opt, chunks, temps, codes,
        lambda ctx, n_points_max: ExomolOpacity.of(ctx, states, trans, broadening, n_points_max, max(1, min(opt.nodes_per_launch, n_nodes)),
                                                   n_nodes, True),
        opacity, lambda timing: "count to ranges %.1f ms, k_exomol_sum %.1f ms" % (timing["prepare_ms"], timing["sum_ms"]), t0, pairs=True)
