"""Line-by-line opacities of one species from a HITRAN line list, on the device (include/helios_hip.h section 11, csrc/lines.hip).

`ktable.py` starts from the files `Out_<name>_<numin>_<numax>_<T>_<pcode>.bin` of HELIOS-K.  This tool makes them: it sums the
Voigt profiles of a line list, every line against every spectral point inside its cut-off, for every (T, P) node asked for.

Line list.  HITRAN's 160-character `.par` records in fixed columns (0-based, end exclusive): molecule 0:2, isotopologue 2:3,
nu_0 3:15 [cm^-1], S_ref 15:25 [cm/molecule at T_ref = 296 K], gamma_air 35:40 and gamma_self 40:45 [cm^-1 atm^-1], E'' 45:55
[cm^-1], n_air 55:59, delta_air 59:67 [cm^-1 atm^-1]; the rest of a record is ignored.  Lines of another isotopologue than the
one chosen are skipped and counted.  Refused, with the line: a record shorter than 67 characters, a field that is not a finite
number, nu_0 <= 0, S_ref < 0; and a list without a line of the chosen isotopologue.

Partition function.  A text file with the columns T [K] and Q(T); `#` lines are skipped, T strictly ascends, Q is interpolated
linearly in T.  A temperature outside the file is refused, and 296 K must be inside.

The contract.  All arithmetic is fp64 and nothing is contracted; H, C, K_B, N_A are phys_const's.  Per node (T, P), with
c2 = H C / K_B, P_atm = P / 1013250 dyne cm^-2 and the molar mass M [g/mol], per line, every statement evaluated left to right:
    S      = S_ref * (Q(296) / Q(T)) * exp(-c2 * E'' * (1/T - 1/296)) * (expm1(-c2 * nu_0 / T) / expm1(-c2 * nu_0 / 296))
    nu_0'  = nu_0 + delta_air * P_atm
    gamma  = (296 / T)^n_air * P_atm * (gamma_air * (1 - x_self) + gamma_self * x_self)
    alpha  = (nu_0' / C) * sqrt(2 * ln 2 * N_A * K_B * T / M)                   the Doppler half width at half maximum
    a      = sqrt(ln 2) / alpha,      y = max(a * gamma, 1e-8),      s = S * a * (1 / sqrt pi)
and per spectral point nu_i = nu_first + i * dnu
    sigma  = sum over the lines with |nu_i - nu_0'| <= C (inclusive) of s * K(a * (nu_i - nu_0'), y),
    kappa  = sigma * N_A / M [cm^2 g^-1], rounded once to fp32 when written.
The lines are sorted by (nu_0, position in the file), and every point adds its terms in ascending order of that index; the
pressure shift may move nu_0' past a neighbour and never changes the order.

K(x, y) = Re w(x + i y), the Faddeeva function, decided on r2 = x * x + y * y:
    r2 <= 42.25          Weideman's rational approximation with N = 40, L = sqrt(40 / sqrt 2): with l = L - i z, Z = (L + i z) / l
                         and p = the polynomial of lines_data.WEIDEMAN_A in Z by Horner, w = 2 p / l^2 + (1 / sqrt pi) / l
    42.25 < r2 <= 225    eight levels of Laplace's continued fraction w = (i / sqrt pi) / (z - 1/2 / (z - 1 / (z - 3/2 / (z - ...)))),
                         a level being one partial numerator k/2: t = z, then t = z - (k/2) / t for k = levels ... 1, w = (i/sqrt pi) / t
    225 < r2 <= 1e4      four levels
    r2 > 1e4             two levels
Complex division is written out (_k_weideman, _k_fraction below are the statements; csrc/lines.hip and tests/lines_reference.py
hold the same ones).  The first boundary stands at |z| = 6.5 and not at 6: the fraction has no term exp(-x^2), which at y = 1e-8
and |z| just above 6 is 1.42e-6 of K, more than the 1e-6 the scheme keeps everywhere; just above 6.5 it is 3.4e-9.  Against mpmath
(tests/golden/lines) the scheme keeps 1.2e-7 relative in the first region, 3.4e-9 in the second and 8e-11 in the two outer ones.  The
clamp y >= 1e-8 closes the domain; it changes only wings eight orders of magnitude below the core.

Not modelled: no renormalisation for the cut wings, no sub-Lorentzian factor, no pedestal subtraction, no line mixing, no
strength cut-off.

Output.  One file per (chunk, T, P): `Out_<name>_<numin:05d>_<numax:05d>_<T:05d>_<pcode>.bin`, raw little-endian fp32 at
nu_i = numin + i * dnu, i = 0 ... (numax - numin) / dnu - 1, which ktable.SpeciesFiles and ktable.spectral_axis read;
`-output_format text` writes the two columns nu and kappa (`.dat`, ktable.read_text_file).  Temperatures are integers in K
because the file name carries them; pressure codes are the keys of ktable.pressure_table().

`backend="device"`: a launch takes `nodes_per_launch` nodes.  k_lines_prepare_nodes writes the four numbers of every line per
node, k_lines_sum_nodes gives a workgroup a tile of TILE_POINTS consecutive points of a node's row and walks the lines that can
reach it, LDS_BLOCK at a time, in order, without atomics; the fp32 slabs stay on the device, and a handle made `with_fp64` keeps the
rows before rounding as well (line_opacity).  `backend="numpy"` computes the same contract on the CPU, line after line over the
points in reach: the checker of the device path, and what a machine without a GPU gets when it asks for it.

`-ktable yes`: from the line list to the species' k-table without the files (line_ktable): k_ktable_bins
(ktable.KTableBuilder.run_device) sorts the slabs on the same stream, and nothing but the table comes back.  The containers are those
`lines.py` followed by `ktable.py` writes, to the bit, and what makes them so is part of the contract: the range is the one chunk
0 ... numax (a chunk's nu is lo + i dnu, so chunks have other bits); the line kernel steps with the `-dnu` given, the k-table's
axis with numax / points, which is what ktable.py computes from a file's length -- the two are not always the same double, and each
side keeps its own; temperatures and pressures are sorted ascending and de-duplicated as ktable.SpeciesFiles does, node = p + np t;
ktable.check_empty_bins and the limit of 2^28 points stand before the first launch.  Refused with `-ktable yes`: `-numin` other
than 0, `-chunk_width`, `-output_format text`, `-output_directory` (files or table, one per call).

The frame -- chunks and file names, the checks of the nodes, the handle's node launches, the slab source and the front of
ktable.build_table, the common options and both ends of main -- is _nodes.py's, which cia.py and exomol.py share.
"""
import argparse
import time

import numpy as np

from . import _nodes
from . import phys_const as pc
from ._tool import dp
from .lines_data import WEIDEMAN_A, WEIDEMAN_L

T_REF = 296.0
ATM = 1013250.0                       # dyne cm^-2
Y_MIN = 1e-8
LN2 = 0.6931471805599453
INV_SQRT_PI = 0.5641895835477563
R2_WEIDEMAN, R2_EIGHT, R2_FOUR = 42.25, 225.0, 1.0e4
LEVELS = (8, 4, 2)                    # of the fraction in the regions beyond R2_WEIDEMAN, R2_EIGHT, R2_FOUR
DEFAULT_CUTOFF = 25.0
RECORD_MIN = 67
# csrc/lines.hip: LINES_THREADS, LINES_PPT, LINES_BLOCK, LINES_FAR (tests/test_gpu_lines.py derives its sizes from these)
THREADS = 256
POINTS_PER_THREAD = 4
TILE_POINTS = THREADS * POINTS_PER_THREAD
LDS_BLOCK = 256
WAVEFRONT = 64
FAR_Z = 101.0                         # a block takes the loop without region branches when every line has a * distance or y beyond it
FIELDS = ("nu0", "s_ref", "gamma_air", "gamma_self", "e_low", "n_air", "delta_air")
_COLUMNS = {"nu0": (3, 15), "s_ref": (15, 25), "gamma_air": (35, 40), "gamma_self": (40, 45), "e_low": (45, 55),
            "n_air": (55, 59), "delta_air": (59, 67)}


# ---- K(x, y) -----------------------------------------------------------------------------------------------------------
def _k_weideman(x, y):
    lr, li = WEIDEMAN_L + y, -x                     # l = L - i z
    nr, ni = WEIDEMAN_L - y, x                      # L + i z
    d = lr * lr + li * li
    zr, zi = (nr * lr + ni * li) / d, (ni * lr - nr * li) / d
    pr, pi = WEIDEMAN_A[0] + 0.0 * x, 0.0 * x
    for a in WEIDEMAN_A[1:]:
        pr, pi = pr * zr - pi * zi + a, pr * zi + pi * zr
    l2r, l2i = lr * lr - li * li, 2.0 * lr * li
    d2 = l2r * l2r + l2i * l2i
    return (2.0 * pr * l2r + 2.0 * pi * l2i) / d2 + INV_SQRT_PI * lr / d


def _k_fraction(x, y, levels):
    tr, ti = x, y
    for k in range(levels, 0, -1):
        c = 0.5 * k
        d = tr * tr + ti * ti
        tr, ti = x - c * tr / d, y + c * ti / d
    return INV_SQRT_PI * ti / (tr * tr + ti * ti)


def region(x, y):
    """0 ... 3 per pair: Weideman, eight, four, two levels"""
    r2 = np.asarray(x, np.float64) ** 2 + np.asarray(y, np.float64) ** 2
    return (r2 > R2_WEIDEMAN).astype(np.int32) + (r2 > R2_EIGHT) + (r2 > R2_FOUR)


def voigt_k(x, y):
    """K(x, y) of arrays of one shape, y > 0"""
    x, y = np.broadcast_arrays(np.asarray(x, np.float64), np.asarray(y, np.float64))
    x, y = x.reshape(-1), y.reshape(-1)
    r2 = x * x + y * y
    out = np.empty(len(x))
    reg = (r2 > R2_WEIDEMAN).astype(np.int8) + (r2 > R2_EIGHT) + (r2 > R2_FOUR)
    for r in range(4):
        m = reg == r
        if m.any():
            with np.errstate(over="ignore", invalid="ignore"):
                out[m] = _k_weideman(x[m], y[m]) if r == 0 else _k_fraction(x[m], y[m], LEVELS[r - 1])
    return out


# ---- the inputs --------------------------------------------------------------------------------------------------------
def read_line_list(path, isotopologue=1):
    """({field: array}, skipped) of a `.par` file: the lines of one isotopologue sorted by (nu_0, position in the file)"""
    cols = dict((k, []) for k in FIELDS)
    skipped = 0
    with open(path) as f:
        for nr, rec in enumerate(f, 1):
            rec = rec.rstrip("\r\n")
            if not rec.strip():
                continue
            where = "line %d of %s (%r)" % (nr, path, rec[:RECORD_MIN])
            if len(rec) < RECORD_MIN:
                raise IOError("lines: %s holds %d characters, a record needs %d" % (where, len(rec), RECORD_MIN))
            if rec[2:3].strip() != str(isotopologue):
                skipped += 1
                continue
            v = {}
            for k in FIELDS:
                lo, hi = _COLUMNS[k]
                try:
                    v[k] = float(rec[lo:hi])
                except ValueError:
                    v[k] = np.nan
                if not np.isfinite(v[k]):
                    raise IOError("lines: %s: %s = %r (columns %d:%d) is not a finite number" % (where, k, rec[lo:hi], lo, hi))
            if not v["nu0"] > 0:
                raise IOError("lines: %s: nu_0 = %r is not > 0" % (where, v["nu0"]))
            if v["s_ref"] < 0:
                raise IOError("lines: %s: S_ref = %r is negative" % (where, v["s_ref"]))
            for k in FIELDS:
                cols[k].append(v[k])
    if not cols["nu0"]:
        raise IOError("lines: %s holds no line of isotopologue %s (%d of other isotopologues)" % (path, isotopologue, skipped))
    return sort_lines(cols), skipped


def sort_lines(lines):
    """the seven arrays as contiguous fp64, sorted by (nu_0, position)"""
    arr = dict((k, np.asarray(lines[k], np.float64).reshape(-1)) for k in FIELDS)
    n = len(arr["nu0"])
    if n == 0 or any(len(arr[k]) != n for k in FIELDS):
        raise ValueError("lines: the seven per-line arrays have one length >= 1")
    for k in FIELDS:
        bad = ~np.isfinite(arr[k])
        if bad.any():
            raise ValueError("lines: line %d: %s = %r is not a finite number" % (int(np.argmax(bad)), k, float(arr[k][np.argmax(bad)])))
    if np.any(arr["nu0"] <= 0):
        j = int(np.argmax(arr["nu0"] <= 0))
        raise ValueError("lines: line %d: nu_0 = %r is not > 0" % (j, float(arr["nu0"][j])))
    if np.any(arr["s_ref"] < 0):
        j = int(np.argmax(arr["s_ref"] < 0))
        raise ValueError("lines: line %d: S_ref = %r is negative" % (j, float(arr["s_ref"][j])))
    order = np.argsort(arr["nu0"], kind="stable")
    return dict((k, np.ascontiguousarray(arr[k][order])) for k in FIELDS)


def read_partition_function(path, tool="lines"):
    """(T, Q) of a two-column text file; `tool`: the word of the caller's messages"""
    t, q = [], []
    with open(path) as f:
        for nr, line in enumerate(f, 1):
            if line.startswith("#") or not line.strip():
                continue
            where = "line %d of %s (%r)" % (nr, path, line.rstrip("\n"))
            col = line.split()
            try:
                v = [float(c) for c in col[:2]]
            except ValueError:
                v = []
            if len(v) < 2 or not np.all(np.isfinite(v)):
                raise IOError("%s: %s does not hold the finite numbers T and Q(T)" % (tool, where))
            if t and not v[0] > t[-1]:
                raise IOError("%s: %s: the temperatures strictly ascend" % (tool, where))
            t.append(v[0]); q.append(v[1])
    if len(t) < 2:
        raise IOError("%s: %s holds fewer than two rows of T and Q(T)" % (tool, path))
    return np.array(t), np.array(q)


def partition_value(q_table, temp, tool="lines"):
    """Q(temp), linear in T between the file's rows; `tool`: the word of the caller's messages"""
    t, q = (np.asarray(a, np.float64) for a in q_table)
    temp = float(temp)
    if not (t[0] <= temp <= t[-1]):
        raise ValueError("%s: T = %.17g K lies outside the partition function's %.17g ... %.17g K" % (tool, temp, t[0], t[-1]))
    j = min(int(np.searchsorted(t, temp, side="right")) - 1, len(t) - 2)
    if temp == t[j]:
        return float(q[j])
    if temp == t[j + 1]:
        return float(q[j + 1])
    return float(q[j] + (q[j + 1] - q[j]) * ((temp - t[j]) / (t[j + 1] - t[j])))


# ---- the contract in numpy ---------------------------------------------------------------------------------------------
def line_strength(lines, temp, q_t, q_ref):
    """S(T) per line [cm / molecule]"""
    c2 = pc.H * pc.C / pc.K_B
    nu0 = lines["nu0"]
    return lines["s_ref"] * (q_ref / q_t) * np.exp(-c2 * lines["e_low"] * (1.0 / temp - 1.0 / T_REF)) \
        * (np.expm1(-c2 * nu0 / temp) / np.expm1(-c2 * nu0 / T_REF))


def line_params(lines, temp, press, q_t, q_ref, molar_mass, self_fraction):
    """[4][lines]: nu_0', s = S a / sqrt pi, a, y of one node"""
    patm = press / ATM
    nu0 = lines["nu0"]
    s = line_strength(lines, temp, q_t, q_ref)
    nu0p = nu0 + lines["delta_air"] * patm
    gamma = (T_REF / temp) ** lines["n_air"] * patm * (lines["gamma_air"] * (1.0 - self_fraction) + lines["gamma_self"] * self_fraction)
    alpha = (nu0p / pc.C) * np.sqrt(2.0 * LN2 * pc.N_A * pc.K_B * temp / molar_mass)
    a = np.sqrt(LN2) / alpha
    y = np.maximum(a * gamma, Y_MIN)
    return np.stack([nu0p, s * a * INV_SQRT_PI, a, y])


def numpy_node(params, nu_first, dnu, n_points, cutoff, molar_mass, pairs=None):
    """kappa64 [n_points] of one node: the lines in ascending order, each over the points inside its cut-off.  `pairs`: a list of
    four counts that receives the pairs evaluated per region"""
    nu = nu_first + np.arange(n_points, dtype=np.float64) * dnu
    sigma = np.zeros(n_points)
    nu0p, s, a, y = params
    lo = np.clip(np.floor((nu0p - cutoff - nu_first) / dnu).astype(np.int64) - 2, 0, n_points)
    hi = np.clip(np.ceil((nu0p + cutoff - nu_first) / dnu).astype(np.int64) + 3, 0, n_points)
    for j in np.nonzero(hi > lo)[0]:
        sl = slice(lo[j], hi[j])
        d = nu[sl] - nu0p[j]
        inside = np.abs(d) <= cutoff
        if not inside.any():
            continue
        x = a[j] * d[inside]
        if pairs is not None:
            pairs += np.bincount(region(x, y[j]), minlength=4)
        term = s[j] * voigt_k(x, y[j])
        part = sigma[sl]
        part[inside] = part[inside] + term
    return sigma * pc.N_A / molar_mass


def count_pairs(nu0p, nu_first, dnu, n_points, cutoff):
    """the pairs (line, point) with |nu_i - nu_0'| <= cutoff, by the test the sums make"""
    nu0p = np.asarray(nu0p, np.float64)
    lo = np.clip(np.floor((nu0p - cutoff - nu_first) / dnu).astype(np.int64) - 2, 0, n_points)
    hi = np.clip(np.ceil((nu0p + cutoff - nu_first) / dnu).astype(np.int64) + 3, 0, n_points)
    for _ in range(6):                  # [lo, hi) shrinks onto the points that pass
        lo = np.where((lo < hi) & (np.abs(nu_first + lo * dnu - nu0p) > cutoff), lo + 1, lo)
        hi = np.where((lo < hi) & (np.abs(nu_first + (hi - 1) * dnu - nu0p) > cutoff), hi - 1, hi)
    return int(np.sum(hi - lo))


# ---- device ------------------------------------------------------------------------------------------------------------
class LineOpacity(_nodes.NodeOpacity):
    """hx_lines: a resident line list of up to n_lines_max lines, nodes of up to n_points_max spectral points, nodes_per_launch
    per launch into fp32 slabs that stay on the device; `with_fp64`: the rows before rounding as well"""

    PREFIX = "hx_lines"

    def __init__(self, ctx, n_lines_max, n_points_max, nodes_per_launch, n_nodes_max, with_fp64=False):
        self.n_lines_max, self.n_points_max = int(n_lines_max), int(n_points_max)
        self.nodes_per_launch, self.n_nodes_max, self.with_fp64 = int(nodes_per_launch), int(n_nodes_max), bool(with_fp64)
        self.n_lines = self.n_nodes = self.n_points = self.rows_run = 0
        self._create(ctx, self.n_lines_max, self.n_points_max, self.nodes_per_launch, self.n_nodes_max, int(self.with_fp64))

    @classmethod
    def of(cls, ctx, lines, n_points_max, nodes_per_launch, n_nodes_max, with_fp64=False):
        """a handle that holds the list"""
        h = cls(ctx, len(lines["nu0"]), n_points_max, nodes_per_launch, n_nodes_max, with_fp64)
        try:
            h.set_lines(lines)
        except Exception:
            h.close()
            raise
        return h

    def set_lines(self, lines):
        arr = [np.ascontiguousarray(lines[k], np.float64).reshape(-1) for k in FIELDS]
        assert all(len(a) == len(arr[0]) for a in arr)
        self._reset_nodes()
        self._call("set_lines", len(arr[0]), *[dp(a) for a in arr])
        self.n_lines = len(arr[0])

    def set_nodes(self, temps, pressures, q_t, q_ref, molar_mass, self_fraction, cutoff, nu_first, dnu, n_points):
        """T, P and Q(T) per node, and what the nodes share; the tiles' line ranges go to the device once, here"""
        arr = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (temps, pressures, q_t)]
        assert len(arr[0]) == len(arr[1]) == len(arr[2])
        self._reset_nodes()
        self._call("set_nodes", len(arr[0]), dp(arr[0]), dp(arr[1]), dp(arr[2]), float(q_ref), float(molar_mass),
                   float(self_fraction), float(cutoff), float(nu_first), float(dnu), int(n_points))
        self.n_nodes, self.n_points = len(arr[0]), int(n_points)

    def _results(self):
        return {"slabs32": ((self.rows_run, self.n_points), np.float32), "kappa64": (self.rows_run, self.n_points),
                "line_params": (self.rows_run, 4, self.n_lines), "timing_ms": 2}


def device_voigt(ctx, x, y):
    """the sum kernels' own K at pairs (x, y)"""
    from . import _lib
    x, y = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (x, y))
    assert len(x) == len(y)
    out = np.zeros(len(x))
    ctx.check(_lib.lib().hx_lines_voigt(ctx.handle, len(x), dp(x), dp(y), dp(out)), "hx_lines_voigt")
    return out


# ---- the library function ----------------------------------------------------------------------------------------------
def _check_node_inputs(temps, pressures, nu_grid, molar_mass, self_fraction, cutoff):
    out = _nodes.check_node_inputs("lines", temps, pressures, nu_grid, molar_mass)
    if not 0.0 <= self_fraction <= 1.0:
        raise ValueError("lines: the self-broadening fraction %r lies outside [0, 1]" % (self_fraction,))
    if not (np.isfinite(cutoff) and cutoff > 0):
        raise ValueError("lines: the cut-off %r is not > 0 cm^-1" % (cutoff,))
    return out


def line_opacity(lines, q_table, temps, pressures_cgs, nu_grid, molar_mass=None, self_fraction=0.0, cutoff=DEFAULT_CUTOFF,
                 backend="device", ctx=None, nodes_per_launch=4, handle=None, timing=None):
    """kappa [T][P][nu] in cm^2 g^-1, fp64.  `lines`: the seven arrays of FIELDS (sorted here); `q_table`: (T, Q); `nu_grid`:
    (nu of point 0, dnu, points); `handle`: a LineOpacity with fp64 rows that already holds the list.  `timing` receives
    prepare_ms, sum_ms and pairs, summed over the nodes, and from the numpy backend pairs_by_region [4]"""
    _nodes.check_backend("lines", backend)
    temps, pressures, (nu_first, dnu, n_points) = _check_node_inputs(temps, pressures_cgs, nu_grid, molar_mass, self_fraction, cutoff)
    if handle is None:
        lines = sort_lines(lines)
    q_ref = partition_value(q_table, T_REF)
    q_t = [partition_value(q_table, t) for t in temps]
    out = np.empty((len(temps), len(pressures), n_points))
    by_region = np.zeros(4, np.int64)
    pairs, ms = 0, np.zeros(2)
    if backend == "numpy":
        for it, t in enumerate(temps):
            for ip, p in enumerate(pressures):
                prm = line_params(lines, t, p, q_t[it], q_ref, molar_mass, self_fraction)
                out[it, ip] = numpy_node(prm, nu_first, dnu, n_points, cutoff, molar_mass, by_region if timing is not None else None)
        pairs = int(by_region.sum())
    else:
        nodes = [(t, p, q_t[it]) for it, t in enumerate(temps) for p in pressures]
        flat = out.reshape(len(nodes), n_points)

        def set_nodes(h, part):
            h.set_nodes([n[0] for n in part], [n[1] for n in part], [n[2] for n in part], q_ref, molar_mass, self_fraction, cutoff,
                        nu_first, dnu, n_points)

        def collect(h, rows):
            nonlocal pairs
            flat[rows] = h.get("kappa64")
            if timing is not None:
                pairs += sum(count_pairs(prm[0], nu_first, dnu, n_points, cutoff) for prm in h.get("line_params"))
        ms = _nodes.nodes_in_turns(
            ctx, handle, lambda c: LineOpacity.of(c, lines, n_points, max(1, min(int(nodes_per_launch), len(nodes))), len(nodes), True),
            nodes, set_nodes, collect)
    if timing is not None:
        timing["prepare_ms"] = timing.get("prepare_ms", 0.0) + float(ms[0])
        timing["sum_ms"] = timing.get("sum_ms", 0.0) + float(ms[1])
        timing["pairs"] = timing.get("pairs", 0) + pairs
        if backend == "numpy":
            timing["pairs_by_region"] = np.asarray(timing.get("pairs_by_region", np.zeros(4, np.int64))) + by_region
    return out


# ---- from the line list to the k-table -----------------------------------------------------------------------------------
class LineSlabs(_nodes.NodeSlabs):
    """ktable.build_table's slabs from a line list (_nodes.NodeSlabs); `ms` and `pairs` hold the kernel times and the pairs
    evaluated once the table is built"""

    TOOL = "lines"

    def __init__(self, lines, q_table, temps, pressures, numax, dnu, n_points, molar_mass, self_fraction, cutoff,
                 nodes_per_launch=4, count=True):
        _nodes.NodeSlabs.__init__(self, temps, pressures, numax, dnu, n_points, nodes_per_launch)
        self.lines, self.molar_mass, self.self_fraction, self.cutoff = lines, molar_mass, self_fraction, cutoff
        self.q_ref = partition_value(q_table, T_REF)
        self.q_t = [partition_value(q_table, t) for t in self.temps]
        self.count, self.pairs, self.by_region = count, 0, np.zeros(4, np.int64)

    def host_slab(self, it, t, p):
        prm = line_params(self.lines, t, p, self.q_t[it], self.q_ref, self.molar_mass, self.self_fraction)
        return numpy_node(prm, 0.0, self.dnu, self.n_points, self.cutoff, self.molar_mass, self.by_region if self.count else None)

    def host_slabs(self, pool, n_points):
        for slab in _nodes.NodeSlabs.host_slabs(self, pool, n_points):
            yield slab
        self.pairs = int(self.by_region.sum())

    def open_handle(self, ctx, per, nodes):
        self.handle = h = LineOpacity.of(ctx, self.lines, self.n_points, per, len(nodes))
        h.set_nodes([n[1] for n in nodes], [n[2] for n in nodes], [self.q_t[n[0]] for n in nodes], self.q_ref, self.molar_mass,
                    self.self_fraction, self.cutoff, 0.0, self.dnu, self.n_points)

    def close(self):
        counted = self.count and self.handle is not None
        _nodes.NodeSlabs.close(self)
        if counted:                                 # nu_0' depends on P alone
            self.pairs = len(self.temps) * sum(count_pairs(self.lines["nu0"] + self.lines["delta_air"] * (p / ATM), 0.0,
                                                           self.dnu, self.n_points, self.cutoff) for p in self.press)


def line_ktable(lines, q_table, temps, pressure_codes, numax, dnu, inter, n_gauss, molar_mass=None, self_fraction=0.0,
                cutoff=DEFAULT_CUTOFF, target=None, backend="device", ctx=None, nodes_per_launch=4, lds_points=None, timing=None):
    """the data sets of `<name>_opac_kdistr` and, with `target` = (temperatures, pressures), of `<name>_opac_ip_kdistr`, as
    ktable.build_species returns them for the directory lines.py would write for the same arguments -- to the bit -- without the
    files.  `temps`: integers in K; `pressure_codes`: keys of ktable.pressure_table(); the range is 0 ... numax in one chunk.
    `timing` receives prepare_ms, sum_ms, pairs and build_table's entries"""
    out, source = _nodes.node_ktable(
        "lines", backend, temps, pressure_codes, numax, dnu,
        lambda t, p, nu_grid: _check_node_inputs(t, p, nu_grid, molar_mass, self_fraction, cutoff),
        lambda t, p, n_points: LineSlabs(sort_lines(lines), q_table, t, p, numax, dnu, n_points, molar_mass, self_fraction, cutoff,
                                         nodes_per_launch, count=timing is not None),
        inter, n_gauss, target, ctx, lds_points, timing)
    if timing is not None:
        timing["prepare_ms"], timing["sum_ms"], timing["pairs"] = float(source.ms[0]), float(source.ms[1]), source.pairs
    return out


# ---- the tool ----------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="lines.py", description="line-by-line opacities of a species from a HITRAN line list")
    p.add_argument("-name", required=True)
    p.add_argument("-line_list", required=True)
    p.add_argument("-partition_function", required=True)
    _nodes.add_node_options(p)
    p.add_argument("-isotopologue", default="1")
    p.add_argument("-molar_mass", type=float, default=None)
    p.add_argument("-self_fraction", type=float, default=0.0)
    p.add_argument("-cutoff", type=float, default=DEFAULT_CUTOFF)
    _nodes.add_ktable_options(p)
    return _nodes.parse_node_args(p, argv)


def main(argv=None):
    """lines.py: the directory of one species, or with -ktable yes its k-table; returns the paths written"""
    opt = parse_args(argv)
    t0 = time.time()
    temps = _nodes.parse_temperatures("lines", opt.temperatures)
    codes, pressures = _nodes.parse_pressure_codes("lines", opt.pressure_codes)
    if opt.ktable == "yes":
        _nodes.refuse_with_ktable("lines", opt)
    chunks = _nodes.chunk_limits("lines", opt.numin, opt.numax, opt.dnu, opt.chunk_width)
    if not 0.0 <= opt.self_fraction <= 1.0:
        raise IOError("lines: -self_fraction %r lies outside [0, 1]" % (opt.self_fraction,))
    molar_mass = _nodes.mass_of("lines", opt.name, opt.molar_mass)
    q_table = read_partition_function(opt.partition_function)
    try:
        for t in [T_REF] + temps:
            partition_value(q_table, t)
    except ValueError as e:
        raise IOError(str(e))
    lines, skipped = read_line_list(opt.line_list, opt.isotopologue)
    print("lines: %d lines of isotopologue %s of %s, %d lines of other isotopologues skipped" % (len(lines["nu0"]), opt.isotopologue,
                                                                                                 opt.line_list, skipped))
    if opt.ktable == "yes":
        return _nodes.main_ktable(
            "lines", opt,
            lambda inter, target, timing: line_ktable(lines, q_table, temps, codes, opt.numax, opt.dnu, inter,
                                                      opt.number_of_gaussian_points, molar_mass, opt.self_fraction, opt.cutoff, target,
                                                      opt.backend, None, opt.nodes_per_launch, None, timing),
            lambda timing: "k_lines_prepare_nodes %.1f ms, k_lines_sum_nodes %.1f ms, k_ktable_bins %.1f ms" % (
                timing["prepare_ms"], timing["sum_ms"], timing["device_ms"][0]), t0, pairs=True)
    n_nodes = len(temps) * len(pressures)
    return _nodes.main_files(
        "lines", opt, chunks, temps, codes,
        lambda ctx, n_points_max: LineOpacity.of(ctx, lines, n_points_max, max(1, min(opt.nodes_per_launch, n_nodes)), n_nodes, True),
        lambda nu_grid, ctx, handle, timing: line_opacity(lines, q_table, temps, pressures, nu_grid, molar_mass, opt.self_fraction,
                                                          opt.cutoff, opt.backend, ctx, opt.nodes_per_launch, handle, timing),
        lambda timing: "k_lines_prepare_nodes %.1f ms, k_lines_sum_nodes_fp64 %.1f ms" % (timing["prepare_ms"], timing["sum_ms"]), t0,
        pairs=True)
