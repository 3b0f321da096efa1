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

`backend="device"`: k_lines_prepare writes the four numbers of every line for the node, k_lines_sum gives a workgroup a tile of
TILE_POINTS consecutive points and walks the lines that can reach it, LDS_BLOCK at a time, in order, without atomics.
`backend="numpy"` computes the same contract on the CPU, line after line over the points in reach: the checker of the device
path, and what a machine without a GPU gets when it asks for it.

`-ktable yes`: from the line list to the species' k-table without the files (line_ktable).  k_lines_prepare_nodes and
k_lines_sum_nodes take `-nodes_per_launch` nodes per launch and leave their fp32 slabs on the device, where k_ktable_bins
(ktable.KTableBuilder.run_device) sorts them on the same stream; nothing but the table comes back.  The containers are the ones
`lines.py` followed by `ktable.py` writes, to the bit, and what makes them so is part of the contract: the range is the one chunk
0 ... numax (a chunk's nu is lo + i dnu, so chunks have other bits); the line kernel steps with the `-dnu` given, the k-table's
axis with numax / points, which is what ktable.py computes from a file's length -- the two are not always the same double, and each
side keeps its own; temperatures and pressures are sorted ascending and de-duplicated as ktable.SpeciesFiles does, node = p + np t;
ktable.check_empty_bins and the limit of 2^28 points stand before the first launch.  Refused with `-ktable yes`: `-numin` other
than 0, `-chunk_width`, `-output_format text`, `-output_directory` (files or table, one per call).
"""
import argparse
import ctypes
import os
import time

import numpy as np

from . import phys_const as pc
from ._tool import DeviceObject, dp
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


def read_partition_function(path):
    """(T, Q) of a two-column text file"""
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
                raise IOError("lines: %s does not hold the finite numbers T and Q(T)" % where)
            if t and not v[0] > t[-1]:
                raise IOError("lines: %s: the temperatures strictly ascend" % where)
            t.append(v[0]); q.append(v[1])
    if len(t) < 2:
        raise IOError("lines: %s holds fewer than two rows of T and Q(T)" % path)
    return np.array(t), np.array(q)


def partition_value(q_table, temp):
    """Q(temp), linear in T between the file's rows"""
    t, q = (np.asarray(a, np.float64) for a in q_table)
    temp = float(temp)
    if not (t[0] <= temp <= t[-1]):
        raise ValueError("lines: T = %.17g K lies outside the partition function's %.17g ... %.17g K" % (temp, t[0], t[-1]))
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
class LineOpacity(DeviceObject):
    """hx_lines: a resident line list of up to n_lines_max lines, nodes of up to n_points_max spectral points"""

    PREFIX = "hx_lines"

    def __init__(self, ctx, n_lines_max, n_points_max, nodes_per_launch=0, n_nodes_max=0):
        """`nodes_per_launch` > 0: the handle also runs up to that many of n_nodes_max nodes per launch into fp32 slabs that
        stay on the device (set_nodes, run_nodes, slab_pointer)"""
        self.n_lines_max, self.n_points_max = int(n_lines_max), int(n_points_max)
        self.nodes_per_launch, self.n_nodes_max = int(nodes_per_launch), int(n_nodes_max)
        self.n_lines = self.n_points = self.n_nodes = self.node_points = self.rows_run = 0
        if self.nodes_per_launch > 0:
            self._create(ctx, self.n_lines_max, self.n_points_max, self.nodes_per_launch, self.n_nodes_max,
                         constructor="create_nodes")
        else:
            self._create(ctx, self.n_lines_max, self.n_points_max)

    def set_lines(self, lines):
        arr = [np.ascontiguousarray(lines[k], np.float64).reshape(-1) for k in FIELDS]
        assert all(len(a) == len(arr[0]) for a in arr)
        self._call("set_lines", len(arr[0]), *[dp(a) for a in arr])
        self.n_lines = len(arr[0])

    def run(self, temp, press, q_t, q_ref, molar_mass, self_fraction, cutoff, nu_first, dnu, n_points):
        self._call("run", float(temp), float(press), float(q_t), float(q_ref), float(molar_mass), float(self_fraction),
                   float(cutoff), float(nu_first), float(dnu), int(n_points))
        self.n_points = int(n_points)

    def set_nodes(self, temps, pressures, q_t, q_ref, molar_mass, self_fraction, cutoff, nu_first, dnu, n_points):
        """T, P and Q(T) per node, and what the nodes share; the tiles' line ranges go to the device once, here"""
        arr = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (temps, pressures, q_t)]
        assert len(arr[0]) == len(arr[1]) == len(arr[2])
        self.n_nodes = self.rows_run = 0
        self._call("set_nodes", len(arr[0]), dp(arr[0]), dp(arr[1]), dp(arr[2]), float(q_ref), float(molar_mass),
                   float(self_fraction), float(cutoff), float(nu_first), float(dnu), int(n_points))
        self.n_nodes, self.node_points = len(arr[0]), int(n_points)

    def run_nodes(self, first, n):
        """queues nodes first ... first + n - 1 into slab rows 0 ... n - 1; returns at once"""
        self._call("run_nodes", int(first), int(n))
        self.rows_run = int(n)

    def slab_pointer(self):
        """device address of the fp32 slabs [nodes_per_launch][...], rows of the last run_nodes with the stride n_points"""
        p = ctypes.c_void_p()
        self._call("device_ptr", b"slabs32", ctypes.byref(p))
        return p

    def _results(self):
        return {"kappa64": self.n_points, "kappa32": (self.n_points, np.float32), "line_params": (4, self.n_lines),
                "slabs32": ((self.rows_run, self.node_points), np.float32), "timing_ms": 2}


def device_voigt(ctx, x, y):
    """k_lines_sum's own K at pairs (x, y)"""
    from . import _lib
    x, y = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (x, y))
    assert len(x) == len(y)
    out = np.zeros(len(x))
    ctx.check(_lib.lib().hx_lines_voigt(ctx.handle, len(x), dp(x), dp(y), dp(out)), "hx_lines_voigt")
    return out


# ---- the library function ----------------------------------------------------------------------------------------------
def _check_node_inputs(temps, pressures, nu_grid, molar_mass, self_fraction, cutoff):
    temps = np.asarray(temps, np.float64).reshape(-1)
    pressures = np.asarray(pressures, np.float64).reshape(-1)
    if len(temps) == 0 or not np.all(np.isfinite(temps) & (temps > 0)):
        raise ValueError("lines: every temperature is a finite number > 0 (got %r)" % (temps.tolist(),))
    if len(pressures) == 0 or not np.all(np.isfinite(pressures) & (pressures > 0)):
        raise ValueError("lines: every pressure is a finite number > 0 dyne cm^-2 (got %r)" % (pressures.tolist(),))
    nu_first, dnu, n_points = float(nu_grid[0]), float(nu_grid[1]), int(nu_grid[2])
    if not (np.isfinite(dnu) and dnu > 0):
        raise ValueError("lines: dnu = %r is not > 0" % (dnu,))
    if n_points < 1 or not np.isfinite(nu_first):
        raise ValueError("lines: the grid (nu_first, dnu, points) = %r needs a finite start and at least one point" % (tuple(nu_grid),))
    if molar_mass is None or not (np.isfinite(molar_mass) and molar_mass > 0):
        raise ValueError("lines: no molar mass (got %r): give one > 0 g/mol" % (molar_mass,))
    if not 0.0 <= self_fraction <= 1.0:
        raise ValueError("lines: the self-broadening fraction %r lies outside [0, 1]" % (self_fraction,))
    if not (np.isfinite(cutoff) and cutoff > 0):
        raise ValueError("lines: the cut-off %r is not > 0 cm^-1" % (cutoff,))
    return temps, pressures, (nu_first, dnu, n_points)


def line_opacity(lines, q_table, temps, pressures_cgs, nu_grid, molar_mass=None, self_fraction=0.0, cutoff=DEFAULT_CUTOFF,
                 backend="device", ctx=None, handle=None, timing=None):
    """kappa [T][P][nu] in cm^2 g^-1, fp64.  `lines`: the seven arrays of FIELDS (sorted here); `q_table`: (T, Q); `nu_grid`:
    (nu of point 0, dnu, points); `handle`: a LineOpacity that already holds the list.  `timing` receives prepare_ms, sum_ms and
    pairs, summed over the nodes, and from the numpy backend pairs_by_region [4]"""
    if backend not in ("device", "numpy"):
        raise ValueError("lines: backend is device or numpy (got %r)" % (backend,))
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
        own_ctx, own_handle = ctx is None and handle is None, handle is None
        if own_ctx:
            from .device import Context
            ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
        try:
            if own_handle:
                handle = LineOpacity(ctx, len(lines["nu0"]), n_points)
                handle.set_lines(lines)
            try:
                for it, t in enumerate(temps):
                    for ip, p in enumerate(pressures):
                        handle.run(t, p, q_t[it], q_ref, molar_mass, self_fraction, cutoff, nu_first, dnu, n_points)
                        out[it, ip] = handle.get("kappa64")
                        if timing is not None:
                            ms += handle.get("timing_ms")
                            pairs += count_pairs(handle.get("line_params")[0], nu_first, dnu, n_points, cutoff)
            finally:
                if own_handle:
                    handle.close()
        finally:
            if own_ctx:
                ctx.close()
    if timing is not None:
        timing["prepare_ms"] = timing.get("prepare_ms", 0.0) + float(ms[0])
        timing["sum_ms"] = timing.get("sum_ms", 0.0) + float(ms[1])
        timing["pairs"] = timing.get("pairs", 0) + pairs
        if backend == "numpy":
            timing["pairs_by_region"] = np.asarray(timing.get("pairs_by_region", np.zeros(4, np.int64))) + by_region
    return out


# ---- files -------------------------------------------------------------------------------------------------------------
def file_name(name, numin, numax, temp, code, ending=".bin"):
    return "Out_%s_%05d_%05d_%05d_%s%s" % (name, numin, numax, temp, code, ending)


def chunk_limits(numin, numax, dnu, chunk_width=None):
    """[(numin, numax, points)] of the files"""
    if not (np.isfinite(dnu) and dnu > 0):
        raise IOError("lines: -dnu %r is not > 0" % (dnu,))
    if numax <= numin:
        raise IOError("lines: -numax %d is not above -numin %d" % (numax, numin))
    width = numax - numin if chunk_width is None else int(chunk_width)
    if width <= 0:
        raise IOError("lines: -chunk_width %r is not > 0" % (chunk_width,))
    out = []
    for lo in range(numin, numax, width):
        hi = min(lo + width, numax)
        n = (hi - lo) / dnu
        if abs(n - round(n)) > 1e-9 * max(n, 1.0) or round(n) < 1:
            raise IOError("lines: dnu = %.17g does not divide the chunk %d ... %d cm^-1 into a whole number of points (%.17g)"
                          % (dnu, lo, hi, n))
        out.append((lo, hi, int(round(n))))
    return out


def write_file(path, nu, kappa64, output_format):
    k32 = np.asarray(kappa64).astype(np.float32)
    if output_format == "binary":
        k32.astype("<f4").tofile(path)
    else:
        with open(path, "w") as f:
            for row in zip(nu, k32):
                f.write("%.12g %.9g\n" % row)


# ---- from the line list to the k-table -----------------------------------------------------------------------------------
MAX_TABLE_POINTS = 1 << 28            # hx_ktable_create


class LineSlabs(object):
    """ktable.build_table's slabs from a line list: one chunk 0 ... numax of `n_points` points, the nodes sorted ascending and
    de-duplicated as ktable.SpeciesFiles does (node = p + np * t).  On the device the slabs never leave it; `ms` and `pairs`
    hold the kernel times and the pairs evaluated once the table is built"""

    def __init__(self, lines, q_table, temps, pressures, numax, dnu, n_points, molar_mass, self_fraction, cutoff,
                 nodes_per_launch=4, count=True):
        self.lines, self.numax, self.dnu, self.n_points = lines, int(numax), float(dnu), int(n_points)
        self.temps, self.press = sorted(set(temps)), sorted(set(pressures))
        self.molar_mass, self.self_fraction, self.cutoff = molar_mass, self_fraction, cutoff
        self.q_ref = partition_value(q_table, T_REF)
        self.q_t = [partition_value(q_table, t) for t in self.temps]
        self.nodes_per_launch, self.count = max(1, int(nodes_per_launch)), count
        self.handle, self.ms, self.pairs, self.by_region = None, np.zeros(2), 0, np.zeros(4, np.int64)

    def axis(self):
        return 0, self.numax, self.numax / self.n_points           # ktable.SpeciesFiles.resolution() of the file not written

    def _check(self, n_points):
        if n_points != self.n_points:
            raise IOError("lines: the k-table's axis 0 ... %d cm^-1 at %.17g cm^-1 has %d points, the line kernel's grid at "
                          "-dnu %.17g has %d" % (self.numax, self.numax / self.n_points, n_points, self.dnu, self.n_points))

    def host_slabs(self, pool, n_points):
        self._check(n_points)
        for it, t in enumerate(self.temps):
            for p in self.press:
                prm = line_params(self.lines, float(t), p, self.q_t[it], self.q_ref, self.molar_mass, self.self_fraction)
                yield numpy_node(prm, 0.0, self.dnu, self.n_points, self.cutoff, self.molar_mass,
                                 self.by_region if self.count else None).astype(np.float32)
        self.pairs = int(self.by_region.sum())

    def feed(self, b, pool, n_points):
        self._check(n_points)
        nodes = [(float(t), p, self.q_t[it]) for it, t in enumerate(self.temps) for p in self.press]
        per = min(self.nodes_per_launch, b.max_tp)
        self.handle = h = LineOpacity(b.ctx, len(self.lines["nu0"]), self.n_points, per, len(nodes))
        h.set_lines(self.lines)
        h.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], [n[2] for n in nodes], self.q_ref, self.molar_mass,
                    self.self_fraction, self.cutoff, 0.0, self.dnu, self.n_points)
        slabs = h.slab_pointer()
        for first in range(0, len(nodes), per):
            n = min(per, len(nodes) - first)
            h.run_nodes(first, n)
            b.run_device(slabs, n, first)

    def close(self):
        h, self.handle = self.handle, None
        if h is not None:
            try:
                self.ms = h.get("timing_ms")
            finally:
                h.close()
            if self.count:                          # nu_0' depends on P alone
                self.pairs = len(self.temps) * sum(count_pairs(self.lines["nu0"] + self.lines["delta_air"] * (p / ATM), 0.0,
                                                               self.dnu, self.n_points, self.cutoff) for p in self.press)


def line_ktable(lines, q_table, temps, pressure_codes, numax, dnu, inter, n_gauss, molar_mass=None, self_fraction=0.0,
                cutoff=DEFAULT_CUTOFF, target=None, backend="device", ctx=None, nodes_per_launch=4, lds_points=None, timing=None):
    """the data sets of `<name>_opac_kdistr` and, with `target` = (temperatures, pressures), of `<name>_opac_ip_kdistr`, as
    ktable.build_species returns them for the directory lines.py would write for the same arguments -- to the bit -- without the
    files.  `temps`: integers in K; `pressure_codes`: keys of ktable.pressure_table(); the range is 0 ... numax in one chunk.
    `timing` receives prepare_ms, sum_ms, pairs and build_table's entries"""
    from . import ktable
    if backend not in ("device", "numpy"):
        raise ValueError("lines: backend is device or numpy (got %r)" % (backend,))
    table = ktable.pressure_table()
    for c in pressure_codes:
        if c not in table:
            raise IOError("lines: pressure code %r is not in the table (n800 ... p400)" % (c,))
    for t in temps:
        if int(t) != t:
            raise IOError("lines: the temperature %r is not an integer in K" % (t,))
    temps, pressures = [int(t) for t in temps], [table[c] for c in pressure_codes]
    n_points = chunk_limits(0, int(numax), dnu)[0][2]
    _check_node_inputs(temps, pressures, (0.0, dnu, n_points), molar_mass, self_fraction, cutoff)
    if n_points > MAX_TABLE_POINTS:
        raise IOError("lines: %d spectral points, the k-table's kernel takes 1 ... %d" % (n_points, MAX_TABLE_POINTS))
    source = LineSlabs(sort_lines(lines), q_table, temps, pressures, numax, dnu, n_points, molar_mass, self_fraction, cutoff,
                       nodes_per_launch, count=timing is not None)
    out = ktable.build_table(source, inter, n_gauss, "hip" if backend == "device" else "numpy", ctx, source.nodes_per_launch,
                             ktable.LDS_POINTS if lds_points is None else lds_points, target, timing)
    if timing is not None:
        timing["prepare_ms"], timing["sum_ms"], timing["pairs"] = float(source.ms[0]), float(source.ms[1]), source.pairs
    return out


# ---- the tool ----------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="lines.py", description="line-by-line opacities of a species from a HITRAN line list")
    p.add_argument("-name", required=True)
    p.add_argument("-line_list", required=True)
    p.add_argument("-partition_function", required=True)
    p.add_argument("-temperatures", required=True, help="integers in K, separated by blanks")
    p.add_argument("-pressure_codes", required=True, help="HELIOS-K's codes, n800 ... p400, separated by blanks")
    p.add_argument("-numin", type=int, default=0)
    p.add_argument("-numax", type=int, required=True)
    p.add_argument("-dnu", type=float, required=True)
    p.add_argument("-output_directory", default=None, help="of the files; required without -ktable yes")
    p.add_argument("-chunk_width", type=int, default=None)
    p.add_argument("-output_format", default="binary", choices=("binary", "text"))
    p.add_argument("-isotopologue", default="1")
    p.add_argument("-molar_mass", type=float, default=None)
    p.add_argument("-self_fraction", type=float, default=0.0)
    p.add_argument("-cutoff", type=float, default=DEFAULT_CUTOFF)
    p.add_argument("-backend", default="device", choices=("device", "numpy"))
    p.add_argument("-ktable", default="no", choices=("yes", "no"),
                   help="the species' k-table in place of the files; the options below are ktable.py's")
    p.add_argument("-grid_format", default="fixed_resolution")
    p.add_argument("-wavelength_grid", default="50 0.34 200")
    p.add_argument("-path_to_grid_file", default=None)
    p.add_argument("-number_of_gaussian_points", type=int, default=20)
    p.add_argument("-directory_with_individual_files", default="./output/")
    p.add_argument("-interpolate", default="yes", choices=("yes", "no"))
    p.add_argument("-temperature_grid", default=None)
    p.add_argument("-pressure_grid", default=None)
    p.add_argument("-container", default="h5", choices=("h5", "npz"))
    p.add_argument("-nodes_per_launch", type=int, default=4)
    opt = p.parse_args(argv)
    if opt.ktable == "no" and opt.output_directory is None:
        p.error("the following arguments are required: -output_directory")
    return opt


def parse_temperatures(text):
    out = []
    for word in str(text).split():
        try:
            t = int(word)
        except ValueError:
            raise IOError("lines: the temperature %r is not an integer in K (the file name carries it)" % (word,))
        if t <= 0:
            raise IOError("lines: the temperature %r is not > 0 K" % (word,))
        out.append(t)
    if not out:
        raise IOError("lines: -temperatures holds no temperature")
    return out


def parse_pressure_codes(text):
    from .ktable import pressure_table
    table = pressure_table()
    codes = str(text).split()
    for c in codes:
        if c not in table:
            raise IOError("lines: pressure code %r is not in the table (n800 ... p400)" % (c,))
    if not codes:
        raise IOError("lines: -pressure_codes holds no code")
    return codes, [table[c] for c in codes]


def _refuse_with_ktable(opt):
    if opt.numin != 0:
        raise IOError("lines: -ktable yes with -numin %d: the k-table's wavelength axis starts at 0 cm^-1, and ktable.py refuses "
                      "a directory whose first chunk does not" % opt.numin)
    if opt.chunk_width is not None:
        raise IOError("lines: -ktable yes with -chunk_width %d: the table is built from the one chunk 0 ... numax; a chunk's "
                      "points are lo + i dnu, which are other bits than 0 + i dnu" % opt.chunk_width)
    if opt.output_format != "binary":
        raise IOError("lines: -ktable yes with -output_format %s: no opacity file is written, the fp32 opacities stay on the "
                      "device" % opt.output_format)
    if opt.output_directory is not None:
        raise IOError("lines: -ktable yes with -output_directory %s: a call writes the files or the table, not both; the table "
                      "goes to -directory_with_individual_files" % opt.output_directory)
    if opt.number_of_gaussian_points < 1:
        raise IOError("lines: -number_of_gaussian_points is an integer >= 1")
    if opt.nodes_per_launch < 1:
        raise IOError("lines: -nodes_per_launch is an integer >= 1")


def _main_ktable(opt, lines, q_table, temps, codes, molar_mass, t0):
    """-ktable yes: `<name>_opac_kdistr` and, with -interpolate yes, `<name>_opac_ip_kdistr`"""
    from . import ktable
    inter = ktable.wavelength_grid(opt.grid_format, opt.wavelength_grid.split(), opt.path_to_grid_file)
    target = ktable.target_grid(opt.temperature_grid, opt.pressure_grid) if opt.interpolate == "yes" else None
    timing = {}
    native, ip = line_ktable(lines, q_table, temps, codes, opt.numax, opt.dnu, inter, opt.number_of_gaussian_points, molar_mass,
                             opt.self_fraction, opt.cutoff, target, opt.backend, None, opt.nodes_per_launch, None, timing)
    stem = os.path.join(opt.directory_with_individual_files, opt.name)
    written = [ktable.write_table("%s_opac_kdistr.%s" % (stem, opt.container), native)]
    if ip is not None:
        written.append(ktable.write_table("%s_opac_ip_kdistr.%s" % (stem, opt.container), ip))
    how = "numpy" if opt.backend == "numpy" else "k_lines_prepare_nodes %.1f ms, k_lines_sum_nodes %.1f ms, k_ktable_bins %.1f ms" % (
        timing["prepare_ms"], timing["sum_ms"], timing["device_ms"][0])
    print("lines: %d nodes of %d points into %d bins x %d Gauss points, %d pairs, %s, %.2f s -> %s" % (
        timing["points"], chunk_limits(0, opt.numax, opt.dnu)[0][2], len(inter) - 1,
        opt.number_of_gaussian_points, timing["pairs"], how, time.time() - t0, ", ".join(written)))
    return written


def main(argv=None):
    """lines.py: the directory of one species, or with -ktable yes its k-table; returns the paths written"""
    opt = parse_args(argv)
    t0 = time.time()
    temps = parse_temperatures(opt.temperatures)
    codes, pressures = parse_pressure_codes(opt.pressure_codes)
    if opt.ktable == "yes":
        _refuse_with_ktable(opt)
    chunks = chunk_limits(opt.numin, opt.numax, opt.dnu, opt.chunk_width)
    if not 0.0 <= opt.self_fraction <= 1.0:
        raise IOError("lines: -self_fraction %r lies outside [0, 1]" % (opt.self_fraction,))
    molar_mass = opt.molar_mass
    if molar_mass is None:
        from .species_data import species_lib
        if opt.name not in species_lib:
            raise IOError("lines: no molar mass: %r is not in species_data.py, give -molar_mass" % (opt.name,))
        molar_mass = species_lib[opt.name].weight
    if not (np.isfinite(molar_mass) and molar_mass > 0):
        raise IOError("lines: no molar mass: -molar_mass %r is not > 0 g/mol" % (molar_mass,))
    q_table = read_partition_function(opt.partition_function)
    try:
        for t in [T_REF] + temps:
            partition_value(q_table, t)
    except ValueError as e:
        raise IOError(str(e))
    lines, skipped = read_line_list(opt.line_list, opt.isotopologue)
    n_lines = len(lines["nu0"])
    print("lines: %d lines of isotopologue %s of %s, %d lines of other isotopologues skipped" % (n_lines, opt.isotopologue,
                                                                                                 opt.line_list, skipped))
    if opt.ktable == "yes":
        return _main_ktable(opt, lines, q_table, temps, codes, molar_mass, t0)
    if opt.numin != 0:
        print("lines: -numin %d is not 0: ktable.py will refuse the directory" % opt.numin)
    directory = os.path.join(str(opt.output_directory), "")
    os.makedirs(directory, exist_ok=True)
    ending = ".bin" if opt.output_format == "binary" else ".dat"
    ctx = handle = None
    timing, written = {}, []
    try:
        if opt.backend == "device":
            from .device import Context
            ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
            handle = LineOpacity(ctx, n_lines, max(c[2] for c in chunks))
            handle.set_lines(lines)
        for lo, hi, n in chunks:
            kappa = line_opacity(lines, q_table, temps, pressures, (float(lo), opt.dnu, n), molar_mass, opt.self_fraction,
                                 opt.cutoff, opt.backend, ctx, handle, timing)
            nu = float(lo) + np.arange(n, dtype=np.float64) * opt.dnu
            for it, t in enumerate(temps):
                for ip, code in enumerate(codes):
                    written.append(directory + file_name(opt.name, lo, hi, t, code, ending))
                    write_file(written[-1], nu, kappa[it, ip], opt.output_format)
    finally:
        if handle is not None:
            handle.close()
        if ctx is not None:
            ctx.close()
    how = "numpy" if opt.backend == "numpy" else "k_lines_prepare %.1f ms, k_lines_sum %.1f ms" % (timing["prepare_ms"],
                                                                                                   timing["sum_ms"])
    print("lines: %d nodes x %d chunks, %d pairs, %s, %.2f s -> %d files in %s" % (
        len(temps) * len(codes), len(chunks), timing["pairs"], how, time.time() - t0, len(written), directory))
    return written
