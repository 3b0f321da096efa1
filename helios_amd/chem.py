"""Equilibrium chemistry of a hydrogen-dominated C-H-O gas, on the device (include/helios_hip.h section 14, csrc/chem.hip).

`helios.py -opacity_mixing on-the-fly`, `premix.py`, `ktable.py -mixed_table_production` and `sweep.py` read the mixing ratios of
`FastChem` species from a FastChem output directory.  This tool writes such a directory from the analytic network of Heng & Lyons
(2016, ApJ 817, 149) and Heng & Tsai (2016, ApJ 829, 104): three net reactions,
    CH4 + H2O <-> CO + 3 H2   (1),      CO2 + H2 <-> CO + H2O   (2),      2 CH4 <-> C2H2 + 3 H2   (3),
and one quintic in the methane abundance.  It gives H2, He, H2O, CO, CH4, CO2 and C2H2 and the mean molecular mass.

The input.  `-gibbs_file`: a text file, lines that start with `#` skipped, the columns T [K], dG1, dG2, dG3 [J/mol] of the three
reactions, T strictly ascending, at least two rows.  The tool holds no thermochemical table: the user supplies it.  Abundances:
n_O = metallicity * O/H and n_C = C/O * n_O; the default O/H is 4.898e-4 (log eps_O = 8.69, Asplund et al. 2009), C/O 0.55, He/H
0.085.

The contract.  All arithmetic is fp64 and nothing is contracted; the constants are phys_const's; every statement left to right.
Per node (T, P), P in bar, with i the last row with T_i <= T, at most rows - 2:
    u = (T - T_i) / (T_{i+1} - T_i),        dG_r = dG_r[i] + u * (dG_r[i+1] - dG_r[i])        (linear between the rows)
    R = K_B * N_A * 1e-7  [J/mol/K]  unless the caller gives another,        rt = R * T
    K1 = exp(-dG1 / rt) / P / P,        K2 = exp(-dG2 / rt),        K3 = exp(-dG3 / rt) / P / P,        d = n_O - n_C
    a_0 = -2 n_C
    a_1 = 8.0*K1/K2*d*d + 1.0 + 2.0*K1*d
    a_2 = 8.0*K1/K2*d + 2.0*K3 + K1
    a_3 = 2.0*K1/K2*(1.0 + 8.0*K3*d) + 2.0*K1*K3
    a_4 = 8.0*K1*K3/K2
    a_5 = 8.0*K1*K3*K3/K2
    f(x) = ((((a_5 x + a_4) x + a_3) x + a_2) x + a_1) x + a_0                                 (Horner from a_5 down)
The result is x = n_CH4, THE ROOT OF f IN [x_min, 2 n_C]: x_min = 0 for d >= 0 and 4(-d) / (1 + sqrt(1 + 16 K3 (-d))) for d < 0, the
positive root of 2 K3 x^2 + x - 2 (n_C - n_O) = 0, below which water would be negative; x = 2 n_C where f(2 n_C) <= 0 by rounding
(all carbon in methane).  f(x_min) <= 0 < f(2 n_C) and f changes sign once in the bracket.  How the root is found is the backend's
business; both backends here bisect on the bit patterns of the ends (the doubles >= 0 are ordered like their patterns), which
collapses the interval in at most 63 halvings wherever the root lies, and return the upper end.  From x:
    b = 1.0 + K1*x,        n_H2O = h = 4.0*n_O / (b + sqrt(b*b + 16.0*K1*x*n_O/K2))              (the oxygen balance; positive terms only)
    n_CO = K1*x*h,        n_CO2 = n_CO*h/K2,        n_C2H2 = K3*x*x,        n_He = 2.0 * He/H
    s = 1.0 + n_He + n_H2O + n_CO + n_CH4 + n_CO2 + n_C2H2                                        (the file's column order)
    H2 = 1.0 / s,  He = n_He / s,  H2O = n_H2O / s,  CO = n_CO / s,  CH4 = x / s,  CO2 = n_CO2 / s,  C2H2 = n_C2H2 / s
    mu = H2*w_H2 + He*w_He + H2O*w_H2O + CO*w_CO + CH4*w_CH4 + CO2*w_CO2 + C2H2*w_C2H2            (species_data.py's weights)
Water is NOT the reference script's `2 K3 x^2 + x + 2 (n_O - n_C)`: that is a difference of large numbers for C/O > 1 and loses up
to 8e-5 in fp64; the oxygen balance 2 n_O = h + n_CO + 2 n_CO2 solved for h is the same number with every digit.

Refused, with the value or the line: a Gibbs file with fewer than two rows, a number that is not finite or T that does not ascend;
a node temperature outside the Gibbs file (clamped dG gives nonsense, and the quintic degenerates below 100 K); P <= 0; an
abundance that is not finite, n_O <= 0, n_C <= 0, He/H < 0; an unknown sweep key; more Gibbs rows than MAX_ROWS, more rows, nodes
or chemistries than the device object was made for -- before any launch.

Not modelled: hydrogen conservation (H2 dominates: the n are per H2), atomic H, nitrogen, condensation, ions, and anything outside
the Gibbs file's temperatures.

`backend="device"`: k_chem_nodes, one thread per node in workgroups of THREADS, the chemistry is blockIdx.y, so all chemistries of
a call (a `-sweep`) are one launch; the Gibbs rows go through LDS once per workgroup (MAX_ROWS rows).  `backend="numpy"` computes
the same statements on the CPU.  The two differ where the device's exp differs from numpy's, a few 1e-16 in K.

The file.  `chem.dat`: one header line `#P(bar) T(k) m(u) H2 He H2O1 C1O1 C1H4 C1O2 C2H2`, then a row per node, T outer and P
inner (entry p + np * t), every number with 17 significant digits, so that Read.load_fastchem_data and ktable_mix.Chemistry read
back the bits that were computed.
"""
import argparse
import os
import time

import numpy as np

from . import phys_const as pc
from ._tool import DeviceObject, dp
from .species_data import species_lib

# csrc/chem.hip: CHEM_THREADS, CHEM_MAX_ROWS, CHEM_PLANES (tests/test_gpu_chem.py derives its sizes from these)
THREADS = 256
MAX_ROWS = 1024
PLANES = 8
MAX_NODES = 1 << 24
MAX_CHEM = 65535

SPECIES = ("H2", "He", "H2O", "CO", "CH4", "CO2", "C2H2")          # the file's column order, and the order of every sum
KEYS = SPECIES + ("mu",)
O_TO_H_SOLAR = 4.898e-4                                            # log eps_O = 8.69 (Asplund et al. 2009)
SWEEP_KEYS = ("c_to_o", "metallicity", "o_to_h")


def weights():
    return np.array([species_lib[s].weight for s in SPECIES], np.float64)


def header():
    return "#P(bar) T(k) m(u) " + " ".join(species_lib[s].fc_name for s in SPECIES)


def default_gas_constant():
    """R in J/mol/K from phys_const's K_B and N_A (erg)"""
    return pc.K_B * pc.N_A * 1e-7


# ---- the input -----------------------------------------------------------------------------------------------------------
class GibbsTable(object):
    """T [K] strictly ascending and dG1, dG2, dG3 [J/mol] per row"""
    __slots__ = ("temp", "dg")

    def __init__(self, temp, dg1, dg2, dg3):
        self.temp = np.ascontiguousarray(temp, np.float64).reshape(-1)
        self.dg = [np.ascontiguousarray(g, np.float64).reshape(-1) for g in (dg1, dg2, dg3)]
        check_table(self)


def check_table(t, where="the Gibbs table"):
    n = len(t.temp)
    if any(len(g) != n for g in t.dg):
        raise IOError("chem: %s: %d temperatures and %s values of dG" % (where, n, [len(g) for g in t.dg]))
    if n < 2:
        raise IOError("chem: %s holds %d rows; dG is linear between at least 2" % (where, n))
    for r in range(n):
        row = [t.temp[r]] + [g[r] for g in t.dg]
        if not np.all(np.isfinite(row)) or not t.temp[r] > 0:
            raise IOError("chem: %s, row %d: T = %r, dG = %r, %r, %r are not finite numbers, T > 0" % ((where, r) + tuple(row)))
        if r and not t.temp[r] > t.temp[r - 1]:
            raise IOError("chem: %s, row %d: T = %.17g does not lie above %.17g: T strictly ascends" % (where, r, t.temp[r],
                                                                                                       t.temp[r - 1]))


def read_gibbs_file(path):
    rows = []
    with open(path) as f:
        for nr, line in enumerate(f, 1):
            text = line.strip()
            if not text or text.startswith("#"):
                continue
            col = text.split()
            try:
                v = [float(c) for c in col[:4]]
            except ValueError:
                v = []
            if len(v) < 4 or not np.all(np.isfinite(v)):
                raise IOError("chem: line %d of %s (%r) does not hold the finite numbers T, dG1, dG2, dG3" % (nr, path, text[:60]))
            if rows and not v[0] > rows[-1][0]:
                raise IOError("chem: line %d of %s: T = %.17g does not lie above %.17g: T strictly ascends" % (nr, path, v[0],
                                                                                                             rows[-1][0]))
            rows.append(v)
    if len(rows) < 2:
        raise IOError("chem: %s holds %d rows; dG is linear between at least 2" % (path, len(rows)))
    a = np.array(rows)
    return GibbsTable(a[:, 0], a[:, 1], a[:, 2], a[:, 3])


def write_gibbs_file(path, temp, dg1, dg2, dg3):
    with open(path, "w") as f:
        f.write("# T [K], dG [J/mol] of CH4 + H2O <-> CO + 3 H2, CO2 + H2 <-> CO + H2O, 2 CH4 <-> C2H2 + 3 H2\n")
        for row in zip(temp, dg1, dg2, dg3):
            f.write(" ".join("%.17g" % v for v in row) + "\n")
    return path


def _as_table(t):
    return t if isinstance(t, GibbsTable) else GibbsTable(*t)


def check_inputs(table, temps, pressures_bar, o_abund, c_abund, he_to_h):
    temps = np.ascontiguousarray(temps, np.float64).reshape(-1)
    press = np.ascontiguousarray(pressures_bar, np.float64).reshape(-1)
    o = np.ascontiguousarray(o_abund, np.float64).reshape(-1)
    c = np.ascontiguousarray(c_abund, np.float64).reshape(-1)
    if len(temps) < 1 or len(press) < 1 or len(o) < 1 or len(o) != len(c):
        raise ValueError("chem: %d temperatures, %d pressures, %d values of n_O and %d of n_C: at least one of each, one n_C per n_O"
                         % (len(temps), len(press), len(o), len(c)))
    for t in temps:
        if not (t >= table.temp[0] and t <= table.temp[-1]):
            raise ValueError("chem: the node temperature %r K lies outside the Gibbs file's %r ... %r K" % (float(t), float(table.temp[0]),
                                                                                                         float(table.temp[-1])))
    for p in press:
        if not (np.isfinite(p) and p > 0):
            raise ValueError("chem: the node pressure %r bar is not a finite number > 0" % (float(p),))
    for name, a in (("n_O", o), ("n_C", c)):
        for v in a:
            if not (np.isfinite(v) and v > 0):
                raise ValueError("chem: %s = %r is not a finite number > 0" % (name, float(v)))
    if not (np.isfinite(he_to_h) and he_to_h >= 0):
        raise ValueError("chem: He/H = %r is not a finite number >= 0" % (he_to_h,))
    return temps, press, o, c


# ---- the contract in numpy ---------------------------------------------------------------------------------------------
def numpy_constants(table, temp, press, gas_constant):
    """K1, K2, K3 at the nodes (arrays of one shape)"""
    t = table.temp
    i = np.clip(np.searchsorted(t, temp, side="right") - 1, 0, len(t) - 2)
    u = (temp - t[i]) / (t[i + 1] - t[i])
    g = [dg[i] + u * (dg[i + 1] - dg[i]) for dg in table.dg]
    rt = gas_constant * temp
    return np.exp(-g[0] / rt) / press / press, np.exp(-g[1] / rt), np.exp(-g[2] / rt) / press / press


def coefficients(k1, k2, k3, n_o, n_c):
    """a_0 ... a_5 with the association the contract fixes"""
    d = n_o - n_c
    return (-2.0 * n_c,
            8.0 * k1 / k2 * d * d + 1.0 + 2.0 * k1 * d,
            8.0 * k1 / k2 * d + 2.0 * k3 + k1,
            2.0 * k1 / k2 * (1.0 + 8.0 * k3 * d) + 2.0 * k1 * k3,
            8.0 * k1 * k3 / k2,
            8.0 * k1 * k3 * k3 / k2)


def horner(a, x):
    return ((((a[5] * x + a[4]) * x + a[3]) * x + a[2]) * x + a[1]) * x + a[0]


def numpy_root(a, k3, n_o, n_c):
    """the root of the quintic in [x_min, 2 n_C] per entry, by bisection on the bit patterns"""
    d = n_o - n_c
    md = np.where(d < 0, -d, 0.0)
    x_min = np.where(d < 0, 4.0 * md / (1.0 + np.sqrt(1.0 + 16.0 * k3 * md)), 0.0)
    x_max = np.ascontiguousarray(np.broadcast_to(2.0 * n_c, x_min.shape))
    hi = x_max.view(np.int64).copy()
    lo = np.ascontiguousarray(x_min).view(np.int64).copy()
    full = ~(horner(a, x_max) > 0.0)
    lo[full] = hi[full]
    for _ in range(64):
        mid = lo + ((hi - lo) >> 1)
        neg = horner(a, mid.view(np.float64)) < 0.0
        lo = np.where(neg, mid, lo)
        hi = np.where(neg, hi, mid)
    return hi.view(np.float64)


def numpy_nodes(table, temps, pressures_bar, o_abund, c_abund, he_to_h, gas_constant=None, wts=None):
    """{key: [chem][T][P]} of the eight results, and "n_CH4", the root itself"""
    table = _as_table(table)
    gas_constant = default_gas_constant() if gas_constant is None else float(gas_constant)
    wts = weights() if wts is None else wts
    temps, press, o, c = [np.asarray(v, np.float64).reshape(-1) for v in (temps, pressures_bar, o_abund, c_abund)]
    shape = (len(o), len(temps), len(press))
    T = np.ascontiguousarray(np.broadcast_to(temps[None, :, None], shape))
    P = np.ascontiguousarray(np.broadcast_to(press[None, None, :], shape))
    n_o = np.ascontiguousarray(np.broadcast_to(o[:, None, None], shape))
    n_c = np.ascontiguousarray(np.broadcast_to(c[:, None, None], shape))
    with np.errstate(over="ignore", invalid="ignore"):
        k1, k2, k3 = numpy_constants(table, T, P, gas_constant)
        x = numpy_root(coefficients(k1, k2, k3, n_o, n_c), k3, n_o, n_c)
        b = 1.0 + k1 * x
        h = 4.0 * n_o / (b + np.sqrt(b * b + 16.0 * k1 * x * n_o / k2))
        co = k1 * x * h
        co2 = co * h / k2
        c2h2 = k3 * x * x
        n_he = 2.0 * float(he_to_h)
        s = 1.0 + n_he + h + co + x + co2 + c2h2
        out = {"H2": 1.0 / s, "He": n_he / s, "H2O": h / s, "CO": co / s, "CH4": x / s, "CO2": co2 / s, "C2H2": c2h2 / s}
        mu = out["H2"] * wts[0]
        for j, name in enumerate(SPECIES[1:], 1):
            mu = mu + out[name] * wts[j]
    out["mu"] = mu
    out["n_CH4"] = x
    return out


# ---- device ------------------------------------------------------------------------------------------------------------
class ChemDevice(DeviceObject):
    """hx_chem: a resident Gibbs table of up to max_rows rows, up to max_nodes nodes and max_chem chemistries per launch"""

    PREFIX = "hx_chem"

    def __init__(self, ctx, max_rows, max_nodes, max_chem):
        if max_rows > MAX_ROWS:
            raise ValueError("chem: %d Gibbs rows, the kernel stages 2 ... %d through LDS" % (max_rows, MAX_ROWS))
        self.max_rows, self.max_nodes, self.max_chem = int(max_rows), int(max_nodes), int(max_chem)
        self.n_nodes = self.n_chem = 0
        self._create(ctx, self.max_rows, self.max_nodes, self.max_chem)

    def set_table(self, table, gas_constant=None):
        table = _as_table(table)
        self.n_nodes = self.n_chem = 0
        self._call("set_table", len(table.temp), dp(table.temp), dp(table.dg[0]), dp(table.dg[1]), dp(table.dg[2]),
                   default_gas_constant() if gas_constant is None else float(gas_constant))

    def set_nodes(self, temps, pressures_bar):
        """T and P per node, arrays of one length"""
        t, p = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (temps, pressures_bar)]
        assert len(t) == len(p)
        self.n_nodes = self.n_chem = 0
        self._call("set_nodes", len(t), dp(t), dp(p))
        self.n_nodes = len(t)

    def run(self, o_abund, c_abund, he_to_h, wts=None):
        """queues the kernel for the abundance pairs; returns at once"""
        o, c = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (o_abund, c_abund)]
        assert len(o) == len(c)
        w = np.ascontiguousarray(weights() if wts is None else wts, np.float64)
        assert len(w) == len(SPECIES)
        self.n_chem = 0
        self._call("run", len(o), dp(o), dp(c), float(he_to_h), dp(w))
        self.n_chem = len(o)

    def _results(self):
        return {"vmr": (self.n_chem, PLANES, self.n_nodes), "timing_ms": 2}


# ---- the library functions -----------------------------------------------------------------------------------------------
def cho_chemistry(gibbs_table, temps, pressures_bar, o_abund, c_abund, he_to_h, backend="device", gas_constant=None, ctx=None,
                  timing=None):
    """{H2, He, H2O, CO, CH4, CO2, C2H2, mu: fp64 [chem][T][P]}.  `gibbs_table`: a GibbsTable or (T, dG1, dG2, dG3); `o_abund`,
    `c_abund`: n_O and n_C, one entry per chemistry; `gas_constant` [J/mol/K]: None is K_B * N_A of phys_const.  `timing` receives
    kernel_ms"""
    if backend not in ("device", "numpy"):
        raise ValueError("chem: backend is device or numpy (got %r)" % (backend,))
    table = _as_table(gibbs_table)
    temps, press, o, c = check_inputs(table, temps, pressures_bar, o_abund, c_abund, he_to_h)
    n_nodes = len(temps) * len(press)
    if len(table.temp) > MAX_ROWS:
        raise ValueError("chem: %d Gibbs rows, the tool takes 2 ... %d" % (len(table.temp), MAX_ROWS))
    if n_nodes > MAX_NODES or len(o) > MAX_CHEM:
        raise ValueError("chem: %d nodes and %d chemistries; a call takes up to %d and %d" % (n_nodes, len(o), MAX_NODES, MAX_CHEM))
    if backend == "numpy":
        out = numpy_nodes(table, temps, press, o, c, he_to_h, gas_constant)
        return {k: out[k] for k in KEYS}
    own_ctx = ctx is None
    if own_ctx:
        from .device import Context
        ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    try:
        h = ChemDevice(ctx, len(table.temp), n_nodes, len(o))
        try:
            h.set_table(table, gas_constant)
            h.set_nodes(np.repeat(temps, len(press)), np.tile(press, len(temps)))
            h.run(o, c, he_to_h)
            vmr = h.get("vmr").reshape(len(o), PLANES, len(temps), len(press))
            if timing is not None:
                timing["kernel_ms"] = timing.get("kernel_ms", 0.0) + float(h.get("timing_ms")[0])
        finally:
            h.close()
    finally:
        if own_ctx:
            ctx.close()
    return {k: np.ascontiguousarray(vmr[:, j]) for j, k in enumerate(KEYS)}


def write_fastchem_directory(directory, temps, pressures_bar, result, chem=0):
    """`directory`/chem.dat of chemistry `chem` of a cho_chemistry result: T outer, P inner; returns the file's path"""
    directory = os.path.join(str(directory), "")
    os.makedirs(directory, exist_ok=True)
    temps, press = np.asarray(temps, np.float64).reshape(-1), np.asarray(pressures_bar, np.float64).reshape(-1)
    cols = [np.asarray(result[k], np.float64)[chem] for k in KEYS]
    for k, a in zip(KEYS, cols):
        if a.shape != (len(temps), len(press)):
            raise ValueError("chem: %s has the shape %r for %d temperatures x %d pressures" % (k, a.shape, len(temps), len(press)))
        if not np.all(np.isfinite(a)):
            t, p = np.argwhere(~np.isfinite(a))[0]
            raise ValueError("chem: %s is not finite at T = %.17g K, P = %.17g bar: the constants overflow there" % (k, temps[t],
                                                                                                                   press[p]))
    path = directory + "chem.dat"
    with open(path, "w") as f:
        f.write(header() + "\n")
        for t in range(len(temps)):
            for p in range(len(press)):
                row = [press[p], temps[t], cols[7][t, p]] + [cols[j][t, p] for j in range(7)]
                f.write(" ".join("%.17g" % v for v in row) + "\n")
    return path


# ---- the tool ----------------------------------------------------------------------------------------------------------
def parse_sweep(text):
    """`c_to_o=0.3,0.55;metallicity=1,10` -> [(key, [values])], in the order given"""
    out = []
    for part in str(text).split(";"):
        key, _, values = part.partition("=")
        key = key.strip()
        if key not in SWEEP_KEYS:
            raise IOError("chem: -sweep: unknown key %r; a sweep goes over %s" % (key, ", ".join(SWEEP_KEYS)))
        if key in [k for k, _v in out]:
            raise IOError("chem: -sweep names %r twice" % (key,))
        try:
            vals = [float(v) for v in values.split(",") if v.strip()]
        except ValueError:
            vals = []
        if not vals:
            raise IOError("chem: -sweep: %r holds no list of numbers for %s" % (part, key))
        out.append((key, vals))
    return out


def sweep_cases(base, sweep):
    """the parameter sets of a sweep, the first key slowest"""
    cases = [dict(base)]
    for key, vals in sweep:
        cases = [dict(c, **{key: v}) for c in cases for v in vals]
    return cases


def sweep_directories(directory, n):
    """`DIR` with `_0`, `_1`, ... behind its name"""
    stem = str(directory).rstrip("/")
    return ["%s_%d/" % (stem, k) for k in range(int(n))]


def sweep_argument(dirs):
    """the list in the form sweep.py's and premix.py's `-sweep` take"""
    return "directory_with_fastchem_files=" + ",".join(dirs)


def abundances(cases):
    o = np.array([c["metallicity"] * c["o_to_h"] for c in cases], np.float64)
    return o, np.array([c["c_to_o"] for c in cases], np.float64) * o


def node_grid(opt):
    """(T [K], P [bar]) of -grid_like, or of -temperature_grid and -pressure_grid"""
    if opt.grid_like is not None:
        if opt.temperature_grid is not None or opt.pressure_grid is not None:
            raise IOError("chem: -grid_like goes without -temperature_grid and -pressure_grid")
        from .continuum import grid_like
        g = grid_like(opt.grid_like)
        return g["temperatures"], g["pressures"] * 1e-6
    if opt.temperature_grid is None or opt.pressure_grid is None:
        raise IOError("chem: give -temperature_grid and -pressure_grid, or -grid_like")
    try:
        a, b, step = [float(v) for v in str(opt.temperature_grid).split()]
        temp = a + step * np.arange(int(round((b - a) / step)) + 1)
        a, b, n = str(opt.pressure_grid).split()
        press = 10.0 ** np.linspace(float(a), float(b), int(n))
    except (ValueError, ZeroDivisionError):
        raise IOError("chem: -temperature_grid takes 'first last step', -pressure_grid 'log10first log10last nodes' in bar")
    if len(temp) < 1 or len(press) < 1 or np.any(np.diff(temp) <= 0) or np.any(np.diff(press) <= 0):
        raise IOError("chem: the grid's nodes must ascend")
    return temp, press


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="chem.py", description="C-H-O equilibrium chemistry as a FastChem output directory")
    p.add_argument("-gibbs_file", required=True, help="T [K], dG1, dG2, dG3 [J/mol] per row")
    p.add_argument("-output_directory", required=True)
    p.add_argument("-o_to_h", type=float, default=O_TO_H_SOLAR)
    p.add_argument("-metallicity", type=float, default=1.0)
    p.add_argument("-c_to_o", type=float, default=0.55)
    p.add_argument("-he_to_h", type=float, default=0.085)
    p.add_argument("-temperature_grid", default=None, help="'first last step' in K")
    p.add_argument("-pressure_grid", default=None, help="'log10first log10last nodes' in bar")
    p.add_argument("-grid_like", default=None, help="an opacity container whose (T, P) nodes the table takes")
    p.add_argument("-backend", default="device", choices=("device", "numpy"))
    p.add_argument("-sweep", default=None, help="\"c_to_o=0.3,0.55,1.1;metallicity=1,10\": one directory per combination")
    return p.parse_args(argv)


def main(argv=None):
    """chem.py: one directory, or one per combination of `-sweep`; returns the directories written"""
    opt = parse_args(argv)
    t0 = time.time()
    base = {"o_to_h": opt.o_to_h, "metallicity": opt.metallicity, "c_to_o": opt.c_to_o}
    sweep = parse_sweep(opt.sweep) if opt.sweep is not None else None
    cases = sweep_cases(base, sweep) if sweep else [base]
    table = read_gibbs_file(opt.gibbs_file)
    temp, press = node_grid(opt)
    o, c = abundances(cases)
    timing = {}
    result = cho_chemistry(table, temp, press, o, c, opt.he_to_h, opt.backend, None, None, timing)
    dirs = sweep_directories(opt.output_directory, len(cases)) if sweep else [os.path.join(str(opt.output_directory), "")]
    for k, d in enumerate(dirs):
        write_fastchem_directory(d, temp, press, result, k)
        print("chem: %s: O/H %.6g x %.6g, C/O %.6g, He/H %.6g" % (d, cases[k]["o_to_h"], cases[k]["metallicity"], cases[k]["c_to_o"],
                                                                  opt.he_to_h))
    how = "numpy" if opt.backend == "numpy" else "k_chem_nodes %.3f ms" % timing["kernel_ms"]
    print("chem: %d chemistries x %d temperatures x %d pressures from %d Gibbs rows, %s, %.2f s" % (
        len(cases), len(temp), len(press), len(table.temp), how, time.time() - t0))
    if sweep:
        print("-sweep \"%s\"" % sweep_argument(dirs))
    return dirs
