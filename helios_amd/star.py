"""Stellar spectrum files from model grids, on the device (include/helios_hip.h section 8, csrc/star.hip).

The reference's star tool (star_tool/functions.py::main_loop with source/tools.py::convert_spectrum and
calc_analyt_planck_in_interval): a star's spectrum -- the blend of up to eight PHOENIX corner files in (T_eff, log g, [M/H]),
or an ASCII, MUSCLES or BT-Settl file -- is re-binned onto the wavelength grid of an opacity container, bins the spectrum does
not cover take pi x the analytic Planck integral at a black-body temperature that is fitted by ten secant steps, and the
result goes to `/<convert_to>/<data_format>/<name>` of the stellar spectrum file that `stellar spectral model = file` reads.

The host reads the files, decides per interface which tabulated points it lies between (fp64, the reference's own
comparisons) and runs the secant steps; the blend, the Planck values and the re-binning run in k_star_blend,
k_star_planck_bins and k_star_rebin_*, or -- `backend="numpy"` -- in vectorised numpy, which is the checker of the device
path and what a machine without a GPU gets when it asks for it.  Nothing is ever fetched: an input that is not there is an
error that names it.
"""
import argparse
import os
import time

import numpy as np

from . import fits_lite
from . import hdf5_lite
from . import phys_const as pc
from ._tool import DeviceObject, dp, ip, vp

PARSEC = 3.0856775814913674e18        # cm: 648000 / pi astronomical units
PHOENIX_WAVE_FILE = "WAVE_PHOENIX-ACES-AGSS-COND-2011.fits"
PLANCK_TERMS = 199
SECANT_STEPS = 10
CHUNK = 1024                          # trapezoids of a long bin that the device stages and sums at a time
NARROW = 16                           # bins of up to this many points: the plain running sum (csrc/star.hip, ST_NARROW)
FORMATS = ("phoenix", "ascii", "muscles", "btsettl")
STAR_KEYS = {"data_format": str, "name": str, "temp": float, "log_g": float, "m": float, "source_file": str,
             "w_conversion_factor": float, "flux_conversion_factor": float, "distance_from_Earth": float, "R_star": float,
             "BB_temp": float}


# ---- the PHOENIX blend ----------------------------------------------------------------------------------------------------
def corner_nodes(teff, log_g, metal):
    """(tdown, tup, gdown, gup, mdown, mup): nodes 100 K apart below 7000 K and 200 K from there, 0.5 in log g and [M/H]"""
    if not (metal >= -2.0 and metal <= 1.0):
        raise ValueError("star: [M/H] = %r lies outside the PHOENIX grid, -2 ... 1 (the reference prints a message there and "
                         "then fails on an undefined name)" % (metal,))
    step = 100 if teff < 7000 else 200
    tdown, tup = int(step * np.floor(teff / step)), int(step * np.ceil(teff / step))
    gdown, gup = float(0.5 * np.floor(log_g / 0.5)), float(0.5 * np.ceil(log_g / 0.5))
    mdown, mup = float(0.5 * np.floor(metal / 0.5)), float(0.5 * np.ceil(metal / 0.5))
    return tdown, tup, gdown, gup, mdown, mup


def corner_name(t, g, m):
    return "{:05d}_{:.2f}_{:.1f}.fits".format(t, g, m)


def blend_plan(teff, log_g, metal):
    """the reference's branch for this star as a list of terms (corner file, (w0, w1, w2)) and the divisor: the flux is
    (sum of ((f * w0) * w1) * w2 in this order) / divisor.  Factors a branch does not have are 1, which changes no bit."""
    tdown, tup, gdown, gup, mdown, mup = corner_nodes(teff, log_g, metal)
    T = {"up": teff - tdown, "down": tup - teff}
    G = {"up": log_g - gdown, "down": gup - log_g}
    M = {"up": metal - mdown, "down": mup - metal}
    t_node, g_node, m_node = tup == tdown, gup == gdown, mup == mdown
    name = lambda t, g, m: corner_name(tup if t == "up" else tdown, gup if g == "up" else gdown, mup if m == "up" else mdown)
    # the order of the terms within every branch is the reference's
    if not t_node and not g_node and not m_node:
        order = [("up", "up", "up"), ("down", "up", "up"), ("up", "down", "up"), ("down", "down", "up"),
                 ("up", "up", "down"), ("down", "up", "down"), ("up", "down", "down"), ("down", "down", "down")]
        terms = [(name(t, g, m), (T[t], G[g], M[m])) for t, g, m in order]
        div = (tup - tdown) * (gup - gdown) * (mup - mdown)
    elif t_node and g_node and m_node:
        terms, div = [(name("up", "up", "up"), (1.0, 1.0, 1.0))], 1.0
    elif t_node and g_node:
        terms = [(name("up", "up", m), (M[m], 1.0, 1.0)) for m in ("up", "down")]
        div = mup - mdown
    elif t_node and m_node:
        terms = [(name("up", g, "up"), (G[g], 1.0, 1.0)) for g in ("up", "down")]
        div = gup - gdown
    elif m_node:
        terms = [(name(t, g, "up"), (T[t], G[g], 1.0)) for g in ("up", "down") for t in ("up", "down")]
        div = (tup - tdown) * (gup - gdown)
    elif g_node:
        terms = [(name(t, "up", m), (T[t], M[m], 1.0)) for m in ("up", "down") for t in ("up", "down")]
        div = (tup - tdown) * (mup - mdown)
    else:
        terms = [(name("up", g, m), (G[g], M[m], 1.0)) for m in ("up", "down") for g in ("up", "down")]
        div = (gup - gdown) * (mup - mdown)
    return terms, float(div)


def numpy_blend(corners, terms, div):
    """`corners`: {file name: fp32 array}"""
    acc = None
    for fname, (w0, w1, w2) in terms:
        t = np.asarray(corners[fname], np.float32).astype(np.float64) * w0 * w1 * w2
        acc = t if acc is None else acc + t
    return acc / div


def _zero_spelling(fname):
    """`..._-0.0.fits` <-> `..._0.0.fits`: the reference names the solar-metallicity corner either way, depending on which side
    [M/H] comes from (0.5 * ceil(-0.4) is -0.0)"""
    if fname.endswith("_-0.0.fits"):
        return fname[:-len("_-0.0.fits")] + "_0.0.fits"
    if fname.endswith("_0.0.fits"):
        return fname[:-len("_0.0.fits")] + "_-0.0.fits"
    return None


class PhoenixDirectory(object):
    """the wavelength file and the corner files of one directory; every file is read once"""

    def __init__(self, path):
        if path is None:
            raise IOError("star: data_format = phoenix needs -phoenix_directory, the directory that holds %s and the corner "
                          "files TTTTT_G.GG_M.M.fits" % PHOENIX_WAVE_FILE)
        self.path, self._flux, self._lam = str(path), {}, None

    def _find(self, fname):
        for cand in (fname, _zero_spelling(fname)):
            if cand is not None and os.path.exists(os.path.join(self.path, cand)):
                return os.path.join(self.path, cand)
        return None

    def require(self, names):
        missing = [n for n in [PHOENIX_WAVE_FILE] + list(names) if self._find(n) is None]
        if missing:
            raise IOError("star: not in %s: %s.  Nothing is fetched; put the files there (corner files are named "
                          "TTTTT_G.GG_M.M.fits)" % (self.path, ", ".join(missing)))

    def wavelengths(self):
        """cm"""
        if self._lam is None:
            self.require([])
            lam = np.asarray(fits_lite.getdata(self._find(PHOENIX_WAVE_FILE), 0)).reshape(-1)
            self._lam = lam.astype(np.float64) * 1e-8
        return self._lam

    def flux(self, fname):
        if fname not in self._flux:
            self.require([fname])
            f = np.asarray(fits_lite.getdata(self._find(fname), 0)).reshape(-1)
            if len(f) != len(self.wavelengths()):
                raise IOError("star: %s holds %d points, the wavelength file %d" % (fname, len(f), len(self.wavelengths())))
            self._flux[fname] = np.ascontiguousarray(f, np.float32)
        return self._flux[fname]


# ---- the other formats ----------------------------------------------------------------------------------------------------
def _need(star, *keys):
    for k in keys:
        if star.get(k) is None:
            raise IOError("star: data_format = %s needs -%s" % (star.get("data_format"), k))


def read_ascii_file(star):
    _need(star, "source_file", "w_conversion_factor", "flux_conversion_factor")
    lam, flux = [], []
    with open(star["source_file"]) as f:
        for _ in range(8):
            next(f)
        for line in f:
            col = line.split()
            if col:
                lam.append(float(col[0]))
                flux.append(float(col[1]))
    lam = np.asarray(lam, np.float64) * star["w_conversion_factor"]
    flux = np.asarray(flux, np.float64) * star["flux_conversion_factor"] * (pc.AU / pc.R_SUN) ** 2
    return lam, flux


def read_muscles_file(star):
    _need(star, "source_file", "w_conversion_factor", "flux_conversion_factor", "distance_from_Earth", "R_star")
    table = fits_lite.getdata(star["source_file"], 1)
    dist, rstar = star["distance_from_Earth"] * PARSEC, star["R_star"] * pc.R_SUN
    # a column's own type times a Python number: fp32 columns are widened first, as numpy 1 widens an fp32 scalar
    lam = np.asarray(table["WAVELENGTH"]).astype(np.float64) * star["w_conversion_factor"]
    flux = np.asarray(table["FLUX"]).astype(np.float64) * star["flux_conversion_factor"] * (dist / rstar) ** 2
    return lam, flux


def read_btsettl_file(star):
    _need(star, "source_file", "w_conversion_factor", "flux_conversion_factor")
    image = np.asarray(fits_lite.getdata(star["source_file"], 0))
    if image.ndim != 2 or image.shape[0] < 2:
        raise IOError("star: %s is not a BT-Settl image of two rows (wavelengths, flux)" % star["source_file"])
    return (image[0].astype(np.float64) * star["w_conversion_factor"],
            image[1].astype(np.float64) * star["flux_conversion_factor"])


def check_ascending(lam, what):
    lam = np.asarray(lam, np.float64)
    if len(lam) < 2 or not np.all(np.diff(lam) > 0):
        k = int(np.argmax(np.diff(lam) <= 0)) if len(lam) >= 2 else 0
        raise IOError("star: the tabulated wavelengths of %s do not ascend (at point %d); the re-binning needs them in "
                      "ascending order" % (what, k + 1))


# ---- the opacity grid -----------------------------------------------------------------------------------------------------
def midpoint_interfaces(lam):
    lam = np.asarray(lam, np.float64)
    inter = np.empty(len(lam) + 1, np.float64)
    inter[0] = lam[0] - (lam[1] - lam[0]) / 2
    inter[1:-1] = (lam[1:] + lam[:-1]) / 2
    inter[-1] = lam[-1] + (lam[-1] - lam[-2]) / 2
    return inter


def read_lambda_grid(path):
    """(centres, interfaces) of an opacity container: `centre wavelengths` or `center wavelengths` with `interface
    wavelengths`, or `wavelengths` alone with mid-point interfaces"""
    from .read import Read
    d = Read._open_table(path)
    try:
        for key in ("centre wavelengths", "center wavelengths"):
            if key in d and "interface wavelengths" in d:
                return np.asarray(d[key], np.float64), np.asarray(d["interface wavelengths"], np.float64)
        if "wavelengths" in d:
            lam = np.asarray(d["wavelengths"], np.float64)
            return lam, midpoint_interfaces(lam)
    finally:
        d.close()
    raise IOError("ERROR: Unable to read wavelength data set!")


def interface_plan(old_lambda, inter):
    """per interface: p_bot = len(np.where(old < interface)) - 1, and whether the interface is evaluated at all (it is not
    below the first and not above the last tabulated wavelength)"""
    old, inter = np.asarray(old_lambda, np.float64), np.asarray(inter, np.float64)
    pbot = (np.searchsorted(old, inter, side="left") - 1).astype(np.int32)
    state = (~(inter < old[0]) & ~(inter > old[-1])).astype(np.int32)
    return pbot, state


# ---- the contract in numpy --------------------------------------------------------------------------------------------------
def planck_prefactor(temp):
    return 2.0 * (pc.K_B / pc.H) ** 3 * pc.K_B * temp ** 4 / pc.C ** 2


GAMMA_SPLIT = 2.0                     # below it a term of the Planck series is taken from the lower incomplete gamma function
GAMMA_TERMS = 26                      # of its series: 2^26 / (5 * 6 * ... * 30) < 1e-24


def lower_gamma4(x):
    """int_0^x t^3 e^-t dt = x^4 e^-x sum_k x^k / (4 * 5 * ... * (4 + k)) for x <= GAMMA_SPLIT: positive terms only"""
    s = np.ones(np.shape(x))
    for k in range(GAMMA_TERMS, 0, -1):
        s = 1.0 + x / (4.0 + k) * s
    x2 = x * x
    return x2 * x2 * np.exp(-x) * (s / 4.0)


def upper_gamma4(x):
    """e^-x (x^3 + 3 x^2 + 6 x + 6), the reference's closed form of int_x^inf t^3 e^-t dt"""
    return np.exp(-x) * (x * x * x + 3.0 * (x * x) + 6.0 * x + 6.0)


def planck_term(a, b):
    """int_a^b t^3 e^-t dt, which is what term n of the reference's series is (times n^4) with a = n y_top, b = n y_bot.  The
    reference takes the closed form at both limits; for small limits both are 6 less a little, and the difference keeps few
    digits (some 1e-11 at 20 micron and 3000 K, 1e-7 at 200 micron and 12000 K).  Here limits below GAMMA_SPLIT go through the
    lower incomplete gamma function instead, so that every term is good to a few ulps times b / |b - a|"""
    small_a, small_b = a < GAMMA_SPLIT, b < GAMMA_SPLIT
    ga, gb = lower_gamma4(np.minimum(a, GAMMA_SPLIT)), lower_gamma4(np.minimum(b, GAMMA_SPLIT))
    upper_a = np.where(small_a, 6.0 - ga, upper_gamma4(a))
    upper_b = np.where(small_b, 6.0 - gb, upper_gamma4(b))
    return np.where(small_a & small_b, gb - ga, upper_a - upper_b)


def numpy_planck_bins(temp, lo, hi):
    """pi x calc_analyt_planck_in_interval(temp, lo, hi) for arrays of limits; 0 K: zeros.  The same 199 terms, each
    evaluated without the reference's cancellation (planck_term)"""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    if temp == 0:
        return np.zeros(lo.shape)
    if temp < 0:
        raise ValueError("Error: extrapolation blackbody temperature cannot be negative.")
    d = planck_prefactor(temp)
    y_top = pc.H * pc.C / (hi * pc.K_B * temp)
    y_bot = pc.H * pc.C / (lo * pc.K_B * temp)
    n = np.arange(1, PLANCK_TERMS + 1, dtype=np.float64)[:, None]
    result = np.empty(lo.shape)
    flat_top, flat_bot, flat = y_top.reshape(-1), y_bot.reshape(-1), result.reshape(-1)
    for k in range(0, len(flat), 4096):          # all terms of 4096 bins at a time; the terms add up in the order of n
        terms = planck_term(n * flat_top[None, k:k + 4096], n * flat_bot[None, k:k + 4096]) / (n * n * n * n)
        flat[k:k + 4096] = np.add.reduce(terms, axis=0)
    result *= d / (hi - lo)
    return np.pi * result


def numpy_interface_values(lam, flux, inter, pbot, state):
    n = len(lam)
    on = state.astype(bool)
    a = np.where(pbot < 0, pbot + n, pbot)           # the index -1 wraps to the last point, as the reference's does
    a = np.where(on, a, 0)
    b = np.where(on, pbot + 1, 1)
    v = flux[a] * (lam[b] - inter) + flux[b] * (inter - lam[a])
    v = v / (lam[b] - lam[a])
    return np.where(on, v, 0.0)


def numpy_rebin(lam, flux, inter, pbot, state, extrapol):
    """convert_spectrum(type='linear') for one spectrum; `extrapol`: the value of every bin that has a 0 on an interface"""
    lam, flux, inter = np.asarray(lam, np.float64), np.asarray(flux, np.float64), np.asarray(inter, np.float64)
    F = numpy_interface_values(lam, flux, inter, pbot, state)
    Fi, Fj, xi, xj = F[:-1], F[1:], inter[:-1], inter[1:]
    ext = (Fi == 0) | (Fj == 0)
    ps, pe = pbot[:-1].astype(np.int64) + 1, pbot[1:].astype(np.int64) + 1
    count = np.where(ext, 0, pe - ps)
    out = np.where(ext, extrapol, (Fi + Fj) / 2.0)
    sel = np.nonzero(count > 0)[0]
    if len(sel):
        s, e = ps[sel], pe[sel]
        first = (Fi[sel] + flux[s]) / 2.0 * (lam[s] - xi[sel])
        last = (flux[e - 1] + Fj[sel]) / 2.0 * (xj[sel] - lam[e - 1])
        trap = np.zeros(len(lam) + 1)
        trap[1:len(lam)] = (flux[:-1] + flux[1:]) / 2.0 * (lam[1:] - lam[:-1])       # trap[p]: between points p - 1 and p
        bounds = np.stack([s + 1, e], 1).reshape(-1)
        mid = np.add.reduceat(trap, bounds)[::2]
        mid = np.where(e - s > 1, mid, 0.0)
        out[sel] = (first + mid + last) / (xj[sel] - xi[sel])
    return out


def fit_index(inter, last_tabulated):
    """the bin whose flux the black body is fitted to: two below the first interface above the last tabulated wavelength
    (Python's index arithmetic, so -1 and -2 are bins counted from the end); None when there is no such interface"""
    above = np.nonzero(np.asarray(inter) > last_tabulated)[0]
    return None if len(above) == 0 else int(above[0]) - 2


def fit_bb_temperature(inter, index, bin_flux, start_temp):
    """ten secant steps from (start - 100, start) that make pi x the Planck value of bin `index` equal `bin_flux`"""
    inter = np.asarray(inter, np.float64)
    lo, hi = inter[index], inter[index + 1]
    value = lambda t: float(numpy_planck_bins(t, np.array([lo]), np.array([hi]))[0])
    new = None
    for n in range(SECANT_STEPS):
        if n == 0:
            before, now = start_temp - 100, start_temp
        else:
            before, now = now, new
        v_before, v_now = value(before), value(now)
        if v_before != v_now:
            new = now - (v_now - bin_flux) / (v_now - v_before) * (now - before)
        else:
            new = now
    return new


# ---- device -------------------------------------------------------------------------------------------------------------
class StarBuilder(DeviceObject):
    """stars that share their tabulated wavelengths and the grid, on the device"""

    PREFIX = "hx_star"
    BLEND, PLANCK, REBIN = 1, 2, 4

    def __init__(self, ctx, n_points, n_corners, n_stars, n_bins, chunk=CHUNK):
        self.n_points, self.n_corners, self.n_stars, self.n_bins = int(n_points), int(n_corners), int(n_stars), int(n_bins)
        self._create(ctx, self.n_points, self.n_corners, self.n_stars, self.n_bins, int(chunk))

    def add_corner(self, slot, flux32):
        f = np.ascontiguousarray(flux32, np.float32)
        assert f.shape == (self.n_points,)
        self._call("add_corner", int(slot), vp(f))

    def set_grid(self, lam, inter, pbot, state):
        a = [np.ascontiguousarray(lam, np.float64), np.ascontiguousarray(inter, np.float64),
             np.ascontiguousarray(pbot, np.int32), np.ascontiguousarray(state, np.int32)]
        assert len(a[0]) == self.n_points and len(a[1]) == len(a[2]) == len(a[3]) == self.n_bins + 1
        self._call("set_grid", dp(a[0]), dp(a[1]), ip(a[2]), ip(a[3]))

    def set_star(self, s, slots, weights, div):
        sl, w = np.ascontiguousarray(slots, np.int32), np.ascontiguousarray(weights, np.float64).reshape(-1)
        assert len(w) == 3 * len(sl)
        self._call("set_star", int(s), len(sl), ip(sl), dp(w), float(div))

    def put_flux(self, s, flux):
        f = np.ascontiguousarray(flux, np.float64)
        assert f.shape == (self.n_points,)
        self._call("put_flux", int(s), dp(f))

    def run(self, stages, bb_temps=None, n_stars=None):
        n = self.n_stars if n_stars is None else int(n_stars)
        t = np.zeros(n, np.float64) if bb_temps is None else np.ascontiguousarray(bb_temps, np.float64)
        assert len(t) == n
        d = np.array([planck_prefactor(float(v)) for v in t], np.float64)
        self._call("run", n, dp(t), dp(d), pc.H * pc.C, pc.K_B, int(stages))

    def _results(self):
        return {"flux": (self.n_stars, self.n_points), "converted": (self.n_stars, self.n_bins),
                "planck": (self.n_stars, self.n_bins), "timing_ms": 4}


# ---- stars onto one grid --------------------------------------------------------------------------------------------------
def start_temperature(star, mode):
    """the black-body temperature of the first conversion: BB_temp, else T_eff; 0 for `none`"""
    if mode == "none":
        return 0.0
    t = star.get("BB_temp")
    if t is None:
        t = star.get("temp")
    if t is None:
        raise IOError("star: the black-body extrapolation of %s needs -temp or -BB_temp (or -bb_extrapolation none)"
                      % star.get("name"))
    if t < 0:
        raise ValueError("Error: extrapolation blackbody temperature cannot be negative.")
    return float(t)


def _check_star(star):
    fmt = star.get("data_format")
    if fmt not in FORMATS:
        raise IOError("star: unknown data format %r (phoenix, ascii, muscles or btsettl)" % (fmt,))
    if not star.get("name"):
        raise IOError("star: every star needs a -name, which is its data set's")
    if fmt == "phoenix":
        _need(star, "temp", "log_g", "m")


def _groups(stars, phoenix):
    """stars that share their tabulated wavelengths: all PHOENIX stars of the directory, and every other star alone.
    A group is (indices, wavelengths, terms per star or None, flux per star or None)"""
    groups, pho = [], [k for k, s in enumerate(stars) if s["data_format"] == "phoenix"]
    if pho:
        plans = [blend_plan(stars[k]["temp"], stars[k]["log_g"], stars[k]["m"]) for k in pho]
        phoenix.require(sorted(set(n for terms, _ in plans for n, _ in terms)))
        lam = phoenix.wavelengths()
        check_ascending(lam, PHOENIX_WAVE_FILE)
        groups.append((pho, lam, plans, None))
    readers = {"ascii": read_ascii_file, "muscles": read_muscles_file, "btsettl": read_btsettl_file}
    for k, s in enumerate(stars):
        if s["data_format"] != "phoenix":
            lam, flux = readers[s["data_format"]](s)
            check_ascending(lam, s["source_file"])
            groups.append(([k], lam, None, [flux]))
    return groups


def convert_stars(stars, inter, bb_extrapolation="automatic", backend="device", phoenix_directory=None, ctx=None, chunk=CHUNK,
                  timing=None):
    """every star of the list onto the grid with the interfaces `inter` in one call; returns per star a dict with `flux` (on
    the grid), `orig_lambda`, `orig_flux`, `BB_temp` (what the returned flux was extrapolated with) and `fit_index`.

    `automatic`: the reference converts with the start temperature, fits the black body to the flux of that conversion, and
    converts once more with the fitted temperature; `fixed`: one conversion with BB_temp or T_eff; `none`: bins outside the
    spectrum are 0."""
    if bb_extrapolation in ("yes", "interactive"):
        raise IOError("star: plot_and_tweak = yes is the reference's interactive mode (a plot and questions on the terminal); "
                      "it is not built -- use -bb_extrapolation automatic, fixed or none")
    if bb_extrapolation not in ("automatic", "fixed", "none"):
        raise IOError("star: -bb_extrapolation is automatic, fixed or none (got %r)" % (bb_extrapolation,))
    if backend not in ("device", "numpy"):
        raise IOError("star: backend is device or numpy (got %r)" % (backend,))
    for s in stars:
        _check_star(s)
    inter = np.asarray(inter, np.float64)
    if len(inter) < 2 or not np.all(np.diff(inter) > 0):
        raise IOError("star: the grid's interface wavelengths do not ascend")
    lo, hi = inter[:-1], inter[1:]
    phoenix = PhoenixDirectory(phoenix_directory) if any(s["data_format"] == "phoenix" for s in stars) else None
    results = [None] * len(stars)
    t0 = time.time()
    groups = _groups(stars, phoenix)
    t_read = time.time() - t0
    own = False
    device_ms = np.zeros(4)
    try:
        for idx, lam, plans, fluxes in groups:
            pbot, state = interface_plan(lam, inter)
            start = [start_temperature(stars[k], bb_extrapolation) for k in idx]
            index = fit_index(inter, lam[-1]) if bb_extrapolation == "automatic" else None
            t1 = time.time()
            if plans is not None:
                names = sorted(set(n for terms, _ in plans for n, _ in terms))
                corners = {n: phoenix.flux(n) for n in names}       # every distinct corner file is read once
            t_read += time.time() - t1
            if backend == "numpy":
                orig = [numpy_blend(corners, *plans[j]) for j in range(len(idx))] if plans is not None else fluxes
                convert = lambda temps: np.stack([numpy_rebin(lam, orig[j], inter, pbot, state,
                                                              numpy_planck_bins(temps[j], lo, hi)) for j in range(len(idx))])
                first = convert(start)
            else:
                if ctx is None:
                    from .device import Context
                    ctx, own = Context(int(os.environ.get("HELIOS_DEVICE", "0"))), True
                b = StarBuilder(ctx, len(lam), len(names) if plans is not None else 0, len(idx), len(inter) - 1, chunk)
                try:
                    b.set_grid(lam, inter, pbot, state)
                    if plans is not None:
                        for slot, n in enumerate(names):
                            b.add_corner(slot, corners[n])
                        for j, (terms, div) in enumerate(plans):
                            b.set_star(j, [names.index(n) for n, _ in terms], [w for _, w in terms], div)
                    else:
                        b.put_flux(0, fluxes[0])
                    b.run((b.BLEND if plans is not None else 0) | b.PLANCK | b.REBIN, start)
                    first = b.get("converted")
                    final = first
                    if index is not None:
                        fitted = [fit_bb_temperature(inter, index, first[j][index], start[j]) for j in range(len(idx))]
                        b.run(b.PLANCK | b.REBIN, fitted)
                        final = b.get("converted")
                    orig = b.get("flux")
                    device_ms += b.get("timing_ms")
                finally:
                    b.close()
            if backend == "numpy":
                final = first
                if index is not None:
                    fitted = [fit_bb_temperature(inter, index, first[j][index], start[j]) for j in range(len(idx))]
                    final = convert(fitted)
            for j, k in enumerate(idx):
                results[k] = {"flux": np.asarray(final[j], np.float64), "orig_lambda": lam, "orig_flux": np.asarray(orig[j]),
                              "BB_temp": fitted[j] if index is not None else start[j], "fit_index": index}
    finally:
        if own:
            ctx.close()
    if timing is not None:
        timing.update(seconds=time.time() - t0, read_seconds=t_read, device_ms=device_ms)
    return results


# ---- output ---------------------------------------------------------------------------------------------------------------
def _existing(path):
    """{data set path without the leading slash: array} of a stellar spectrum file that is already there"""
    if not os.path.exists(path):
        return {}
    if path.endswith(".npz"):
        return dict(np.load(path))
    f, out = hdf5_lite.File(path, "r"), {}
    try:
        todo = ["/" + k for k in f.keys("/")]
        while todo:
            name = todo.pop()
            if f.is_dataset(name):
                out[name.strip("/")] = f.read(name)
            else:
                todo += [name + "/" + k for k in f.keys(name)]
    finally:
        f.close()
    return out


def write_star_file(path, datasets):
    """adds the data sets (paths such as `r50_kdistr/phoenix/gj1214`) to the file: an existing file is extended, an existing
    data set replaced.  HDF5 through h5py or hdf5_lite for names ending in `.h5`, where one of them is there; `.npz`
    otherwise, with the paths (no leading slash) as keys, which Read.read_star takes.  Returns the path written."""
    path = str(path)
    datasets = {k.strip("/"): np.asarray(v, np.float64) for k, v in datasets.items()}
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    if path.endswith(".h5"):
        try:
            import h5py
        except ImportError:
            h5py = None
        if h5py is not None:
            with h5py.File(path, "a") as f:
                for k, v in datasets.items():
                    if k in f:
                        del f[k]
                    f.create_dataset(k, data=v)
            return path
        if not hdf5_lite.available():
            path = os.path.splitext(path)[0] + ".npz"
    elif not path.endswith(".npz"):
        path = path + ".npz"
    merged = _existing(path)
    merged.update(datasets)
    if path.endswith(".npz"):
        np.savez(path, **merged)
    else:
        hdf5_lite.write(path, merged)
    return path


def save_to_dat(path, lamda, flux):
    """the reference's two-column text format; wavelengths in micron"""
    with open(path, "w") as f:
        f.writelines("{:<15}{:<25}".format("lambda [um]", "flux [erg s^-1 cm^-3]"))
        for l, v in zip(lamda, flux):
            f.writelines("\n{:<15.7e}{:<25.7e}".format(l, v))


def star_datasets(stars, results, convert_to, centres):
    out = {"%s/lambda" % convert_to: np.asarray(centres, np.float64)}
    for s, r in zip(stars, results):
        out["%s/%s/%s" % (convert_to, s["data_format"], s["name"])] = r["flux"]
        if s["data_format"] == "phoenix":
            out["original/phoenix/%s" % s["name"]] = r["orig_flux"]
            out["original/phoenix/lambda"] = r["orig_lambda"]
    return out


# ---- the tool -------------------------------------------------------------------------------------------------------------
def read_star_list(path):
    """one star per line: `key=value` pairs with the keys of the command line (name, data_format, temp, log_g, m, source_file,
    w_conversion_factor, flux_conversion_factor, distance_from_Earth, R_star, BB_temp); `#` starts a comment"""
    stars = []
    with open(path) as f:
        for nr, line in enumerate(f, 1):
            line = line.split("#")[0].split()
            if not line:
                continue
            star = {}
            for item in line:
                key, eq, value = item.partition("=")
                if not eq or key not in STAR_KEYS:
                    raise IOError("star: line %d of %s: %r is not one of %s=..." % (nr, path, item, ", ".join(sorted(STAR_KEYS))))
                star[key] = STAR_KEYS[key](value)
            stars.append(star)
    if not stars:
        raise IOError("star: %s lists no star" % path)
    return stars


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="star.py", description="stellar spectrum files on the opacity grid")
    p.add_argument("-data_format", default=None)
    p.add_argument("-name", default=None)
    p.add_argument("-temp", type=float, default=None)
    p.add_argument("-log_g", type=float, default=None)
    p.add_argument("-m", type=float, default=None)
    p.add_argument("-source_file", default=None)
    p.add_argument("-w_conversion_factor", type=float, default=None)
    p.add_argument("-flux_conversion_factor", type=float, default=None)
    p.add_argument("-distance_from_Earth", type=float, default=None)
    p.add_argument("-R_star", type=float, default=None)
    p.add_argument("-convert_to", default="r50_kdistr")
    p.add_argument("-opac_file_for_lambdagrid", required=True)
    p.add_argument("-output_file", default="./output/star_2022.h5")
    p.add_argument("-BB_temp", type=float, default=None)
    p.add_argument("-bb_extrapolation", default="automatic")
    p.add_argument("-save_ascii", default="no", choices=("yes", "no"))
    p.add_argument("-phoenix_directory", default=None)
    p.add_argument("-backend", default="device", choices=("device", "numpy"))
    p.add_argument("-star_list", default=None)
    return p.parse_args(argv)


def main(argv=None):
    """star.py: the stars of the command line or of -star_list onto the grid of the opacity container; returns the path
    written"""
    opt = parse_args(argv)
    if opt.star_list is not None:
        stars = read_star_list(opt.star_list)
    else:
        stars = [{k: getattr(opt, k) for k in STAR_KEYS if getattr(opt, k) is not None}]
    if opt.BB_temp is not None:
        for s in stars:
            s.setdefault("BB_temp", opt.BB_temp)
    centres, inter = read_lambda_grid(opt.opac_file_for_lambdagrid)
    timing = {}
    results = convert_stars(stars, inter, opt.bb_extrapolation, opt.backend, opt.phoenix_directory, timing=timing)
    written = write_star_file(opt.output_file, star_datasets(stars, results, opt.convert_to, centres))
    for s, r in zip(stars, results):
        if opt.bb_extrapolation == "none":
            how = "bins outside it 0"
        else:
            how = "bins outside it a black body of %.3f K%s" % (r["BB_temp"], "" if r["fit_index"] is None else
                                                                " (fitted to bin %d)" % r["fit_index"])
        print("star: %s, %d points onto %d bins, %s -> /%s/%s/%s" % (s["name"], len(r["orig_lambda"]), len(centres), how,
                                                                       opt.convert_to, s["data_format"], s["name"]))
        if opt.save_ascii == "yes":
            stem = os.path.join(os.path.dirname(written), s["name"])
            save_to_dat(stem + "_orig.dat", r["orig_lambda"] * 1e4, r["orig_flux"])
            save_to_dat(stem + "_" + opt.convert_to + ".dat", np.asarray(centres) * 1e4, r["flux"])
    print("star: %d star%s in %.2f s (%.2f s reading) -> %s" % (len(stars), "" if len(stars) == 1 else "s", timing["seconds"],
                                                                  timing["read_seconds"], written))
    return written
