"""The analytic tables of the k-table tool: Rayleigh cross-sections per species and the H-, He- continuum containers
(the second stage of the reference's tool, ktable/source_ktable/combination.py with rayleigh.py and continuous.py).

The contract, in cm and cgs.  `lam` is a bin's centre; `mu` = fl(lam * 1e4) is its wavelength in micron as a double -- every
branch below is decided on that double, as the reference decides it.

  Rayleigh, molecules and He   24 pi^3 / (n_ref^2 lam^4) ((n^2 - 1) / (n^2 + 2))^2 King, with n - 1 and King from the fits of
                               continuum_data.RAYLEIGH in nu = 1 / lam (N2: one fit at and below 21 360 cm^-1, one above)
  Rayleigh, H                  the ten-term series of continuum_data.H_SERIES;   e-: phys_const.SIGMA_T
  H-_bf  [cm^2 g^-1]           1e-18 mu^3 x^1.5 sum_k C_k x^(k/2) / m_H with x = 1/mu - 1/mu_0 for 0.125 <= mu <= 1.6419, else 0
  H-_ff  [cm^2 g^-1]           1e-29 sum_n theta^((n+1)/2) (A_n mu^2 + B_n + C_n/mu + ... + F_n/mu^4) P / m_H with theta =
                               5040 / T; 0 for mu < 0.1823, the short-wavelength set for mu < 0.3645, the other from there on
  He-    [cm^2 g^-1]           10^v P / m_He with v bilinear in (T, log10 mu) over log10 of the extended table of `he_table`,
                               v = -30 where T or log10 mu (as a double) lies outside the table

The values do not depend on the Gauss point: a container repeats each over y.

Two backends.  numpy: everything above, vectorised in fp64 -- and always the Rayleigh file, which is nbin numbers per species:
there is no device work in it worth a launch.  hip: k_ktable_continuum (csrc/ktable.hip) fills the containers slab by slab of
(T, P) rows.  Both form n^2 - 1 as d (2 + d) from d = n - 1 and x as (mu_0 - mu) / (mu mu_0): neither cancels, so both stay
within a few ulps of the contract where the reference's own arithmetic loses six digits (n^2 - 1) or more (x near mu_0).  The
H-_ff fit cancels in itself (to 1e-5 of its terms at 50 K, 0.38 micron): numpy sums it in long double, the kernel in
double-double, and each rounds once.
"""
import ctypes
import os

import numpy as np

from . import continuum_data as cd
from . import phys_const as pc
from .species_data import species_lib

CONTINUUM_KINDS = {"H-_bf": 0, "H-_ff": 1, "He-": 2}
SLAB_BYTES = 256 << 20        # device scratch for one slab of (T, P) rows


# ---- species names -------------------------------------------------------------------------------------------------------------
def continuum_species(text):
    """`H-,He-` -> container names in the order given; `H-` stands for both of its parts, as in the species file"""
    out = []
    for name in [s.strip() for s in str(text).split(",") if s.strip()]:
        parts = ("H-_bf", "H-_ff") if name == "H-" else (name,)
        for p in parts:
            if p not in CONTINUUM_KINDS:
                raise IOError("ktable: no continuum table for %r; implemented: H- (H-_bf and H-_ff) and He-" % name)
            if p not in out:
                out.append(p)
    if not out:
        raise IOError("ktable: -continuum_species names no species")
    return out


def rayleigh_species(text):
    out = []
    for name in [s.strip() for s in str(text).split(",") if s.strip()]:
        if name == "H2O":
            raise IOError("ktable: the Rayleigh cross-section of H2O depends on its mixing ratio, so it cannot be tabulated per "
                          "species; it is computed on the device at run time (h2o_rayleigh_cross)")
        if name not in cd.RAYLEIGH_SPECIES:
            raise IOError("ktable: no Rayleigh cross-section for %r; implemented: %s" % (name, ", ".join(cd.RAYLEIGH_SPECIES)))
        if name not in out:
            out.append(name)
    if not out:
        raise IOError("ktable: -rayleigh_species names no species")
    return out


# ---- Rayleigh (host only) --------------------------------------------------------------------------------------------------------
def _index_minus_one(fit, nu, nu2):
    if fit["form"] == "cauchy":
        return fit["scale"] * (1 + fit["b"] * nu2)
    if fit["form"] == "sellmeier":
        d = fit["scale"] * (fit["a"] + fit["b"] / (fit["c"] - nu2))
        if "split_nu" in fit:
            blue = fit["scale"] * (fit["a_blue"] + fit["b_blue"] / (fit["c"] - nu2))
            d = np.where(nu <= fit["split_nu"], d, blue)
        return d
    return fit["scale"] * sum(b / (c - nu2) for b, c in zip(fit["b"], fit["c"]))


def rayleigh_cross_section(name, lam):
    """sigma [cm^2] of one species at the wavelengths lam [cm]"""
    lam = np.asarray(lam, np.float64)
    if name == "e-":
        return np.full(lam.shape, pc.SIGMA_T)
    if name == "H":
        r2 = (cd.H_SERIES_LYMAN / lam) ** 2
        series = np.zeros_like(lam)
        for c in cd.H_SERIES[::-1]:
            series = series * r2 + c
        return cd.H_SERIES_SIGMA_T * r2 * r2 * series
    fit = cd.RAYLEIGH[name]
    nu = 1.0 / lam
    nu2 = nu * nu
    d = _index_minus_one(fit, nu, nu2)
    n2m1 = d * (2 + d)                                   # n^2 - 1 without the cancellation
    k0, k1, k2, k4 = fit["king"]
    king = k0 + k1 * nu + k2 * nu2 + k4 * nu2 * nu2
    return 24.0 * np.pi ** 3 / (fit["n_ref"] ** 2 * lam ** 4) * (n2m1 / (n2m1 + 3)) ** 2 * king


# ---- the continuum in numpy ----------------------------------------------------------------------------------------------------
def species_mass(name):
    return species_lib[name].weight * pc.AMU


def he_table():
    """(T nodes [12], log10 mu nodes [22], log10 k [12][22]) of the extended He- table, all fp64, T ascending"""
    temp = np.sort(np.array([cd.THETA_K / th for th in cd.HEM_THETA + (cd.HEM_THETA_FLOOR,)], np.float64))
    lam = np.array(cd.HEM_LAMBDA + cd.HEM_LAMBDA_LONG, np.float64)
    k = np.empty((len(temp), len(lam)), np.float64)
    for t in range(len(temp)):
        row = max(t - 1, 0)                              # the 50 K row repeats the coldest row of the table
        k[t, :len(cd.HEM_LAMBDA)] = cd.HEM_K[row]
        k[t, len(cd.HEM_LAMBDA):] = cd.HEM_LONG[row] * lam[len(cd.HEM_LAMBDA):] ** 2
    return temp, np.log10(lam), np.log10(k * cd.HEM_UNIT)


def he_micron_limits(xnodes):
    """the smallest and the largest double mu whose fp64 log10 lies inside the table: the reference compares log10 mu, and
    several doubles next to 200 share its logarithm"""
    lo, hi = cd.HEM_LAMBDA[0], cd.HEM_LAMBDA_LONG[-1]
    while np.log10(np.nextafter(lo, 0.0)) >= xnodes[0]:
        lo = np.nextafter(lo, 0.0)
    while np.log10(np.nextafter(hi, np.inf)) <= xnodes[-1]:
        hi = np.nextafter(hi, np.inf)
    return float(lo), float(hi)


def _cell(nodes, v):
    return np.clip(np.searchsorted(nodes, v, side="right") - 1, 0, len(nodes) - 2)


def continuum_coefficients(name):
    """the flat coefficient array hx_continuum_table takes for this kind (include/helios_hip.h section 7)"""
    if name == "H-_bf":
        return np.array((species_mass("H"), cd.HM_BF_LAMBDA_MIN, cd.HM_BF_LAMBDA_0) + cd.HM_BF_C, np.float64)
    if name == "H-_ff":
        sets = [cd.HM_FF[r][term] for r in ("short", "long") for term in "ABCDEF"]
        head = [species_mass("H"), cd.HM_FF_LAMBDA_MIN, cd.HM_FF_LAMBDA_SPLIT, cd.THETA_K]
        return np.concatenate((head, np.ravel(sets))).astype(np.float64)
    temp, x, logk = he_table()
    lo, hi = he_micron_limits(x)
    return np.concatenate(([species_mass("He"), lo, hi, cd.HEM_FILL_LOG10], temp, x, logk.ravel())).astype(np.float64)


def numpy_continuum(name, wave, temp, press, rows=None):
    """k[row][x] of the (T, P) rows `rows` (node = p + npress * t; all by default), fp64"""
    wave, temp, press = [np.asarray(a, np.float64) for a in (wave, temp, press)]
    rows = np.arange(len(temp) * len(press)) if rows is None else np.asarray(rows)
    T, P = temp[rows // len(press)][:, None], press[rows % len(press)][:, None]
    mu = wave * 1e4
    if name == "H-_bf":
        inside = (mu >= cd.HM_BF_LAMBDA_MIN) & (mu <= cd.HM_BF_LAMBDA_0)
        m = np.where(inside, mu, 1.0)
        x = (cd.HM_BF_LAMBDA_0 - m) / (m * cd.HM_BF_LAMBDA_0)
        s = np.sqrt(x)
        f = np.zeros_like(m)
        for c in cd.HM_BF_C[::-1]:
            f = f * s + c
        k = np.where(inside, 1e-18 * m ** 3 * (x * s) * f, 0.0) / species_mass("H")
        return np.repeat(k[None, :], len(rows), axis=0)
    if name == "H-_ff":
        # next to 0.3645 micron and at low T the fit's terms cancel to one part in 1e3 ... 1e5: summed in long double (64
        # mantissa bits where the platform has them) and rounded once
        LD = np.longdouble
        m, theta = mu.astype(LD), LD(cd.THETA_K) / T.astype(LD)
        total = np.zeros((len(rows), len(mu)), LD)
        for n in range(6):
            g = {r: (LD(cd.HM_FF[r]["A"][n]) * m ** 2 + LD(cd.HM_FF[r]["B"][n]) + LD(cd.HM_FF[r]["C"][n]) / m
                     + LD(cd.HM_FF[r]["D"][n]) / m ** 2 + LD(cd.HM_FF[r]["E"][n]) / m ** 3 + LD(cd.HM_FF[r]["F"][n]) / m ** 4)
                 for r in ("short", "long")}
            total = total + theta ** (LD(n + 2) / 2) * np.where(mu < cd.HM_FF_LAMBDA_SPLIT, g["short"], g["long"])[None, :]
        k = 1e-29 * total.astype(np.float64) * P / species_mass("H")
        return np.where((mu < cd.HM_FF_LAMBDA_MIN)[None, :], 0.0, k)
    if name == "He-":
        tn, xn, logk = he_table()
        lo, hi = he_micron_limits(xn)
        x = np.log10(mu)
        i, j = _cell(tn, T[:, 0])[:, None], _cell(xn, x)[None, :]
        ft = (T - tn[i]) / (tn[i + 1] - tn[i])
        fx = ((x[None, :] - xn[j]) / (xn[j + 1] - xn[j]))
        v = (logk[i, j] * (1 - ft) + logk[i + 1, j] * ft) * (1 - fx) + (logk[i, j + 1] * (1 - ft) + logk[i + 1, j + 1] * ft) * fx
        inside = ((T >= tn[0]) & (T <= tn[-1])) & ((mu >= lo) & (mu <= hi))[None, :]
        return 10.0 ** np.where(inside, v, cd.HEM_FILL_LOG10) * P / species_mass("He")
    raise IOError("ktable: no continuum table for %r" % (name,))


# ---- the device ------------------------------------------------------------------------------------------------------------------
class ContinuumBuilder(object):
    """the grid of one directory on the device and a scratch of `slab_rows` (T, P) rows"""

    def __init__(self, ctx, wave, n_gauss, temp, press, slab_rows=None, guard_rows=0):
        from . import _lib
        self.ctx, self._l = ctx, _lib.lib()
        self.nbin, self.ny, self.ntemp, self.npress = len(wave), int(n_gauss), len(temp), len(press)
        self.row_len = self.nbin * self.ny
        nodes = self.ntemp * self.npress
        if slab_rows is None:
            slab_rows = max(1, SLAB_BYTES // (8 * self.row_len))
        self.slab_rows = max(1, min(int(slab_rows), nodes, 65535))
        self.d_wave, self.d_temp, self.d_press = [ctx.to_gpu(np.ascontiguousarray(a, np.float64)) for a in (wave, temp, press)]
        self.d_out = ctx.empty((self.slab_rows + int(guard_rows)) * self.row_len, np.float64)
        self.d_coef = {}
        self.kernel_ms = 0.0

    def run(self, name, first_row, rows, timed=False):
        """fills the scratch with the rows first_row ... first_row + rows - 1 of the container"""
        if name not in self.d_coef:
            self.d_coef[name] = self.ctx.to_gpu(continuum_coefficients(name))
        coef = self.d_coef[name]
        if timed:
            self.ctx.timer_start()
        self.ctx.check(self._l.hx_continuum_table(self.ctx.handle, CONTINUUM_KINDS[name], coef.d, coef.size, self.d_wave.d,
                                                  self.nbin, self.ny, self.d_temp.d, self.ntemp, self.d_press.d, self.npress,
                                                  self.d_out.d, int(first_row), int(rows)), "hx_continuum_table")
        if timed:
            self.kernel_ms += self.ctx.timer_stop_ms()

    def table(self, name, out=None, timed=False):
        """the whole container [t][p][x][y], slab by slab through the scratch"""
        nodes = self.ntemp * self.npress
        out = np.empty(nodes * self.row_len, np.float64) if out is None else out
        for first in range(0, nodes, self.slab_rows):
            rows = min(self.slab_rows, nodes - first)
            self.run(name, first, rows, timed)
            part = out[first * self.row_len:(first + rows) * self.row_len]
            self.ctx.check(self._l.hx_d2h(self.ctx.handle, part.ctypes.data_as(ctypes.c_void_p), self.d_out.ptr, part.nbytes),
                           "hx_d2h")
        return out

    def close(self):
        for a in [self.d_wave, self.d_temp, self.d_press, self.d_out] + list(self.d_coef.values()):
            a.free()


# ---- files -------------------------------------------------------------------------------------------------------------------------
GRID_KEYS = ("interface wavelengths", "center wavelengths", "wavelength width of bins", "ypoints", "pressures", "temperatures")


def _open(path):
    from .read import Read
    return Read._open_table(path)


def grid_like(path):
    """the six grid arrays of an existing `_opac_ip_kdistr` container, bit for bit"""
    if not os.path.exists(path):
        raise IOError("ktable: -grid_like: no such container: %s" % path)
    d = _open(path)
    missing = [k for k in GRID_KEYS if k not in d]
    if missing:
        raise IOError("ktable: -grid_like: %s has no %s; it takes a k-distribution container" % (path, ", ".join(missing)))
    return {k: np.array(np.asarray(d[k], np.float64).reshape(-1)) for k in GRID_KEYS}


def grid_from(inter, n_gauss, temp, press):
    from .ktable import grid_datasets
    centre, width, yg = grid_datasets(inter, n_gauss)
    return {"interface wavelengths": np.asarray(inter, np.float64), "center wavelengths": centre,
            "wavelength width of bins": width, "ypoints": yg, "pressures": np.asarray(press, np.float64),
            "temperatures": np.asarray(temp, np.float64)}


def build_continuum(name, grid, backend="hip", ctx=None, builder=None, timing=None):
    """datasets of `<name>_opac_ip_kdistr` on `grid`"""
    wave, ny = grid["center wavelengths"], len(grid["ypoints"])
    if backend == "numpy":
        k = np.repeat(numpy_continuum(name, wave, grid["temperatures"], grid["pressures"]).reshape(-1), ny)
    elif backend == "hip":
        own = builder is None
        b = ContinuumBuilder(ctx, wave, ny, grid["temperatures"], grid["pressures"]) if own else builder
        try:
            before = b.kernel_ms
            k = b.table(name, timed=timing is not None)
            if timing is not None:
                timing["kernel_ms"] = b.kernel_ms - before
        finally:
            if own:
                b.close()
    else:
        raise IOError("ktable: backend is hip or numpy (got %r)" % (backend,))
    return dict(grid, kpoints=k)


def write_rayleigh_file(directory, container, wave, names):
    """writes or extends `scat_cross_sections.<container>`: `wavelengths` once, `rayleigh_<name>` per species; a data set that
    is already there is kept as it is.  Returns (path, names written, names kept)."""
    from .premix import write_premixed_table
    stem = os.path.join(directory, "scat_cross_sections")
    have, found = {}, None
    for ext in (".h5", ".npz"):
        if os.path.exists(stem + ext):
            found, container = stem + ext, ext[1:]
            break
    if found is not None:
        d = _open(found)
        have = {k: np.array(np.asarray(d[k], np.float64)) for k in d.keys()}
        d.close()                                        # the file is written anew below
    wave = np.asarray(wave, np.float64)
    if "wavelengths" in have and (len(have["wavelengths"]) != len(wave) or np.any(have["wavelengths"] != wave)):
        raise IOError("ktable: %s holds other wavelengths than the grid asked for; all tables of a directory share one grid"
                      % found)
    have.setdefault("wavelengths", wave)
    new, kept = [], []
    for name in names:
        if "rayleigh_" + name in have:
            kept.append(name)
        else:
            have["rayleigh_" + name] = rayleigh_cross_section(name, wave)
            new.append(name)
    return write_premixed_table("%s.%s" % (stem, container), have), new, kept
