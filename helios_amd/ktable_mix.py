"""Premixed k-tables by weighted sum: the mixing stage of the k-table tool (include/helios_hip.h section 9,
csrc/ktable_mix.hip).

Stage 2 of the reference's tool (ktable/source_ktable/combination.py with rayleigh.py, continuous.py and
source/species_database.py): `ktable.py -mixed_table_production yes` turns the species' containers of a directory and a
FastChem output into the `mixed_opac_kdistr` file a premixed run reads.  The contract:

  species file     two header lines, then `name absorbing scattering mixing_ratio`.  The first absorbing species moves to the
                   front, the others keep their order; sums run in that order.  Weight and FastChem name: species_data.py
  final grid       the reference's hard-coded 120 x 28 nodes, or -temperature_grid / -pressure_grid (ktable.target_grid)
  mixing ratios    a number: constant.  `a&b` (CIA pairs, H-_ff, He-): two constants.  `FastChem`: the species' column (or the
                   two columns `X&Y`) of chem.dat, or of chem_low.dat + chem_high.dat concatenated.  The chemistry's nodes are
                   the de-duplicated Tk and Pbar * 1e6 in order of appearance, entry p + np_chem * t; bilinear in T and log10 P
                   with the reference's four branches and term order.  Left node = the last node <= the target; a target below
                   the first node, or a left node that is the last one, clamps the axis (ktable.regrid_plan differs where a
                   target EQUALS the first node: it clamps there, this rule interpolates with weight 0 on the right node)
  mu [amu]         with any FastChem species: FastChem's `mu` column, interpolated like a mixing ratio.  Otherwise
                   sum x_i w_i / sum x_i over the species whose mixing ratio is ONE number, constant over the grid
  opacities        a line absorber or CIA table: `<name>_opac_ip_kdistr` as it is where it exists, else `<name>_opac_kdistr`
                   re-gridded as ktable.numpy_regrid / k_ktable_regrid do, and the `_ip_` container written.  H-_bf, H-_ff,
                   He-: their container where it exists, else built as -continuum_species builds them, and written
  kpoints          [t][p][x][y] = sum_s m_s[t,p] k_s[t][p][x][y], m_s = x_s * x2_s * weight_s / mu evaluated left to right in
                   fp64 on the host (x2 = 1 for single species); from zeros, in file order, one rounded product and one
                   rounded add per term
  Rayleigh         [t][p][x] = sum_s x_s[t,p] sigma_s[x] over the scattering species in file order (a pair: its FIRST mixing
                   ratio); sigma_s from scat_cross_sections where the data set exists, else computed and appended there.  H2O per
                   node: 24 pi^3 / (n_ref^2 lam^4) A^2 King for lam <= 2.5 micron, else 0, with n_ref = x P / (k_B T), A =
                   delta (a0 + a1 delta + a2 theta + a3 L^2 theta + a4 / L^2 + a5 / (L^2 - L_UV^2) + a6 / (L^2 - L_IR^2) + a7
                   delta^2), delta = x P m_H2O / (k_B T) [g cm^-3], theta = T / 273.15, L = lam / 0.589 micron, King = (6 + 3 *
                   3e-4) / (6 - 7 * 3e-4).  A species without an implemented cross-section: a warning, no contribution
  the file         mixed_opac_kdistr.<h5|npz>: pressures, temperatures, meanmolmass, kpoints, weighted Rayleigh cross-sections,
                   wavelengths, center wavelengths, interface wavelengths, wavelength width of bins, ypoints, included
                   molecules, FastChem path, units.  MKS: pressures and kpoints * 1e-1, cross-sections * 1e-4, the wavelength
                   data sets * 1e-2

Where this departs from the reference, on purpose: a water mixing ratio of exactly 0 contributes exactly 0 (the reference
forms 0 * inf there); the water cross-section uses A itself, where the reference goes through n^2 = (2A + 1) / (1 - A) and
back, which loses every digit of A below 1e-16 / A; a missing mean molecular mass is refused with the reason (the reference
fails later with a TypeError); `temperatures` is written as doubles.

Two backends: numpy (the checker, and what a machine without a GPU gets) and hip -- the tables stay on the device in a
`Mixer`, and every further chemistry of a sweep is one upload of mixing ratios and one kernel pass.
"""
import os
import time

import numpy as np

from . import continuum
from . import continuum_data as cd
from . import phys_const as pc
from ._tool import DeviceObject, dp
from .ktable import numpy_regrid, regrid_args, target_grid, write_table
from .species_data import species_lib

CONTINUUM = ("H-_bf", "H-_ff", "He-")
H2O_KING = (6 + 3 * 3e-4) / (6 - 7 * 3e-4)
H2O_LIMIT = 2.5e-4          # cm, inclusive
H2O_A = (0.244257733, 0.974634476e-2, -0.373234996e-2, 0.268678472e-3, 0.158920570e-2, 0.245934259e-2, 0.900704920,
         -0.166626219e-1)
H2O_UV, H2O_IR, H2O_LAMBDA_0 = 0.229202, 5.432937, 0.589e-4
NO_ABSORBER = "Whoops! At least one species needs to be absorbing. Please check your 'final species' file."
WAVE_KEYS = ("interface wavelengths", "center wavelengths", "wavelength width of bins", "ypoints")


# ---- the species file ----------------------------------------------------------------------------------------------------
class MixSpecies(object):
    __slots__ = ("name", "absorbing", "scattering", "mixing_ratio", "weight", "fc_name")

    def pair(self):
        return "CIA" in self.name or self.name in ("H-_ff", "He-")


def is_number(text):
    try:
        float(text)
        return True
    except ValueError:
        return False


def read_final_species_file(path):
    out = []
    with open(path) as f:
        lines = f.readlines()[2:]
    for line in lines:
        col = line.split()
        if not col:
            continue
        if len(col) < 4:
            raise IOError("ktable: a line of %s needs `name absorbing scattering mixing_ratio` (got %r)" % (path, line.strip()))
        sp = MixSpecies()
        sp.name, sp.absorbing, sp.scattering, sp.mixing_ratio = col[0], col[1] == "yes", col[2] == "yes", col[3]
        out.append(sp)
    first = [i for i, sp in enumerate(out) if sp.absorbing]
    if not first:
        raise IOError(NO_ABSORBER)
    out.insert(0, out.pop(first[0]))
    for sp in out:
        if sp.name not in species_lib:
            raise IOError("Oops! Species '%s' was not found in the species data base. Please check that the name is spelled "
                          "correctly. If so, add the relevant information to helios_amd/species_data.py and try again." % sp.name)
        sp.weight, sp.fc_name = species_lib[sp.name].weight, species_lib[sp.name].fc_name
        if sp.mixing_ratio == "FastChem":
            if sp.fc_name is None:
                raise IOError("Oops! FastChem name for species %s unknown. FastChem does not provide it; give its mixing ratio "
                              "as a number." % sp.name)
        else:
            parts = sp.mixing_ratio.split("&")
            if len(parts) != (2 if sp.pair() else 1) or not all(is_number(v) for v in parts):
                raise IOError("ktable: the mixing ratio of %s is %s or FastChem (got %r)"
                              % (sp.name, "two numbers `a&b`" if sp.pair() else "one number", sp.mixing_ratio))
    return out


# ---- the chemistry ---------------------------------------------------------------------------------------------------------
def _in_order(values):
    out = []
    for v in values:
        if v not in out:
            out.append(v)
    return out


class Chemistry(object):
    """a FastChem output directory: chem.dat, or chem_low.dat + chem_high.dat concatenated (Read.load_fastchem_data)"""

    def __init__(self, path):
        strip = " !#$%&'()*,./:;<=>?@[\\]^{|}~"
        self.path = path if path.endswith("/") else path + "/"

        def table(name):
            return np.genfromtxt(self.path + name, names=True, dtype=None, skip_header=0, deletechars=strip)
        if os.path.exists(self.path + "chem.dat"):
            self.parts = [table("chem.dat")]
        elif os.path.exists(self.path + "chem_low.dat") and os.path.exists(self.path + "chem_high.dat"):
            self.parts = [table("chem_low.dat"), table("chem_high.dat")]
        else:
            raise IOError("ktable: no chem.dat, nor chem_low.dat and chem_high.dat, in %s" % self.path)
        self.temp = np.asarray(_in_order(self.column("Tk")), np.float64)
        self.press = np.asarray([p * 1e6 for p in _in_order(self.column("Pbar"))], np.float64)
        if len(self.column("Tk")) != len(self.temp) * len(self.press):
            raise IOError("ktable: %s holds %d rows for %d temperatures x %d pressures" % (self.path, len(self.column("Tk")),
                                                                                            len(self.temp), len(self.press)))

    def column(self, name):
        try:
            return np.concatenate([np.asarray(p[name], np.float64).reshape(-1) for p in self.parts])
        except ValueError:
            raise IOError("ktable: the FastChem output in %s has no column %r" % (self.path, name))


def vmr_plan(old, new):
    """per target node: the last source node <= it, and whether the axis is clamped there"""
    old, new = np.asarray(old, np.float64), np.asarray(new, np.float64)
    le = old[None, :] <= new[:, None]
    any_le = le.any(axis=1)
    left = np.where(any_le, len(old) - 1 - np.argmax(le[:, ::-1], axis=1), 0).astype(np.int32)
    reduced = (~any_le | (left == len(old) - 1)).astype(np.int32)
    return left, reduced


def interpolate_vmr(chem_temp, chem_press, vmr, temp_new, press_new, what="mixing ratio"):
    """a chemistry column [p + np_chem * t] on the final grid [p + np * t]"""
    T, Tn = np.asarray(chem_temp, np.float64), np.asarray(temp_new, np.float64)
    lp, lpn = np.log10(np.asarray(chem_press, np.float64)), np.log10(np.asarray(press_new, np.float64))
    v = np.asarray(vmr, np.float64).reshape(len(T), len(lp))
    tl, tr = vmr_plan(T, Tn)
    pl, pr = vmr_plan(chem_press, press_new)
    t1, p1 = np.minimum(tl + 1, len(T) - 1), np.minimum(pl + 1, len(lp) - 1)
    a, b = (Tn - T[tl])[:, None], (T[t1] - Tn)[:, None]
    c, d = (lpn - lp[pl])[None, :], (lp[p1] - lpn)[None, :]
    dT, dP = (T[t1] - T[tl])[:, None], (lp[p1] - lp[pl])[None, :]
    I, J, I1, J1 = tl[:, None], pl[None, :], t1[:, None], p1[None, :]
    rt, rp = tr[:, None] != 0, pr[None, :] != 0
    with np.errstate(all="ignore"):
        both = v[I, J] + np.zeros((len(Tn), len(lpn)))
        only_p = (v[I, J1] * c + v[I, J] * d) / dP
        only_t = (v[I1, J] * a + v[I, J] * b) / dT
        full = (v[I1, J1] * a * c + v[I1, J] * a * d + v[I, J1] * b * c + v[I, J] * b * d) / (dT * dP)
    out = np.where(rt & rp, both, np.where(rt, only_p, np.where(rp, only_t, full)))
    bad = np.argwhere(np.isnan(out))
    if len(bad):
        raise IOError("ktable: the %s is NaN at the final grid's node with the indices pressure: %d, temperature: %d"
                      % (what, bad[0][1], bad[0][0]))
    return out.reshape(-1)


def mixing_ratios(species, chem, temp, press):
    """x[s][node], x2[s][node] (1 for single species) and mu[node] in amu"""
    nodes = len(temp) * len(press)
    x, x2 = np.ones((len(species), nodes)), np.ones((len(species), nodes))
    for s, sp in enumerate(species):
        if sp.mixing_ratio == "FastChem":
            names = sp.fc_name.split("&") if sp.pair() else [sp.fc_name]
            if len(names) != (2 if sp.pair() else 1):
                raise IOError("ktable: the FastChem name %r of %s does not fit a %s" % (sp.fc_name, sp.name,
                                                                                      "pair" if sp.pair() else "single species"))
            cols = [interpolate_vmr(chem.temp, chem.press, chem.column(n), temp, press, "mixing ratio of " + sp.name)
                    for n in names]
        else:
            cols = [np.ones(nodes) * float(v) for v in sp.mixing_ratio.split("&")]
        x[s] = cols[0]
        if sp.pair():
            x2[s] = cols[1]
    if chem is not None and any(sp.mixing_ratio == "FastChem" for sp in species):
        mu = interpolate_vmr(chem.temp, chem.press, chem.column("mu"), temp, press, "mean molecular mass")
    else:
        total = weighted = 0
        for sp in species:
            if is_number(sp.mixing_ratio):
                weighted += float(sp.mixing_ratio) * sp.weight
                total += float(sp.mixing_ratio)
        if not total > 0:
            raise IOError("ktable: no mean molecular mass: no species takes its mixing ratio from FastChem, and none has a "
                          "single constant mixing ratio (pairs `a&b` do not count) to form sum x w / sum x from")
        mu = np.ones(nodes) * weighted / total
    return x, x2, mu


def mass_mixing_ratios(species, x, x2, mu):
    return np.stack([x[s] * x2[s] * sp.weight / mu for s, sp in enumerate(species)])


# ---- the contract in numpy -----------------------------------------------------------------------------------------------
def h2o_cross_section(wave, temp, press, f):
    """sigma [node][x] of water vapour at the mixing ratios f[node] (stage 2's formula; 0 where f is 0)"""
    wave, f = np.asarray(wave, np.float64), np.asarray(f, np.float64)
    T = np.repeat(np.asarray(temp, np.float64), len(press))[:, None]
    P = np.tile(np.asarray(press, np.float64), len(temp))[:, None]
    f = f[:, None]
    a0, a1, a2, a3, a4, a5, a6, a7 = H2O_A
    with np.errstate(all="ignore"):
        kt = pc.K_B * T
        delta = f * P * (species_lib["H2O"].weight * pc.AMU) / kt
        n_ref = f * P / kt
        theta = T / 273.15
        L = wave[None, :] / H2O_LAMBDA_0
        l2 = L * L
        A = delta * (a0 + a1 * delta + a2 * theta + a3 * l2 * theta + a4 / l2 + a5 / (l2 - H2O_UV * H2O_UV)
                     + a6 / (l2 - H2O_IR * H2O_IR) + a7 * (delta * delta))
        lam2 = (wave * wave)[None, :]
        sig = 24.0 * (np.pi * np.pi * np.pi) / ((n_ref * n_ref) * (lam2 * lam2)) * (A * A) * H2O_KING
    return np.where((wave[None, :] <= H2O_LIMIT) & (f != 0.0), sig, 0.0)


def numpy_sum(tables, mmr, nodes, nc):
    """`tables`: per species the table on the final grid or None"""
    acc = np.zeros((nodes, nc))
    for k, m in zip(tables, mmr):
        if k is not None:
            acc = acc + m[:, None] * np.asarray(k, np.float64).reshape(nodes, nc)
    return acc.reshape(-1)


def numpy_scat(sigmas, x, wave, temp, press):
    """`sigmas`: per species None, sigma[nbin] or the string "H2O" """
    nodes = len(temp) * len(press)
    acc = np.zeros((nodes, len(wave)))
    for sig, xs in zip(sigmas, x):
        if sig is None:
            continue
        if isinstance(sig, str):
            acc = acc + xs[:, None] * h2o_cross_section(wave, temp, press, xs)
        else:
            acc = acc + xs[:, None] * np.asarray(sig, np.float64)[None, :]
    return acc.reshape(-1)


# ---- the device ----------------------------------------------------------------------------------------------------------
class Mixer(DeviceObject):
    """the species' tables on the final grid, resident on the device; `run` is one chemistry"""

    PREFIX = "hx_ktmix"

    def __init__(self, ctx, nbin, ny, nt, npress, nspecies):
        self.nbin, self.ny, self.nt, self.np, self.ns = int(nbin), int(ny), int(nt), int(npress), int(nspecies)
        self.nc, self.nodes = self.nbin * self.ny, self.nt * self.np
        self._create(ctx, self.nbin, self.ny, self.nt, self.np, self.ns)
        self.temp = self.press = None

    def set_grid(self, wave, temp, press):
        a = [np.ascontiguousarray(v, np.float64) for v in (wave, temp, press)]
        assert len(a[0]) == self.nbin and len(a[1]) == self.nt and len(a[2]) == self.np
        self._call("set_grid", *[dp(v) for v in a])
        self.temp, self.press = a[1], a[2]

    def set_species(self, s, table):
        t = None
        if table is not None:
            t = np.ascontiguousarray(table, np.float64).reshape(-1)
            if t.size != self.nodes * self.nc:
                raise IOError("ktable: a table of %d entries for a grid of %d" % (t.size, self.nodes * self.nc))
        self._call("set_species", int(s), dp(t))

    def set_species_native(self, s, table, temp_old, press_old):
        assert self.temp is not None, "set the grid first"
        t = np.ascontiguousarray(table, np.float64).reshape(-1)
        if t.size != len(temp_old) * len(press_old) * self.nc:
            raise IOError("ktable: a native table of %d entries for %d x %d nodes" % (t.size, len(temp_old), len(press_old)))
        plan = regrid_args(temp_old, press_old, self.temp, self.press)
        self._call("set_species_native", int(s), dp(t), len(temp_old), len(press_old), *plan)

    def set_rayleigh(self, s, sigma, is_h2o=False):
        g = None if sigma is None else np.ascontiguousarray(sigma, np.float64)
        assert g is None or len(g) == self.nbin
        self._call("set_rayleigh", int(s), dp(g), 1 if is_h2o else 0)

    def run(self, mmr, vmr_scat):
        m, v = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (mmr, vmr_scat)]
        assert m.size == v.size == self.ns * self.nodes
        self._call("run", dp(m), dp(v))

    def _results(self):
        table = {"timing_ms": 4, "kpoints": self.nodes * self.nc, "kpoints_guard": self.nc, "scat_cross": self.nodes * self.nbin,
                 "scat_cross_guard": self.nbin}
        table.update(("species_%d" % s, self.nodes * self.nc) for s in range(self.ns))
        return table


# ---- containers ------------------------------------------------------------------------------------------------------------
def _find(directory, stem):
    for ext in (".h5", ".npz"):
        p = os.path.join(directory, stem + ext)
        if os.path.exists(p):
            return p
    return None


def _read(path, keys):
    d = continuum._open(path)
    missing = [k for k in keys if k not in d]
    if missing:
        raise IOError("ktable: %s has no %s; the mixing stage takes k-distribution containers" % (path, ", ".join(missing)))
    return {k: np.array(np.asarray(d[k], np.float64).reshape(-1)) for k in keys}


def _same(a, b):
    return len(a) == len(b) and bool(np.all(a == b))


class Resolver(object):
    """finds, re-grids or builds every absorber's table on the final grid, and the Rayleigh cross-sections"""

    def __init__(self, directory, container, temp, press, backend, ctx, fallback_grid=None):
        self.dir, self.container, self.backend, self.ctx = directory, container, backend, ctx
        self.temp, self.press = np.asarray(temp, np.float64), np.asarray(press, np.float64)
        self.grid, self.fallback, self.written = None, fallback_grid, []

    def _check_grid(self, data, path):
        if self.grid is None:
            self.grid = {k: data[k] for k in WAVE_KEYS}
        elif not all(_same(self.grid[k], data[k]) for k in WAVE_KEYS):
            raise IOError("ktable: %s holds other bins or Gauss points than the containers before it; all tables of a call "
                          "share one grid" % path)

    def prepare(self, species):
        """the wavelength grid: that of the first absorber's container that exists, else the tool's options"""
        for sp in species:
            if sp.absorbing:
                path = _find(self.dir, sp.name + "_opac_ip_kdistr") or _find(self.dir, sp.name + "_opac_kdistr")
                if path is not None:
                    self._check_grid(_read(path, WAVE_KEYS), path)
                    return
        if self.fallback is None:
            raise IOError("ktable: no container of an absorbing species in %s to take the wavelength grid from" % self.dir)
        self.grid = {k: np.asarray(self.fallback[k], np.float64) for k in WAVE_KEYS}

    def full_grid(self):
        return dict(self.grid, pressures=self.press, temperatures=self.temp)

    def absorber(self, sp, mixer=None, slot=None):
        """the table on the final grid (numpy backend), or None once it is in the mixer's slot"""
        nc = len(self.grid["center wavelengths"]) * len(self.grid["ypoints"])
        path = _find(self.dir, sp.name + "_opac_ip_kdistr")
        if path is not None:
            data = _read(path, continuum.GRID_KEYS + ("kpoints",))
            self._check_grid(data, path)
            if not (_same(data["temperatures"], self.temp) and _same(data["pressures"], self.press)):
                raise IOError("ktable: %s stands on other (T, P) nodes than the final grid; remove it, or give the grid it was "
                              "made on with -temperature_grid and -pressure_grid" % path)
            if data["kpoints"].size != len(self.temp) * len(self.press) * nc:
                raise IOError("ktable: %s holds %d kpoints for %d nodes x %d entries" % (path, data["kpoints"].size,
                                                                                        len(self.temp) * len(self.press), nc))
            k = data["kpoints"]
        elif sp.name in CONTINUUM:
            k = continuum.build_continuum(sp.name, self.full_grid(), self.backend, self.ctx)["kpoints"]
            self._write_ip(sp.name, k)
        else:
            path = _find(self.dir, sp.name + "_opac_kdistr")
            if path is None:
                raise IOError("ktable: neither %s_opac_ip_kdistr nor %s_opac_kdistr (.h5 or .npz) in %s" % (sp.name, sp.name,
                                                                                                       self.dir))
            data = _read(path, continuum.GRID_KEYS + ("kpoints",))
            self._check_grid(data, path)
            if data["kpoints"].size != len(data["temperatures"]) * len(data["pressures"]) * nc:
                raise IOError("ktable: %s holds %d kpoints for %d x %d nodes x %d entries"
                              % (path, data["kpoints"].size, len(data["temperatures"]), len(data["pressures"]), nc))
            if mixer is not None:
                mixer.set_species_native(slot, data["kpoints"], data["temperatures"], data["pressures"])
                self._write_ip(sp.name, mixer.get("species_%d" % slot))
                return None
            k = numpy_regrid(data["pressures"], data["temperatures"], data["kpoints"], self.temp, self.press,
                             len(self.grid["center wavelengths"]), len(self.grid["ypoints"]))
            self._write_ip(sp.name, k)
        if mixer is not None:
            mixer.set_species(slot, k)
            return None
        return k

    def _write_ip(self, name, k):
        path = "%s_opac_ip_kdistr.%s" % (os.path.join(self.dir, name), self.container)
        self.written.append(write_table(path, dict(self.full_grid(), kpoints=k)))

    def rayleigh(self, sp):
        """None (with the reference's warning), "H2O", or sigma[nbin]"""
        if sp.name == "H2O":
            return "H2O"
        if sp.name not in cd.RAYLEIGH_SPECIES:
            print("WARNING WARNING WARNING: Rayleigh scattering cross sections for species", sp.name,
                  "not found. Please double-check! Continuing without those... ")
            return None
        wave = self.grid["center wavelengths"]
        for attempt in (0, 1):
            path = _find(self.dir, "scat_cross_sections")
            if path is not None:
                d = continuum._open(path)
                sig = np.array(np.asarray(d["rayleigh_" + sp.name], np.float64).reshape(-1)) if "rayleigh_" + sp.name in d else None
                d.close()
                if sig is not None:
                    if len(sig) != len(wave):
                        raise IOError("ktable: rayleigh_%s of %s holds %d values for %d bins" % (sp.name, path, len(sig), len(wave)))
                    return sig
            if attempt == 0:
                made = continuum.write_rayleigh_file(self.dir, self.container, wave, [sp.name])[0]
                if made not in self.written:
                    self.written.append(made)
        raise IOError("ktable: rayleigh_%s could not be written to %s" % (sp.name, self.dir))


# ---- the stage --------------------------------------------------------------------------------------------------------------
def output_datasets(grid, temp, press, mu, kpoints, scat, names, fastchem_path, units):
    if units not in ("CGS", "MKS"):
        raise IOError("ktable: -units_of_mixed_opacity_table is CGS or MKS (got %r)" % (units,))
    p, k, s, w = (1e-1, 1e-1, 1e-4, 1e-2) if units == "MKS" else (None,) * 4

    def scaled(a, f):
        a = np.asarray(a, np.float64)
        return a if f is None else a * f
    return {"pressures": scaled(press, p), "temperatures": np.asarray(temp, np.float64), "meanmolmass": mu,
            "kpoints": scaled(kpoints, k), "weighted Rayleigh cross-sections": scaled(scat, s),
            "included molecules": np.array(names), "wavelengths": scaled(grid["center wavelengths"], w),
            "FastChem path": np.array(str(fastchem_path or "")), "units": np.array(units),
            "center wavelengths": scaled(grid["center wavelengths"], w),
            "interface wavelengths": scaled(grid["interface wavelengths"], w),
            "wavelength width of bins": scaled(grid["wavelength width of bins"], w), "ypoints": grid["ypoints"]}


def sweep_directories(text):
    """`path_to_fastchem_output=a/,b/` -> [a/, b/] (premix.py's syntax)"""
    key, _, values = str(text).partition("=")
    dirs = [v for v in values.split(",") if v]
    if key.strip() != "path_to_fastchem_output" or ";" in values or not dirs:
        raise IOError("ktable.py sweeps over chemistry only: -sweep \"path_to_fastchem_output=a/,b/\" (got %r)" % (text,))
    return dirs


def mix_tables(species_file, directory, fastchem_dirs, out_paths, temp, press, units="CGS", backend="hip", ctx=None,
               container="h5", fallback_grid=None, timing=None):
    """one mixed table per FastChem directory (None: no chemistry is read) over one set of resident species tables; returns
    the paths written, the containers made on the way first"""
    if backend not in ("hip", "numpy"):
        raise IOError("ktable: backend is hip or numpy (got %r)" % (backend,))
    species = read_final_species_file(species_file)
    needs_chem = any(sp.mixing_ratio == "FastChem" for sp in species)
    if needs_chem and any(d is None for d in fastchem_dirs):
        raise IOError("ktable: the species file takes mixing ratios from FastChem; give -path_to_fastchem_output")
    temp, press = np.asarray(temp, np.float64), np.asarray(press, np.float64)
    res = Resolver(directory, container, temp, press, backend, ctx, fallback_grid)
    res.prepare(species)
    wave, ny = res.grid["center wavelengths"], len(res.grid["ypoints"])
    nodes, nc = len(temp) * len(press), len(wave) * ny
    mixer, tables, written = None, [None] * len(species), []
    t0 = time.time()
    try:
        if backend == "hip":
            mixer = Mixer(ctx, len(wave), ny, len(temp), len(press), len(species))
            mixer.set_grid(wave, temp, press)
        sigmas = []
        for s, sp in enumerate(species):
            if sp.absorbing:
                tables[s] = res.absorber(sp, mixer, s)
            sig = res.rayleigh(sp) if sp.scattering else None
            sigmas.append(sig)
            if mixer is not None and sig is not None:
                mixer.set_rayleigh(s, None if isinstance(sig, str) else sig, isinstance(sig, str))
        t_tables = time.time() - t0
        names = [sp.name for sp in species if sp.absorbing]
        for fc, path in zip(fastchem_dirs, out_paths):
            t1 = time.time()
            chem = Chemistry(fc) if needs_chem else None
            x, x2, mu = mixing_ratios(species, chem, temp, press)
            mmr = mass_mixing_ratios(species, x, x2, mu)
            if mixer is not None:
                mixer.run(mmr, x)
                kpoints, scat = mixer.get("kpoints"), mixer.get("scat_cross")
                if timing is not None:
                    timing.setdefault("device_ms", []).append(mixer.get("timing_ms"))
            else:
                kpoints = numpy_sum(tables, mmr, nodes, nc)
                scat = numpy_scat(sigmas, x, wave, temp, press)
            data = output_datasets(res.grid, temp, press, mu, kpoints, scat, names, chem.path if chem else "", units)
            written.append(write_table(path, data))
            print("ktable: mixed table of %d absorbers and %d scatterers on %d x %d (T, P) nodes, %d bins x %d Gauss points in "
                  "%.2f s -> %s" % (len(names), sum(g is not None for g in sigmas), len(temp), len(press), len(wave), ny,
                                    time.time() - t1, written[-1]))
        if timing is not None:
            timing["tables_seconds"], timing["seconds"] = t_tables, time.time() - t0
    finally:
        if mixer is not None:
            mixer.close()
    return res.written + written


def run(opt, inter, ctx):
    """the stage as ktable.py calls it"""
    from .premix import sweep_argument, sweep_output_paths
    if opt.path_to_final_species_file is None:
        raise IOError("ktable: -mixed_table_production yes needs -path_to_final_species_file")
    temp, press = target_grid(opt.temperature_grid, opt.pressure_grid)
    out = os.path.join(opt.mixed_table_output_directory, "mixed_opac_kdistr." + opt.container)
    if opt.sweep is not None:
        dirs = sweep_directories(opt.sweep)
        paths = sweep_output_paths(out, len(dirs))
    else:
        dirs, paths = [opt.path_to_fastchem_output], [out]
    fallback = continuum.grid_from(inter, opt.number_of_gaussian_points, temp, press)
    written = mix_tables(opt.path_to_final_species_file, opt.directory_with_individual_files, dirs, paths, temp, press,
                         opt.units_of_mixed_opacity_table, opt.backend, ctx, opt.container, fallback)
    if opt.sweep is not None:
        print("-sweep \"%s\"" % sweep_argument(written[-len(dirs):]))
    return written
