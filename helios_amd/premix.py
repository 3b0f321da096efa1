"""Premixed k-tables built on the device from the on-the-fly species set (include/helios_hip.h section 5,
csrc/premix.hip).

Where every species' mixing ratio is a constant or a FastChem table, the on-the-fly mix of a level is a function of (T, P)
alone.  `build_premixed_table` evaluates it on the species tables' own (T, P) nodes -- optionally refined -- with the
refresh's species loop (random overlap or correlated-k), `write_premixed_table` stores the result under the dataset names
`Read.read_opac_file` expects of a premixed table, and a run on that file pays the premixed path's price.  The cell-error
map says how far the premixed look-up's bilinear value is from the on-the-fly mix at the centre of every table cell.
"""
import argparse
import os
import time

import numpy as np

from . import hdf5_lite
from . import host_functions as hsfunc
from ._tool import DeviceObject, dp

RO_NY = 20          # most Gauss points the random-overlap kernels hold (csrc/random_overlap.h, ro::NY; fewer: random_overlap_ny.h)
UNIFORM_RTOL = 1e-9


# ---- the arithmetic of the options (no device) -----------------------------------------------------------------------
def parse_refine(text):
    """`-premix_refine nT,nP` -> (nT, nP), integers >= 1"""
    try:
        parts = [int(v) for v in str(text).replace(" ", "").split(",")]
    except ValueError:
        parts = []
    if len(parts) != 2 or min(parts) < 1:
        raise IOError("-premix_refine takes two integers >= 1, 'nT,nP' (got %r)" % (text,))
    return parts[0], parts[1]


def output_grid_size(ntemp, npress, refine=(1, 1)):
    """nodes of the output table: every cell of the species tables' grid divided into refine[0] x refine[1] cells"""
    return (int(ntemp) - 1) * int(refine[0]) + 1, (int(npress) - 1) * int(refine[1]) + 1


def sweep_output_paths(path, n):
    """`FILE` with `_0`, `_1`, ... before the extension"""
    stem, ext = os.path.splitext(str(path))
    return ["%s_%d%s" % (stem, k, ext) for k in range(int(n))]


def sweep_argument(paths):
    """the list in the form sweep.py's `-sweep` expects"""
    return "path_to_opacity_file=" + ",".join(paths)


def parse_args(argv=None):
    """the options premix.py adds to helios.py's; returns (options, remaining helios.py arguments)"""
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("-premix_output", default="premixed_opac.h5")
    p.add_argument("-premix_refine", default="1,1")
    p.add_argument("-premix_cell_error", default="yes", choices=("yes", "no"))
    p.add_argument("-sweep", default=None)
    opt, rest = p.parse_known_args(argv)
    opt.refine = parse_refine(opt.premix_refine)
    opt.cell_error = opt.premix_cell_error == "yes"
    opt.fastchem_dirs = None
    if opt.sweep is not None:
        key, _, values = str(opt.sweep).partition("=")
        dirs = [v for v in values.split(",") if v]
        if key.strip() != "directory_with_fastchem_files" or ";" in values or not dirs:
            raise IOError("premix.py sweeps over chemistry only: -sweep \"directory_with_fastchem_files=a/,b/\" (got %r)"
                          % (opt.sweep,))
        opt.fastchem_dirs = dirs
    return opt, rest


def _uniform(nodes, what):
    a = np.asarray(nodes, np.float64)
    want = a[0] + (a[-1] - a[0]) * np.arange(len(a)) / (len(a) - 1.0)
    if np.any(np.abs(a - want) > UNIFORM_RTOL * np.maximum(np.abs(want), 1.0 if what.startswith("log10") else 0.0)):
        raise IOError("premix: the species tables' %s nodes are not uniform (to %g relative): the premixed look-up takes its "
                      "nodes as uniform in T and in log10 P" % (what, UNIFORM_RTOL))


def check_sources(species_list):
    for sp in species_list:
        if sp.source_for_vmr == "file":
            raise IOError("premix: the mixing ratio of %s comes from a vertical-profile file, which is not a function of "
                          "(T, P); give it as a constant or as FastChem" % sp.name)


def check_species(quant):
    """refusals, before anything is allocated"""
    check_sources(quant.species_list)
    ck = str(getattr(quant, "kcoeff_mixing", "RO")) == "correlated-k"
    if not ck and int(quant.ny) > RO_NY:
        raise IOError("premix: random-overlap mixing holds at most %d Gauss points per bin (the tables have %d); use "
                      "k_coefficients_mixing_method = correlated-k" % (RO_NY, int(quant.ny)))
    if int(quant.ntemp) < 2 or int(quant.npress) < 2:
        raise IOError("premix: the species tables need at least two temperature and two pressure nodes")
    _uniform(quant.ktemp, "temperature")
    _uniform(np.log10(np.asarray(quant.kpress, np.float64)), "log10 pressure")


def species_mixing_ratios(quant, reader):
    """per species: (vmr table on the species' (T, P) nodes or None, constant)"""
    out = []
    if any(sp.source_for_vmr == "FastChem" for sp in quant.species_list):
        reader.load_fastchem_data()
    for sp in quant.species_list:
        if sp.source_for_vmr == "FastChem":
            sp.vmr_pretab = reader.read_fastchem_vmr_and_interpolate_to_opacity_PT_grid(quant, sp)
            out.append((np.ascontiguousarray(sp.vmr_pretab, np.float64), 0.0))
        else:
            src = str(sp.source_for_vmr)
            value = float(np.prod([float(v) for v in src.split("&")])) if "CIA" in sp.name else float(src)
            out.append((None, value))
    return out


# ---- device -----------------------------------------------------------------------------------------------------------
class Premixer(DeviceObject):
    """the species tables on the device (uploaded once) and the runs over them"""

    PREFIX = "hx_premix"

    def __init__(self, ctx, nbin, ny, ntemp, npress, nspecies, refine=(1, 1), correlated_k=False):
        self.nbin, self.ny, self.nspecies = int(nbin), int(ny), int(nspecies)
        self.nT, self.nP = output_grid_size(ntemp, npress, refine)
        self._create(ctx, int(nbin), int(ny), int(ntemp), int(npress), int(nspecies), int(refine[0]), int(refine[1]),
                     1 if correlated_k else 0)

    def set_grid(self, wave, gauss_y, gauss_w, ktemp, kpress):
        a = [np.ascontiguousarray(v, np.float64) for v in (wave, gauss_y, gauss_w, ktemp, kpress)]
        self._call("set_grid", *[dp(v) for v in a])

    def set_species(self, s, pretab, scat_cross, vmr_table, vmr_const, weight, absorbing, scattering, is_h2o=0, is_cia=0,
                    in_mu=1):
        a = [None if v is None else np.ascontiguousarray(v, np.float64) for v in (pretab, scat_cross, vmr_table)]
        self._call("set_species", int(s), dp(a[0]), dp(a[1]), dp(a[2]), float(vmr_const), float(weight), int(absorbing),
                   int(scattering), int(is_h2o), int(is_cia), int(in_mu))

    def set_species_separable(self, s, kxy, ftp):
        a, b = np.ascontiguousarray(kxy, np.float64), np.ascontiguousarray(ftp, np.float64)
        self._call("set_species_separable", int(s), dp(a), dp(b))

    def set_species_vmr(self, s, vmr_table, vmr_const=0.0):
        t = None if vmr_table is None else np.ascontiguousarray(vmr_table, np.float64)
        self._call("set_species_vmr", int(s), dp(t), float(vmr_const))

    def set_slab_rows(self, rows):
        self._call("set_slab_rows", int(rows))

    def run(self, cell_error=True):
        self._call("run", 1 if cell_error else 0)

    def _results(self):
        nT, nP, nc = self.nT, self.nP, self.nbin * self.ny
        return {"temperatures": nT, "pressures": nP, "kpoints": nT * nP * nc, "scat_cross": nT * nP * self.nbin,
                "meanmolmass": nT * nP, "cell_error_max": (nT - 1) * (nP - 1), "cell_error_mean": (nT - 1) * (nP - 1),
                "timing_ms": 4}


def _settings(quant, refine, cell_error):
    return "refine=%d,%d; kcoeff_mixing=%s; cell_error=%s; species=%s" % (
        refine[0], refine[1], getattr(quant, "kcoeff_mixing", "RO"), "yes" if cell_error else "no",
        ",".join("%s:%s" % (sp.name, sp.source_for_vmr) for sp in quant.species_list))


def _collect(pm, quant, reader, refine, cell_error):
    d = {
        "pressures": pm.get("pressures"),
        "temperatures": pm.get("temperatures"),
        "meanmolmass": pm.get("meanmolmass"),
        "kpoints": pm.get("kpoints"),
        "weighted Rayleigh cross-sections": pm.get("scat_cross"),
        "included molecules": np.array([sp.name for sp in quant.species_list]),
        "center wavelengths": np.asarray(quant.opac_wave, np.float64),
        "interface wavelengths": np.asarray(quant.opac_interwave, np.float64),
        "wavelength width of bins": np.asarray(quant.opac_deltawave, np.float64),
        "ypoints": np.asarray(quant.gauss_y, np.float64),
        "units": np.array("CGS"),
        "FastChem path": np.array(str(getattr(reader, "fastchem_path", "") or "")),
        "premix settings": np.array(_settings(quant, refine, cell_error)),
    }
    if cell_error:
        d["premix cell error max"] = pm.get("cell_error_max")
        d["premix cell error mean"] = pm.get("cell_error_mean")
    return d


def make_premixer(quant, ctx, refine=(1, 1)):
    """a Premixer holding the species tables of `quant` (read by Read.read_species_*); mixing ratios are set per run"""
    from numpy.polynomial.legendre import leggauss
    gw = leggauss(int(quant.ny))[1] if int(quant.ny) > 1 else np.array([2.0])      # host_functions.set_up_numerical_parameters
    pm = Premixer(ctx, quant.nbin, quant.ny, quant.ntemp, quant.npress, len(quant.species_list), refine,
                  str(getattr(quant, "kcoeff_mixing", "RO")) == "correlated-k")
    try:
        pm.set_grid(quant.opac_wave, quant.gauss_y, gw, quant.ktemp, quant.kpress)
        for s, sp in enumerate(quant.species_list):
            h2o_scat = sp.scattering == "yes" and sp.name == "H2O"
            scat = None
            if sp.scattering == "yes" and not h2o_scat:
                scat = np.asarray(sp.scat_cross_sect_pretab, np.float64)[:int(quant.nbin)]
            pm.set_species(s, sp.opacity_pretab if sp.absorbing == "yes" else None, scat, None, 0.0, sp.weight,
                           sp.absorbing == "yes", sp.scattering == "yes", is_h2o=1 if h2o_scat else 0,
                           is_cia=1 if "CIA" in sp.name else 0, in_mu=1 if hsfunc._counts_for_mu(sp) else 0)
    except Exception:
        pm.close()
        raise
    return pm


def build_premixed_table(quant, reader, refine=(1, 1), cell_error=True, ctx=None, premixer=None):
    """the datasets of a premixed table of `quant`'s species set with the chemistry `reader` points at.  `premixer`: species
    tables already on the device (a sweep over chemistries uploads them once)."""
    refine = (int(refine[0]), int(refine[1]))
    if min(refine) < 1:
        raise IOError("premix: refinement factors are integers >= 1")
    check_species(quant)
    own_ctx = own_pm = False
    if premixer is None:
        if ctx is None:
            from .device import Context
            ctx, own_ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0"))), True
        premixer, own_pm = make_premixer(quant, ctx, refine), True
    try:
        for s, (table, const) in enumerate(species_mixing_ratios(quant, reader)):
            premixer.set_species_vmr(s, table, const)
        premixer.run(cell_error)
        return _collect(premixer, quant, reader, refine, cell_error)
    finally:
        if own_pm:
            premixer.close()
        if own_ctx:
            ctx.close()


def write_premixed_table(path, datasets):
    """`.npz` with the dataset names as keys; anything else as HDF5 through libhdf5 where it is present -- without it the
    same datasets go to `<path stem>.npz`.  Returns the path written."""
    path = str(path)
    if not path.endswith(".npz") and not hdf5_lite.available():
        path = os.path.splitext(path)[0] + ".npz"
    if os.path.dirname(path):
        os.makedirs(os.path.dirname(path), exist_ok=True)
    if path.endswith(".npz"):
        np.savez(path, **datasets)
    else:
        hdf5_lite.write(path, datasets)
    return path


def read_species_inputs(argv):
    """helios.py's reading of the on-the-fly input: species file, per-species containers, Rayleigh cross-sections"""
    from . import quantities as quant_mod
    from . import read as read_mod
    reader, quant = read_mod.Read(), quant_mod.Store()
    reader.read_param_file_and_command_line(quant, reader.cloud, argv)
    reader.read_species_file(quant)
    check_sources(quant.species_list)      # before the containers are read
    reader.read_species_opacities(quant)
    reader.read_species_scat_cross_sections(quant)
    return quant, reader


def summary_line(datasets, seconds):
    nT, nP = len(datasets["temperatures"]), len(datasets["pressures"])
    line = "premix: %d nodes (%d x %d) in %.2f s" % (nT * nP, nT, nP, seconds)
    if "premix cell error max" in datasets:
        e = np.asarray(datasets["premix cell error max"])
        line += ", cell error largest %.3e, median %.3e" % (e.max(), np.median(e))
    return line


def main(argv=None):
    """premix.py: one table, or one per FastChem directory of `-sweep`; returns the paths written"""
    opt, rest = parse_args(argv)
    quant, reader = read_species_inputs(rest)
    check_species(quant)
    from .device import Context
    ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    pm = None
    try:
        pm = make_premixer(quant, ctx, opt.refine)
        dirs = opt.fastchem_dirs or [reader.fastchem_path]
        paths = sweep_output_paths(opt.premix_output, len(dirs)) if opt.fastchem_dirs else [opt.premix_output]
        written = []
        for d, path in zip(dirs, paths):
            reader.fastchem_path = d
            t0 = time.time()
            data = build_premixed_table(quant, reader, opt.refine, opt.cell_error, premixer=pm)
            written.append(write_premixed_table(path, data))
            print(summary_line(data, time.time() - t0) + " -> " + written[-1])
        if opt.fastchem_dirs:
            print("-sweep \"%s\"" % sweep_argument(written))
        return written
    finally:
        if pm is not None:
            pm.close()
        ctx.close()
