"""Premixed opacity tables for the table-sweep tests: small `.npz` containers with the dataset names of the reference's
k-table tool (what `Read.read_opac_file` reads), built from helios_amd/synthetic.py.  Tables of one sweep share the grid and
differ in all three arrays: the k-table (another seed, scaled), the Rayleigh cross-sections (scaled) and the mean molecular
mass."""
import os

import numpy as np

from helios_amd import synthetic as syn

# (seed, factor on the opacities, mean molecular mass [amu], factor on the Rayleigh cross-sections)
CHEMISTRIES = ((11, 1.0, 2.3, 1.0), (12, 3.0, 2.6, 2.0), (13, 10.0, 4.0, 0.5), (14, 0.3, 3.1, 4.0))


def table_arrays(nbin, seed, scale, mu, ray, ny=20, ntemp=6, npress=5, tmax=None):
    """dataset name -> array of one premixed table (`tmax`: another temperature grid, same size)"""
    interwave, wave, deltawave = syn.wavelength_grid(nbin)
    gauss_y, _w = syn.gauss_points(ny)
    ktemp, kpress = syn.tp_grid(ntemp, npress)
    if tmax is not None:
        ktemp = np.linspace(100.0, float(tmax), ntemp)
    rng = np.random.default_rng(seed)
    return {"kpoints": syn.ktable(rng, nbin, ny, ktemp, kpress, gauss_y) * scale,
            "weighted Rayleigh cross-sections": syn.rayleigh_table(wave, ntemp, npress) * ray,
            "meanmolmass": np.full(ntemp * npress, float(mu)) * np.linspace(1.0, 1.05, ntemp * npress),
            "center wavelengths": wave, "interface wavelengths": interwave, "wavelength width of bins": deltawave,
            "ypoints": gauss_y, "temperatures": ktemp, "pressures": kpress}


def write_table(path, nbin, seed, scale, mu, ray, **kw):
    np.savez(path, **table_arrays(nbin, seed, scale, mu, ray, **kw))
    return path


def write_chemistries(directory, nbin, count=3, **kw):
    """`count` tables on one grid, one file each; returns their paths"""
    os.makedirs(directory, exist_ok=True)
    return [write_table(os.path.join(directory, "chem%d.npz" % k), nbin, *CHEMISTRIES[k], **kw) for k in range(count)]
