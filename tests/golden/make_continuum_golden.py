"""What the REFERENCE's k-table tool computes for the Rayleigh file and the continuum containers
(tests/golden/ktable_continuum/reference.npz).

    /opt/conda/bin/python3.9 tests/golden/make_continuum_golden.py

Needs the interpreter that has astropy (the reference's constants) and a SciPy that still has `interp2d` (the reference's He-
interpolation; SciPy 1.7.1 here).  The reference's `Rayleigh_scat` (ktable/source_ktable/rayleigh.py) and `ContiClass`
(continuous.py) are imported at run time and called as its combination.py calls them -- per wavelength, with the grid's last
wavelength as the Rayleigh limit, the continuum divided by the mass of H or He -- on a grid of wavelengths that straddles every
branch of the formulas.  Results only are stored.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ktable_continuum")
REF = "/root/reference"
sys.dont_write_bytecode = True

TEMPERATURES = [50.0, 1400.0, 2000.0, 5040.0, 6000.0]          # the table's floor, two of its nodes, two between
PRESSURES = [1.0, 10 ** 3.33333333, 1e9]
RAYLEIGH = ["H2", "He", "H", "CO2", "CO", "O2", "N2", "e-"]


def wavelengths():
    """cm, ascending.  Around every threshold: the double whose product with 1e4 IS the threshold in micron, and its neighbours
    a part in 1e12 and a part in 1e6 away"""
    out = []
    for edge in (0.125, 0.1823, 0.3645, 1.6419, 0.5063, 200.0):
        at = edge * 1e-4
        for cand in (at, np.nextafter(at, 0), np.nextafter(at, 1)):
            if cand * 1e4 == edge:
                at = cand
        assert at * 1e4 == edge, edge
        out += [at * (1 - 1e-6), at * (1 - 1e-12), at, at * (1 + 1e-12), at * (1 + 1e-6)]
    split = 1 / 21360.0
    out += [split * (1 - 1e-9), split, split * (1 + 1e-9)]
    out += [1e-5, 1.5e-5, 2.2e-5, 15.1878e-4, 30e-4]
    out += list(10 ** np.linspace(np.log10(0.3e-4), np.log10(199e-4), 28))
    return np.unique(np.asarray(out, np.float64))


def import_reference():
    for gone, fn in (("asscalar", lambda a: a.item()), ("alen", len)):       # named by astropy 4.3.1 at import, never called
        if not hasattr(np, gone):
            setattr(np, gone, fn)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "ktable"))
    from source_ktable import rayleigh, continuous
    from source import phys_const as pc
    from source import species_database as sd
    return rayleigh.Rayleigh_scat(), continuous.ContiClass(), pc, sd


def main():
    import scipy
    ray, conti, pc, sd = import_reference()
    k_x = [float(v) for v in wavelengths()]
    limit = k_x[-1]
    d = {"wavelengths": np.array(k_x), "temperatures": np.array(TEMPERATURES), "pressures": np.array(PRESSURES),
         "sigma_T": np.float64(pc.SIGMA_T), "versions": np.array("scipy %s, numpy %s" % (scipy.__version__, np.__version__))}
    fits = {"H2": (ray.index_h2, ray.n_ref_h2, lambda l: ray.King_h2), "He": (ray.index_he, ray.n_ref_he, lambda l: ray.King_he),
            "CO": (ray.index_co, ray.n_ref_co, lambda l: ray.King_co), "CO2": (ray.index_co2, ray.n_ref_co2, ray.King_co2),
            "N2": (ray.index_n2, ray.n_ref_n2, ray.King_n2), "O2": (ray.index_o2, ray.n_ref_o2, ray.King_o2)}
    for name in RAYLEIGH:
        if name == "e-":
            sigma = [pc.SIGMA_T for _ in k_x]
        elif name == "H":
            sigma = [ray.cross_sect_h(l) for l in k_x]
        else:
            index, n_ref, king = fits[name]
            sigma = [ray.cross_sect(l, index(l), n_ref, king(l), limit) for l in k_x]
        d["rayleigh_" + name] = np.array(sigma, np.float64)
    m_h, m_he = sd.species_lib["H"].weight * pc.AMU, sd.species_lib["He"].weight * pc.AMU
    he = conti.include_he_min_opacity()
    bf, ff, hem = [], [], []
    for T in TEMPERATURES:
        for P in PRESSURES:
            for l in k_x:
                bf.append(conti.h_min_bf_cross_sect(l) / m_h)
                ff.append(conti.h_min_ff_cross_sect(l, T, P) / m_h)
                hem.append(10 ** he(T, np.log10(l * 1e4))[0] * P / m_he)
    shape = (len(TEMPERATURES), len(PRESSURES), len(k_x))
    d["cont_H-_bf"], d["cont_H-_ff"], d["cont_He-"] = [np.array(v, np.float64).reshape(shape) for v in (bf, ff, hem)]
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "reference.npz")
    np.savez_compressed(path, **d)
    print("wrote %s, %d bytes, %d wavelengths; sigma_T = %r" % (path, os.path.getsize(path), len(k_x), pc.SIGMA_T))


if __name__ == "__main__":
    main()
