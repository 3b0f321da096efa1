"""What the REFERENCE's mixing stage computes (tests/golden/ktable_mix/*.npz).

    /opt/conda/bin/python3.9 tests/golden/make_mixed_golden.py

Needs the interpreter make_continuum_golden.py needs (astropy, h5py, a SciPy with `interp2d`).  Seeded inputs go to a temporary
directory -- native containers of 4 bins x 3 Gauss points, a 4 x 4 FastChem output, a species file -- and the reference's
`Comb.combine_all_species` runs on them with its `Rayleigh_scat` and `ContiClass`, on its hard-coded 120 x 28 grid.  Stored: the
inputs, every data set of the mixed file, the `_ip_` containers the reference wrote (case a), and next to each expected array
`eps_ref`, the reference's largest relative deviation from the long-double restatement of tests/ktable_mix_reference.py.
Data only; nothing of the reference's text.
"""
import os
import shutil
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ktable_mix")
sys.dont_write_bytecode = True
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import make_continuum_golden as mcg          # noqa: E402
import make_ktable_golden as mkg             # noqa: E402
import ktable_mix_reference as kr            # noqa: E402
from helios_amd import continuum             # noqa: E402
from helios_amd.ktable import default_target_grid      # noqa: E402

MIXED_KEYS = ("pressures", "temperatures", "meanmolmass", "kpoints", "weighted Rayleigh cross-sections", "wavelengths",
              "center wavelengths", "interface wavelengths", "wavelength width of bins", "ypoints")


def h5_writer(stem, data):
    import h5py
    with h5py.File(stem + ".h5", "w") as f:
        for k, v in data.items():
            f.create_dataset(k, data=v)


def h5_read(path):
    import h5py
    with h5py.File(path, "r") as f:
        return {k: np.asarray(f[k][()]) for k in f.keys()}


def containers(grid, temp, press):
    nc = len(grid["center wavelengths"]) * len(grid["ypoints"])
    out = {}
    for name, (T, P) in kr.NATIVE.items():
        out[name + "_opac_kdistr"] = dict(grid, temperatures=np.array(T), pressures=np.array(P),
                                          kpoints=kr.native_table(name, nc))
    out["CIA_H2H2_opac_ip_kdistr"] = dict(grid, temperatures=temp, pressures=press,
                                          kpoints=kr.cia_ip_table(len(temp) * len(press), nc))
    return out


def run_reference(comb, ray, conti, root, units):
    p = mkg.Param()
    p.format, p.units = "k-distribution", units
    p.individual_calc_path = os.path.join(root, "opac") + "/"
    p.final_species_file_path = os.path.join(root, "final_species.dat")
    p.fastchem_path = os.path.join(root, "chem") + "/"
    p.final_path = os.path.join(root, "mixed") + "/"
    c = comb.Comb()
    c.combine_all_species(p, ray, conti)
    return h5_read(os.path.join(p.final_path, "mixed_opac_kdistr.h5"))


def failure(comb, ray, conti, tmp, species):
    root = tempfile.mkdtemp(dir=tmp)
    kr.write_inputs(root, species, {}, {}, h5_writer)
    try:
        run_reference(comb, ray, conti, root, "CGS")
    except Exception as e:          # noqa: BLE001 -- the text is the result
        return "%s: %s" % (type(e).__name__, e)
    return "no exception"


def main():
    _bio, comb = mkg.import_reference()
    ray, conti, _pc, _sd = mcg.import_reference()
    kr.require_extended_precision()
    temp, press = default_target_grid()
    grid = kr.grid_arrays()
    wave, ny = grid["center wavelengths"], len(grid["ypoints"])
    cols = kr.chemistry()
    n_chem = len(kr.CHEM_T) * len(kr.CHEM_PBAR)
    on_node = [p * 1e6 in press for p in kr.CHEM_PBAR]
    assert on_node[0] and sum(on_node) >= 2, on_node
    cases = {"a": (kr.SPECIES_A, {"chem.dat": kr.chem_text(cols, range(n_chem))}, "CGS"),
             "b": (kr.SPECIES_A, {"chem_low.dat": kr.chem_text(cols, range(8)),
                                  "chem_high.dat": kr.chem_text(cols, range(8, n_chem))}, "MKS"),
             "c": (kr.SPECIES_C, {}, "CGS")}
    scale = {"pressures": 1e-1, "kpoints": 1e-1, "weighted Rayleigh cross-sections": 1e-4}
    os.makedirs(OUT, exist_ok=True)
    tmp = tempfile.mkdtemp()
    try:
        inputs = containers(grid, temp, press)
        for tag, (species, chem_files, units) in cases.items():
            root = tempfile.mkdtemp(dir=tmp)
            kr.write_inputs(root, species, chem_files, inputs, h5_writer)
            mixed = run_reference(comb, ray, conti, root, units)
            made = {n: h5_read(os.path.join(root, "opac", n + "_opac_ip_kdistr.h5"))["kpoints"]
                    for n in ("H2O", "CO2", "H-_bf", "H-_ff", "He-")}
            sig_ref = h5_read(os.path.join(root, "opac", "scat_cross_sections.h5"))
            # the restatement, from the contract's own tables
            tables = {"CIA_H2H2": ("final", inputs["CIA_H2H2_opac_ip_kdistr"]["kpoints"])}
            for n in ("H2O", "CO2"):
                c = inputs[n + "_opac_kdistr"]
                tables[n] = ("native", c["temperatures"], c["pressures"], c["kpoints"])
            for n in ("H-_bf", "H-_ff", "He-"):
                tables[n] = ("final", np.repeat(continuum.numpy_continuum(n, wave, temp, press).reshape(-1), ny))
            sigmas = {n: continuum.rayleigh_cross_section(n, wave) for n in ("H2", "He", "CO2")}
            case = dict(grid, temperatures=temp, pressures=press, species=list(species))
            if chem_files:
                order = ["chem.dat"] if "chem.dat" in chem_files else ["chem_low.dat", "chem_high.dat"]
                case["chem"] = kr.chem_parsed([chem_files[k] for k in order])
            want = kr.reference_case(case, tables, sigmas)
            d = {"units": np.array(units), "species_text": np.array(kr.species_text(species))}
            for k in MIXED_KEYS:
                d["mixed " + k] = np.asarray(mixed[k], np.float64)
            for k, v in want.items():
                got = np.asarray(mixed[k], np.float64) / (scale.get(k, 1.0) if units == "MKS" else 1.0)
                d["eps_ref " + k] = np.float64(kr.relative_deviation(got, v))
                print("case %s: %s: eps_ref %.3e, min %.3e" % (tag, k, d["eps_ref " + k], got.min()))
            for name, text in chem_files.items():
                d["chem_text " + name] = np.array(text)
            np.savez_compressed(os.path.join(OUT, tag + ".npz"), **d)
            if tag == "a":
                for n, c in inputs.items():
                    if n.endswith("_opac_kdistr"):
                        for k in ("temperatures", "pressures", "kpoints"):
                            d_in = "native %s %s" % (n[:-len("_opac_kdistr")], k)
                            made[d_in] = c[k]
                for n in ("H2", "He", "CO2"):
                    made["rayleigh_" + n] = np.asarray(sig_ref["rayleigh_" + n], np.float64)
                for n in ("H-_bf", "H-_ff", "He-"):
                    print("reference container %s: min %.6e" % (n, made[n].min()))
                lines = {k: v for k, v in made.items() if not k.startswith(("H-", "He-"))}
                conts = {k: v for k, v in made.items() if k.startswith(("H-", "He-"))}
                np.savez_compressed(os.path.join(OUT, "a_containers_lines.npz"), **lines)
                np.savez_compressed(os.path.join(OUT, "a_containers_continuum.npz"), **conts)
        # the failures and the findings
        none_absorbing = [(n, "no", s, r) for n, _a, s, r in kr.SPECIES_C]
        unknown = list(kr.SPECIES_C) + [("XYZ2", "yes", "no", "1e-3")]
        no_fc = list(kr.SPECIES_C) + [("TiH", "yes", "no", "FastChem")]
        with np.errstate(all="ignore"):
            zero = ray.cross_sect(1e-4, ray.index_h2o(1e-4, np.float64(1e6), np.float64(1000.0), np.float64(0.0)),
                                  ray.n_ref_h2o(np.float64(1e6), np.float64(1000.0), np.float64(0.0)), ray.King_h2o, 2.5e-4)
        f = {"no absorbing species": np.array(failure(comb, ray, conti, tmp, none_absorbing)),
             "unknown species": np.array(failure(comb, ray, conti, tmp, unknown)),
             "FastChem name missing": np.array(failure(comb, ray, conti, tmp, no_fc)),
             "water cross-section at mixing ratio 0": np.float64(zero)}
        for k, v in f.items():
            print("%s -> %s" % (k, v))
        np.savez_compressed(os.path.join(OUT, "d.npz"), **f)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    for name in sorted(os.listdir(OUT)):
        print("%s: %d bytes" % (name, os.path.getsize(os.path.join(OUT, name))))


if __name__ == "__main__":
    main()
