"""The premixed-table tool without a device: options, refusals, the file round trip, grid and sweep arithmetic."""
import importlib.util
import os

import numpy as np
import pytest

from helios_amd import hdf5_lite
from helios_amd import premix
from helios_amd import quantities as quant_mod
from helios_amd import read as read_mod


def _host_golden_module():
    spec = importlib.util.spec_from_file_location(
        "make_host_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_host_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    return mk


SPECIES_NO_FILE = ("species      absorbing       scattering         mixing_ratio\n\n"
                   "H2   no  yes  FastChem\n\nH2O  yes yes FastChem\n\nCO2  yes no  3e-4\nCH4 yes no 1e-4\n"
                   "H-   yes no  FastChem\nHe  no yes 0.15\nCIA_H2H2 yes no FastChem\nCIA_H2He yes no 0.85&0.15\n")


def _argv(wd):
    return ["-parameter_file", "/nonexistent", "-opacity_mixing", "on-the-fly",
            "-path_to_species_file", os.path.join(wd, "species.dat"),
            "-directory_with_fastchem_files", os.path.join(wd, "chem") + "/",
            "-directory_with_opacity_files", os.path.join(wd, "opac") + "/"]


def test_cli_parsing():
    opt, rest = premix.parse_args(["-premix_output", "out/solar.h5", "-premix_refine", "2,3", "-premix_cell_error", "no",
                                   "-name", "x", "-k_coefficients_mixing_method", "correlated-k"])
    assert opt.premix_output == "out/solar.h5" and opt.refine == (2, 3) and opt.cell_error is False
    assert opt.fastchem_dirs is None and rest == ["-name", "x", "-k_coefficients_mixing_method", "correlated-k"]
    opt, rest = premix.parse_args(["-sweep", "directory_with_fastchem_files=a/,b/,c/"])
    assert opt.fastchem_dirs == ["a/", "b/", "c/"] and opt.refine == (1, 1) and opt.cell_error is True and rest == []
    for bad in ("0,1", "2", "a,b", "1,2,3", "1.5,2"):
        with pytest.raises(IOError, match="premix_refine"):
            premix.parse_args(["-premix_refine", bad])
    with pytest.raises(IOError, match="directory_with_fastchem_files"):
        premix.parse_args(["-sweep", "internal_temperature=100,200"])
    with pytest.raises(SystemExit):
        premix.parse_args(["-premix_cell_error", "maybe"])


def test_refuses_a_vertical_profile_file_before_reading_any_table(tmp_path):
    wd = str(tmp_path)
    _host_golden_module().write_species_inputs(wd, nbin=5, ny=20)        # its species file has two `file` sources
    for f in os.listdir(os.path.join(wd, "opac")):                       # no table may be needed to refuse
        os.remove(os.path.join(wd, "opac", f))
    with pytest.raises(IOError, match="CO2 comes from a vertical-profile file.*not a function of"):
        premix.read_species_inputs(_argv(wd))


def _read(wd, extra=()):
    with open(os.path.join(wd, "species.dat"), "w") as f:
        f.write(SPECIES_NO_FILE)
    return premix.read_species_inputs(_argv(wd) + list(extra))


def test_refuses_nodes_that_are_not_uniform(tmp_path):
    wd = str(tmp_path)
    _host_golden_module().write_species_inputs(wd, nbin=5, ny=20)
    quant, _reader = _read(wd)
    premix.check_species(quant)                                          # 200, 1000, 1800 K and 1e2, 1e5, 1e8: uniform
    good_T, good_P = quant.ktemp.copy(), quant.kpress.copy()
    quant.ktemp = good_T * np.array([1.0, 1.0 + 1e-7, 1.0])
    with pytest.raises(IOError, match="temperature nodes are not uniform"):
        premix.check_species(quant)
    quant.ktemp = good_T * np.array([1.0, 1.0 + 1e-11, 1.0])             # within 1e-9
    premix.check_species(quant)
    quant.kpress = good_P * np.array([1.0, 1.001, 1.0])
    with pytest.raises(IOError, match="log10 pressure nodes are not uniform"):
        premix.check_species(quant)


def test_refuses_more_than_twenty_gauss_points_with_random_overlap(tmp_path):
    wd = str(tmp_path)
    _host_golden_module().write_species_inputs(wd, nbin=5, ny=24)
    quant, _reader = _read(wd)
    assert int(quant.ny) == 24 and quant.kcoeff_mixing == "RO"
    with pytest.raises(IOError, match="at most 20 Gauss points"):
        premix.check_species(quant)
    with pytest.raises(IOError, match="at most 20 Gauss points"):       # ... and before a device is asked for
        premix.build_premixed_table(quant, _reader, ctx=None)
    quant_ck, _r = _read(wd, ["-k_coefficients_mixing_method", "correlated-k"])
    premix.check_species(quant_ck)


def _datasets(nT=4, nP=3, nbin=5, ny=20, seed=1):
    rng = np.random.default_rng(seed)
    inter = 1e-4 * 2.0 ** np.arange(nbin + 1)
    return {
        "pressures": 10.0 ** np.linspace(0.0, 8.0, nP), "temperatures": np.linspace(100.0, 2900.0, nT),
        "meanmolmass": rng.uniform(2.0, 30.0, nT * nP), "kpoints": 10.0 ** rng.uniform(-12, 3, nT * nP * nbin * ny),
        "weighted Rayleigh cross-sections": 10.0 ** rng.uniform(-30, -24, nT * nP * nbin),
        "included molecules": np.array(["H2O", "CO2", "CIA_H2H2"]),
        "center wavelengths": 0.5 * (inter[1:] + inter[:-1]), "interface wavelengths": inter,
        "wavelength width of bins": np.diff(inter), "ypoints": (np.arange(ny) + 0.5) / ny, "units": np.array("CGS"),
        "FastChem path": np.array("chem/"), "premix settings": np.array("refine=1,1"),
        "premix cell error max": rng.uniform(0, 1, (nT - 1) * (nP - 1)),
        "premix cell error mean": rng.uniform(0, 1, (nT - 1) * (nP - 1)),
    }


@pytest.mark.parametrize("ext", [".npz", ".h5"])
def test_writer_and_reader_round_trip(tmp_path, ext):
    if ext == ".h5" and not hdf5_lite.available():
        pytest.skip("no libhdf5 on this host")
    d = _datasets()
    path = premix.write_premixed_table(str(tmp_path / "sub" / ("table" + ext)), d)
    assert path.endswith(ext) and os.path.exists(path)
    q = quant_mod.Store()
    opac_k = read_mod.Read().read_opac_file(q, path, type="premixed")
    from helios_amd import phys_const as pc
    np.testing.assert_array_equal(opac_k, d["kpoints"])
    np.testing.assert_array_equal(q.opac_scat_cross, d["weighted Rayleigh cross-sections"])
    np.testing.assert_array_equal(q.opac_meanmass, d["meanmolmass"] * pc.AMU)
    for attr, name in (("opac_wave", "center wavelengths"), ("opac_interwave", "interface wavelengths"),
                       ("opac_deltawave", "wavelength width of bins"), ("gauss_y", "ypoints"),
                       ("ktemp", "temperatures"), ("kpress", "pressures")):
        np.testing.assert_array_equal(getattr(q, attr), d[name], err_msg=name)
    assert (int(q.nbin), int(q.ny), int(q.ntemp), int(q.npress)) == (5, 20, 4, 3)
    t = read_mod.Read._open_table(path)                                  # the additions ride along
    np.testing.assert_array_equal(np.asarray(t["premix cell error max"], float), d["premix cell error max"])
    np.testing.assert_array_equal(np.asarray(t["premix cell error mean"], float), d["premix cell error mean"])


def test_without_libhdf5_the_table_goes_to_an_npz_of_the_same_names(tmp_path, monkeypatch):
    monkeypatch.setattr(hdf5_lite, "available", lambda: False)
    path = premix.write_premixed_table(str(tmp_path / "table.h5"), _datasets())
    assert path == str(tmp_path / "table.npz") and sorted(np.load(path).keys()) == sorted(_datasets().keys())


def test_output_grid_arithmetic():
    assert premix.output_grid_size(30, 20) == (30, 20)
    assert premix.output_grid_size(30, 20, (2, 2)) == (59, 39)
    assert premix.output_grid_size(6, 5, (4, 1)) == (21, 5)
    assert premix.output_grid_size(2, 2, (3, 7)) == (4, 8)


def test_numbering_of_sweep_outputs():
    paths = premix.sweep_output_paths("out/grid.h5", 3)
    assert paths == ["out/grid_0.h5", "out/grid_1.h5", "out/grid_2.h5"]
    assert premix.sweep_output_paths("grid.v2.npz", 2) == ["grid.v2_0.npz", "grid.v2_1.npz"]
    assert premix.sweep_argument(paths) == "path_to_opacity_file=out/grid_0.h5,out/grid_1.h5,out/grid_2.h5"
    from helios_amd import sweep as sw
    assert [o["path_to_opacity_file"] for o in sw.expand_sweep(premix.sweep_argument(paths))] == paths
