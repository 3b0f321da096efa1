"""The Rayleigh file and the continuum containers of ktable.py (helios_amd/continuum.py): the numpy backend against what the
reference computes (tests/golden/ktable_continuum, made by tests/golden/make_continuum_golden.py) under the rule of
tests/test_ktable.py -- max(1e-13, 8 eps_ref), eps_ref the reference's own deviation from the long-double restatement, here
per entry -- and the files the tool writes, read back by the product's readers.  No GPU.

Measured (profiles/ktable_continuum_parity.json): the reference's eps_ref reaches 9e-12 for the Rayleigh species (n^2 - 1),
1.4e-4 for H-_bf a part in 1e12 below 1.6419 micron, 5e-11 for H-_ff (50 K, 0.38 micron); the numpy backend stays within
2e-14 of the restatement everywhere."""
import json
import os

import numpy as np
import pytest

import continuum_reference as cr
import ktable_cases as kc
from helios_amd import continuum, ktable
from helios_amd import continuum_data as cd


@pytest.fixture(scope="module")
def golden():
    return np.load(cr.GOLDEN)


def _record(name, rec):
    """added to the JSON file that KTABLE_CONTINUUM_PARITY_JSON names, if it is set"""
    path = os.environ.get("KTABLE_CONTINUUM_PARITY_JSON")
    if path:
        have = json.load(open(path)) if os.path.exists(path) else {}
        have[name] = rec
        json.dump(have, open(path, "w"), indent=1, sort_keys=True)


def test_the_golden_straddles_every_branch(golden):
    mu = golden["wavelengths"] * 1e4
    assert 55 <= len(mu) <= 70 and np.all(np.diff(mu) > 0)
    for edge in (0.125, 0.1823, 0.3645, 1.6419, 0.5063, 200.0):
        assert np.any(mu == edge) and np.any((mu < edge) & (mu > edge * (1 - 2e-12))) and np.any((mu > edge) & (mu < edge * (1 + 2e-12)))
    nu = 1.0 / golden["wavelengths"]
    assert np.any(nu <= 21360) and np.any((nu > 21360) & (nu < 21360 * (1 + 2e-9)))
    assert list(golden["temperatures"]) == [50.0, 1400.0, 2000.0, 5040.0, 6000.0] and len(golden["pressures"]) == 3
    assert float(golden["sigma_T"]) == continuum.pc.SIGMA_T


@pytest.mark.parametrize("name", cd.RAYLEIGH_SPECIES)
def test_rayleigh_against_the_reference(golden, name):
    w = golden["wavelengths"]
    rec = cr.check(continuum.rayleigh_cross_section(name, w), golden["rayleigh_" + name], cr.rayleigh(name, w), "rayleigh_" + name)
    assert rec["own_max_deviation_from_long_double"] < 1e-13
    _record("rayleigh_" + name, rec)


@pytest.mark.parametrize("name", sorted(continuum.CONTINUUM_KINDS))
def test_continuum_against_the_reference(golden, name):
    w, T, P = golden["wavelengths"], golden["temperatures"], golden["pressures"]
    got = continuum.numpy_continuum(name, w, T, P)
    assert got.shape == (15, len(w))
    rec = cr.check(got, golden["cont_" + name], cr.continuum(name, w, T, P), name)
    assert rec["own_max_deviation_from_long_double"] < 1e-13
    if name != "He-":
        assert rec["zeros"] > 0               # He- is 1e-30 P / m outside its table, never 0
    _record(name, rec)
    # a subset of rows is the same rows
    np.testing.assert_array_equal(continuum.numpy_continuum(name, w, T, P, rows=[4, 14]), got[[4, 14]])


def test_species_names():
    assert continuum.continuum_species("H-,He-") == ["H-_bf", "H-_ff", "He-"]
    assert continuum.continuum_species(" He- , H-_ff,H-") == ["He-", "H-_ff", "H-_bf"]
    with pytest.raises(IOError, match="no continuum table for 'H2-'"):
        continuum.continuum_species("H-,H2-")
    assert continuum.rayleigh_species("H2,He,H,CO2,CO,O2,N2,e-") == ["H2", "He", "H", "CO2", "CO", "O2", "N2", "e-"]
    with pytest.raises(IOError, match="depends on its mixing ratio.*h2o_rayleigh_cross"):
        continuum.rayleigh_species("H2,H2O")
    with pytest.raises(IOError, match="no Rayleigh cross-section for 'CH4'; implemented: H2, He, H, CO2, CO, O2, N2, e-"):
        continuum.rayleigh_species("CH4")


def test_refusals_of_the_tool(tmp_path):
    wd = str(tmp_path)
    base = ["-directory_with_individual_files", wd, "-backend", "numpy", "-container", "npz"]
    with pytest.raises(IOError, match="sampling is not built"):
        ktable.main(base + ["-continuum_species", "H-", "-format", "sampling"])
    with pytest.raises(IOError, match="mixing ratio"):
        ktable.main(base + ["-rayleigh_species", "H2O"])
    with pytest.raises(IOError, match="implemented: H2, He"):
        ktable.main(base + ["-rayleigh_species", "H2,Xe"])
    with pytest.raises(IOError, match="no such container"):
        ktable.main(base + ["-continuum_species", "He-", "-grid_like", os.path.join(wd, "none.npz")])
    with pytest.raises(SystemExit):
        ktable.parse_args(base)
    assert os.listdir(wd) == []


class _Q(object):
    pass


def _read_directory(wd, species_text, nlayer=3):
    """the product's readers on a directory of containers, as premix.py and helios.py call them"""
    from helios_amd.read import Read, Species
    q, r = _Q(), Read()
    q.fl_prec, q.nlayer, q.ninterface, q.iso = np.float64, nlayer, nlayer + 1, 0
    r.opacity_path = wd if wd.endswith("/") else wd + "/"
    q.species_list = [Species(name=n, absorbing=a, scattering=s, source_for_vmr="1e-3") for n, a, s in species_text]
    r.read_species_opacities(q)
    r.read_species_scat_cross_sections(q)
    return q


def _containers():
    """.h5 is a case only where an HDF5 library can be loaded: without one the tool writes .npz whatever it is asked for"""
    from helios_amd import hdf5_lite
    return ["npz", "h5"] if hdf5_lite.available() else ["npz"]


@pytest.mark.parametrize("container", _containers())
def test_written_files_read_back(tmp_path, container):
    """the tool on its own grid options: three containers and the Rayleigh file, read by Read.read_species_opacities and
    Read.read_species_scat_cross_sections unchanged"""
    wd = os.path.join(str(tmp_path), "opac")
    written = ktable.main(["-continuum_species", "H-,He-", "-rayleigh_species", "H2,He,H,CO2,CO,O2,N2,e-", "-wavelength_grid",
                           "8 0.1 250", "-number_of_gaussian_points", "7", "-temperature_grid", "50 6000 1487.5", "-pressure_grid",
                           "0 9 3", "-directory_with_individual_files", wd, "-backend", "numpy", "-container", container])
    assert [os.path.basename(p) for p in written] == [n + "_opac_ip_kdistr." + container for n in ("H-_bf", "H-_ff", "He-")] + [
        "scat_cross_sections." + container]
    inter = ktable.wavelength_grid("fixed_resolution", "8 0.1 250".split())
    centre, width, yg = ktable.grid_datasets(inter, 7)
    T, P = ktable.target_grid("50 6000 1487.5", "0 9 3")
    q = _read_directory(wd, [("H-_bf", "yes", "no"), ("H-_ff", "yes", "no"), ("He-", "yes", "no")] +
                        [(n, "no", "yes") for n in cd.RAYLEIGH_SPECIES])
    np.testing.assert_array_equal(np.asarray(q.opac_interwave, np.float64), inter)
    np.testing.assert_array_equal(np.asarray(q.opac_wave, np.float64), centre)
    np.testing.assert_array_equal(np.asarray(q.opac_deltawave, np.float64), width)
    np.testing.assert_array_equal(np.asarray(q.gauss_y, np.float64), yg)
    np.testing.assert_array_equal(np.asarray(q.ktemp, np.float64), T)
    np.testing.assert_array_equal(np.asarray(q.kpress, np.float64), P)
    assert int(q.ny) == 7 and int(q.nbin) == len(centre) and int(q.ntemp) == 5 and int(q.npress) == 3
    for sp in q.species_list[:3]:
        want = np.repeat(continuum.numpy_continuum(sp.name, centre, T, P).reshape(-1), 7)         # [t][p][x][y]
        np.testing.assert_array_equal(np.asarray(sp.opacity_pretab, np.float64), want)
    for sp in q.species_list[3:]:
        want = continuum.rayleigh_cross_section(sp.name, centre)
        np.testing.assert_array_equal(np.asarray(sp.scat_cross_sect_pretab, np.float64), want)
        np.testing.assert_array_equal(sp.scat_cross_sect_layer, np.tile(want, 3))
    table = continuum._open(written[-1])
    np.testing.assert_array_equal(np.asarray(table["wavelengths"], np.float64), centre)


def test_grid_like_is_bit_for_bit_and_existing_rayleigh_data_stay(tmp_path):
    """a species container made by the tool from HELIOS-K files gives its grid to the analytic tables; a second call finds
    rayleigh_H2 -- replaced by other numbers in between -- and leaves it, adding what is new"""
    g = kc.load("a")
    wd = str(tmp_path)
    kc.write_dir(os.path.join(wd, "hk"), g)
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nXX %s\n" % os.path.join(wd, "hk"))
    out = os.path.join(wd, "opac")
    common = ["-directory_with_individual_files", out, "-backend", "numpy", "-container", "npz"]
    first = ktable.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-wavelength_grid", "20 30 2000",
                         "-number_of_gaussian_points", "8", "-temperature_grid", "200 400 100", "-pressure_grid", "4 8 3"] + common)
    src = np.load(first[1])
    written = ktable.main(["-continuum_species", "H-_ff", "-rayleigh_species", "H2", "-grid_like", first[1]] + common)
    assert [os.path.basename(p) for p in written] == ["H-_ff_opac_ip_kdistr.npz", "scat_cross_sections.npz"]
    made = np.load(written[0])
    for key in continuum.GRID_KEYS:
        assert made[key].tobytes() == src[key].tobytes() and made[key].dtype == src[key].dtype, key
    assert made["kpoints"].shape == src["kpoints"].shape
    # species and analytic tables in one call share the grid as well
    both = ktable.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-wavelength_grid", "20 30 2000",
                        "-number_of_gaussian_points", "8", "-temperature_grid", "200 400 100", "-pressure_grid", "4 8 3",
                        "-continuum_species", "He-"] + ["-directory_with_individual_files", os.path.join(wd, "both"), "-backend",
                                                       "numpy", "-container", "npz"])
    assert [os.path.basename(p) for p in both] == ["XX_opac_kdistr.npz", "XX_opac_ip_kdistr.npz", "He-_opac_ip_kdistr.npz"]
    for key in continuum.GRID_KEYS:
        assert np.load(both[2])[key].tobytes() == np.load(both[1])[key].tobytes(), key
    # an existing data set is kept
    scat = dict(np.load(written[1]))
    marked = scat["rayleigh_H2"] * 3.0
    np.savez(written[1], wavelengths=scat["wavelengths"], rayleigh_H2=marked)
    again = ktable.main(["-rayleigh_species", "H2,He", "-grid_like", first[1]] + common)
    scat = np.load(again[0])
    assert sorted(scat.files) == ["rayleigh_H2", "rayleigh_He", "wavelengths"]
    np.testing.assert_array_equal(scat["rayleigh_H2"], marked)
    np.testing.assert_array_equal(scat["rayleigh_He"], continuum.rayleigh_cross_section("He", src["center wavelengths"]))
    # another grid in the same directory is refused
    with pytest.raises(IOError, match="share one grid"):
        ktable.main(["-rayleigh_species", "CO", "-wavelength_grid", "20 30 1000"] + common)
