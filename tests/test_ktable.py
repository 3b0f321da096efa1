"""Species k-tables from HELIOS-K output (helios_amd/ktable.py): the host logic and the numpy backend against what the
reference's k-table tool made of the same files (tests/golden/ktable, tests/golden/make_ktable_golden.py).  No GPU."""
import os
import re

import numpy as np
import pytest

import ktable_cases as kc
from helios_amd import ktable

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_file_names():
    assert ktable.parse_file_name("Out_00000_00100_00300_n100.bin") == (None, 0, 100, 300, "n100")
    assert ktable.parse_file_name("Out_my_mol_01_00000_00050_00300_p100.bin") == ("my_mol_01", 0, 50, 300, "p100")
    assert ktable.parse_file_name("Out_h2o_01000_02000_01500_p033.dat") == ("h2o", 1000, 2000, 1500, "p033")
    for bad in ("Info_00000.bin", "Out_1_2_3.bin", "Out_a_b_c_n100.bin"):
        with pytest.raises(IOError):
            ktable.parse_file_name(bad)


def test_pressure_table_is_the_references():
    g = kc.load("a")
    table = ktable.pressure_table()
    assert sorted(table) == [str(c) for c in g["press_codes"]]
    np.testing.assert_array_equal([table[str(c)] for c in g["press_codes"]], g["press_values"])


def test_target_grids():
    temp, press = ktable.default_target_grid()
    assert len(temp) == 120 and temp[0] == 50 and temp[-1] == 6000 and len(press) == 28
    assert press[0] == 1.0 and press[-1] == 1e9 and press[1] == 10 ** 0.33333333 and np.all(np.diff(press) > 0)
    t, p = ktable.target_grid("100 300 100", "2 6 5")
    np.testing.assert_array_equal(t, [100.0, 200.0, 300.0])
    np.testing.assert_allclose(p, [1e2, 1e3, 1e4, 1e5, 1e6], rtol=1e-15)
    with pytest.raises(IOError):
        ktable.target_grid("100 300", None)


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_grids_are_bit_equal(case, tmp_path):
    g = kc.load(case)
    if case == "a":
        inter = ktable.wavelength_grid("fixed_resolution", g["wavelength_grid"])
    else:
        path = os.path.join(str(tmp_path), "grid.dat")
        with open(path, "w") as f:
            f.write("".join("%.17e\n" % v for v in g["interfaces"]))
        inter = ktable.wavelength_grid("file", grid_file=path)
    centre, width, y = ktable.grid_datasets(inter, 20)
    np.testing.assert_array_equal(inter, g["interface wavelengths"])
    np.testing.assert_array_equal(centre, g["center wavelengths"])
    np.testing.assert_array_equal(width, g["wavelength width of bins"])
    np.testing.assert_array_equal(y, g["ypoints"])


def test_bin_ranges_and_the_empty_bin_rule():
    lam = ktable.spectral_axis(0, 50, 0.05)
    assert len(lam) == 1000 and lam[-1] == 10000.0 and lam[-2] == 1 / 0.05 and np.all(np.diff(lam) > 0)
    g = kc.load("b")
    start, end = ktable.bin_ranges(lam, g["interfaces"])
    assert list(end - start)[2:4] == [1, 2]                   # the one-point and the two-point bin
    for x in range(len(start)):
        inside = (g["interfaces"][x] <= lam) & (lam < g["interfaces"][x + 1])
        assert np.array_equal(np.nonzero(inside)[0], np.arange(start[x], end[x]))
    assert ktable.check_empty_bins(lam, g["interfaces"], start, end) == []
    # bins below the data are filled: the scan has not passed a point
    low = np.array([1e-3, 5e-3, 1e-2, lam[0], lam[3]])
    s, e = ktable.bin_ranges(lam, low)
    assert list(e - s) == [0, 0, 0, 3] and ktable.check_empty_bins(lam, low, s, e) == [0, 1, 2]
    # bins above the grid's last point as well, once that point was matched
    high = np.array([50.0, 20000.0, 30000.0])
    s, e = ktable.bin_ranges(lam, high)
    assert list(e - s) == [1, 0] and ktable.check_empty_bins(lam, high, s, e) == [1]
    # an interior bin without points is the reference's error
    bad = g["empty_bin_interfaces"]
    s, e = ktable.bin_ranges(lam, bad)
    assert str(g["empty_bin_error"]).startswith("IndexError") and list(e - s)[1] == 0
    with pytest.raises(IndexError, match="must be finer"):
        ktable.check_empty_bins(lam, bad, s, e)


def test_the_error_case_end_to_end(tmp_path):
    g = kc.load("b")
    d = kc.write_dir(os.path.join(str(tmp_path), "hk"), g)
    with pytest.raises(IndexError, match="must be finer"):
        ktable.build_species(d, g["empty_bin_interfaces"], 20, backend="numpy")


def test_refusals(tmp_path):
    wd = str(tmp_path)
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nXX %s\n" % wd)
    base = ["-path_to_individual_species_file", os.path.join(wd, "list.dat")]
    with pytest.raises(IOError, match="sampling is not built"):
        ktable.parse_args(base + ["-format", "sampling"])
    with pytest.raises(IOError, match="native_helios-k"):
        ktable.wavelength_grid("native_helios-k")
    g = kc.load("b")
    inter = g["interfaces"]
    k = kc.files_of(g)["Out_my_mol_01_00000_00050_00300_n100.bin"]
    # a first chunk that does not start at 0
    d = os.path.join(wd, "late")
    os.makedirs(d)
    k.tofile(os.path.join(d, "Out_00050_00100_00300_n100.bin"))
    with pytest.raises(IOError, match="not at 0"):
        ktable.build_species(d, inter, 20, backend="numpy")
    # a file whose point count is not the first file's resolution
    d = os.path.join(wd, "short")
    os.makedirs(d)
    k.tofile(os.path.join(d, "Out_00000_00050_00300_n100.bin"))
    k[:-1].tofile(os.path.join(d, "Out_00000_00050_00300_p000.bin"))
    with pytest.raises(IOError, match="resolution"):
        ktable.build_species(d, inter, 20, backend="numpy")
    # a pressure code outside the table
    d = os.path.join(wd, "code")
    os.makedirs(d)
    k.tofile(os.path.join(d, "Out_00000_00050_00300_n123.bin"))
    with pytest.raises(IOError, match="pressure code"):
        ktable.build_species(d, inter, 20, backend="numpy")
    with pytest.raises(TypeError, match="no .dat files"):
        ktable.build_species(d, inter, 20, heliosk_format="text", backend="numpy")
    with pytest.raises(IOError, match="backend"):
        ktable.build_species(d, inter, 20, backend="eager")


@pytest.mark.parametrize("case,suffix,n_gauss,text", kc.CASES)
def test_numpy_backend_against_the_reference(case, suffix, n_gauss, text, tmp_path):
    """every entry of every table, at max(1e-13, 8 eps_ref) in log10 k; over the bins the reference computed in double at
    that bound with the scan's own eps_ref (a few 1e-14)"""
    g = kc.load(case)
    d = kc.write_dir(os.path.join(str(tmp_path), "hk"), g, text=text)
    native, ip = ktable.build_species(d, kc.interfaces(g), n_gauss, "text" if text else "binary", backend="numpy")
    assert ip is None
    kc.check(g, suffix, native["kpoints"], "numpy " + case)
    np.testing.assert_array_equal(native["pressures"], g["pressures"])
    np.testing.assert_array_equal(native["temperatures"], g["temperatures"])
    if n_gauss == 20:
        np.testing.assert_array_equal(native["ypoints"], g["ypoints"])


def test_regridding_against_the_reference():
    """nodes below, on, between and above the source's in T and in P; bound max(1e-13, 8 eps_ref) with the reference's
    routine as measured against extended precision"""
    g = kc.load("a")
    nx = len(g["center wavelengths"])
    got = ktable.numpy_regrid(g["pressures"], g["temperatures"], g["kpoints"], g["regrid_temperatures"], g["regrid_pressures"],
                              nx, 20)
    dev = np.abs(np.log10(got) - np.log10(g["regrid_kpoints"])).max()
    tol = max(1e-13, 8 * float(g["eps_ref_regrid"]))
    print("regrid: deviation %.3e, eps_ref %.3e, bound %.3e" % (dev, float(g["eps_ref_regrid"]), tol))
    assert dev <= tol
    left, red = ktable.regrid_plan(g["temperatures"], g["regrid_temperatures"])
    assert list(left) == [0, 0, 0, 1, 1] and list(red) == [1, 1, 0, 1, 1]


def test_written_tables_read_back(tmp_path):
    """the tool on case b with the numpy backend: both containers, read by the product's reader as a species table"""
    from helios_amd.read import Read
    g = kc.load("b")
    wd = str(tmp_path)
    d = kc.write_dir(os.path.join(wd, "hk"), g)
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species      path\n\nXX %s\n" % d)
    with open(os.path.join(wd, "grid.dat"), "w") as f:
        f.write("".join("%.17e\n" % v for v in g["interfaces"]))
    for container in ("npz", "h5"):
        out = os.path.join(wd, "out_" + container)
        written = ktable.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-grid_format", "file",
                               "-path_to_grid_file", os.path.join(wd, "grid.dat"), "-directory_with_individual_files", out,
                               "-backend", "numpy", "-container", container, "-temperature_grid", "200 400 100",
                               "-pressure_grid", "4 8 3"])
        assert [os.path.basename(w).split(".")[0] for w in written] == ["XX_opac_kdistr", "XX_opac_ip_kdistr"]

        class Q(object):
            pass
        q = Q()
        k = np.asarray(Read().read_opac_file(q, written[0], type="species", read_grid_parameters=True), np.float64)
        kc.check(g, "", k, "written " + container)
        np.testing.assert_array_equal(np.asarray(q.opac_interwave, np.float64), g["interface wavelengths"])
        np.testing.assert_array_equal(np.asarray(q.opac_wave, np.float64), g["center wavelengths"])
        np.testing.assert_array_equal(np.asarray(q.gauss_y, np.float64), g["ypoints"])
        np.testing.assert_array_equal(np.asarray(q.kpress, np.float64), g["pressures"])
        np.testing.assert_array_equal(np.asarray(q.ktemp, np.float64), g["temperatures"])
        q = Q()
        kip = np.asarray(Read().read_opac_file(q, written[1], type="species", read_grid_parameters=True), np.float64)
        assert int(q.ntemp) == 3 and int(q.npress) == 3 and int(q.nbin) == 6 and int(q.ny) == 20
        want = ktable.numpy_regrid(g["pressures"], g["temperatures"], k, [200.0, 300.0, 400.0], [1e4, 1e6, 1e8], 6, 20)
        np.testing.assert_array_equal(kip, want)


def test_header_and_bindings_in_step():
    from helios_amd import _lib
    text = open(_lib.HEADER_PATH).read()
    names = set(re.findall(r"\b(hx_ktable_[a-z_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", text, flags=re.S)))
    assert names == {"hx_ktable_create", "hx_ktable_destroy", "hx_ktable_set_grid", "hx_ktable_run", "hx_ktable_put",
                     "hx_ktable_regrid", "hx_ktable_get"}
    protos = _lib.prototypes()
    lib = _lib.lib()
    for n in names:
        assert n in protos and hasattr(lib, n), n
    assert len(protos["hx_ktable_create"][1]) == 8 and len(protos["hx_ktable_regrid"][1]) == 13


def test_readers_are_bounded():
    assert ktable.MAX_READERS <= 16
