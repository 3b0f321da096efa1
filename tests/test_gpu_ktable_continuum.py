"""k_ktable_continuum (csrc/ktable.hip) against the long-double restatement of tests/continuum_reference.py under the rule of
the k-table tests -- within max(1e-13, 8 eps64) of the restatement per entry, eps64 the numpy backend's own deviation from it
there, zeros exactly zero -- at the smallest shapes that reach every path of its store loop; the two backends on a whole tool
call; and the chain: species tables, H- containers and the Rayleigh file written by ktable.py alone, read by helios.py on the fly and by premix.py.
Nothing here reads the reference tree."""
import os

import numpy as np
import pytest

import continuum_reference as cr
import ktable_cases as kc
from helios_amd import continuum, ktable

pytestmark = pytest.mark.gpu

TEMPS, PRESS = [50.0, 1400.0, 2000.0, 5040.0, 6000.0], [1.0, 10 ** 3.33333333, 1e9]
SENTINEL = -7.25
_exact = {}


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def exact(name):
    """the restatement on the 257 wavelengths and 5 x 3 nodes, once per kind; the smaller shapes are subsets of it"""
    if name not in _exact:
        w = cr.branch_wavelengths(257)
        _exact[name] = (w, cr.continuum(name, w, TEMPS, PRESS))
    return _exact[name]


def subset(name, nbin, it, ip):
    w_all, ex = exact(name)
    w = cr.branch_wavelengths(nbin)
    at = np.searchsorted(w_all, w)
    assert np.array_equal(w_all[at], w)
    return w, ex[np.ix_(it, ip, at)]


# nbin: one thread, either side of a wavefront, more than one workgroup with a short last one
@pytest.mark.parametrize("nbin", [1, 63, 65, 257])
@pytest.mark.parametrize("name", sorted(continuum.CONTINUUM_KINDS))
def test_kernel_against_the_restatement(ctx, name, nbin):
    """ny = 1, 7, 20 (odd rows: tiles that start off 16 bytes); 2 x 2 and 5 x 3 nodes; the whole grid in one call, one row per
    call, four rows per call (the last slab of the 15 rows is short).  A sentinel row behind the slab stays untouched."""
    for it, ip in (([0, 4], [0, 2]), (list(range(5)), list(range(3)))):
        T, P = [TEMPS[i] for i in it], [PRESS[i] for i in ip]
        w, ex = subset(name, nbin, it, ip)
        host = continuum.numpy_continuum(name, w, T, P)
        nodes = len(T) * len(P)
        for ny in (1, 7, 20):
            want_exact = np.repeat(ex.reshape(-1), ny)
            want_host = np.repeat(host.reshape(-1), ny)
            row_len = nbin * ny
            for slab in sorted({nodes, 1, 4} if nodes == 15 else {nodes, 1}):
                b = continuum.ContinuumBuilder(ctx, w, ny, T, P, slab_rows=slab, guard_rows=1)
                try:
                    got = np.empty(nodes * row_len)
                    for first in range(0, nodes, slab):
                        rows = min(slab, nodes - first)
                        b.d_out.set(np.full(b.d_out.size, SENTINEL))
                        b.run(name, first, rows)
                        buf = b.d_out.get()
                        got[first * row_len:(first + rows) * row_len] = buf[:rows * row_len]
                        assert np.all(buf[rows * row_len:] == SENTINEL), (name, nbin, ny, slab, first)
                    np.testing.assert_array_equal(b.table(name), got)          # the slab loop of the product
                finally:
                    b.close()
                what = "%s nbin %d ny %d nodes %d slab %d" % (name, nbin, ny, nodes, slab)
                assert np.all(got != SENTINEL), what
                cr.check_exact(got, want_host, want_exact, what)


def test_refusals_of_the_entry_point(ctx):
    from helios_amd._lib import HeliosHipError
    b = continuum.ContinuumBuilder(ctx, cr.branch_wavelengths(5), 3, TEMPS, PRESS)
    try:
        for first, rows in ((0, 0), (14, 2), (-1, 1), (15, 1)):
            with pytest.raises(HeliosHipError, match="hx_continuum_table"):
                b.run("He-", first, rows)
        coef = ctx.to_gpu(continuum.continuum_coefficients("H-_bf"))
        rc = b._l.hx_continuum_table(ctx.handle, 1, coef.d, coef.size, b.d_wave.d, 5, 3, b.d_temp.d, 5, b.d_press.d, 3, b.d_out.d, 0, 1)
        assert rc != 0
        coef.free()
    finally:
        b.close()


def test_the_two_backends_on_a_whole_call(tmp_path):
    """ktable.py -continuum_species "H-,He-" at 65 bins x 20 Gauss points x (5 x 3), device and numpy, entry by entry"""
    import ktable as ktable_tool
    wd = str(tmp_path)
    inter = 10 ** np.linspace(np.log10(0.1e-4), np.log10(230e-4), 66)
    with open(os.path.join(wd, "grid.dat"), "w") as f:
        f.write("".join("%.17e\n" % v for v in inter))
    argv = ["-continuum_species", "H-,He-", "-grid_format", "file", "-path_to_grid_file", os.path.join(wd, "grid.dat"),
            "-temperature_grid", "50 6000 1487.5", "-pressure_grid", "0 9 3", "-container", "npz"]
    dev = ktable_tool.main(argv + ["-directory_with_individual_files", os.path.join(wd, "dev")])
    host = ktable_tool.main(argv + ["-directory_with_individual_files", os.path.join(wd, "host"), "-backend", "numpy"])
    assert [os.path.basename(p) for p in dev] == ["H-_bf_opac_ip_kdistr.npz", "H-_ff_opac_ip_kdistr.npz", "He-_opac_ip_kdistr.npz"]
    for name, pd, ph in zip(("H-_bf", "H-_ff", "He-"), dev, host):
        d, h = np.load(pd), np.load(ph)
        for key in continuum.GRID_KEYS:
            assert d[key].tobytes() == h[key].tobytes(), key
        assert d["kpoints"].shape == (5 * 3 * 65 * 20,)
        ex = cr.continuum(name, d["center wavelengths"], d["temperatures"], d["pressures"])
        rec = cr.check_exact(d["kpoints"], h["kpoints"], np.repeat(ex.reshape(-1), 20), "tool, " + name)
        assert (rec["zeros"] > 0) == (name != "He-")


def test_the_chain_from_files_this_repository_wrote(tmp_path):
    """two synthetic HELIOS-K species through ktable.py; H- and the Rayleigh file through ktable.py with -grid_like; helios.py on
    the fly and premix.py on that directory.  The scattering cross-section of every layer, and of every node of the premixed
    table, is sum vmr sigma of the restatement to 1e-12 (the product's Rayleigh values lie within 1e-14 of it)."""
    import helios
    import ktable as ktable_tool
    import premix as premix_tool
    from test_gpu_ktable import _otf_argv
    wd = str(tmp_path)
    g = kc.load("a")
    kc.write_dir(os.path.join(wd, "hk_h2o"), g)
    kc.write_dir(os.path.join(wd, "hk_co2"), g, scale=0.25)
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nH2O %s\nCO2 %s\n" % (os.path.join(wd, "hk_h2o"), os.path.join(wd, "hk_co2")))
    opac = os.path.join(wd, "opac")
    first = ktable_tool.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-wavelength_grid", "10 30 2000",
                              "-temperature_grid", "200 800 200", "-pressure_grid", "3 7 5", "-directory_with_individual_files",
                              opac, "-container", "npz"])
    second = ktable_tool.main(["-continuum_species", "H-", "-rayleigh_species", "H2,He", "-grid_like", first[1],
                               "-directory_with_individual_files", opac, "-container", "npz"])
    assert [os.path.basename(p) for p in second] == ["H-_bf_opac_ip_kdistr.npz", "H-_ff_opac_ip_kdistr.npz",
                                                     "scat_cross_sections.npz"]
    with open(os.path.join(wd, "species.dat"), "w") as f:
        f.write("species      absorbing       scattering         mixing_ratio\n\nH2O  yes no 1e-3\nH-  yes no 1e-9\n"
                "H2   no  yes  0.85\nHe  no yes 0.15\n")
    wave = np.load(first[1])["center wavelengths"]
    nbin = len(wave)
    assert 35 <= nbin <= 50
    want = (0.85 * cr.rayleigh("H2", wave) + 0.15 * cr.rayleigh("He", wave)).astype(np.float64)
    run = helios.run_helios(_otf_argv(wd) + ["-opacity_mixing", "on-the-fly", "-name", "chain", "-output_directory", wd + "/",
                                            "-energy_budget_correction", "no", "-internal_temperature", "100",
                                            "-number_of_layers", "15", "-maximum_number_of_iterations", "20000",
                                            "-radiative_equilibrium_criterion", "1e-4", "-convective_adjustment", "no",
                                            "-toa_pressure", "1e3", "-boa_pressure", "1e7"])
    print("iterations %d, T %.1f ... %.1f" % (run.iter_value, run.T_lay.min(), run.T_lay.max()))
    assert int(run.nbin) == nbin and int(run.ny) == 20 and int(run.nlayer) == 15
    assert 3 < int(run.iter_value) < 20000 and np.all(np.isfinite(run.T_lay))
    assert [sp.name for sp in run.species_list] == ["H2O", "H-_bf", "H-_ff", "H2", "He"]
    scat = np.asarray(run.scat_cross_lay, np.float64).reshape(15, nbin)
    np.testing.assert_allclose(scat, np.tile(want, (15, 1)), rtol=1e-12, atol=0)
    table = os.path.join(wd, "mix.npz")
    assert premix_tool.main(_otf_argv(wd) + ["-premix_output", table]) == [table]
    t = np.load(table)
    assert t["kpoints"].shape == (4 * 5 * nbin * 20,) and np.all(t["kpoints"] > 0)
    np.testing.assert_allclose(t["weighted Rayleigh cross-sections"].reshape(20, nbin), np.tile(want, (20, 1)), rtol=1e-12, atol=0)
