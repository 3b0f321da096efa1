"""k_ktable_bins and k_ktable_regrid (csrc/ktable.hip) against what the reference's k-table tool made of the same HELIOS-K
files (tests/golden/ktable) and against the numpy backend; batching and the two sort paths; the tool end to end into
helios.py and premix.py.  Nothing here reads the reference tree."""
import json
import os

import numpy as np
import pytest

import ktable_cases as kc
from helios_amd import ktable
from helios_amd._tool import dp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


@pytest.mark.parametrize("case,suffix,n_gauss,text", kc.CASES)
def test_device_against_the_reference_and_numpy(ctx, case, suffix, n_gauss, text, tmp_path):
    """every entry of every table at max(1e-13, 8 eps_ref) in log10 k against the reference -- over the bins the reference
    computed in double at that bound with the scan's own eps_ref -- and against the numpy backend at 1e-13 + 8 x that scan
    noise (both scan in double, in different orders).  The figures are added to the JSON file that the
    environment variable KTABLE_PARITY_JSON names, if it is set (profiles/ktable_parity.json was written that way)."""
    g = kc.load(case)
    d = kc.write_dir(os.path.join(str(tmp_path), "hk"), g, text=text)
    fmt = "text" if text else "binary"
    native, _ = ktable.build_species(d, kc.interfaces(g), n_gauss, fmt, backend="hip", ctx=ctx)
    host, _ = ktable.build_species(d, kc.interfaces(g), n_gauss, fmt, backend="numpy")
    record = {}
    dev_np = float(np.abs(np.log10(native["kpoints"]) - np.log10(host["kpoints"])).max())
    print("device against numpy, %s%s: %.3e" % (case, suffix, dev_np))
    try:
        kc.check(g, suffix, native["kpoints"], "device " + case, record)
    finally:
        path = os.environ.get("KTABLE_PARITY_JSON")
        if path and record:
            have = json.load(open(path)) if os.path.exists(path) else {}
            for k in record:
                record[k]["deviation_from_numpy_backend"] = dev_np
            have.update(record)
            json.dump(have, open(path, "w"), indent=1, sort_keys=True)
    scan = float(g["eps_ref_floored_bins" + suffix]) if "eps_ref_floored_bins" + suffix in g.files else float(g["eps_ref" + suffix])
    assert dev_np <= 1e-13 + 8 * scan


def test_regridding_on_the_device(ctx):
    g = kc.load("a")
    nx = len(g["center wavelengths"])
    b = ktable.KTableBuilder(ctx, 2000, nx, 20, 4)
    try:
        ctx.check(b._l.hx_ktable_put(b.handle, dp(np.ascontiguousarray(g["kpoints"], np.float64))), "hx_ktable_put")
        b.regrid(g["temperatures"], g["pressures"], g["regrid_temperatures"], g["regrid_pressures"])
        got = b.get("kpoints_ip")
        np.testing.assert_array_equal(b.get("kpoints"), g["kpoints"])
    finally:
        b.close()
    dev = np.abs(np.log10(got) - np.log10(g["regrid_kpoints"])).max()
    tol = max(1e-13, 8 * float(g["eps_ref_regrid"]))
    print("regrid on the device: deviation %.3e, bound %.3e" % (dev, tol))
    assert dev <= tol
    host = ktable.numpy_regrid(g["pressures"], g["temperatures"], g["kpoints"], g["regrid_temperatures"], g["regrid_pressures"],
                               nx, 20)
    assert np.abs(np.log10(got) - np.log10(host)).max() <= 1e-13


def test_batching_is_invisible(ctx, tmp_path):
    g = kc.load("a")
    d = kc.write_dir(os.path.join(str(tmp_path), "hk"), g)
    one, _ = ktable.build_species(d, kc.interfaces(g), 20, backend="hip", ctx=ctx, tp_per_launch=1)
    four, _ = ktable.build_species(d, kc.interfaces(g), 20, backend="hip", ctx=ctx, tp_per_launch=4)
    np.testing.assert_array_equal(one["kpoints"], four["kpoints"])


@pytest.mark.parametrize("case,small", [("a", 16), ("c", 1024), ("c", 8192)])
def test_the_two_sort_paths_agree(ctx, case, small, tmp_path):
    """bins that fit the LDS sort, sorted there and -- with a lower threshold -- through the scratch: identical bits"""
    g = kc.load(case)
    d = kc.write_dir(os.path.join(str(tmp_path), "hk"), g)
    lds, _ = ktable.build_species(d, kc.interfaces(g), 20, backend="hip", ctx=ctx)
    scratch, _ = ktable.build_species(d, kc.interfaces(g), 20, backend="hip", ctx=ctx, lds_points=small)
    np.testing.assert_array_equal(lds["kpoints"], scratch["kpoints"])


def _tool_on_two_species(wd, extra=()):
    import ktable as ktable_tool
    g = kc.load("a")
    kc.write_dir(os.path.join(wd, "hk_h2o"), g)
    kc.write_dir(os.path.join(wd, "hk_co2"), g, scale=0.25)
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nH2O %s\nCO2 %s\n" % (os.path.join(wd, "hk_h2o"), os.path.join(wd, "hk_co2")))
    written = ktable_tool.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-wavelength_grid",
                                "20 30 2000", "-directory_with_individual_files", os.path.join(wd, "opac"), "-container", "npz"]
                               + list(extra))
    nbin = len(g["center wavelengths"])
    rng = np.random.default_rng(4)
    np.savez(os.path.join(wd, "opac", "scat_cross_sections.npz"), rayleigh_H2=10.0 ** rng.uniform(-28, -24, nbin),
             rayleigh_He=10.0 ** rng.uniform(-29, -25, nbin))
    with open(os.path.join(wd, "species.dat"), "w") as f:
        f.write("species      absorbing       scattering         mixing_ratio\n\nH2O  yes no 1e-3\nCO2  yes no  3e-4\n"
                "H2   no  yes  0.85\nHe  no yes 0.15\n")
    return written, g


def _otf_argv(wd):
    return ["-parameter_file", "/nonexistent", "-path_to_species_file", os.path.join(wd, "species.dat"),
            "-directory_with_fastchem_files", os.path.join(wd, "chem") + "/",
            "-directory_with_opacity_files", os.path.join(wd, "opac") + "/"]


def test_from_helios_k_files_to_a_converged_run(tmp_path):
    """ktable.py on case a for two species, then helios.py on the fly on the written `_ip_` containers (the reference's
    hard-coded 120 x 28 grid): it reads them and converges.  Case a's bins lie between 30 and 2000 micron, where a 5000 K star
    has next to none of its flux: the energy-budget correction, which rescales the star to the flux the bins miss, is off, and
    the column is heated from below (100 K), so that its emission falls into the bins"""
    import helios
    from test_gpu_premix import RUN
    wd = str(tmp_path)
    written, g = _tool_on_two_species(wd)
    assert [os.path.basename(w) for w in written] == ["H2O_opac_kdistr.npz", "H2O_opac_ip_kdistr.npz", "CO2_opac_kdistr.npz",
                                                      "CO2_opac_ip_kdistr.npz"]
    kc.check(g, "", np.load(written[0])["kpoints"], "tool")
    ip = np.load(written[1])
    assert ip["temperatures"].shape == (120,) and ip["pressures"].shape == (28,)
    run = helios.run_helios(_otf_argv(wd) + ["-opacity_mixing", "on-the-fly", "-name", "kt", "-output_directory", wd + "/",
                                            "-energy_budget_correction", "no", "-internal_temperature", "100"] + RUN)
    print("iterations %d, T %.1f ... %.1f" % (run.iter_value, run.T_lay.min(), run.T_lay.max()))
    assert int(run.nbin) == len(g["center wavelengths"]) and int(run.ny) == 20
    assert 3 < int(run.iter_value) < 20000 and np.all(np.isfinite(run.T_lay))


def test_the_same_set_through_premix(tmp_path):
    """premix.py takes nodes uniform in T and log10 P, so the tool writes its `_ip_` containers on such a grid here"""
    import premix as premix_tool
    wd = str(tmp_path)
    _tool_on_two_species(wd, ["-temperature_grid", "200 800 200", "-pressure_grid", "4 7 4"])
    table = os.path.join(wd, "mix.npz")
    assert premix_tool.main(_otf_argv(wd) + ["-premix_output", table]) == [table]
    t = np.load(table)
    assert t["kpoints"].shape == (4 * 4 * len(t["center wavelengths"]) * 20,) and np.all(t["kpoints"] > 0)
