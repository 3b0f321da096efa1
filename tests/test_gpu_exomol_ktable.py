"""exomol.py -ktable yes on the device: the containers equal, as raw bytes, the ones exomol.py followed by ktable.py writes on the
device, and the device's files equal the numpy backend's under fp32 rounding of rows held to the rule; and one chain from synthetic
ExoMol files through `_opac_ip_kdistr` into an on-the-fly helios.py run that converges."""
import os

import numpy as np
import pytest

import exomol_cases as ec

pytestmark = pytest.mark.gpu


def test_the_fused_containers_equal_the_two_step_routes_on_the_device(tmp_path, capsys):
    """`exomol.py` then `ktable.py` against `exomol.py -ktable yes`, all on the device, four nodes in launches of 3 and 1"""
    import exomol as exomol_tool
    import ktable as ktable_tool
    from test_exomol_ktable import tool_case
    wd = str(tmp_path)
    st, tr, entries, pf = ec.write_files(wd, tool_case())
    argv = ["-name", "H2O", "-states", st, "-trans", tr, "-partition_function", pf, "-broadeners", " ".join(entries), "-temperatures",
            "900 300", "-pressure_codes", "p000 n300", "-numax", "2000", "-dnu", "0.05", "-strength_cutoff", "1e-40",
            "-nodes_per_launch", "3"]
    grid = ["-wavelength_grid", "20 6 40", "-number_of_gaussian_points", "8", "-container", "npz", "-temperature_grid", "200 1000 400",
            "-pressure_grid", "2 6 3"]
    files = exomol_tool.main(argv + ["-output_directory", os.path.join(wd, "opac", "H2O")])
    assert len(files) == 4 and all(os.path.getsize(f) == 4 * 40000 for f in files)
    text = capsys.readouterr().out
    assert "900 K, p000: 300 of 300 transitions kept" in text and "300 K, n300: 150 of 300 transitions kept" in text
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nH2O %s\n" % os.path.join(wd, "opac", "H2O"))
    want = ktable_tool.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-directory_with_individual_files",
                             os.path.join(wd, "two_step")] + grid)
    got = exomol_tool.main(argv + ["-ktable", "yes", "-directory_with_individual_files", os.path.join(wd, "fused")] + grid)
    assert [os.path.basename(p) for p in got] == ["H2O_opac_kdistr.npz", "H2O_opac_ip_kdistr.npz"]
    assert [os.path.basename(p) for p in want] == [os.path.basename(p) for p in got]
    for g, w in zip(got, want):
        with np.load(g) as a, np.load(w) as b:
            assert sorted(a.files) == sorted(b.files)
            for k in b.files:
                assert a[k].tobytes() == b[k].tobytes(), (os.path.basename(g), k)
            assert np.all(np.isfinite(a["kpoints"])) and a["kpoints"].max() > 1e3 * a["kpoints"].min()
    text = capsys.readouterr().out
    assert [int(line.split(": ")[2].split()[0]) for line in text.splitlines() if "transitions kept" in line] == [150, 150, 300, 300]
    host = exomol_tool.main(argv + ["-backend", "numpy", "-output_directory", os.path.join(wd, "opac_numpy")])
    for d, h in zip(files, host):                      # both backends lie under the rule: their fp32 roundings differ by an ulp at most
        a, b = np.fromfile(d, "<f4"), np.fromfile(h, "<f4")
        assert np.array_equal(a == 0, b == 0) and np.all(np.abs(a.view(np.int32) - b.view(np.int32)) <= 1), os.path.basename(d)


def test_the_chain_from_exomol_files_to_a_converged_run(tmp_path):
    """H2O from synthetic `.states`, `.trans` and `.broad` files through `exomol.py -ktable yes` with a strength cut, Rayleigh H2
    and He with -grid_like, and helios.py on the fly with twelve layers.  A is drawn from 1e-7 ... 1e-3 s^-1, which puts the
    opacities where the other chains of this suite have theirs (up to 100 cm^2 g^-1)"""
    import exomol as exomol_tool
    import helios
    import ktable as ktable_tool
    from test_gpu_ktable import _otf_argv
    wd = str(tmp_path)
    case = ec.build("chain", ec.pattern("alternating", 400), grid=(20.0, 0.1, 3300), cutoff=10.0, seed=33, n_broadeners=2,
                    nodes=[(200.0, 1e3), (500.0, 1e5), (800.0, 1e7)], s_min=1e-45, log_a=(-7.0, -3.0))
    st, tr, entries, pf = ec.write_files(wd, case)
    opac = os.path.join(wd, "opac")
    grids = ["-wavelength_grid", "10 30 2000", "-temperature_grid", "200 800 200", "-pressure_grid", "3 7 5",
             "-directory_with_individual_files", opac, "-container", "npz"]
    written = exomol_tool.main(["-name", "H2O", "-states", st, "-trans", tr, "-partition_function", pf, "-broadeners", " ".join(entries),
                                "-temperatures", "200 500 800", "-pressure_codes", "n300 p100", "-numax", "400", "-dnu", "0.1",
                                "-cutoff", "10", "-strength_cutoff", "1e-45", "-ktable", "yes"] + grids)
    assert [os.path.basename(p) for p in written] == ["H2O_opac_kdistr.npz", "H2O_opac_ip_kdistr.npz"]
    with np.load(written[1]) as t:
        assert t["temperatures"].tolist() == [200.0, 400.0, 600.0, 800.0] and len(t["pressures"]) == 5
        assert np.all(np.isfinite(t["kpoints"])) and 1.0 < t["kpoints"].max() < 1e3
    ktable_tool.main(["-rayleigh_species", "H2,He", "-grid_like", written[1], "-directory_with_individual_files", opac, "-container",
                      "npz"])
    with open(os.path.join(wd, "species.dat"), "w") as f:
        f.write("species      absorbing       scattering         mixing_ratio\n\nH2O  yes no 1e-3\nH2   no  yes  0.85\nHe  no yes 0.15\n")
    run = helios.run_helios(
        _otf_argv(wd) + ["-opacity_mixing", "on-the-fly", "-name", "exomol", "-output_directory", wd + "/",
                         "-energy_budget_correction", "no", "-internal_temperature", "100", "-number_of_layers", "12",
                         "-maximum_number_of_iterations", "20000", "-radiative_equilibrium_criterion", "1e-4",
                         "-convective_adjustment", "no", "-toa_pressure", "1e3", "-boa_pressure", "1e7"])
    print("iterations %d, T %.1f ... %.1f" % (run.iter_value, run.T_lay.min(), run.T_lay.max()))
    assert int(run.nlayer) == 12 and int(run.ny) == 20
    assert [sp.name for sp in run.species_list] == ["H2O", "H2", "He"]
    assert 3 < int(run.iter_value) < 20000 and np.all(np.isfinite(run.T_lay))
