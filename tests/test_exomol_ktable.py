"""exomol.py -ktable yes with the numpy backend: the containers are, data set by data set and as raw bytes, the ones exomol.py
(files) followed by ktable.py writes; every refusal with its reason; and the empty-bin rule stands before the first node."""
import os

import numpy as np
import pytest

import exomol_cases as ec
from helios_amd import exomol, ktable

GRID = ["-wavelength_grid", "20 6 40", "-number_of_gaussian_points", "8", "-container", "npz"]


def tool_case():
    """300 transitions over 150 ... 1950 cm^-1, two broadeners; about half of them culled at 300 K and fewer at 900 K"""
    return ec.build("ktable", ec.pattern("alternating", 300), grid=(150.0, 0.05, 36000), cutoff=25.0, seed=21, n_broadeners=2,
                    nodes=[(300.0, 1e3), (900.0, 1e6)], s_min=1e-40)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("exomol_ktable"))
    st, tr, entries, pf = ec.write_files(wd, tool_case())
    return {"wd": wd, "files": ["-states", st, "-trans", tr, "-partition_function", pf, "-broadeners", " ".join(entries)]}


def _argv(inputs, *more):
    return ["-name", "H2O"] + inputs["files"] + ["-temperatures", "900 300", "-pressure_codes", "p000 n300", "-numax", "2000", "-dnu",
                                                 "0.05", "-strength_cutoff", "1e-40", "-backend", "numpy"] + list(more)


@pytest.fixture(scope="module")
def two_step(inputs):
    """{interpolate: paths} of exomol.py (files) followed by ktable.py, computed once"""
    wd = inputs["wd"]
    out = os.path.join(wd, "opac", "H2O")
    written = exomol.main(_argv(inputs, "-output_directory", out))
    assert [os.path.basename(w) for w in written] == ["Out_H2O_00000_02000_00900_p000.bin", "Out_H2O_00000_02000_00900_n300.bin",
                                                      "Out_H2O_00000_02000_00300_p000.bin", "Out_H2O_00000_02000_00300_n300.bin"]
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nH2O %s\n" % out)
    paths = {}
    for interpolate in ("yes", "no"):
        paths[interpolate] = ktable.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-backend", "numpy",
                                          "-directory_with_individual_files", os.path.join(wd, "two_step_" + interpolate),
                                          "-interpolate", interpolate] + GRID)
    return paths


def same_containers(got, want):
    assert [os.path.basename(p) for p in got] == [os.path.basename(p) for p in want]
    for g, w in zip(got, want):
        with np.load(g) as a, np.load(w) as b:
            assert sorted(a.files) == sorted(b.files)
            for k in b.files:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (g, k)
                assert a[k].tobytes() == b[k].tobytes(), (os.path.basename(g), k)


def test_the_containers_are_the_two_step_routes_to_the_byte(inputs, two_step, capsys):
    got = exomol.main(_argv(inputs, "-ktable", "yes", "-directory_with_individual_files", os.path.join(inputs["wd"], "fused_yes")) + GRID)
    assert [os.path.basename(p) for p in got] == ["H2O_opac_kdistr.npz", "H2O_opac_ip_kdistr.npz"]
    same_containers(got, two_step["yes"])
    text = capsys.readouterr().out
    kept = [int(line.split(": ")[2].split()[0]) for line in text.splitlines() if "transitions kept" in line]
    assert len(kept) == 4 and kept[0] == kept[1] < kept[2] == kept[3] <= 300 and "300 K, n300" in text     # nodes ascending: T, then P
    with np.load(got[0]) as t:
        assert t["temperatures"].tolist() == [300.0, 900.0] and t["pressures"].tolist() == [1e3, 1e6]
        k = t["kpoints"].reshape(4, -1, 8)
        assert np.all(np.isfinite(k)) and k.max() > 1e3 * k.min()


def test_without_interpolation_only_the_native_container_is_written(inputs, two_step):
    out = os.path.join(inputs["wd"], "fused_no")
    got = exomol.main(_argv(inputs, "-ktable", "yes", "-interpolate", "no", "-directory_with_individual_files", out) + GRID)
    assert os.listdir(out) == ["H2O_opac_kdistr.npz"]
    same_containers(got, two_step["no"])


def test_the_library_function_returns_build_species_data_sets(inputs, two_step):
    case = tool_case()
    inter = ktable.wavelength_grid("fixed_resolution", "20 6 40".split())
    timing = {}
    native, ip = exomol.exomol_ktable(case.states, case.trans, case.broadening, ec.q_table(), [900, 300, 900], ["p000", "n300"], 2000,
                                      0.05, inter, 8, ec.M_H2O, 25.0, 1e-40, backend="numpy", timing=timing)
    assert ip is None and timing["points"] == 4 and len(timing["kept"]) == 4 and timing["resolution"] == 2000 / 40000
    with np.load(two_step["no"][0]) as want:
        assert sorted(native) == sorted(want.files)
        for k in want.files:
            assert np.asarray(native[k]).tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("more,reason", [
    (["-numin", "100"], r"-ktable yes with -numin 100: the k-table's wavelength axis starts at 0 cm\^-1"),
    (["-chunk_width", "500"], r"-ktable yes with -chunk_width 500: the table is built from the one chunk 0 \.\.\. numax"),
    (["-output_format", "text"], r"-ktable yes with -output_format text: no opacity file is written"),
    (["-output_directory", "somewhere"], r"-ktable yes with -output_directory somewhere: a call writes the files or the table"),
])
def test_refusals_with_their_reasons(inputs, more, reason, monkeypatch):
    monkeypatch.setattr(exomol, "numpy_node", lambda *a, **k: pytest.fail("a node was computed"))
    with pytest.raises(IOError, match=reason):
        exomol.main(_argv(inputs, "-ktable", "yes", "-directory_with_individual_files", os.path.join(inputs["wd"], "refused")) + GRID + more)
    assert not os.path.exists(os.path.join(inputs["wd"], "refused"))


def test_without_ktable_the_output_directory_is_required(inputs, capsys):
    with pytest.raises(SystemExit):
        exomol.main(_argv(inputs))
    assert "the following arguments are required: -output_directory" in capsys.readouterr().err


def test_an_empty_interior_bin_is_refused_before_a_node_is_computed(inputs, monkeypatch):
    """at 0.05 cm^-1 the points next to 5 micron (2000 cm^-1) lie 1.25e-8 cm apart: a bin of 1e-9 cm between them holds none"""
    calls = []
    real = exomol.numpy_node
    monkeypatch.setattr(exomol, "numpy_node", lambda *a, **k: calls.append(1) or real(*a, **k))
    lam = ktable.spectral_axis(0, 2000, 2000 / 40000)
    mid = 0.5 * (lam[10] + lam[11])
    grid = os.path.join(inputs["wd"], "grid.txt")
    with open(grid, "w") as f:
        for v in (lam[2] * 1.0000001, mid - 5e-10, mid + 5e-10, lam[30] * 1.0000001):
            f.write("%.17g\n" % v)
    out = os.path.join(inputs["wd"], "empty_bin")
    with pytest.raises(IndexError, match="k-distribution construction failed: the original wavelength grid must be finer .*bin 1"):
        exomol.main(_argv(inputs, "-ktable", "yes", "-grid_format", "file", "-path_to_grid_file", grid, "-container", "npz",
                          "-number_of_gaussian_points", "8", "-directory_with_individual_files", out))
    assert calls == [] and not os.path.exists(out)
