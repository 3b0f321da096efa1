"""lines.py with the numpy backend: the contract against the restatements of tests/lines_reference.py under the rule of
tests/lines_cases.py, every refusal with its message, and the files the tool writes as ktable.py reads them."""
import os

import numpy as np
import pytest

import lines_cases as lc
import lines_reference as lr
from helios_amd import ktable, lines

NODES = [(300.0, 1e3), (900.0, 1e6), (1500.0, 1e8)]         # K, dyne cm^-2: y from the clamp's neighbourhood to far beyond |z| = 100
GRID = (100.0, 0.05, 1000)                                   # 100 ... 150 cm^-1
CUTOFF = 5.0


@pytest.fixture(scope="module")
def some_lines():
    return lc.join(lc.synthetic_lines(40, 92.0, 158.0, seed=7), lc.one_line(120.0, s_ref=3e-20))


@pytest.mark.parametrize("temp,press", NODES)
def test_numpy_backend_against_the_restatement(some_lines, temp, press):
    kappa = lines.line_opacity(some_lines, lc.q_table(), [temp], [press], GRID, lc.M_H2O, 0.25, CUTOFF, backend="numpy")
    assert kappa.shape == (1, 1, GRID[2]) and kappa.dtype == np.float64
    ld, f64 = lc.restated(some_lines, temp, press, 0.25, CUTOFF, *GRID)
    lc.check_rule(kappa, ld, f64, "numpy backend at %g K, %g dyne cm^-2" % (temp, press))
    assert np.count_nonzero(kappa) > 900


@pytest.mark.parametrize("temp,press", NODES)
def test_line_params_against_the_restatement(some_lines, temp, press):
    q = lc.q_table()
    got = lines.line_params(some_lines, temp, press, lines.partition_value(q, temp), lines.partition_value(q, 296.0), lc.M_H2O, 0.25)
    ld, f64 = lc.restated_params(some_lines, temp, press, 0.25)
    lc.check_rule(got, ld, f64, "line_params at %g K, %g dyne cm^-2" % (temp, press))


def test_several_nodes_in_one_call_and_the_pair_count(some_lines):
    timing = {}
    kappa = lines.line_opacity(some_lines, lc.q_table(), [300.0, 900.0], [1e3, 1e6], GRID, lc.M_H2O, 0.25, CUTOFF, backend="numpy",
                               timing=timing)
    assert kappa.shape == (2, 2, GRID[2])
    one = lines.line_opacity(some_lines, lc.q_table(), [900.0], [1e6], GRID, lc.M_H2O, 0.25, CUTOFF, backend="numpy")
    assert np.array_equal(kappa[1, 1], one[0, 0])
    q = lc.q_table()
    pairs = sum(lines.count_pairs(lines.line_params(some_lines, t, p, lines.partition_value(q, t), lines.partition_value(q, 296.0),
                                                    lc.M_H2O, 0.25)[0], GRID[0], GRID[1], GRID[2], CUTOFF)
                for t in (300.0, 900.0) for p in (1e3, 1e6))
    assert timing["pairs"] == pairs == int(timing["pairs_by_region"].sum()) and pairs > 4 * 20 * 200


def test_the_partition_function_is_interpolated_linearly():
    t, q = lc.q_table()
    assert lines.partition_value((t, q), 300.0) == q[5] and lines.partition_value((t, q), 3000.0) == q[-1]
    assert lines.partition_value((t, q), 296.0) == q[4] + (q[5] - q[4]) * ((296.0 - 250.0) / 50.0)
    with pytest.raises(ValueError, match=r"T = 3001 K lies outside the partition function's 50 \.\.\. 3000 K"):
        lines.partition_value((t, q), 3001.0)


# ---- the tool ----------------------------------------------------------------------------------------------------------
def _inputs(wd, n=30, isotopologues=None, table=None):
    line = lc.synthetic_lines(n, 5.0, 95.0, seed=9)
    lc.write_par_file(os.path.join(wd, "list.par"), line, isotopologues)
    lc.write_q_file(os.path.join(wd, "q.txt"), table)
    return line


def _argv(wd, **over):
    opt = {"name": "H2O", "line_list": os.path.join(wd, "list.par"), "partition_function": os.path.join(wd, "q.txt"),
           "temperatures": "300 900", "pressure_codes": "n300 p000", "numin": "0", "numax": "100", "dnu": "0.25",
           "output_directory": os.path.join(wd, "out"), "backend": "numpy", "cutoff": "5"}
    opt.update(over)
    argv = []
    for k, v in opt.items():
        if v is not None:
            argv += ["-" + k, str(v)]
    return argv


def test_file_names_sizes_content_and_what_ktable_reads(tmp_path, capsys):
    wd = str(tmp_path)
    _inputs(wd)
    written = lines.main(_argv(wd, chunk_width=50))
    names = sorted(os.path.basename(w) for w in written)
    assert names == sorted("Out_H2O_%05d_%05d_%05d_%s.bin" % (lo, lo + 50, t, c) for lo in (0, 50) for t in (300, 900)
                           for c in ("n300", "p000"))
    assert sorted(os.listdir(os.path.join(wd, "out"))) == names
    assert all(os.path.getsize(w) == 4 * 200 for w in written)
    parsed, _ = lines.read_line_list(os.path.join(wd, "list.par"))
    table = ktable.pressure_table()
    for lo in (0, 50):
        kappa = lines.line_opacity(parsed, lc.q_table(), [300, 900], [table["n300"], table["p000"]], (float(lo), 0.25, 200),
                                   18.0153, 0.0, 5.0, backend="numpy")
        for it, t in enumerate((300, 900)):
            for ip, c in enumerate(("n300", "p000")):
                got = np.fromfile(os.path.join(wd, "out", "Out_H2O_%05d_%05d_%05d_%s.bin" % (lo, lo + 50, t, c)), "<f4")
                assert np.array_equal(got.view(np.uint32), kappa[it, ip].astype(np.float32).view(np.uint32))
                assert np.count_nonzero(got) > 100
    files = ktable.SpeciesFiles(os.path.join(wd, "out"))
    assert files.file_name == "H2O" and files.numin == [0, 50] and files.numax == [50, 100] and files.temps == [300, 900]
    assert files.codes == ["n300", "p000"] and files.resolution() == 0.25
    assert len(ktable.spectral_axis(files.numin[0], files.numax[-1], files.resolution())) == 400
    assert len(files.read_point(900, "p000", 0.25)) == 400
    out = capsys.readouterr().out
    assert "30 lines of isotopologue 1" in out and "0 lines of other isotopologues skipped" in out and "will refuse" not in out


def test_text_output_is_what_read_text_file_takes(tmp_path):
    wd = str(tmp_path)
    _inputs(wd)
    binary = lines.main(_argv(wd, temperatures="300", pressure_codes="p000"))
    text = lines.main(_argv(wd, temperatures="300", pressure_codes="p000", output_format="text",
                            output_directory=os.path.join(wd, "text")))
    assert [os.path.basename(t) for t in text] == ["Out_H2O_00000_00100_00300_p000.dat"]
    got = ktable.read_text_file(text[0])
    assert np.array_equal(got.view(np.uint32), np.fromfile(binary[0], "<f4").view(np.uint32))
    rows = np.loadtxt(text[0])
    assert rows.shape == (400, 2) and np.array_equal(rows[:, 0], np.arange(400) * 0.25)


def test_a_skipped_isotopologue_is_counted_and_printed(tmp_path, capsys):
    wd = str(tmp_path)
    iso = [1, 2, 1, 3, 1] * 6
    line = _inputs(wd, isotopologues=iso)
    parsed, skipped = lines.read_line_list(os.path.join(wd, "list.par"))
    assert skipped == 12 and len(parsed["nu0"]) == 18
    assert np.array_equal(parsed["nu0"], np.array([float("%.6f" % v) for v in line["nu0"][np.array(iso) == 1]]))
    second, skipped = lines.read_line_list(os.path.join(wd, "list.par"), isotopologue=2)
    assert skipped == 24 and len(second["nu0"]) == 6
    lines.main(_argv(wd, temperatures="300", pressure_codes="p000"))
    assert "18 lines of isotopologue 1" in capsys.readouterr().out
    lines.main(_argv(wd, temperatures="300", pressure_codes="p000", isotopologue=2, output_directory=os.path.join(wd, "iso2")))
    out = capsys.readouterr().out
    assert "6 lines of isotopologue 2" in out and "24 lines of other isotopologues skipped" in out


def test_numin_other_than_zero_is_allowed_and_announced(tmp_path, capsys):
    wd = str(tmp_path)
    _inputs(wd)
    written = lines.main(_argv(wd, numin=50, temperatures="300", pressure_codes="p000"))
    assert [os.path.basename(w) for w in written] == ["Out_H2O_00050_00100_00300_p000.bin"]
    assert "-numin 50 is not 0: ktable.py will refuse the directory" in capsys.readouterr().out
    with pytest.raises(IOError, match="the first chunk starts at 50"):
        ktable.SpeciesFiles(os.path.join(wd, "out"))


def test_lines_are_sorted_by_nu0_then_position(tmp_path):
    wd = str(tmp_path)
    line = lc.join(lc.one_line(50.0, s_ref=1e-21), lc.one_line(20.0, s_ref=2e-21), lc.one_line(50.0, s_ref=3e-21),
                   lc.one_line(20.0, s_ref=4e-21))
    shuffled = dict((k, line[k][[2, 0, 3, 1]]) for k in lr.FIELDS)          # 50 (1e-21), 20 (2e-21), 50 (3e-21), 20 (4e-21)
    lc.write_par_file(os.path.join(wd, "list.par"), shuffled)
    parsed, _ = lines.read_line_list(os.path.join(wd, "list.par"))
    assert parsed["nu0"].tolist() == [20.0, 20.0, 50.0, 50.0] and parsed["s_ref"].tolist() == [2e-21, 4e-21, 1e-21, 3e-21]


# ---- refusals ----------------------------------------------------------------------------------------------------------
def _edit(path, row, lo, hi, text):
    rows = open(path).read().split("\n")
    rows[row] = rows[row][:lo] + text.rjust(hi - lo) + rows[row][hi:]
    open(path, "w").write("\n".join(rows))


@pytest.mark.parametrize("edit,message", [
    ((3, 0, 160, "x" * 60), r"line 4 of .*list\.par .* holds 60 characters, a record needs 67"),
    ((2, 15, 25, "1.0e-2x"), r"line 3 of .*s_ref = '   1.0e-2x' \(columns 15:25\) is not a finite number"),
    ((2, 45, 55, "nan"), r"line 3 of .*e_low = '       nan' \(columns 45:55\) is not a finite number"),
    ((2, 35, 40, "inf"), r"line 3 of .*gamma_air = '  inf' \(columns 35:40\) is not a finite number"),
    ((0, 3, 15, "0.0"), r"line 1 of .*nu_0 = 0\.0 is not > 0"),
    ((0, 3, 15, "-5.0"), r"line 1 of .*nu_0 = -5\.0 is not > 0"),
    ((1, 15, 25, "-1.0e-22"), r"line 2 of .*S_ref = -1e-22 is negative"),
])
def test_a_bad_record_is_refused_with_its_line(tmp_path, edit, message):
    wd = str(tmp_path)
    _inputs(wd)
    row, lo, hi, text = edit
    if hi - lo == 160:
        rows = open(os.path.join(wd, "list.par")).read().split("\n")
        rows[row] = rows[row][:60]
        open(os.path.join(wd, "list.par"), "w").write("\n".join(rows))
    else:
        _edit(os.path.join(wd, "list.par"), row, lo, hi, text)
    with pytest.raises(IOError, match=message):
        lines.main(_argv(wd))
    assert not os.path.exists(os.path.join(wd, "out")) or not os.listdir(os.path.join(wd, "out"))


@pytest.mark.parametrize("over,message", [
    ({"temperatures": "300 0"}, r"the temperature '0' is not > 0 K"),
    ({"temperatures": "300 -40"}, r"the temperature '-40' is not > 0 K"),
    ({"temperatures": "300.5"}, r"the temperature '300\.5' is not an integer in K"),
    ({"temperatures": "300 4000"}, r"T = 4000 K lies outside the partition function's 50 \.\.\. 3000 K"),
    ({"temperatures": "40"}, r"T = 40 K lies outside the partition function's 50 \.\.\. 3000 K"),
    ({"pressure_codes": "n300 p450"}, r"pressure code 'p450' is not in the table"),
    ({"dnu": "0"}, r"-dnu 0\.0 is not > 0"),
    ({"dnu": "-0.25"}, r"-dnu -0\.25 is not > 0"),
    ({"dnu": "0.3"}, r"dnu = 0\.2999\d* does not divide the chunk 0 \.\.\. 100 cm\^-1 into a whole number of points"),
    ({"dnu": "0.4", "chunk_width": "25"}, r"dnu = 0\.40\d* does not divide the chunk 0 \.\.\. 25 cm\^-1 into a whole number of points"),
    ({"numax": "0"}, r"-numax 0 is not above -numin 0"),
    ({"numin": "100"}, r"-numax 100 is not above -numin 100"),
    ({"name": "XYZ"}, r"no molar mass: 'XYZ' is not in species_data\.py, give -molar_mass"),
    ({"molar_mass": "0"}, r"no molar mass: -molar_mass 0\.0 is not > 0"),
    ({"self_fraction": "1.5"}, r"-self_fraction 1\.5 lies outside \[0, 1\]"),
    ({"self_fraction": "-0.1"}, r"-self_fraction -0\.1 lies outside \[0, 1\]"),
    ({"isotopologue": "4"}, r"holds no line of isotopologue 4 \(30 of other isotopologues\)"),
])
def test_a_bad_option_is_refused_with_its_value(tmp_path, over, message):
    wd = str(tmp_path)
    _inputs(wd)
    with pytest.raises(IOError, match=message):
        lines.main(_argv(wd, **over))
    assert not os.path.exists(os.path.join(wd, "out")) or not os.listdir(os.path.join(wd, "out"))


def test_a_partition_file_without_296_k_or_out_of_order_is_refused(tmp_path):
    wd = str(tmp_path)
    _inputs(wd, table=(np.array([300.0, 400.0, 1000.0]), np.array([1.0, 2.0, 3.0])))
    with pytest.raises(IOError, match=r"T = 296 K lies outside the partition function's 300 \.\.\. 1000 K"):
        lines.main(_argv(wd, temperatures="400"))
    lc.write_q_file(os.path.join(wd, "q.txt"), (np.array([100.0, 400.0, 400.0]), np.array([1.0, 2.0, 3.0])))
    with pytest.raises(IOError, match=r"line 4 of .*q\.txt .*: the temperatures strictly ascend"):
        lines.main(_argv(wd, temperatures="400"))


def test_a_given_molar_mass_scales_kappa(tmp_path):
    wd = str(tmp_path)
    _inputs(wd)
    a = lines.main(_argv(wd, temperatures="300", pressure_codes="p000"))
    b = lines.main(_argv(wd, temperatures="300", pressure_codes="p000", name="XYZ", molar_mass=18.0153))
    assert os.path.basename(b[0]) == "Out_XYZ_00000_00100_00300_p000.bin"
    assert np.array_equal(np.fromfile(a[0], "<f4"), np.fromfile(b[0], "<f4"))


def test_the_library_function_refuses_what_it_cannot_compute(some_lines):
    q = lc.q_table()
    with pytest.raises(ValueError, match="no molar mass"):
        lines.line_opacity(some_lines, q, [300.0], [1e6], GRID, None, backend="numpy")
    with pytest.raises(ValueError, match=r"the self-broadening fraction 2\.0 lies outside \[0, 1\]"):
        lines.line_opacity(some_lines, q, [300.0], [1e6], GRID, 18.0, 2.0, backend="numpy")
    with pytest.raises(ValueError, match=r"dnu = 0\.0 is not > 0"):
        lines.line_opacity(some_lines, q, [300.0], [1e6], (0.0, 0.0, 10), 18.0, backend="numpy")
    with pytest.raises(ValueError, match="backend is device or numpy"):
        lines.line_opacity(some_lines, q, [300.0], [1e6], GRID, 18.0, backend="cuda")
    bad = dict(some_lines, nu0=some_lines["nu0"].copy())
    bad["nu0"][3] = -1.0
    with pytest.raises(ValueError, match=r"line 3: nu_0 = -1\.0 is not > 0"):
        lines.line_opacity(bad, q, [300.0], [1e6], GRID, 18.0, backend="numpy")
