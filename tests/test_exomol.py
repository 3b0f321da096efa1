"""exomol.py on the CPU: the readers with every refusal and its message, the broadening table, the numpy backend under the rule of
tests/exomol_cases.py on the cases the device is held to, and the files the tool writes."""
import os

import numpy as np
import pytest

import exomol_cases as ec
from helios_amd import exomol


def small_states():
    return {"E": np.array([0.0, 50.0, 1000.0, 1100.0]), "g": np.array([1.0, 3.0, 3.0, 6.0]), "J": np.array([0.0, 1.0, 1.0, 2.5]),
            "jidx": np.array([0, 2, 2, 5], np.int32)}


def write(path, text):
    with open(path, "w") as f:
        f.write(text)
    return str(path)


# ---- states ----------------------------------------------------------------------------------------------------------------
def test_states_with_half_integer_j_and_columns_after_j(tmp_path):
    path = ec.write_states(str(tmp_path / "s.states"), small_states())
    got = exomol.read_states(path)
    want = small_states()
    for k in ("E", "g", "J", "jidx"):
        assert np.array_equal(got[k], want[k]), k
    assert got["jidx"].dtype == np.int32 and got["jidx"][3] == 5


@pytest.mark.parametrize("text,reason", [
    ("1 0.0 1 0\n3 5.0 3 1\n", r"line 2 of .*: id 3 where 2 is expected; the ids are 1, 2, \.\.\. in file order"),
    ("2 0.0 1 0\n", r"line 1 of .*: id 2 where 1 is expected"),
    ("1 0.0 1\n", r"line 1 of .* holds 3 columns, a state needs id, E, g and J"),
    ("1 abc 1 0\n", r"line 1 of .*: E = 'abc' is not a finite number"),
    ("1 0.0 1 0\n2 nan 1 0\n", r"line 2 of .*: E = 'nan' is not a finite number"),
    ("1 0.0 1 0.25\n", r"line 1 of .*: J = 0\.25; J is >= 0 and 2 J a whole number"),
    ("1 0.0 1 -1\n", r"line 1 of .*: J = -1; J is >= 0"),
    ("\n\n", r"holds no state"),
])
def test_states_refused_with_the_line(tmp_path, text, reason):
    with pytest.raises(IOError, match=reason):
        exomol.read_states(write(tmp_path / "bad.states", text))


def test_a_missing_file_is_an_error(tmp_path):
    with pytest.raises(IOError):
        exomol.read_states(str(tmp_path / "nothing.states"))
    with pytest.raises(IOError):
        exomol.read_transitions([str(tmp_path / "nothing.trans")], small_states())


# ---- transitions -----------------------------------------------------------------------------------------------------------
def test_transitions_are_gathered_sorted_and_the_downward_ones_skipped(tmp_path):
    """nu_0 is E[up] - E[low] from the states whatever a fourth column says; 3 -> 4 and 1 -> 1 have nu_0 <= 0"""
    path = ec.write_trans(str(tmp_path / "t.trans"), [3, 2, 2, 0, 3], [0, 1, 3, 0, 1], [5.0, 4.0, 3.0, 2.0, 1.0], fourth_column=True)
    trans, skipped = exomol.read_transitions(path, small_states())
    assert skipped == 2
    assert trans["nu0"].tolist() == [950.0, 1050.0, 1100.0] and trans["up"].tolist() == [2, 3, 3] and trans["low"].tolist() == [1, 1, 0]
    assert trans["A"].tolist() == [4.0, 1.0, 5.0] and trans["up"].dtype == np.int32


def test_bz2_files_are_read_as_the_plain_ones(tmp_path):
    states = small_states()
    plain = exomol.read_transitions(ec.write_trans(str(tmp_path / "t.trans"), [3, 2], [0, 1], [5.0, 4.0]),
                                    exomol.read_states(ec.write_states(str(tmp_path / "s.states"), states)))[0]
    packed_states = exomol.read_states(ec.write_states(str(tmp_path / "s.states.bz2"), states))
    packed = exomol.read_transitions(ec.write_trans(str(tmp_path / "t.trans.bz2"), [3, 2], [0, 1], [5.0, 4.0]), packed_states)[0]
    assert open(str(tmp_path / "t.trans.bz2"), "rb").read(3) == b"BZh"
    for k in plain:
        assert np.array_equal(plain[k], packed[k]), k
    assert np.array_equal(packed_states["E"], states["E"])


def test_two_trans_files_in_both_orders_give_two_tie_orders(tmp_path):
    orders = {}
    for first in (True, False):
        case, parts = ec.tie_case(first)
        paths = [ec.write_trans(str(tmp_path / ("%d_%s.trans" % (k, first))), *part) for k, part in enumerate(parts)]
        trans, skipped = exomol.read_transitions(paths, case.states)
        assert skipped == 0 and np.all(np.diff(trans["nu0"]) >= 0)
        for k in trans:
            assert np.array_equal(trans[k], case.trans[k]), k
        orders[first] = trans
    a, b = orders[True], orders[False]
    assert a["nu0"].tolist() == b["nu0"].tolist() == [975.0, 975.0, 1000.0, 1000.0, 1060.0]
    assert a["up"].tolist() == [5, 6, 3, 4, 3] and b["up"].tolist() == [6, 5, 4, 3, 3]        # file order inside every tie


@pytest.mark.parametrize("text,reason", [
    ("3 1 1.0\n5 1 1.0\n", r"line 2 of .*: upper id = 5 lies outside the states' 1 \.\.\. 4"),
    ("3 0 1.0\n", r"line 1 of .*: lower id = 0 lies outside the states' 1 \.\.\. 4"),
    ("3 1.5 1.0\n", r"line 1 of .*: lower id = 1\.5 lies outside the states' 1 \.\.\. 4"),
    ("3 1 x\n", r"line 1 of .*: A = 'x' is not a finite number"),
    ("3 1 inf\n", r"line 1 of .*: A = 'inf' is not a finite number"),
    ("3 1 -2.0\n", r"line 1 of .*: A = -2\.0 is negative"),
    ("3 1\n", r"line 1 of .* holds 2 columns, a transition needs upper id, lower id and A"),
    ("1 3 1.0\n2 2 1.0\n", r"no transition is left of .* \(2 with nu_0 <= 0 skipped\)"),
])
def test_transitions_refused_with_file_and_line(tmp_path, text, reason):
    path = write(tmp_path / "bad.trans", text)
    with pytest.raises(IOError, match=reason) as e:
        exomol.read_transitions([path], small_states())
    assert "bad.trans" in str(e.value)


# ---- broadening ------------------------------------------------------------------------------------------------------------
def test_broad_rows_of_other_codes_are_skipped_and_counted(tmp_path):
    rows = {0: (0.1, 0.5), 1: (0.09, 0.45), 4: (0.08, 0.4)}
    got, skipped = exomol.read_broad(ec.write_broad(str(tmp_path / "b.broad"), rows, other_codes=2))
    assert got == rows and skipped == 2


def test_a_second_a0_row_for_one_j_is_refused_with_both_lines(tmp_path):
    path = write(tmp_path / "twice.broad", "a0 0.1 0.5 0\na1 0.1 0.5 1 2\na0 0.09 0.4 1.5\na0 0.2 0.6 1.5\n")
    with pytest.raises(IOError, match=r"line 4 of .*twice\.broad.*: a second a0 row for J'' = 1\.5; the first is line 3"):
        exomol.read_broad(path)


def test_the_table_takes_the_defaults_where_the_file_holds_no_row(tmp_path, capsys):
    h2 = ec.write_broad(str(tmp_path / "h2.broad"), {0: (0.1, 0.5), 3: (0.08, 0.4), 9: (0.01, 0.1)}, other_codes=1)
    he = ec.write_broad(str(tmp_path / "he.broad"), {1: (0.05, 0.3)})
    entries = exomol.parse_broadeners("H2:0.85:%s He:0.15:%s:0.02:0.25" % (h2, he), (0.07, 0.5))
    assert entries == [("H2", 0.85, h2, 0.07, 0.5), ("He", 0.15, he, 0.02, 0.25)]
    x, table = exomol.broadening_table(entries, 5, print)
    assert x.tolist() == [0.85, 0.15] and table.shape == (2, 6, 2)
    assert table[0].tolist() == [[0.1, 0.5], [0.07, 0.5], [0.07, 0.5], [0.08, 0.4], [0.07, 0.5], [0.07, 0.5]]     # jidx 9 lies beyond
    assert table[1].tolist() == [[0.02, 0.25], [0.05, 0.3]] + [[0.02, 0.25]] * 4
    text = capsys.readouterr().out
    assert "1 rows of other codes than a0 skipped" in text and "the fractions of the 2 broadeners sum to 1" in text
    x, table = exomol.broadening_table(exomol.parse_broadeners(None, (0.06, 0.4)), 2)
    assert x.tolist() == [1.0] and table.tolist() == [[[0.06, 0.4]] * 3]


@pytest.mark.parametrize("text,reason", [
    ("H2:0.85", r"entry 'H2:0\.85' is not name:fraction:file"),
    ("H2:0:f.broad", r"the fraction 0 is not > 0"),
    ("H2:-0.1:f.broad", r"the fraction -0\.1 is not > 0"),
    ("H2:abc:f.broad", r"fraction and defaults are finite numbers"),
    ("H2:0.5:f.broad:0.07", r"is not name:fraction:file\[:gamma_default:n_default\]"),
])
def test_broadener_entries_refused(text, reason):
    with pytest.raises(IOError, match=reason):
        exomol.parse_broadeners(text)


# ---- the numpy backend -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("label", ec.case_labels())
def test_the_numpy_backend_under_the_rule(label):
    """kept set identical to the restatement's; the four numbers and kappa under the rule"""
    case = ec.make(label)
    for node, (temp, press) in enumerate(case.nodes):
        r = ec.restated(case, node)
        prm, kept = exomol.node_params(case.states, case.trans, case.broadening, temp, press, case.q(temp), case.molar_mass, case.s_min)
        assert np.array_equal(kept, r["kept"]), label
        if len(kept):
            ec.check_rule(prm, r["params_ld"], r["params_f64"], label + ", line_params")
            assert np.array_equal(prm[0], case.trans["nu0"][kept])
        timing = {}
        kappa = exomol.exomol_opacity(case.states, case.trans, case.broadening, ec.q_table(), [temp], [press], case.grid, case.molar_mass,
                                      case.cutoff, case.s_min, backend="numpy", timing=timing)
        assert kappa.shape == (1, 1, case.grid[2]) and timing["kept"].tolist() == [[len(kept)]]
        ec.check_rule(kappa[0, 0], r["ld"], r["f64"], label + ", kappa")
        if len(kept) == 0:
            assert not kappa.any() and timing["pairs"] == 0


def test_the_patterns_are_what_their_names_say():
    n = 2 * ec.B + 1
    for name in ec.PATTERNS:
        assert np.array_equal(ec.restated(ec.make("pattern: " + name), 0)["kept"], np.nonzero(ec.pattern(name, n))[0]), name
    hot = ec.make("broadeners: 2")
    assert len(ec.restated(hot, 1)["kept"]) == ec.B + 1 > len(ec.restated(hot, 0)["kept"])          # 1500 K keeps them all


def test_the_cut_off_to_the_ulp_and_ties_in_both_orders():
    for e_up, points in ((100.0, list(range(300, 501))), (float(np.nextafter(100.0, 0.0)), list(range(300, 500)))):
        case = ec.two_states_case(e_up)
        r = ec.restated(case, 0)
        kappa = exomol.exomol_opacity(case.states, case.trans, case.broadening, ec.q_table(), [300.0], [1e5], case.grid, case.molar_mass,
                                      case.cutoff, 0.0, backend="numpy")[0, 0]
        ec.check_rule(kappa, r["ld"], r["f64"], case.label)
        assert np.nonzero(kappa)[0].tolist() == points
    rows = []
    for first in (True, False):
        case, _ = ec.tie_case(first)
        r = ec.restated(case, 0)
        kappa = exomol.exomol_opacity(case.states, case.trans, case.broadening, ec.q_table(), [500.0], [1e6], case.grid, case.molar_mass,
                                      case.cutoff, 0.0, backend="numpy")[0, 0]
        ec.check_rule(kappa, r["ld"], r["f64"], case.label)
        rows.append(kappa)
    assert np.allclose(rows[0], rows[1], rtol=1e-11, atol=0) and np.count_nonzero(rows[0]) == 2 * 201      # 975 and 1000 +- 5 cm^-1


def test_refusals_of_the_library_function():
    case = ec.make("count: 63")
    args = (case.states, case.trans, case.broadening, ec.q_table())
    with pytest.raises(ValueError, match=r"the strength cut-off -1\.0 is not a finite number >= 0"):
        exomol.exomol_opacity(*args, [700.0], [1e5], case.grid, ec.M_H2O, 2.0, -1.0, backend="numpy")
    with pytest.raises(ValueError, match="no molar mass"):
        exomol.exomol_opacity(*args, [700.0], [1e5], case.grid, None, backend="numpy")
    with pytest.raises(ValueError, match="every temperature is a finite number > 0"):
        exomol.exomol_opacity(*args, [-700.0], [1e5], case.grid, ec.M_H2O, backend="numpy")
    with pytest.raises(ValueError, match=r"T = 10 K lies outside the partition function's 50 \.\.\. 3000 K"):
        exomol.exomol_opacity(*args, [10.0], [1e5], case.grid, ec.M_H2O, backend="numpy")
    with pytest.raises(ValueError, match="backend is device or numpy"):
        exomol.exomol_opacity(*args, [700.0], [1e5], case.grid, ec.M_H2O, backend="cuda")


# ---- the tool ------------------------------------------------------------------------------------------------------------------
def test_the_file_routes_names_and_contents(tmp_path, capsys):
    """Out_<name>_<numin:05d>_<numax:05d>_<T:05d>_<pcode>.bin, fp32 of the library function's rows; the partition function need not
    hold 296 K; the counts kept are printed per node"""
    import exomol as exomol_tool
    wd = str(tmp_path)
    case = ec.build("tool", ec.pattern("alternating", 120), grid=(900.0, 0.25, 800), seed=9, n_broadeners=2)
    st, tr, entries, _ = ec.write_files(wd, case)
    pf = os.path.join(wd, "hot.pf")
    ec.write_q_file(pf, (np.array([500.0, 1000.0, 2000.0]), np.array([500.0, 1000.0, 2000.0]) ** 1.5))
    argv = ["-name", "H2O", "-states", st, "-trans", tr, "-partition_function", pf, "-broadeners", " ".join(entries), "-temperatures",
            "700 1500", "-pressure_codes", "p000", "-numin", "900", "-numax", "1100", "-dnu", "0.25", "-cutoff", "2.0",
            "-strength_cutoff", "1e-34", "-backend", "numpy", "-output_directory", os.path.join(wd, "opac")]
    written = exomol_tool.main(argv)
    assert [os.path.basename(w) for w in written] == ["Out_H2O_00900_01100_00700_p000.bin", "Out_H2O_00900_01100_01500_p000.bin"]
    text = capsys.readouterr().out
    assert "exomol: 700 K, p000: 60 of 120 transitions kept" in text and "exomol: 1500 K, p000: 120 of 120 transitions kept" in text
    assert "0 with nu_0 <= 0 skipped" in text and "sum to 1" in text
    q = (np.array([500.0, 1000.0, 2000.0]), np.array([500.0, 1000.0, 2000.0]) ** 1.5)
    want = exomol.exomol_opacity(case.states, case.trans, case.broadening, q, [700.0, 1500.0], [1e6], (900.0, 0.25, 800), ec.M_H2O, 2.0,
                                 1e-34, backend="numpy")
    for k, w in enumerate(written):
        assert np.fromfile(w, "<f4").tobytes() == want[k, 0].astype("<f4").tobytes()
    chunks = exomol_tool.main(argv[:-1] + [os.path.join(wd, "chunks"), "-chunk_width", "100", "-output_format", "text"])
    assert [os.path.basename(w) for w in chunks] == ["Out_H2O_00900_01000_00700_p000.dat", "Out_H2O_00900_01000_01500_p000.dat",
                                                     "Out_H2O_01000_01100_00700_p000.dat", "Out_H2O_01000_01100_01500_p000.dat"]


def test_the_tools_refusals(tmp_path):
    import exomol as exomol_tool
    wd = str(tmp_path)
    case = ec.make("count: 63")
    st, tr, entries, pf = ec.write_files(wd, case)
    base = ["-name", "H2O", "-states", st, "-trans", tr, "-partition_function", pf, "-temperatures", "700", "-pressure_codes", "p000",
            "-numax", "1300", "-dnu", "0.25", "-backend", "numpy", "-output_directory", os.path.join(wd, "out")]
    with pytest.raises(IOError, match=r"-strength_cutoff -1\.0 is not a finite number >= 0"):
        exomol_tool.main(base + ["-strength_cutoff", "-1"])
    with pytest.raises(IOError, match=r"-default_broadening '0\.07': gamma >= 0 and n"):
        exomol_tool.main(base + ["-default_broadening", "0.07"])
    with pytest.raises(IOError):
        exomol_tool.main(base + ["-broadeners", "H2:1.0:%s" % os.path.join(wd, "missing.broad")])
    with pytest.raises(IOError, match=r"exomol: T = 5000 K lies outside the partition function"):
        exomol_tool.main(base[:9] + ["5000"] + base[10:])
    with pytest.raises(IOError, match="no molar mass: 'XYZ' is not in species_data.py"):
        exomol_tool.main(["-name", "XYZ"] + base[2:])
    assert not os.path.exists(os.path.join(wd, "out"))
