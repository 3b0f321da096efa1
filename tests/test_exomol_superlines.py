"""Super-lines of exomol.py with the numpy backend, under the rule of tests/exomol_superline_cases.py: the node's list and kappa
against the long-double restatement, identical classes, cells and order, the strength that is kept, the degenerate settings,
weak transitions on their cells' centres, chunks, the k-table route, the refusals and the host form of the tile ranges."""
import os

import numpy as np
import pytest

import exomol_cases as ec
import exomol_superline_cases as sc
from helios_amd import exomol, ktable

B, WAVE, TILE = sc.B, sc.WAVE, sc.TILE


def node_of(case, node=0):
    temp, press = case.nodes[node]
    return exomol.superline_node(case.states, case.trans, case.broadening, temp, press, case.q(temp), case.molar_mass, case.s_min,
                                 case.s_sl, case.step)


def opacity(case, backend="numpy", timing=None, **kw):
    """kappa [node][point] of the case's nodes, each a (T, P) pair of its own"""
    rows = []
    for temp, press in case.nodes:
        rows.append(exomol.exomol_opacity(case.states, case.trans, case.broadening, ec.q_table(), [temp], [press], case.grid,
                                          case.molar_mass, case.cutoff, case.s_min, backend=backend, timing=timing, **kw)[0, 0])
    return np.array(rows)


@pytest.fixture(scope="module")
def sizes():
    return sc.layout("sizes", sc.sizes_layout(), seed=3, n_broadeners=2)


@pytest.fixture(scope="module")
def moving():
    return sc.layout("moving", sc.spread(["wmsd" * 10, "m" * 5, "ddd" + "w", "s" * 3]), seed=4,
                     nodes=[(700.0, 1e5), (1500.0, 1e7), (2500.0, 1e3)])


def test_the_list_and_kappa_lie_under_the_rule_and_the_order_is_the_restatements(sizes, moving):
    for case in (sizes, moving):
        timing = {}
        kappa = opacity(case, timing=timing, superline_threshold=case.s_sl, superline_step=case.step)
        for node in range(len(case.nodes)):
            label = "%s, node %d" % (case.label, node)
            got = node_of(case, node)
            r = sc.check_list(got["params"], (len(got["strong"]), len(got["weak"]), len(got["cells"])), case, node, label)
            want = r["list_f64"]
            assert np.array_equal(got["keys"], want["keys"]) and np.array_equal(got["keys"], r["list_ld"]["keys"]), label
            for k in ("kept", "strong", "weak", "cells"):
                assert np.array_equal(got[k], want[k]) and np.array_equal(got[k], r["list_ld"][k]), (label, k)
            assert np.array_equal(np.lexsort((got["keys"][:, 2], got["keys"][:, 1], got["keys"][:, 0])), np.arange(len(got["keys"])))
            ec.check_rule(kappa[node], r["ld"], r["f64"], label + ", kappa")
    assert (timing["strong"][0, 0], timing["weak"][0, 0], timing["superlines"][0, 0]) == (len(got["strong"]), len(got["weak"]),
                                                                                         len(got["cells"]))
    classes = [sc.classes_at(moving, node) for node in range(3)]
    assert classes[0].count("d") > classes[1].count("d") and classes[0].count("s") < classes[2].count("s")     # the nodes differ


def test_the_layout_holds_what_it_is_meant_to(sizes):
    """cells of every size around the wavefront and the block; the cell of 700 starts at the last lane of a block"""
    got = node_of(sizes)
    cell = np.floor(sizes.trans["nu0"] / sizes.step).astype(np.int64)
    per_cell = dict((int(c), int(np.count_nonzero(cell[got["weak"]] == c))) for c in got["cells"])
    assert set(sc.SIZES) <= set(per_cell.values())
    first = int(np.nonzero(cell == [c for c, k in per_cell.items() if k == 700][0])[0][0])
    assert first % B == B - 1 and first + 700 > 3 * B
    classes = sc.classes_at(sizes)
    assert classes[0] == "w" and classes[-1] == "w" and "d" in classes
    lonely = [c for c in np.unique(cell) if c not in per_cell]
    assert len(lonely) == 3                                      # two cells of strong and one of dropped transitions only


def test_no_strength_is_thrown_away(sizes, moving):
    for case in (sizes, moving):
        for node, (temp, _) in enumerate(case.nodes):
            got = node_of(case, node)
            s = exomol.strengths(case.states, case.trans, temp, case.q(temp))
            total, kept = float(np.sum(got["S_c"]) + np.sum(s[got["strong"]])), float(np.sum(s[got["kept"]]))
            assert abs(total / kept - 1.0) <= 1e-13, (case.label, node, total, kept)
            assert len(got["kept"]) == len(got["strong"]) + len(got["weak"]) and len(got["weak"]) > len(got["cells"]) > 0


def test_a_threshold_at_or_below_the_cut_gives_the_plain_result_bit_for_bit(sizes):
    plain = opacity(sizes)
    for s_sl in (sizes.s_min, 0.0, 0.5 * sizes.s_min):
        timing = {}
        got = opacity(sizes, timing=timing, superline_threshold=s_sl, superline_step=sizes.step)
        assert np.array_equal(got.view(np.uint64), plain.view(np.uint64)), s_sl
        assert timing["weak"][0, 0] == 0 == timing["superlines"][0, 0] and timing["strong"][0, 0] == timing["kept"][0, 0]
    prm, idx = exomol.node_params(sizes.states, sizes.trans, sizes.broadening, 700.0, 1e5, sizes.q(700.0), sizes.molar_mass, sizes.s_min)
    prm_sl, idx_sl = exomol.node_params(sizes.states, sizes.trans, sizes.broadening, 700.0, 1e5, sizes.q(700.0), sizes.molar_mass,
                                        sizes.s_min, superline_threshold=0.0, superline_step=sizes.step)
    assert np.array_equal(prm.view(np.uint64), prm_sl.view(np.uint64)) and np.array_equal(idx, idx_sl)


def test_an_infinite_threshold_makes_every_kept_transition_weak(sizes):
    case = sizes.with_levels(s_sl=np.inf)
    got = node_of(case)
    assert len(got["strong"]) == 0 and len(got["weak"]) == len(got["kept"]) > 0 and got["params"].shape[1] == len(got["cells"])
    r = sc.check_list(got["params"], (0, len(got["weak"]), len(got["cells"])), case, 0, "S_sl = inf")
    kappa = opacity(case, superline_threshold=np.inf, superline_step=case.step)[0]
    ec.check_rule(kappa, r["ld"], r["f64"], "S_sl = inf, kappa")


def test_underflowed_strengths_under_no_cut_make_a_super_line_of_strength_zero():
    case = sc.layout("zeros", sc.spread(["zzz", "swz", "w"]), seed=8, s_min=0.0)
    got = node_of(case)
    assert got["cells"].tolist() == [sc.FIRST_CELL + 8, sc.FIRST_CELL + 17, sc.FIRST_CELL + 26] and got["S_c"][0] == 0.0 < got["S_c"][1]
    assert got["params"][1, 0] == 0.0 and got["params"][3, 0] == 1e-8 and np.all(np.isfinite(got["params"]))
    r = sc.check_list(got["params"], (1, 6, 3), case, 0, "zeros")
    ec.check_rule(opacity(case, superline_threshold=case.s_sl, superline_step=case.step)[0], r["ld"], r["f64"], "zeros, kappa")


def test_one_weak_transition_on_its_cells_centre_reproduces_the_plain_kappa():
    """d = 0.25: (c + 0.5) d is an exact double and so is every nu_0 placed there; the super-line is the transition"""
    case = sc.layout("centred", sc.spread(["w"] * 40, gap=3), seed=9, centred=True, s_sl=np.inf, n_broadeners=2)
    assert np.array_equal(case.trans["nu0"], (np.floor(case.trans["nu0"] / 0.25) + 0.5) * 0.25)
    got = node_of(case)
    assert got["params"].shape == (4, 40) and np.array_equal(got["params"][0], case.trans["nu0"])
    plain = opacity(case)[0]
    merged = opacity(case, superline_threshold=np.inf, superline_step=0.25)[0]
    assert np.array_equal(plain == 0, merged == 0) and plain.max() > 0
    lit = plain > 0
    assert np.max(np.abs(merged[lit] / plain[lit] - 1.0)) <= 1e-13


def test_the_host_tile_ranges_hold_every_entry_the_per_point_test_passes():
    """a super-line above a strong nu_0 of its cell at a tile boundary: the list's nu descends there, and a reach without the
    step would lose the super-line"""
    boundary = int(round((1000.0 + TILE * sc.DNU) / sc.STEP))                      # the cell that begins at point TILE
    cells = [(boundary - 2 * 8 - 1, "sw"), (boundary - 8 - 1, "wws"), (boundary, "sww"), (boundary + 8 + 1, "ws")]
    case = sc.layout("tile boundary", cells, grid=(1000.0, sc.DNU, 2 * TILE + 5), seed=10)
    got = node_of(case)
    nu = got["params"][0]
    assert np.any(np.diff(nu) < 0) and np.all(np.diff(nu) > -case.step)
    ranges = exomol.tile_ranges(nu, *case.grid, case.cutoff, case.step)
    sc.check_ranges(ranges, nu, case, "tile boundary")
    sizes = sc.layout("sizes, three tiles", sc.spread(["sw" * 20, "wws" * 30, "s" * 10], gap=1200), grid=(1000.0, sc.DNU, 3 * TILE + 37),
                      seed=11)
    nu = node_of(sizes)["params"][0]
    sc.check_ranges(exomol.tile_ranges(nu, *sizes.grid, sizes.cutoff, sizes.step), nu, sizes, "three tiles")
    prm = exomol.node_params(sizes.states, sizes.trans, sizes.broadening, 700.0, 1e5, sizes.q(700.0), sizes.molar_mass, sizes.s_min)[0]
    plain = exomol.tile_ranges(prm[0], *sizes.grid, sizes.cutoff)                   # step 0: today's ranges
    assert plain.shape == (4, 2) and np.all(plain[:, 0] <= plain[:, 1])


# ---- the tool -----------------------------------------------------------------------------------------------------------------
def tool_case():
    """about a third of each class over 150 ... 1950 cm^-1, cells of 0.05 cm^-1 around whole wavenumbers"""
    rng = np.random.default_rng(77)
    cells = sorted(set(int(c) for c in rng.integers(150 * 20, 1950 * 20, 120)))
    kinds = ["".join(rng.choice(list("swwd"), int(rng.integers(1, 6)))) for _ in cells]
    return sc.layout("tool", list(zip(cells, kinds)), grid=(0.0, 0.05, 40000), cutoff=25.0, seed=12, n_broadeners=2, step=0.05,
                     nodes=[(300.0, 1e3), (900.0, 1e6)], s_min=1e-40, s_sl=1e-23)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("exomol_superlines"))
    st, tr, entries, pf = ec.write_files(wd, tool_case())
    return {"wd": wd, "files": ["-states", st, "-trans", tr, "-partition_function", pf, "-broadeners", " ".join(entries)]}


def _argv(inputs, *more):
    return ["-name", "H2O"] + inputs["files"] + ["-temperatures", "900 300", "-pressure_codes", "p000 n300", "-numax", "2000", "-dnu",
                                                 "0.05", "-strength_cutoff", "1e-40", "-backend", "numpy"] + list(more)


def kept_lines(text):
    return [line for line in text.splitlines() if "transitions kept" in line]


def test_without_the_option_the_printed_lines_keep_their_form_and_a_threshold_below_the_cut_writes_the_same_files(inputs, capsys):
    wd = inputs["wd"]
    plain = exomol.main(_argv(inputs, "-output_directory", os.path.join(wd, "plain")))
    lines = kept_lines(capsys.readouterr().out)
    n = len(tool_case().trans["nu0"])
    assert len(lines) == 4 and all(line.endswith("of %d transitions kept" % n) and line.startswith("exomol: ") for line in lines)
    below = exomol.main(_argv(inputs, "-output_directory", os.path.join(wd, "below"), "-superline_threshold", "1e-41"))
    text = kept_lines(capsys.readouterr().out)
    assert all(t.startswith(p + ": ") and " 0 weak in 0 super-lines" in t for t, p in zip(text, lines))
    for a, b in zip(plain, below):
        assert os.path.basename(a) == os.path.basename(b) and open(a, "rb").read() == open(b, "rb").read()


def test_a_chunked_run_forms_the_super_lines_of_a_one_chunk_run(inputs, capsys, monkeypatch):
    wd = inputs["wd"]
    lists = []
    real = exomol.superline_node
    monkeypatch.setattr(exomol, "superline_node", lambda *a: lists.append(real(*a)) or lists[-1])
    more = ("-superline_threshold", "1e-23")                     # the step is -dnu
    one = exomol.main(_argv(inputs, "-output_directory", os.path.join(wd, "one"), *more))
    text_one = kept_lines(capsys.readouterr().out)
    n_one = len(lists)
    chunked = exomol.main(_argv(inputs, "-output_directory", os.path.join(wd, "chunked"), "-chunk_width", "500", *more))
    assert n_one == 4 and len(lists) == 4 + 16 and len(one) == 4 and len(chunked) == 16
    assert kept_lines(capsys.readouterr().out) == text_one and " strong, " in text_one[0] and " super-lines" in text_one[0]
    assert lists[0]["params"].shape[1] < len(lists[0]["kept"])
    for k, node in enumerate(lists[4:]):
        want = lists[k % 4]
        for name in ("params", "keys", "cells", "S_c"):
            assert np.array_equal(node[name], want[name]), (k, name)
    for node in range(4):                                        # a chunk's points lo + i dnu are other bits than 0 + i dnu
        whole = np.fromfile(one[node], "<f4")
        parts = np.concatenate([np.fromfile(chunked[4 * c + node], "<f4") for c in range(4)])
        assert whole.shape == parts.shape and whole.max() > 0 and np.array_equal(whole == 0, parts == 0)


def test_the_ktable_containers_equal_the_two_step_routes_bytes(inputs, capsys):
    from test_exomol_ktable import GRID, same_containers
    wd = inputs["wd"]
    more = ("-superline_threshold", "1e-23", "-superline_step", "0.1")
    out = os.path.join(wd, "opac", "H2O")
    exomol.main(_argv(inputs, "-output_directory", out, *more))
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nH2O %s\n" % out)
    want = ktable.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-backend", "numpy",
                        "-directory_with_individual_files", os.path.join(wd, "two_step")] + GRID)
    capsys.readouterr()
    got = exomol.main(_argv(inputs, "-ktable", "yes", "-directory_with_individual_files", os.path.join(wd, "fused"), *more) + GRID)
    same_containers(got, want)
    text = kept_lines(capsys.readouterr().out)
    assert len(text) == 4 and all(" weak in " in t for t in text) and "300 K, n300" in text[0]
    plain = exomol.main(_argv(inputs, "-ktable", "yes", "-directory_with_individual_files", os.path.join(wd, "fused_plain")) + GRID)
    with np.load(got[0]) as a, np.load(plain[0]) as b:
        assert a["kpoints"].shape == b["kpoints"].shape and not np.array_equal(a["kpoints"], b["kpoints"])


# ---- refusals -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("threshold,step,reason", [
    (float("nan"), 0.25, r"the super-line threshold nan is not a number >= 0 cm / molecule"),
    (-1e-30, 0.25, r"the super-line threshold -1e-30 is not a number >= 0 cm / molecule"),
    (1e-23, 0.0, r"the super-line step 0\.0 is not a finite number > 0 cm\^-1"),
    (1e-23, -0.25, r"the super-line step -0\.25 is not a finite number > 0 cm\^-1"),
    (1e-23, float("inf"), r"the super-line step inf is not a finite number > 0 cm\^-1"),
    (1e-23, float("nan"), r"the super-line step nan is not a finite number > 0 cm\^-1"),
    (1e-23, 2.5, r"the super-line step 2\.5 is greater than the cut-off 2\.0 cm\^-1"),
    (1e-23, 1e-7, r"the super-line step 1e-07 puts the largest nu_0 = 1\d\d\d\.\d+ into cell \d+\.0, cells are numbered below 2\^31"),
    (None, 0.25, r"a super-line step \(0\.25\) without a super-line threshold"),
])
def test_the_library_refuses_with_the_value(sizes, threshold, step, reason, monkeypatch):
    monkeypatch.setattr(exomol, "numpy_node", lambda *a, **k: pytest.fail("a node was computed"))
    with pytest.raises(ValueError, match=reason):
        opacity(sizes, superline_threshold=threshold, superline_step=step)
    inter = ktable.wavelength_grid("fixed_resolution", "20 6 40".split())
    with pytest.raises(ValueError, match=reason):
        exomol.exomol_ktable(sizes.states, sizes.trans, sizes.broadening, ec.q_table(), [700], ["p000"], 2000, 0.05, inter, 8, ec.M_H2O,
                             2.0, 1e-40, backend="numpy", superline_threshold=threshold, superline_step=step)


@pytest.mark.parametrize("more,reason", [
    (["-superline_step", "0.05"], r"-superline_step 0\.05 without -superline_threshold"),
    (["-superline_threshold", "-1"], r"the super-line threshold -1\.0 is not a number >= 0"),
    (["-superline_threshold", "nan"], r"the super-line threshold nan is not a number >= 0"),
    (["-superline_threshold", "1e-23", "-superline_step", "0"], r"the super-line step 0\.0 is not a finite number > 0"),
    (["-superline_threshold", "1e-23", "-superline_step", "30"], r"the super-line step 30\.0 is greater than the cut-off 25\.0"),
    (["-superline_threshold", "1e-23", "-superline_step", "1e-7"], r"the super-line step 1e-07 puts the largest nu_0 = .* into cell"),
])
def test_the_tool_refuses_with_the_value(inputs, more, reason, monkeypatch):
    monkeypatch.setattr(exomol, "numpy_node", lambda *a, **k: pytest.fail("a node was computed"))
    out = os.path.join(inputs["wd"], "refused")
    with pytest.raises(IOError, match=reason):
        exomol.main(_argv(inputs, "-output_directory", out) + more)
    assert not os.path.exists(out)
    with pytest.raises(IOError, match=reason):
        exomol.main(_argv(inputs, "-ktable", "yes", "-directory_with_individual_files", out) + more)
    assert not os.path.exists(out)


def test_a_threshold_without_a_step_takes_dnu(sizes):
    a = opacity(sizes, superline_threshold=sizes.s_sl)
    b = opacity(sizes, superline_threshold=sizes.s_sl, superline_step=sizes.grid[1])
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    with pytest.raises(ValueError, match=r"the super-line threshold 1e-23 without a super-line step"):
        exomol.node_params(sizes.states, sizes.trans, sizes.broadening, 700.0, 1e5, sizes.q(700.0), sizes.molar_mass, sizes.s_min,
                           superline_threshold=1e-23)
