"""k_exomol_classify, _cells, _merge and the widened k_exomol_ranges (csrc/exomol.hip) through hx_exomol_set_superlines and exomol.py
on the device, under the rule of tests/exomol_superline_cases.py.  The sizes come from the constants the module exports: cells of
weak transitions around the wavefront and the compaction block and across three block boundaries, cells of one class only and of
all three, point counts around the tile, the cut-off to the ulp at a super-line, a super-line above a strong nu_0 of its cell at a
tile boundary, nodes that move transitions between the classes; launches against their repetition and against their nodes run
alone, the degenerate thresholds against the plain handle, the handle's refusals and the k-table route."""
import os

import numpy as np
import pytest

import exomol_cases as ec
import exomol_superline_cases as sc
from helios_amd import exomol
from helios_amd._lib import HeliosHipError

pytestmark = pytest.mark.gpu

TILE, B, WAVE = sc.TILE, sc.B, sc.WAVE


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def run(ctx, case, per=None, superlines=True, with_fp64=True):
    """per node: kappa64, slabs32, kept, counts (strong, weak, super-lines), line_params, tile_ranges; `per` nodes per launch"""
    nodes = case.nodes
    per = len(nodes) if per is None else per
    h = exomol.ExomolOpacity.of(ctx, case.states, case.trans, case.broadening, case.grid[2], per, len(nodes), with_fp64)
    rows = []
    try:
        if superlines:
            h.set_superlines(case.s_sl, case.step)
        h.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], [case.q(n[0]) for n in nodes], case.molar_mass, case.cutoff,
                    case.s_min, *case.grid)
        for first in range(0, len(nodes), per):
            n = min(per, len(nodes) - first)
            h.run_nodes(first, n)
            k64 = h.get("kappa64") if with_fp64 else [None] * n
            k32, kept, prm, ranges = h.get("slabs32"), h.get("kept"), h.get("line_params"), h.get("tile_ranges")
            counts = h.get("superline_counts") if superlines else np.stack([kept, 0 * kept, 0 * kept], axis=1)
            assert counts.shape == (n, 3) and counts.dtype == np.int32 and len(prm) == n
            for r in range(n):
                rows.append({"kappa64": k64[r], "slabs32": k32[r], "kept": int(kept[r]), "counts": tuple(int(c) for c in counts[r]),
                             "line_params": prm[r], "tile_ranges": ranges[r]})
        timing = h.get("timing_ms")
    finally:
        h.close()
    assert timing.shape == (2,) and timing[0] > 0 and timing[1] > 0
    return rows


def check(case, rows):
    """every node of the case against its restatement; returns the rows"""
    assert len(rows) == len(case.nodes)
    for node, row in enumerate(rows):
        label = "%s, node %d" % (case.label, node)
        r = sc.check_list(row["line_params"], row["counts"], case, node, label)
        assert row["kept"] == row["counts"][0] + row["counts"][1] == len(r["list_f64"]["kept"]), label
        assert row["line_params"].shape[1] == row["counts"][0] + row["counts"][2], label
        ec.check_rule(row["kappa64"], r["ld"], r["f64"], label + ", kappa64")
        with np.errstate(over="ignore"):
            assert np.array_equal(row["slabs32"].view(np.uint32), row["kappa64"].astype(np.float32).view(np.uint32)), label
        sc.check_ranges(row["tile_ranges"], row["line_params"][0], case, label)
        assert np.array_equal(row["tile_ranges"], exomol.tile_ranges(row["line_params"][0], *case.grid, case.cutoff, case.step)), label
    return rows


def same_bits(a, b, label, with_ranges=True):
    assert a["kept"] == b["kept"], label
    for k in ("kappa64", "line_params"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (label, k)
    assert np.array_equal(a["slabs32"].view(np.uint32), b["slabs32"].view(np.uint32)), label
    if with_ranges:
        assert a["counts"] == b["counts"] and np.array_equal(a["tile_ranges"], b["tile_ranges"]), label


@pytest.fixture(scope="module")
def sizes():
    return sc.layout("sizes", sc.sizes_layout(), seed=3, n_broadeners=2)


# ---- cells ---------------------------------------------------------------------------------------------------------------------
def test_cells_of_every_size_and_class_under_the_rule_and_twice_the_same_bits(ctx, sizes):
    """weak cells of 1, 63, 64, 65, 255, 256, 257 and 700, the last from the last lane of a block across three boundaries; cells of
    strong and of dropped transitions only; the classes interleaved; a weak first and last transition; two broadeners"""
    row = check(sizes, run(ctx, sizes))[0]
    want = sc.restated(sizes, 0)["list_f64"]
    cell = np.floor(sizes.trans["nu0"] / sizes.step).astype(np.int64)
    per_cell = [int(np.count_nonzero(cell[want["weak"]] == c)) for c in want["cells"]]
    assert set(sc.SIZES) <= set(per_cell)
    first = int(np.nonzero(cell == want["cells"][per_cell.index(700)])[0][0])
    assert first % B == B - 1 and first + 700 > 3 * B
    classes = sc.classes_at(sizes)
    assert classes[0] == "w" == classes[-1] and row["counts"] == (classes.count("s"), classes.count("w"), len(per_cell))
    assert len(np.unique(cell)) == len(per_cell) + 3             # two cells of strong, one of dropped transitions only
    same_bits(row, run(ctx, sizes)[0], "the launch again")


def test_the_degenerate_thresholds_against_the_plain_handle(ctx, sizes):
    """S_sl <= S_min: no transition is weak and the output is the plain handle's bit for bit (its ranges reach further);
    S_sl = +inf: every kept transition is weak"""
    plain = run(ctx, sizes, superlines=False)[0]
    for s_sl in (sizes.s_min, 0.0):
        row = run(ctx, sizes.with_levels(s_sl=s_sl))[0]
        assert row["counts"] == (plain["kept"], 0, 0), s_sl
        same_bits(row, plain, "S_sl = %g" % s_sl, with_ranges=False)
    every = sizes.with_levels(s_sl=np.inf)
    row = check(every, run(ctx, every))[0]
    assert row["counts"][0] == 0 and row["counts"][1] == plain["kept"] and row["line_params"].shape[1] == row["counts"][2] > 0


def test_underflowed_strengths_under_no_cut_make_a_super_line_of_strength_zero(ctx):
    case = sc.layout("zeros", sc.spread(["zzz", "swz", "w"]), seed=8, s_min=0.0)
    row = check(case, run(ctx, case))[0]
    assert row["counts"] == (1, 6, 3) and row["line_params"][1, 0] == 0.0 and row["line_params"][3, 0] == 1e-8


@pytest.mark.parametrize("n_points", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 37])
def test_point_counts_around_the_tile(ctx, n_points):
    at = sorted(set(sc.FIRST_CELL + int(round(f * (n_points - 1))) for f in (0.0, 0.2, 0.5, 0.77, 1.0)) | {sc.FIRST_CELL - 5})
    kinds = ["sww", "w" * (WAVE + 1), "ws", "dwd", "wsw", "s"]
    case = sc.layout("points: %d" % n_points, list(zip(at, kinds)), grid=(1000.0, sc.DNU, n_points), seed=300 + n_points)
    row = check(case, run(ctx, case))[0]
    assert row["counts"][2] >= 1 and row["kappa64"].max() > 0


# ---- many occupied cells: the wavefronts, mask words and workgroups of k_exomol_cells beyond the first ----------------------------
CELL_KINDS = ["w", "s", "d", "sw", "ws", "wd", "dw", "ss", "dd", "wsw", "sws", "swd", "m", "ms", "wm"]


def many_cells(n_cells, seed, nodes=(sc.NODE,)):
    """n_cells occupied cells side by side, emitting and not; around every multiple of the wavefront and of the compaction block
    the cells before, at and after it hold strong transitions with and without weak ones, so a strong transition's position
    depends on the mask words and on the cells' block offsets on both sides of the boundary"""
    rng = np.random.default_rng(seed)
    choice = [k for k in CELL_KINDS if len(nodes) > 1 or "m" not in k]          # the moving class needs two temperatures
    kinds = [str(k) for k in rng.choice(choice, n_cells)]
    for edge in sorted(set(list(range(WAVE, n_cells, WAVE)) + list(range(B, n_cells, B)))):
        for k, kind in ((edge - 2, "d"), (edge - 1, "sw"), (edge, "ws"), (edge + 1, "s"), (edge + 2, "wsw")):
            if 0 <= k < n_cells:
                kinds[k] = kind
    case = sc.layout("%d cells" % n_cells, list(zip(range(sc.FIRST_CELL + 4, sc.FIRST_CELL + 4 + n_cells), kinds)), seed=seed,
                     n_broadeners=2, nodes=nodes)
    assert len(np.unique(np.floor(case.trans["nu0"] / case.step))) == n_cells
    return case


@pytest.mark.parametrize("n_cells", [WAVE - 1, WAVE, WAVE + 1, B - 1, B, B + 1, 3 * B + WAVE + 7])
def test_occupied_cells_around_the_wavefront_and_the_block(ctx, n_cells):
    """63, 64, 65, 255, 256, 257 and 3 * 256 + 71 occupied cells: more than one wavefront of cells, more than one mask word, more
    than one workgroup of cells and a scan over several cell counts"""
    case = many_cells(n_cells, 500 + n_cells)
    row = check(case, run(ctx, case))[0]
    want = sc.restated(case, 0)["list_f64"]
    assert 0 < row["counts"][2] == len(want["cells"]) < n_cells and row["counts"][0] > n_cells // 4
    emits = np.isin(np.arange(sc.FIRST_CELL + 4, sc.FIRST_CELL + 4 + n_cells), want["cells"])
    if n_cells > WAVE:                                            # emitting and silent cells on both sides of a boundary
        assert emits[WAVE - 1] and emits[WAVE] and not emits[WAVE + 1 if WAVE + 1 < n_cells else WAVE - 2]
    if n_cells > B:
        assert emits[B - 1] and emits[B] and not emits[B - 2] and np.count_nonzero(~emits) > n_cells // 8


def test_many_cells_in_three_nodes_each_node_alone_and_the_launch_again(ctx):
    """3 * 256 + 71 occupied cells at three nodes whose temperatures change which cells emit"""
    case = many_cells(3 * B + WAVE + 7, 77, nodes=[(700.0, 1e5), (1500.0, 1e7), (2500.0, 1e3)])
    batch = check(case, run(ctx, case))
    cold, hot = (set(sc.restated(case, node)["list_f64"]["cells"].tolist()) for node in (0, 2))
    assert cold - hot and hot - cold and batch[0]["counts"][0] < batch[2]["counts"][0]      # cells that stop and that start to emit
    alone, again = run(ctx, case, per=1), run(ctx, case)
    for node in range(3):
        same_bits(batch[node], alone[node], "node %d alone" % node)
        same_bits(batch[node], again[node], "node %d again" % node)


def test_a_step_with_more_cells_after_one_with_fewer_on_one_handle(ctx):
    """the per-cell arrays grow with the second call; then the first step again, in the arrays of the larger one"""
    fine = many_cells(2 * B + WAVE + 3, 88)
    coarse = sc.Case(fine.label + ", step 2", fine.states, fine.raw, fine.broadeners, fine.nodes, fine.s_min, fine.grid, fine.cutoff,
                     fine.s_sl, 2.0)
    n_coarse = len(np.unique(np.floor(coarse.trans["nu0"] / 2.0)))
    assert WAVE < n_coarse < B < 2 * B < len(np.unique(np.floor(fine.trans["nu0"] / fine.step)))     # one workgroup of cells, then three
    temp, press = fine.nodes[0]
    h = exomol.ExomolOpacity.of(ctx, fine.states, fine.trans, fine.broadening, fine.grid[2], 1, 1, True)
    rows = []
    try:
        for case in (coarse, fine, coarse, fine):
            h.set_superlines(case.s_sl, case.step)
            h.set_nodes([temp], [press], [case.q(temp)], case.molar_mass, case.cutoff, case.s_min, *case.grid)
            h.run_nodes(0, 1)
            rows.append({"kappa64": h.get("kappa64")[0], "slabs32": h.get("slabs32")[0], "kept": int(h.get("kept")[0]),
                         "counts": tuple(int(c) for c in h.get("superline_counts")[0]), "line_params": h.get("line_params")[0],
                         "tile_ranges": h.get("tile_ranges")[0]})
    finally:
        h.close()
    check(coarse, rows[0:1])
    check(fine, rows[1:2])
    assert rows[0]["counts"][2] <= n_coarse < rows[1]["counts"][2]
    same_bits(rows[0], rows[2], "the coarse step again")
    same_bits(rows[1], rows[3], "the fine step again")


# ---- placements ----------------------------------------------------------------------------------------------------------------
def test_a_super_line_at_the_cut_off_distance_from_a_point_and_one_ulp_inside(ctx):
    """nu_c = 400.5 * 0.25 = 100.125 whatever the transition's nu_0 in the cell: the points at 75 and 125.25 lie exactly 25.125
    away and are in; with the cut-off one ulp shorter both are out"""
    for cutoff, lit in ((25.125, list(range(300, 502))), (float(np.nextafter(25.125, 0.0)), list(range(301, 501)))):
        case = sc.layout("cut-off %.17g" % cutoff, [(400, "w")], grid=(0.0, 0.25, 801), cutoff=cutoff, seed=21, s_sl=np.inf)
        row = check(case, run(ctx, case))[0]
        assert row["counts"] == (0, 1, 1) and row["line_params"][0, 0] == 100.125 != case.trans["nu0"][0]
        assert np.nonzero(row["kappa64"])[0].tolist() == lit


def test_a_super_line_above_a_strong_transition_of_its_cell_across_a_tile_boundary(ctx):
    """the cell that begins at point TILE: its super-line comes first in the list and lies above the strong nu_0 that follows;
    both reach points of both tiles"""
    boundary = int(round((1000.0 + TILE * sc.DNU) / sc.STEP))
    cells = [(boundary - 2 * 8 - 1, "sw"), (boundary - 8 - 1, "wws"), (boundary, "sww"), (boundary + 8 + 1, "ws")]
    case = sc.layout("tile boundary", cells, grid=(1000.0, sc.DNU, 3 * TILE + 37), seed=10)
    row = check(case, run(ctx, case))[0]
    nu = row["line_params"][0]
    k = int(np.nonzero(nu == (boundary + 0.5) * sc.STEP)[0][0])
    assert nu[k + 1] < nu[k] and np.floor(nu[k + 1] / sc.STEP) == boundary
    assert row["tile_ranges"][0][1] > k + 1 and row["tile_ranges"][1][0] <= k


# ---- launches -------------------------------------------------------------------------------------------------------------------
def test_three_nodes_that_move_transitions_between_the_classes_and_each_node_alone(ctx):
    case = sc.layout("moving", sc.spread(["wmsd" * 10, "m" * 5, "ddd" + "w", "s" * 3, "w" * (B + 7), "mdw" * 30]), seed=4, n_broadeners=2,
                     nodes=[(700.0, 1e5), (1500.0, 1e7), (2500.0, 1e3)])
    batch = check(case, run(ctx, case))
    assert batch[0]["counts"][0] < batch[2]["counts"][0] and batch[0]["kept"] < batch[1]["kept"]
    assert batch[0]["counts"] != batch[1]["counts"]
    alone = run(ctx, case, per=1)
    pairs = run(ctx, case, per=2)
    for node in range(3):
        same_bits(batch[node], alone[node], "node %d alone" % node)
        same_bits(batch[node], pairs[node], "node %d in launches of 2 + 1" % node)
    lean = run(ctx, case, with_fp64=False)
    for node in range(3):
        assert np.array_equal(lean[node]["slabs32"].view(np.uint32), batch[node]["slabs32"].view(np.uint32)), node


def test_the_library_function_on_the_device_under_the_rule(ctx, sizes):
    case = sizes
    timing, host_timing = {}, {}
    args = (case.states, case.trans, case.broadening, ec.q_table(), [700.0], [1e5], case.grid, case.molar_mass, case.cutoff, case.s_min)
    dev = exomol.exomol_opacity(*args, backend="device", ctx=ctx, timing=timing, superline_threshold=case.s_sl, superline_step=case.step)
    host = exomol.exomol_opacity(*args, backend="numpy", timing=host_timing, superline_threshold=case.s_sl, superline_step=case.step)
    r = sc.restated(case, 0)
    ec.check_rule(dev[0, 0], r["ld"], r["f64"], "exomol_opacity on the device")
    ec.check_rule(host[0, 0], r["ld"], r["f64"], "numpy")
    for k in ("kept", "strong", "weak", "superlines"):
        assert np.array_equal(timing[k], host_timing[k]), k
    assert timing["pairs"] == host_timing["pairs"] > 0 and timing["sum_ms"] > 0


# ---- the handle -----------------------------------------------------------------------------------------------------------------
def test_the_handle_drops_keeps_and_refuses(ctx, sizes):
    case = sizes
    node = ([700.0], [1e5], [case.q(700.0)], case.molar_mass, case.cutoff, case.s_min)
    h = exomol.ExomolOpacity(ctx, len(case.states["E"]), len(case.trans["nu0"]), 2, case.grid[2], 1, 1, True)
    try:
        h.set_states(case.states)
        h.set_broadening(*case.broadening)
        with pytest.raises(HeliosHipError, match=r"hx_exomol_set_superlines: no transitions \(hx_exomol_set_transitions\)"):
            h.set_superlines(1e-23, 0.25)
        h.set_transitions(case.trans)
        with pytest.raises(HeliosHipError, match=r"S_sl = nan is not a number >= 0"):
            h.set_superlines(float("nan"), 0.25)
        with pytest.raises(HeliosHipError, match=r"S_sl = -1e-30 is not a number >= 0"):
            h.set_superlines(-1e-30, 0.25)
        with pytest.raises(HeliosHipError, match=r"the step -0\.25 is not a finite number > 0, or 0 for none"):
            h.set_superlines(1e-23, -0.25)
        with pytest.raises(HeliosHipError, match=r"the step inf is not a finite number > 0, or 0 for none"):
            h.set_superlines(1e-23, float("inf"))
        with pytest.raises(HeliosHipError, match=r"the step nan is not a finite number > 0, or 0 for none"):
            h.set_superlines(1e-23, float("nan"))
        with pytest.raises(HeliosHipError, match=r"the step 9.9999999999999995e-08 puts the largest nu_0 = 1\d\d\d\.\d+ into cell "
                                                 r"1\d{10}, cells are numbered below 2\^31"):
            h.set_superlines(1e-23, 1e-7)
        assert h.superlines is None
        h.set_nodes(*(node + case.grid))
        h.run_nodes(0, 1)
        with pytest.raises(HeliosHipError, match=r"no super-lines are set \(hx_exomol_set_superlines\)"):
            h.get("superline_counts")
        plain = h.get("kappa64")[0]
        h.set_superlines(case.s_sl, 2.5)                                              # wider than the cut-off of 2
        with pytest.raises(HeliosHipError, match=r"no nodes \(hx_exomol_set_nodes\)"):
            h.run_nodes(0, 1)
        with pytest.raises(HeliosHipError, match=r"the super-line step 2\.5 is greater than the cut-off 2"):
            h.set_nodes(*(node + case.grid))
        h.set_superlines(case.s_sl, case.step)
        h.set_nodes(*(node + case.grid))
        with pytest.raises(HeliosHipError, match="no nodes have been run"):
            h.get("superline_counts")
        h.run_nodes(0, 1)
        merged, counts = h.get("kappa64")[0], h.get("superline_counts")[0]
        with pytest.raises(HeliosHipError, match="unknown name 'kappa32'"):
            h.get("kappa32")
        h.set_nodes(*(node + case.grid))                                              # set_nodes keeps the setting
        h.run_nodes(0, 1)
        assert np.array_equal(h.get("kappa64")[0].view(np.uint64), merged.view(np.uint64)) and h.superlines == (case.s_sl, case.step)
        h.set_transitions(case.trans)                                                 # set_transitions drops it
        assert h.superlines is None
        h.set_nodes(*(node + case.grid))
        h.run_nodes(0, 1)
        assert np.array_equal(h.get("kappa64")[0].view(np.uint64), plain.view(np.uint64))
        assert int(h.get("kept")[0]) == counts[0] + counts[1]
        with pytest.raises(HeliosHipError, match=r"no super-lines are set"):
            h.get("superline_counts")
        h.set_superlines(case.s_sl, case.step)
        h.set_superlines(0.0, 0.0)                                                    # step 0 turns them off
        h.set_nodes(*(node + case.grid))
        h.run_nodes(0, 1)
        assert np.array_equal(h.get("kappa64")[0].view(np.uint64), plain.view(np.uint64))
        h.set_superlines(case.s_sl, case.step)                                        # a refusal leaves them off and the nodes dropped,
        h.set_nodes(*(node + case.grid))                                              # whichever value it refuses
        h.run_nodes(0, 1)
        for bad in ((float("nan"), case.step), (case.s_sl, -1.0), (case.s_sl, 1e-7)):
            with pytest.raises(HeliosHipError, match="hx_exomol_set_superlines"):
                h.set_superlines(*bad)
            assert h.superlines is None
            with pytest.raises(HeliosHipError, match=r"no nodes \(hx_exomol_set_nodes\)"):
                h.run_nodes(0, 1)
            h.set_nodes(*(node + case.grid))
            h.run_nodes(0, 1)
            with pytest.raises(HeliosHipError, match=r"no super-lines are set"):
                h.get("superline_counts")
            assert h.get("line_params")[0].shape == (4, int(h.get("kept")[0]))
            assert np.array_equal(h.get("kappa64")[0].view(np.uint64), plain.view(np.uint64)), bad
            h.set_superlines(case.s_sl, case.step)
            h.set_nodes(*(node + case.grid))
            h.run_nodes(0, 1)
            assert np.array_equal(h.get("kappa64")[0].view(np.uint64), merged.view(np.uint64)), bad
    finally:
        h.close()
    r = sc.restated(case, 0)
    ec.check_rule(merged, r["ld"], r["f64"], "after the refusals")
    assert tuple(counts) == (len(r["list_f64"]["strong"]), len(r["list_f64"]["weak"]), len(r["list_f64"]["cells"]))
    assert not np.array_equal(merged, plain)


# ---- the tool -------------------------------------------------------------------------------------------------------------------
def test_the_fused_containers_equal_the_two_step_routes_on_the_device(tmp_path, capsys):
    """`exomol.py` then `ktable.py` against `exomol.py -ktable yes`, all on the device with super-lines, four nodes in launches
    of 3 + 1"""
    import exomol as exomol_tool
    import ktable as ktable_tool
    from test_exomol_superlines import kept_lines, tool_case
    wd = str(tmp_path)
    st, tr, entries, pf = ec.write_files(wd, tool_case())
    argv = ["-name", "H2O", "-states", st, "-trans", tr, "-partition_function", pf, "-broadeners", " ".join(entries), "-temperatures",
            "900 300", "-pressure_codes", "p000 n300", "-numax", "2000", "-dnu", "0.05", "-strength_cutoff", "1e-40",
            "-nodes_per_launch", "3", "-superline_threshold", "1e-23", "-superline_step", "0.1"]
    grid = ["-wavelength_grid", "20 6 40", "-number_of_gaussian_points", "8", "-container", "npz", "-temperature_grid", "200 1000 400",
            "-pressure_grid", "2 6 3"]
    files = exomol_tool.main(argv + ["-output_directory", os.path.join(wd, "opac", "H2O")])
    device_lines = kept_lines(capsys.readouterr().out)
    assert len(files) == 4 and all(os.path.getsize(f) == 4 * 40000 for f in files)
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nH2O %s\n" % os.path.join(wd, "opac", "H2O"))
    want = ktable_tool.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-directory_with_individual_files",
                             os.path.join(wd, "two_step")] + grid)
    capsys.readouterr()
    got = exomol_tool.main(argv + ["-ktable", "yes", "-directory_with_individual_files", os.path.join(wd, "fused")] + grid)
    assert [os.path.basename(p) for p in got] == ["H2O_opac_kdistr.npz", "H2O_opac_ip_kdistr.npz"]
    for g, w in zip(got, want):
        with np.load(g) as a, np.load(w) as b:
            assert sorted(a.files) == sorted(b.files)
            for k in b.files:
                assert a[k].tobytes() == b[k].tobytes(), (os.path.basename(g), k)
            assert np.all(np.isfinite(a["kpoints"])) and a["kpoints"].max() > 0
    fused_lines = kept_lines(capsys.readouterr().out)
    assert sorted(fused_lines) == sorted(device_lines) and all(" weak in " in line for line in fused_lines)
    exomol_tool.main(argv + ["-backend", "numpy", "-output_directory", os.path.join(wd, "opac_numpy")])
    assert kept_lines(capsys.readouterr().out) == device_lines                   # one set of classes and cells on both backends
