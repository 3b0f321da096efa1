"""k_exomol_count, _scan, _prepare, _ranges and _sum (csrc/exomol.hip) through hx_exomol and exomol.py on the device, under the rule
of tests/exomol_cases.py: transition counts around the wavefront and the compaction block, kept patterns, point counts around the
tile, the cut-off to the ulp, ties, the gather's edges and several broadeners -- all derived from the constants the module exports;
a batch against its nodes run alone, S_min = 0 against a cut that keeps everything, the tile ranges, and the handle's refusals."""
import numpy as np
import pytest

import exomol_cases as ec
from helios_amd import exomol
from helios_amd._lib import HeliosHipError

pytestmark = pytest.mark.gpu

TILE, B = ec.TILE, ec.B


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def run(ctx, case, per=None, with_fp64=True):
    """([per node: kappa64, slabs32, kept, line_params, tile_ranges], timing_ms) of the case's nodes, `per` per launch"""
    nodes = case.nodes
    per = len(nodes) if per is None else per
    h = exomol.ExomolOpacity.of(ctx, case.states, case.trans, case.broadening, case.grid[2], per, len(nodes), with_fp64)
    rows = []
    try:
        h.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], [case.q(n[0]) for n in nodes], case.molar_mass, case.cutoff,
                    case.s_min, *case.grid)
        for first in range(0, len(nodes), per):
            n = min(per, len(nodes) - first)
            h.run_nodes(first, n)
            k64 = h.get("kappa64") if with_fp64 else [None] * n
            k32, kept, prm, ranges = h.get("slabs32"), h.get("kept"), h.get("line_params"), h.get("tile_ranges")
            assert k32.shape == (n, case.grid[2]) and k32.dtype == np.float32 and kept.shape == (n,) and len(prm) == n
            for r in range(n):
                assert prm[r].shape == (4, kept[r])
                rows.append({"kappa64": k64[r], "slabs32": k32[r], "kept": int(kept[r]), "line_params": prm[r], "tile_ranges": ranges[r]})
        timing = h.get("timing_ms")
    finally:
        h.close()
    assert timing.shape == (2,) and timing[0] > 0 and timing[1] > 0
    return rows, timing


def check_ranges(case, row, label):
    """a tile's range holds every kept transition that the per-point test passes for one of the tile's points, and none beyond
    the cut-off widened as lines_tile_ranges widens it"""
    nu_first, dnu, n_points = case.grid
    nu = nu_first + np.arange(n_points, dtype=np.float64) * dnu
    nu0, ranges = row["line_params"][0], row["tile_ranges"]
    widen = case.cutoff * (1.0 + exomol.RANGE_WIDEN[0]) + exomol.RANGE_WIDEN[1]
    assert ranges.shape == (-(-n_points // TILE), 2), label
    for t, (lo, hi) in enumerate(ranges):
        pts = nu[t * TILE:(t + 1) * TILE]
        assert 0 <= lo <= hi <= row["kept"], (label, t, lo, hi)
        reached = np.nonzero((np.abs(pts[:, None] - nu0[None, :]) <= case.cutoff).any(axis=0))[0]
        assert np.all((reached >= lo) & (reached < hi)), (label, t, lo, hi, reached[:3], reached[-3:])
        inside = nu0[lo:hi]
        assert np.all((inside >= pts[0] - widen) & (inside <= pts[-1] + widen)), (label, t, lo, hi)


def check(case, rows):
    """every node of the case against its restatement; returns the rows"""
    assert len(rows) == len(case.nodes)
    for node, row in enumerate(rows):
        label = "%s, node %d" % (case.label, node)
        r = ec.restated(case, node)
        assert row["kept"] == len(r["kept"]), (label, row["kept"], len(r["kept"]))
        assert np.array_equal(row["line_params"][0], case.trans["nu0"][r["kept"]]), label
        if row["kept"]:
            ec.check_rule(row["line_params"], r["params_ld"], r["params_f64"], label + ", line_params")
        else:
            assert not row["kappa64"].any() and not row["slabs32"].any(), label
        ec.check_rule(row["kappa64"], r["ld"], r["f64"], label + ", kappa64")
        with np.errstate(over="ignore"):
            assert np.array_equal(row["slabs32"].view(np.uint32), row["kappa64"].astype(np.float32).view(np.uint32)), label
        check_ranges(case, row, label)
    return rows


def same_bits(a, b, label):
    assert a["kept"] == b["kept"], label
    for k in ("kappa64", "line_params"):
        assert np.array_equal(a[k].view(np.uint64), b[k].view(np.uint64)), (label, k)
    assert np.array_equal(a["slabs32"].view(np.uint32), b["slabs32"].view(np.uint32)), label
    assert np.array_equal(a["tile_ranges"], b["tile_ranges"]), label


# ---- the case list: counts, patterns, grid sizes, broadeners ------------------------------------------------------------------
@pytest.mark.parametrize("label", ec.case_labels())
def test_the_cases_under_the_rule(ctx, label):
    case = ec.make(label)
    rows = check(case, run(ctx, case)[0])
    kind, _, what = label.partition(": ")
    if kind == "pattern":
        n = 2 * B + 1
        want = {"none": 0, "first": 1, "last": 1, "all": n, "alternating": B + 1, "run across a block boundary": 20,
                "a kept block beside a culled block": B + 1}[what]
        assert rows[0]["kept"] == want
        if what in ("first", "last"):
            assert rows[0]["line_params"][0, 0] == case.trans["nu0"][0 if what == "first" else -1]
    if kind == "broadeners":
        assert rows[1]["kept"] == B + 1 > rows[0]["kept"]                    # the hot node keeps what the cold one culls


def test_the_gathers_edges_are_in_the_cases():
    """the last transition's upper state is the table's last state, a kept lower state has the table's last jidx, and kept lower
    states lie beyond the `.broad` rows' last J''"""
    case = ec.make("pattern: all")
    n_states = len(case.states["E"])
    jx = case.states["jidx"][case.trans["low"]]
    assert int(case.trans["up"][-1]) == n_states - 1 and int(jx.max()) == case.broadening[1].shape[1] - 1 == int(2 * ec.J_TOP)
    assert np.count_nonzero(jx > int(2 * ec.J_FILE)) > 10
    beyond = case.broadening[1][0, int(2 * ec.J_FILE) + 1:]
    assert np.all(beyond == [0.07, 0.5])


# ---- placements ---------------------------------------------------------------------------------------------------------------
def test_a_line_on_a_point_and_one_ulp_beside_it_with_the_cut_off_at_a_point_distance(ctx):
    """nu_0 = 100 on point 400 of a grid of step 1/4: the points at 75 and 125 lie exactly C = 25 away and are in; with nu_0 one
    ulp below 100 the point at 125 is out and the one at 75 stays in"""
    case = ec.two_states_case(100.0)
    row = check(case, run(ctx, case)[0])[0]
    assert row["line_params"][0, 0] == 100.0 and int(np.argmax(row["kappa64"])) == 400
    assert np.nonzero(row["kappa64"])[0].tolist() == list(range(300, 501))
    below = float(np.nextafter(100.0, 0.0))
    case = ec.two_states_case(below)
    row = check(case, run(ctx, case)[0])[0]
    assert row["line_params"][0, 0] == below and 125.0 - below > 25.0
    assert np.nonzero(row["kappa64"])[0].tolist() == list(range(300, 500))


def test_ties_in_both_file_orders(ctx):
    rows = []
    for first in (True, False):
        case, _ = ec.tie_case(first)
        rows.append(check(case, run(ctx, case)[0])[0])
    a, b = rows
    assert a["kept"] == b["kept"] == 5 and np.array_equal(a["line_params"][0], b["line_params"][0])
    assert np.array_equal(a["line_params"][1, [0, 1, 2, 3]], b["line_params"][1, [1, 0, 3, 2]])      # each pair in the other order
    assert not np.array_equal(a["line_params"][1], b["line_params"][1])


# ---- launches -------------------------------------------------------------------------------------------------------------------
def test_a_row_of_a_batch_equals_the_row_of_the_node_run_alone(ctx):
    """seven nodes that mix temperatures and pressures, in launches of 3 + 3 + 1, against every node in a launch of its own"""
    nodes = [(500.0, 1e3), (700.0, 1e7), (1500.0, 1e5), (700.0, 1e3), (2500.0, 1e7), (500.0, 1e5), (1500.0, 1e3)]
    case = ec.build("seven nodes", ec.pattern("alternating", 2 * B + 1), grid=(1000.0, ec.DNU, TILE + 37), seed=7, n_broadeners=2,
                    nodes=nodes)
    batch = check(case, run(ctx, case, per=3)[0])
    alone = run(ctx, case, per=1)[0]
    for node in range(7):
        same_bits(batch[node], alone[node], "node %d" % node)
    assert len(set(row["kept"] for row in batch)) > 1
    lean = run(ctx, case, per=3, with_fp64=False)[0]                           # the handle without fp64 rows: the same slabs
    for node in range(7):
        assert np.array_equal(lean[node]["slabs32"].view(np.uint32), batch[node]["slabs32"].view(np.uint32)), node


def test_no_cut_equals_a_cut_below_every_strength(ctx):
    case = ec.build("no cut", ec.pattern("all", 2 * B + 1), seed=11, n_broadeners=3, s_min=0.0)
    assert float(exomol.strengths(case.states, case.trans, 700.0, case.q(700.0)).min()) > 1e-40
    without = check(case, run(ctx, case)[0])[0]
    low = case.with_s_min(1e-60)
    same_bits(without, check(low, run(ctx, low)[0])[0], "S_min = 0 against 1e-60")
    assert without["kept"] == 2 * B + 1


def test_the_library_function_on_the_device_equals_the_numpy_backend_under_the_rule(ctx):
    case = ec.make("broadeners: 3")
    temps, press = [700.0, 1500.0], [1e5, 1e7]
    args = (case.states, case.trans, case.broadening, ec.q_table(), temps, press, case.grid, case.molar_mass, case.cutoff, case.s_min)
    timing = {}
    dev = exomol.exomol_opacity(*args, backend="device", ctx=ctx, nodes_per_launch=3, timing=timing)
    host_timing = {}
    host = exomol.exomol_opacity(*args, backend="numpy", timing=host_timing)
    assert dev.shape == host.shape == (2, 2, case.grid[2]) and timing["sum_ms"] > 0 and timing["pairs"] == host_timing["pairs"] > 0
    assert np.array_equal(timing["kept"], host_timing["kept"]) and timing["kept"][1, 0] > timing["kept"][0, 0]
    for it, t in enumerate(temps):
        for jp, p in enumerate(press):
            node = ec.Case("library function", case.states, case.raw, case.broadeners, [(t, p)], case.s_min, case.grid, case.cutoff)
            r = ec.restated(node, 0)
            ec.check_rule(dev[it, jp], r["ld"], r["f64"], "exomol_opacity on the device at %g K, %g" % (t, p))
            ec.check_rule(host[it, jp], r["ld"], r["f64"], "numpy at %g K, %g" % (t, p))


@pytest.mark.parametrize("superlines", [None, (1e-22, 0.25)])
def test_a_handle_made_for_fewer_nodes_takes_them_in_turns(ctx, superlines):
    """three nodes through a handle made for two, two per launch: turns of 2 + 1 and a short last launch, on ec.GRID's one full
    tile and one point.  Bit for bit what the same call gives with a handle of its own, which takes the three in one turn, and
    the same counts per node; the handle given stays open and is set to the call's super-lines.  The list is the smallest of
    the cases that the cut divides: 63 transitions, 32 of them kept at 700 K and all of them in the hotter nodes; under
    S_sl = 1e-22 every node has strong and weak transitions, and a cell that merges two"""
    case = ec.make("count: 63")
    assert case.grid == ec.GRID and case.grid[2] == TILE + 1
    more = {} if superlines is None else {"superline_threshold": superlines[0], "superline_step": superlines[1]}
    args = (case.states, case.trans, case.broadening, ec.q_table(), [700.0, 1500.0, 2500.0], [1e5], case.grid, case.molar_mass,
            case.cutoff, case.s_min)
    own, turns = {}, {}
    want = exomol.exomol_opacity(*args, backend="device", ctx=ctx, timing=own, **more)
    h = exomol.ExomolOpacity.of(ctx, case.states, case.trans, case.broadening, TILE + 1, 2, 2, True)
    try:
        got = exomol.exomol_opacity(*args, backend="device", ctx=ctx, handle=h, timing=turns, **more)
        assert h.handle and h.n_nodes == 1 and h.rows_run == 1 and h.superlines == superlines
    finally:
        h.close()
    assert got.shape == (3, 1, TILE + 1) and np.all(np.count_nonzero(got, axis=2) > 400)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    assert turns["kept"].reshape(-1).tolist() == own["kept"].reshape(-1).tolist() == [32, 63, 63]
    assert turns["pairs"] == own["pairs"] > 0 and turns["sum_ms"] > 0 and own["sum_ms"] > 0
    if superlines is None:
        assert "weak" not in turns and "weak" not in own
    else:
        for k in ("strong", "weak", "superlines"):
            assert np.array_equal(turns[k], own[k]), k
        assert np.all(turns["strong"] > 0) and np.all(turns["superlines"] > 0) and np.any(turns["weak"] > turns["superlines"])
        assert np.array_equal(turns["strong"] + turns["weak"], turns["kept"])


# ---- the handle -----------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_counts_and_leave_the_handle_usable(ctx):
    case = ec.make("count: 65")
    n_states, n_trans, n_points = len(case.states["E"]), 65, case.grid[2]
    node = ([700.0], [1e5], [case.q(700.0)], case.molar_mass, case.cutoff, case.s_min)
    small = exomol.ExomolOpacity(ctx, n_states - 1, n_trans, 1, n_points, 1, 1)
    try:
        with pytest.raises(HeliosHipError, match=r"%d states, the handle holds 1 \.\.\. %d" % (n_states, n_states - 1)) as e:
            small.set_states(case.states)
        assert "status 1:" in str(e.value)
        with pytest.raises(HeliosHipError, match=r"no states \(hx_exomol_set_states\)"):
            small.set_transitions(case.trans)
    finally:
        small.close()
    h = exomol.ExomolOpacity(ctx, n_states, n_trans - 1, 1, n_points, 2, 3, True)
    try:
        h.set_states(case.states)
        with pytest.raises(HeliosHipError, match=r"65 transitions, the handle holds 1 \.\.\. 64"):
            h.set_transitions(case.trans)
        fewer = dict((k, case.trans[k][:64]) for k in case.trans)
        with pytest.raises(HeliosHipError, match=r"2 broadeners, the handle holds 1 \.\.\. 1"):
            h.set_broadening(*exomol.broadening_table(ec.broadeners(2), int(case.states["jidx"].max())))
        with pytest.raises(HeliosHipError, match=r"30 rows per broadener, the states' largest 2 J = 31 needs 32"):
            h.set_broadening(case.broadening[0], case.broadening[1][:, :30])
        h.set_broadening(*case.broadening)
        unsorted = dict((k, fewer[k][::-1].copy()) for k in fewer)
        with pytest.raises(HeliosHipError, match=r"transition 1: nu_0 = .* lies below transition 0's .*: the list is sorted"):
            h.set_transitions(unsorted)
        outside = dict(fewer, up=fewer["up"].copy())
        outside["up"][5] = n_states
        with pytest.raises(HeliosHipError, match=r"transition 5: states %d -> %d, the table holds 0 \.\.\. %d"
                           % (n_states, fewer["low"][5], n_states - 1)):
            h.set_transitions(outside)
        downward = dict(fewer, up=fewer["low"].copy(), low=fewer["up"].copy())
        with pytest.raises(HeliosHipError, match=r"transition 0: nu_0 = -.* is not > 0"):
            h.set_transitions(downward)
        negative = dict(fewer, A=-fewer["A"])
        with pytest.raises(HeliosHipError, match=r"transition 0: A = -.* is not a finite number >= 0"):
            h.set_transitions(negative)
        with pytest.raises(HeliosHipError, match=r"no transitions \(hx_exomol_set_transitions\)"):
            h.set_nodes(*(node + case.grid))
        h.set_transitions(fewer)
        with pytest.raises(HeliosHipError, match=r"no nodes \(hx_exomol_set_nodes\)"):
            h.run_nodes(0, 1)
        with pytest.raises(HeliosHipError, match=r"%d spectral points, the handle holds 1 \.\.\. %d" % (n_points + 1, n_points)):
            h.set_nodes(*(node + (case.grid[0], case.grid[1], n_points + 1)))
        with pytest.raises(HeliosHipError, match=r"4 nodes, the handle holds 1 \.\.\. 3"):
            h.set_nodes(*(([700.0] * 4, [1e5] * 4, [case.q(700.0)] * 4) + node[3:] + case.grid))
        with pytest.raises(HeliosHipError, match=r"node 1: T = -700 is not a finite number > 0"):
            h.set_nodes(*(([700.0, -700.0], [1e5] * 2, [case.q(700.0)] * 2) + node[3:] + case.grid))
        with pytest.raises(HeliosHipError, match=r"S_min = -1 is not a finite number >= 0"):
            h.set_nodes(*(node[:5] + (-1.0,) + case.grid))
        h.set_nodes(*(([700.0, 900.0], [1e5] * 2, [case.q(700.0), case.q(900.0)]) + node[3:] + case.grid))
        with pytest.raises(HeliosHipError, match="no nodes have been run"):
            h.get("kappa64")
        with pytest.raises(HeliosHipError, match="no nodes have been run"):
            h.get("line_params")
        with pytest.raises(HeliosHipError, match=r"nodes 1 \.\.\. 2, hx_exomol_set_nodes gave 0 \.\.\. 1"):
            h.run_nodes(1, 2)
        with pytest.raises(HeliosHipError, match=r"3 nodes in one call, the handle holds 1 \.\.\. 2 per launch"):
            h.run_nodes(0, 3)
        with pytest.raises(HeliosHipError, match="unknown name 'kappa32'"):
            h.get("kappa32")
        h.run_nodes(0, 1)
        got, kept = h.get("kappa64")[0], int(h.get("kept")[0])
    finally:
        h.close()
    first = ec.Case("after the refusals", case.states, tuple(case.trans[k][:64] for k in ("up", "low", "A")), case.broadeners, [ec.NODE],
                    case.s_min, case.grid, case.cutoff)
    r = ec.restated(first, 0)
    assert kept == len(r["kept"])
    ec.check_rule(got, r["ld"], r["f64"], "after the refusals")
    lean = exomol.ExomolOpacity.of(ctx, case.states, case.trans, case.broadening, n_points, 1, 1)
    try:
        lean.set_nodes(*(node + case.grid))
        lean.run_nodes(0, 1)
        with pytest.raises(HeliosHipError, match="the handle keeps no fp64 rows"):
            lean.get("kappa64")
    finally:
        lean.close()
