"""hx_lines has one path, nodes per launch, where it had a single-node path beside it.  What the single-node kernels and the node
kernels gave on the commit before (8102017) was recorded on an MI355X into tests/golden/lines/parent_bits.npz, for the cases
of lines_cases.parent_bit_cases(); the one path gives the same bits.  The two sum kernels give the same slabs, and a handle made
for fewer nodes takes a call's nodes in turns."""
import numpy as np
import pytest

import lines_cases as lc
from helios_amd import lines
from helios_amd._lib import HeliosHipError

pytestmark = pytest.mark.gpu

CASES = dict((c["name"], c) for c in lc.parent_bit_cases())


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def same_bits(got, want, label):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (label, got.dtype, want.dtype, got.shape, want.shape)
    assert got.tobytes() == want.tobytes(), (label, int(np.count_nonzero(got != want)))


def in_launches(ctx, case, with_fp64):
    """{name: rows of every node} of the case through a handle of the case's sizes, launch after launch"""
    line, nodes, grid, per = case["line"], case["nodes"], case["grid"], case["per_launch"]
    q = lc.q_table()
    names = ("slabs32", "kappa64", "line_params") if with_fp64 else ("slabs32",)
    h = lines.LineOpacity(ctx, len(line["nu0"]) + case["more_lines"], grid[2] + case["more_points"], per, len(nodes), with_fp64)
    try:
        h.set_lines(line)
        h.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], [lines.partition_value(q, n[0]) for n in nodes],
                    lines.partition_value(q, 296.0), lc.M_H2O, case["x_self"], case["cutoff"], *grid)
        rows = dict((k, []) for k in names)
        for first in range(0, len(nodes), per):
            h.run_nodes(first, min(per, len(nodes) - first))
            for k in names:
                rows[k].append(h.get(k))
        if not with_fp64:
            with pytest.raises(HeliosHipError, match="the handle keeps no fp64 rows"):
                h.get("kappa64")
        return dict((k, np.concatenate(v)) for k, v in rows.items())
    finally:
        h.close()


@pytest.mark.parametrize("name", ["case1", "case2", "case3"])
def test_the_bits_of_the_commit_before(ctx, name):
    """rows of a handle with fp64 rows against what hx_lines_run gave node by node; slabs of a plain handle against what
    hx_lines_run_nodes gave"""
    case, want = CASES[name], lc.parent_bits()
    got = in_launches(ctx, case, True)
    same_bits(got["kappa64"], want[name + "_kappa64"], name + ", kappa64")
    same_bits(got["slabs32"], want[name + "_kappa32"], name + ", slabs32 beside the fp64 rows")
    same_bits(got["line_params"], want[name + "_line_params"], name + ", line_params")
    if name + "_slabs32" in want:
        same_bits(in_launches(ctx, case, False)["slabs32"], want[name + "_slabs32"], name + ", slabs32 of a plain handle")
    assert np.count_nonzero(got["kappa64"]) > 0


@pytest.mark.parametrize("per_launch", [4, 3])
def test_line_opacity_gives_the_bits_of_the_commit_before(ctx, per_launch):
    """2 x 2 nodes in one launch, and in turns of 3 + 1"""
    case, want = CASES["case4"], lc.parent_bits()
    timing = {}
    got = lines.line_opacity(case["line"], lc.q_table(), case["temps"], case["press"], case["grid"], lc.M_H2O, case["x_self"],
                             case["cutoff"], backend="device", ctx=ctx, nodes_per_launch=per_launch, timing=timing)
    same_bits(got, want["case4_kappa64"], "line_opacity, %d nodes per launch" % per_launch)
    assert timing["pairs"] == int(want["case4_pairs"]) > 0 and timing["sum_ms"] > 0 and timing["prepare_ms"] > 0


def test_the_two_sum_kernels_give_the_same_slabs(ctx):
    """case 2: two tiles with the last one partial, two LDS blocks, strides other than the counts, launches of 2 + 1 nodes"""
    plain, fp64 = in_launches(ctx, CASES["case2"], False), in_launches(ctx, CASES["case2"], True)
    same_bits(plain["slabs32"], fp64["slabs32"], "k_lines_sum_nodes against k_lines_sum_nodes_fp64")
    with np.errstate(over="ignore"):
        same_bits(fp64["slabs32"], fp64["kappa64"].astype(np.float32), "a slab is its fp64 row rounded once")


def test_a_handle_made_for_fewer_nodes_takes_them_in_turns(ctx):
    """three nodes through a handle made for two nodes and one per launch: turns of 2 + 1, on case 2's list and grid.  Bit for
    bit what the same call gives with a handle of its own, which takes the three in one launch; the handle given stays open"""
    case = CASES["case2"]
    line = lines.sort_lines(case["line"])
    temps, press = [300.0, 900.0, 1500.0], [1e5]
    args = (lc.q_table(), temps, press, case["grid"], lc.M_H2O, case["x_self"], case["cutoff"])
    own, turns = {}, {}
    want = lines.line_opacity(line, *args, backend="device", ctx=ctx, timing=own)
    h = lines.LineOpacity.of(ctx, line, case["grid"][2], 1, 2, True)
    try:
        got = lines.line_opacity(line, *args, backend="device", ctx=ctx, handle=h, timing=turns)
        assert h.handle and h.n_nodes == 1 and h.rows_run == 1               # left open, after the turn of one node
    finally:
        h.close()
    assert got.shape == (3, 1, case["grid"][2]) and len({row.tobytes() for row in got[:, 0]}) == 3
    same_bits(got, want, "in turns")
    assert turns["pairs"] == own["pairs"] > 0 and turns["sum_ms"] > 0 and own["sum_ms"] > 0
