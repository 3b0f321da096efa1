"""The cases of tests/test_gpu_conv_edges.py on helios_amd/host_functions.py alone: every case keeps every discrete
comparison at least 1e-10 from its limit (flags are discrete, and the device's pow may differ from numpy's by an ulp),
and has the structure it is named for.  This is what keeps the GPU suite from passing on cases that test nothing."""
import numpy as np
import pytest

import conv_cases as cc
from helios_amd import host_functions as hs

CASES = cc.all_cases()


def zones_of(flags, L):
    s, e = hs._zones([bool(v) for v in flags], L)
    return list(zip(s, e))


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def run(case):
        if case.name not in cache:
            c, F_up, F_down, F_net, mmm = cc.host_inputs(case)
            q = cc.make_quant(case, c, case.T, F_up, F_down, F_net, mmm)
            rec = cc.run_host(q)
            cache[case.name] = (q, rec)
        return cache[case.name]
    return run


def test_case_names_are_unique_and_the_list_is_complete():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    have = {c.L for c in cc.adjust_cases()}
    assert {2, 3, 8, 63, 64, 65, 66, 127, 128, 129, 255, 256, 257, 313, 314} <= have
    assert cc.conv_smem_bytes(313) <= 48 * 1024 < cc.conv_smem_bytes(314)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_margin_of_every_comparison(case, runs):
    q, rec = runs(case)
    assert rec.n_compare > 0
    assert rec.margin >= cc.MARGIN_MIN, "adiabat / surface comparison %.3e from its limit" % rec.margin
    assert rec.kink >= cc.MARGIN_MIN, "kink rule: neighbours %.3e apart" % rec.kink
    # the marking of the second half-step sees the adjusted profile: the same margin there
    q2 = cc.make_quant(case, cc.base_case(case.L, case.regime, case.k, case.T_star), q.T_lay, q.F_up_tot, q.F_down_tot,
                       q.F_net, q.meanmolmass_lay, conv_layer=q.conv_layer)
    with cc.recording(q2) as rec2:
        hs.mark_convective_layers(q2, stitching=1)
    assert rec2.margin >= cc.MARGIN_MIN and rec2.kink >= cc.MARGIN_MIN


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_structure_the_case_is_named_for(case, runs):
    q, rec = runs(case)
    L, ex = case.L, case.expect
    starts, ends = rec.zones[-1]
    final = list(zip(starts, ends))
    assert final == case.expect_zones
    assert max([e - max(s, 0) + 1 for s, e in final] or [0]) == case.n_max
    if "start" in ex:
        assert ex["start"] in starts
    if "end" in ex:
        assert ex["end"] in ends
    if "nzones" in ex:
        assert len(final) == ex["nzones"]
    if "min_zones" in ex:
        assert len(final) >= ex["min_zones"] and len(final) > 64      # starts / ends fill over more than one ballot round
        rounds = -(-(L + 1) // 64)                                     # the walk covers layers -1 .. L - 1, 64 a round
        assert rounds >= 4 and max(ends) >= 64 * (rounds - 1) - 1      # ... and boundaries turn up in the last one
    if "min_longest" in ex:
        assert case.n_max >= ex["min_longest"]
    if "lim" in ex:
        assert cc.find_lim(case.p_lay) == ex["lim"]
        if case.regime == "high":
            assert (case.p_lay > 10).all()
        if case.regime == "low":
            assert (case.p_lay <= 10).all()
        if case.regime == "break":
            assert case.p_lay[case.k - 1] > 10 >= case.p_lay[case.k] and 0 < case.k < L - 1
    if "stale" in ex:
        lim = cc.find_lim(case.p_lay)
        assert all(j > lim and case.conv_layer0[j] == 1 and q.conv_layer[j] == 1 for j in ex["stale"])
        assert all(j in {i for s, e in final for i in range(s, e + 1)} for j in ex["stale"])
    if "ignored" in ex or case.steep:
        for a, b in case.steep:
            for i in range(a, b):       # super-adiabatic by a wide margin, above the break, not flagged, not touched
                assert case.p_lay[i] <= 10
                assert case.T[i + 1] < 0.99 * case.T[i] * (case.p_lay[i + 1] / case.p_lay[i]) ** cc.KAPPA
            assert not q.conv_unstable[a:b + 1].any() and not q.conv_layer[a:b + 1].any()
            np.testing.assert_array_equal(q.T_lay[a:b + 1], case.T[a:b + 1])
    if ex.get("untouched"):
        np.testing.assert_array_equal(q.T_lay, case.T)
        assert not q.conv_layer.any() and not q.conv_unstable.any()
    else:
        assert np.abs(q.T_lay / case.T - 1.0).max() > 1e-9 or case.n_max <= 1
    if "stitch" in ex:
        stitching, before, after = rec.layers[-1]
        assert stitching == 1
        zb = zones_of(before, L)
        assert len(zb) == 3
        gaps = [case.p_lay[zb[n + 1][0]] / case.p_lay[zb[n][1]] for n in range(2)]
        assert sum(g > 1 / np.e for g in gaps) == 1 and gaps[0] > 1 / np.e > gaps[1]
        if ex["stitch"]:
            assert case.it == 5001 and len(zones_of(after, L)) == 2 and after[11] == after[12] == 1
        else:
            assert case.it == 5000 and np.array_equal(before, after)
    if "tests" in ex:
        assert rec.tests == ex["tests"]
        for n, (branch, outcome) in enumerate(zip(ex["branches"], ex["outcomes"])):
            if branch == "gap":
                assert case.p_lay[starts[n + 1]] / case.p_lay[ends[n]] < 1 / np.e
                assert rec.tests[n] == int((ends[n] + starts[n + 1]) / 2) and rec.below[n] == rec.tests[n] - 1
            elif branch == "top":
                assert n == len(final) - 1 and rec.tests[n] == int(0.8 * ends[n] + 0.2 * L)
            elif branch == "wrap":
                assert rec.tests[n] == 0 and rec.below[n] == -1        # numpy wraps it to L - 1
                assert abs(q.F_add_heat_sum[L - 1]) > 0.05 * q.F_intern
            f = rec.fudge[n]
            if outcome == "lo":
                assert f == 0.99 and not rec.nan[n]
            elif outcome == "hi":
                assert f == 1.01
            elif outcome == "mid":
                assert 0.99 + 1e-5 < f < 1.01 - 1e-5 and abs(f - 1) > 1e-5
            elif outcome == "nan":
                assert rec.nan[n] and f == 0.99
        if case.dampara <= 0:
            want = [0.5, 4.0] if case.T_star > 10 else [8.0, 8.0]
            assert rec.dampara == want[-len(rec.dampara):]
        else:
            assert rec.dampara == [2.5] * len(rec.dampara)


def test_the_surface_always_brings_layer_0():
    """why no case has `ends = -1`: both rules set the surface entry and layer 0 together"""
    for case in CASES:
        if case.surface:
            assert case.expect_zones[0][0] == -1 and case.expect_zones[0][1] >= 0
    alone = [c for c in CASES if c.expect_zones[:1] == [(-1, 0)]]
    merged = [c for c in CASES if c.expect_zones and c.expect_zones[0][0] == -1 and c.expect_zones[0][1] > 0]
    assert alone and merged


def test_batch_columns_differ():
    cols = cc.batch_columns()
    assert len(cols) == 3 and len({c.L for c in cols}) == 1
    assert not np.array_equal(cols[0].T, cols[1].T) and not np.array_equal(cols[1].T, cols[2].T)
