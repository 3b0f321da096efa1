"""The cases of tests/test_gpu_rad_edges.py without a GPU: under the long-double restatement of tests/rad_cases.py every
case takes the branches its design numbers say, every discrete comparison stays at least 1e-10 from its limit (flags are
discrete, and the device's pow may differ from the host's by an ulp; 1e-10 is the value tests/test_conv_cases.py uses,
1e5 above any such difference -- a condition on the inputs, not a measurement), the CPU oracle agrees with the
restatement within the bounds of the GPU test, and, where it is built, the reference's own rad_temp_iter agrees with the
oracle.  This is what keeps the GPU suite from passing on cases that test nothing."""
import copy

import numpy as np
import pytest

import rad_cases as rc

CASES = rc.all_cases()


@pytest.fixture(scope="module")
def runs():
    cache = {}

    def run(case):
        if case.name not in cache:
            cache[case.name] = rc.restate(case)
        return cache[case.name]
    return run


def test_the_list_covers_what_it_is_meant_to():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    assert {c.L for c in CASES} >= set(rc.SIZES) == {2, 3, 127, 128, 1023, 1024}
    it20 = {c.it for c in CASES if c.adapt == 20 and c.foreplay == 7}
    assert it20 >= {0, 6, 7, 19, 20, 39, 9999, 10000, 10019}
    assert {c.adapt for c in CASES} >= {1, 2, 20}
    assert any(c.foreplay == 10000 and c.it == 10000 for c in CASES)
    assert any(c.tstep != 0 for c in CASES) and any(c.no_atmo == 1 for c in CASES)
    assert any(c.smooth == 1 and (c.p_lay == 1e6).any() and (c.p_lay < 1e6).any() and (c.p_lay > 1e6).any() for c in CASES)
    assert any(c.smooth == 1 and c.p_lay[0] < 1e6 for c in CASES)        # only `i > 0` keeps layer 0 out


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_margin_of_every_comparison(case, runs):
    _out, margins = runs(case)
    assert len(margins) >= 2 * (case.L + 1)
    worst = min(margins, key=lambda t: t[2])
    assert worst[2] >= rc.MARGIN_MIN, "%s at entry %d: %.3e from its limit" % worst


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_branches_the_case_is_named_for(case, runs):
    out, _m = runs(case)
    L, ex = case.L, case.expect
    np.testing.assert_array_equal(out["abort"], ex["abort"])
    assert out["ghost"] == ex["ghost"]
    for k in ("clamp500", "clamp_hi", "clamp_lo", "shrink", "grow"):
        assert out[k] == ex[k], k
    # the prefactor: what the iteration makes of it, then one division or product
    base = np.array(case.pref) if case.base == "keep" else np.full(L + 1, case.base)
    want = base.copy()
    want[ex["shrink"]] = base[ex["shrink"]] / 1.5
    want[ex["grow"]] = base[ex["grow"]] * 1.1
    if case.tstep != 0:
        want = np.array(case.pref)
    np.testing.assert_array_equal(out["pref"], want)
    np.testing.assert_array_equal(out["T_store"], case.T if ex["stores"] else case.T_store)
    if case.tstep == 0 and case.adapt == 1:
        assert ex["stores"] and ex["shrink"] == [i for i in range(L + 1) if i not in case.zero]
    # the step itself: its sign, its size, the clamps
    step = (out["T"] - case.T.astype(rc.LD)).astype(np.float64)
    free = [i for i in range(L + 1) if i not in ex["clamp_hi"] + ex["clamp_lo"] and not (case.no_atmo and i < L)]
    np.testing.assert_allclose(step[free], case.step[free], rtol=1e-6, atol=1e-9)
    assert all(abs(case.step[i]) == 500.0 for i in ex["clamp500"])
    assert all(out["T64"][i] == rc.T_MAX for i in ex["clamp_hi"]) and all(out["T64"][i] == rc.T_MIN for i in ex["clamp_lo"])
    assert all(step[i] == 0 and out["T64"][i] == case.T[i] for i in case.zero)
    if case.no_atmo:
        assert (out["T64"][:L] == rc.T_MIN).all() and out["T64"][L] != rc.T_MIN
    if case.name.startswith("clamp500") and case.it != 19:
        assert ex["clamp500"] == [1, 3] + ([4] if case.name.endswith("501") else [])
        assert [np.sign(case.step[i]) for i in (0, 2)] == ([1, -1] if "_up_" in case.name else [-1, 1])
    if case.name == "T_clamps":
        assert ex["clamp_hi"] == [0, 4] and ex["clamp_lo"] == [2]
    if case.name.startswith("dF_zero"):
        assert case.zero == [0, 1, 2, 4] and case.F_intern == case.F_net[0]
        assert ex["grow"] == ([0, 1, 2, 4] if case.it == 19 else []) and ex["shrink"] == ([3] if case.it == 19 else [])
    if case.name.startswith("conv_"):
        n0 = dict(conv_all=[], conv_but_first=[0], conv_but_last=[L - 1], conv_but_ghost=[L], conv_none=list(range(L + 1)))
        assert [i for i in range(L + 1) if not out["abort"][i]] == n0[case.name]
        assert np.abs(case.heat_sum).min() > 0 and np.abs(case.F_smooth_sum).min() > 0
        assert len(set(case.heat_sum + case.F_smooth_sum)) == L        # a wrong index gives another sum
    if case.name.startswith("ghost_"):
        assert out["ghost"] == (0 if case.name == "ghost_F_net0" else 1)
        assert out["abort"][0] == 1                                     # between 0.5 and 1 local_limit, or the other sign
    if case.tstep != 0:      # the ghost layer reads index 0, and index L - 1 would give another step
        j0, j1 = 0, L - 1
        f = lambda j: case.g / (case.c_p[j] / (case.mmm[j] / rc.pc.AMU)) / (case.p_int[j] - case.p_int[j + 1])
        assert abs(f(j1) / f(j0) - 1) > 0.1
    if case.smooth == 1:
        if case.name in rc.EXPECT_SMOOTHED:
            assert out["smoothed"] == rc.EXPECT_SMOOTHED[case.name]
        fs = out["F_smooth"].astype(np.float64)
        if L >= 8:
            assert (fs > 0).any() and (fs < 0).any() and fs[0] == 0 and fs[L - 1] == 0     # pow(., 7) of both signs
        assert all(fs[i] == 0 for i in range(L) if i not in out["smoothed"])
    if case.L in rc.SIZES and case.name.startswith("L"):
        assert ex["shrink"] and ex["grow"] and 0 < ex["abort"].sum() < L + 1


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_the_cpu_oracle_agrees_with_the_restatement(case, runs, port):
    rc.check_against(rc.run_impl(port, case), case, runs(case)[0], "oracle")


def reference_in_lockstep(ref, case):
    """the reference's rad_temp_iter as a GPU runs one block of it.  With smooth = 1 every layer reads its neighbours'
    temperatures before the block's barrier and writes its own after it; the host build (oracle/ref_driver.cpp) runs one
    emulated thread at a time, so that layer i would read the stepped tlay[i - 1].  As ref_corr_inc_energy does for the
    same kind of kernel, every emulated thread gets the pristine arrays: entry i is taken from a call in which the entries
    before it cannot move (a prefactor of 0, or with a physical time step a mean molecular mass of 0, makes their delta_T
    an exact 0), so that thread i sees the temperatures, and the F_smooth of the layers below it, as they were.  The ghost
    layer reads no temperature but its own, and index 0 of c_p and mmm: it is taken from the call that freezes nothing"""
    if case.smooth != 1:
        return rc.run_impl(ref, case)
    assert case.base == "keep"            # (an iteration that resets the prefactor would undo the freezing)
    out = None
    for i in range(case.L):
        frozen = copy.copy(case)
        frozen.pref, frozen.mmm = np.array(case.pref), np.array(case.mmm)
        frozen.pref[:i] = 0.0
        frozen.mmm[:i] = 0.0
        d = rc.run_impl(ref, frozen)
        np.testing.assert_array_equal(d["T"][:i], case.T[:i])              # the entries before it stood still
        if out is None:
            out = {k: v.copy() for k, v in d.items()}
        for k, v in d.items():
            out[k][i] = v[i]
    return out


def test_the_reference_kernel_agrees_with_the_oracle(port, ref):
    """the reference's own rad_temp_iter (oracle/_ref) against orc_rad_temp_iter on the same cases, in the style of
    test_oracle_stages_vs_ref.py::test_conv_temp_iter.  Left out, and only these: cases with dF == 0 (the reference
    multiplies by an uninitialised value there, the oracle defines delta_T = 0), and smoothing with more than 16
    layers (the reference's barrier is block-local)"""
    compared, left_out = 0, {}
    for case in CASES:
        if case.zero:
            left_out[case.name] = "dF == 0: uninitialised value in the reference"
            continue
        if case.smooth == 1 and case.L > 16:
            left_out[case.name] = "smooth = 1 over more than one block of the reference"
            continue
        a, b = rc.run_impl(port, case), reference_in_lockstep(ref, case)
        for k in ("T", "T_store", "pref", "F_smooth", "F_smooth_sum"):
            np.testing.assert_allclose(b[k], a[k], rtol=1e-13, atol=1e-300, err_msg="%s, %s" % (k, case.name))
        np.testing.assert_allclose(b["F_net_diff"][:case.L], a["F_net_diff"][:case.L], rtol=1e-13, atol=1e-300)
        np.testing.assert_array_equal(b["abort"], a["abort"], err_msg=case.name)
        compared += 1
    assert set(left_out) == {c.name for c in CASES if c.zero or (c.smooth == 1 and c.L > 16)}
    assert compared >= 0.75 * len(CASES), (compared, len(CASES), left_out)
