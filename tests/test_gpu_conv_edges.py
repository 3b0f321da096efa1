"""The two convection half-steps of the device loop -- k_rt_conv_adjust and k_rt_totals_c (csrc/rt_kernels.h) with the
workgroup-cooperative code of csrc/conv_adjust.h -- at their edges, against helios_amd/host_functions.py on IDENTICAL
inputs: zone boundaries on both sides of a 64-lane ballot round, more zones than one round compacts, more layers than
one pass of the 256 / 1024 thread strides and of the 256-wide totals loop, both sides of the 48 KB dynamic-LDS line
(L = 313 / 314), the three regimes of the `p_lay <= 10` break with stale flags above it, stitching at 5000 / 5001, every
branch of the flux-test index and of the fudge factor under every choice of the damping parameter, and a three-column
batch with a finished column in the middle.  The cases are tests/conv_cases.py; tests/test_conv_cases.py proves without
a GPU that each has the structure it is named for, and every run here asserts again, on what the device really saw,
that no discrete comparison is closer than 1e-10 to its limit.

Bounds.  Flags: exact.  Adjusted T_lay: rtol = max(1e-13, 4 (n_max + 2) 2^-53), n_max the longest zone (both sides do
the same operations in the same order and differ in pow alone).  Entries outside every zone, and a finished column: bit
for bit.  Wavelength totals: (nbin ny + 16) 2^-52 relative against the long-double sum (every term is non-negative).
Temperature step: the rtols of test_convection_steps_on_device_match_host_functions.

With the environment variable CONV_EDGES_JSON set, the largest deviations per layer count go into the file it names."""
import ctypes
import json
import os

import numpy as np
import pytest

import conv_cases as cc
from helios_amd import host_functions as hs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


@pytest.fixture(scope="module")
def batches(ctx):
    """one batch per (L, pressure grid, T_star[, columns]), shared by the cases on it: every case sets all it reads"""
    from helios_amd.rt import batch_from_case
    have = {}

    def get(case, ncol=1):
        key = case.batch_key() + (ncol,)
        if key not in have:
            c = cc.base_case(case.L, case.regime, case.k, case.T_star)
            rt = batch_from_case(ctx, c, ncol=ncol)
            have[key] = (rt, c)
            rt.set_state(-1, "kappa_lay", np.full(case.L, cc.KAPPA))
            rt.set_state(-1, "kappa_int", np.full(case.L + 1, cc.KAPPA))
            rt.set_state(-1, "dampara", np.array([-1.0]))
            rt.build_planck_table(1 if c.T_star > 10 else 0)
            rt.conv_advance(0)                      # F_net, F_up_tot, F_down_tot hold real fluxes from here on
        return have[key]
    yield get
    for rt, _c in have.values():
        rt.close()


def record(L, what, value):
    print("L = %d  %s: %.3e" % (L, what, value))
    path = os.environ.get("CONV_EDGES_JSON")
    if path:
        have = json.load(open(path)) if os.path.exists(path) else {}
        key = "%d %s" % (L, what)
        have[key] = max(float(value), have.get(key, 0.0))
        json.dump(have, open(path, "w"), indent=1, sort_keys=True)


def h2d(ctx, rt, name, col, array):
    """a chosen array into the batch's device memory through the library's own copy"""
    a = np.ascontiguousarray(array, np.float64)
    ctx.check(ctx._l.hx_h2d(ctx.handle, rt.device_ptr(name, col), a.ctypes.data_as(ctypes.c_void_p), a.nbytes), "hx_h2d")


def prepare(ctx, rt, c, case, col=0, done=0):
    L = case.L
    rt.set_temperatures(col, case.T)
    rt.set_state(col, "kappa_lay", np.full(L, cc.KAPPA))
    rt.set_state(col, "kappa_int", np.full(L + 1, cc.KAPPA))
    rt.set_state(col, "c_p_lay", np.asarray(c.c_p_lay, np.float64))
    rt.set_state(col, "conv_layer", case.conv_layer0)
    rt.set_state(col, "conv_unstable", case.conv_unstable0)
    rt.set_state(col, "dampara", np.array([case.dampara]))
    rt.set_state(col, "done", np.array([done], np.int32))
    rt.set_column_heating(col, np.zeros(L), np.zeros(L) if case.heat_sum is None else case.heat_sum)
    if case.fluxes:
        F_up, F_down = cc.apply_fluxes(case, rt.get("F_up_tot", col), rt.get("F_down_tot", col), c.F_intern)
        h2d(ctx, rt, "F_up_tot", col, F_up)
        h2d(ctx, rt, "F_down_tot", col, F_down)


def adjust_against_host(rt, c, case, col=0):
    """conv_adjust(case.it) on column `col` against hs.convective_adjustment on what the device saw"""
    L = case.L
    seen = {n: rt.get(n, col) for n in ("T_lay", "F_net", "F_up_tot", "F_down_tot", "F_smooth_sum", "F_add_heat_sum",
                                        "conv_layer", "conv_unstable")}
    np.testing.assert_array_equal(seen["T_lay"], case.T)
    np.testing.assert_array_equal(seen["conv_layer"], case.conv_layer0)
    rt.conv_adjust(case.it)
    mmm = rt.get("meanmolmass_lay", col)                       # what the adjustment saw on the device
    q = cc.make_quant(case, c, seen["T_lay"], seen["F_up_tot"], seen["F_down_tot"], seen["F_net"], mmm,
                      conv_layer=seen["conv_layer"], conv_unstable=seen["conv_unstable"],
                      F_smooth_sum=seen["F_smooth_sum"])
    q.F_add_heat_sum = seen["F_add_heat_sum"].copy()
    rec = cc.run_host(q)
    assert rec.margin >= cc.MARGIN_MIN and rec.kink >= cc.MARGIN_MIN, (rec.margin, rec.kink)
    assert list(zip(*rec.zones[-1])) == case.expect_zones
    T_dev = rt.get("T_lay", col)
    np.testing.assert_array_equal(rt.get("conv_layer", col), q.conv_layer, err_msg=case.name)
    np.testing.assert_array_equal(rt.get("conv_unstable", col), q.conv_unstable, err_msg=case.name)
    dev = float(np.abs(T_dev / q.T_lay - 1.0).max())
    record(L, "adjusted T_lay (%s, rtol %.2e)" % (case.name, case.rtol), dev)
    record(L, "adjusted T_lay", dev)
    np.testing.assert_allclose(T_dev, q.T_lay, rtol=case.rtol, atol=0, err_msg=case.name)
    touched = np.zeros(L + 1, bool)
    for starts, ends in rec.zones:
        for s, e in zip(starts, ends):
            touched[max(s, 0):e + 1] = True
            if s == -1:
                touched[L] = True
    np.testing.assert_array_equal(T_dev[~touched], case.T[~touched], err_msg="layers outside every zone, " + case.name)
    if "outcomes" in case.expect:                              # the fudge factors the fluxes on the device give
        for n, o in enumerate(case.expect["outcomes"]):
            f = rec.fudge[n]
            assert rec.tests[n] == case.expect["tests"][n]
            assert {"lo": f == 0.99 and not rec.nan[n], "hi": f == 1.01, "mid": 0.99 < f < 1.01 and f != 1.0,
                    "nan": rec.nan[n] and f == 0.99}[o], (case.name, n, o, f)
    return q, rec, T_dev, mmm


@pytest.mark.parametrize("case", cc.adjust_cases(), ids=lambda c: c.name)
def test_adjust_half_against_host_functions(ctx, batches, case):
    rt, c = batches(case)
    prepare(ctx, rt, c, case)
    mmm0 = rt.get("meanmolmass_lay")
    q, rec, T_dev, mmm = adjust_against_host(rt, c, case)
    if case.expect.get("untouched"):
        np.testing.assert_array_equal(T_dev, case.T)
    if case.name == "it_7":        # the mean molecular mass is re-evaluated before the adjustment when it % 10 == 0 only
        np.testing.assert_array_equal(mmm, mmm0)
    if case.name == "it_10":
        import oracle
        want = np.zeros(case.L)
        oracle.port.meanmolmass_interpol(np.ascontiguousarray(case.T), c.ktemp, want, c.opac_meanmass,
                                         np.ascontiguousarray(case.p_lay), c.kpress, c.npress, c.ntemp, case.L)
        assert np.abs(mmm / mmm0 - 1.0).max() > 1e-6
        np.testing.assert_allclose(mmm, want, rtol=1e-13)


def test_three_column_batch_with_a_finished_column(ctx, batches):
    """L = 65, three different profiles; column 1 is done and must come back bit for bit, columns 0 and 2 must each
    equal their own host result (the mean molecular mass is strided by L + 1, the other layer arrays by L)"""
    cols = cc.batch_columns()
    rt, c = batches(cols[0], ncol=3)
    for k, case in enumerate(cols):
        case.it = 10
        prepare(ctx, rt, c, case, col=k, done=1 if k == 1 else 0)
    stale = np.zeros(cols[1].L + 1, np.int32)
    stale[[2, 3, 30, 65]] = 1
    rt.set_state(1, "conv_unstable", stale)
    rt.set_state(1, "conv_layer", stale[::-1].copy())
    before = {n: rt.get(n, 1) for n in ("T_lay", "conv_layer", "conv_unstable", "marked_red")}
    seen = [{n: rt.get(n, k) for n in ("T_lay", "F_net", "F_up_tot", "F_down_tot", "F_smooth_sum", "F_add_heat_sum",
                                       "conv_layer", "conv_unstable")} for k in range(3)]
    rt.conv_adjust(10)
    for n, v in before.items():
        np.testing.assert_array_equal(rt.get(n, 1), v, err_msg="finished column: " + n)
    mmms = [rt.get("meanmolmass_lay", k) for k in range(3)]
    assert np.abs(mmms[0] / mmms[2] - 1.0).max() > 1e-6            # a wrong stride would show
    for k in (0, 2):
        case, s = cols[k], seen[k]
        q = cc.make_quant(case, c, s["T_lay"], s["F_up_tot"], s["F_down_tot"], s["F_net"], mmms[k],
                          conv_layer=s["conv_layer"], conv_unstable=s["conv_unstable"], F_smooth_sum=s["F_smooth_sum"])
        rec = cc.run_host(q)
        assert rec.margin >= cc.MARGIN_MIN and rec.kink >= cc.MARGIN_MIN
        assert list(zip(*rec.zones[-1])) == case.expect_zones
        np.testing.assert_array_equal(rt.get("conv_layer", k), q.conv_layer)
        np.testing.assert_array_equal(rt.get("conv_unstable", k), q.conv_unstable)
        T_dev = rt.get("T_lay", k)
        record(case.L, "adjusted T_lay (batch column %d)" % k, float(np.abs(T_dev / q.T_lay - 1.0).max()))
        np.testing.assert_allclose(T_dev, q.T_lay, rtol=case.rtol, atol=0, err_msg="column %d" % k)
    rt.set_state(1, "done", np.zeros(1, np.int32))


PHASES = (("it7", 7, 1e-8), ("it400_open", 400, 1e-8), ("it400_latch", 400, 1e30))


@pytest.mark.parametrize("L", cc.ADVANCE_L)
def test_advance_half_against_host_functions(ctx, batches, L):
    """k_rt_totals_c after the adjustment: totals over more than one pass of its 256-wide loop, marking and equilibrium
    test with 1024 threads, the latch of `done` / `iters_done`, the temperature step"""
    import oracle
    case = cc.advance_case(L)
    rt, c = batches(case)
    X, Y, I = c.nbin, c.ny, L + 1
    assert 2 * I >= 256                          # 256 is exactly one pass of the totals loop, 258 the first with two
    for phase, it, limit in PHASES:
        case.it = it
        prepare(ctx, rt, c, case)
        rt.set_convergence_limit(0, limit)
        q, rec, T_dev, mmm = adjust_against_host(rt, c, case)
        layer_adj = rt.get("conv_layer")
        pref0, store0 = rt.get("delta_t_prefactor"), rt.get("T_store")
        rt.conv_advance(it)
        F_up, F_down, F_net = rt.get("F_up_tot"), rt.get("F_down_tot"), rt.get("F_net")
        dw = np.asarray(c.opac_deltawave, np.longdouble)
        bound = (X * Y + 16) * 2.0 ** -52
        for name, tot in (("F_up", F_up), ("F_down", F_down)):
            band = rt.get(name + "_band").reshape(I, X).astype(np.longdouble)
            assert (band >= 0).all()
            want = (band * dw[None, :]).sum(axis=1)
            dev = float(np.abs(tot.astype(np.longdouble) - want).max() if (want == 0).any()
                        else np.abs(tot.astype(np.longdouble) / want - 1).max())
            record(L, "%s_tot against the long-double sum" % name, dev)
            assert (np.abs(tot.astype(np.longdouble) - want) <= bound * want).all(), (name, phase)
        np.testing.assert_array_equal(F_net, F_up - F_down)
        # marking and equilibrium test, fed with the device's own profile and fluxes
        q2 = cc.make_quant(case, c, T_dev, F_up, F_down, F_net, mmm, conv_layer=layer_adj, rad_convergence_limit=limit,
                           F_smooth_sum=rt.get("F_smooth_sum"))
        with cc.recording(q2) as rec2:
            hs.mark_convective_layers(q2, stitching=1)
        assert rec2.margin >= cc.MARGIN_MIN and rec2.kink >= cc.MARGIN_MIN, (rec2.margin, rec2.kink)
        crit = hs.check_for_radiative_eq(q2)
        norm = q2.F_down_tot[L] + q2.F_intern
        dF = np.append(np.abs(q2.F_intern + q2.F_add_heat_sum + q2.F_smooth_sum - q2.F_net[1:]),
                       abs(q2.F_intern - q2.F_net[0]))
        assert np.abs(dF / (limit * norm) - 1.0).min() >= cc.MARGIN_MIN
        np.testing.assert_array_equal(rt.get("conv_layer"), q2.conv_layer, err_msg=phase)
        np.testing.assert_array_equal(rt.get("marked_red"), q2.marked_red, err_msg=phase)
        assert q2.conv_layer.sum() > 0
        go = (not crit) or it < 400 or int(q2.conv_layer.sum()) == 0
        assert crit == (1 if phase == "it400_latch" else 0) and go == (phase != "it400_latch")
        assert int(rt.get("done")[0]) == (0 if go else 1), phase
        if not go:
            assert int(rt.get("iters_done")[0]) == it
            for n, v in (("T_lay", T_dev), ("delta_t_prefactor", pref0), ("T_store", store0)):
                np.testing.assert_array_equal(rt.get(n), v, err_msg="latched column: " + n)
            continue
        T_o, pref_o, store_o = T_dev.copy(), pref0.copy(), store0.copy()
        oracle.port.conv_temp_iter(np.asarray(F_net, np.float64), np.zeros(L), T_o, q2.p_lay, q2.p_int, store_o, pref_o,
                                   rt.get("marked_red"), np.asarray(rt.get("F_add_heat_lay"), np.float64), np.zeros(L),
                                   np.zeros(L), L, it, int(c.adapt_interval), 0, float(c.F_intern))
        T_new = rt.get("T_lay")
        assert np.abs(T_new - T_dev).max() > 0                      # the temperature step was taken
        record(L, "conv_temp_iter T_lay", float(np.abs(T_new / T_o - 1.0).max()))
        np.testing.assert_allclose(T_new, T_o, rtol=1e-12, err_msg="conv_temp_iter, " + phase)
        np.testing.assert_allclose(rt.get("delta_t_prefactor"), pref_o, rtol=1e-14, err_msg="prefactor, " + phase)
        np.testing.assert_allclose(rt.get("T_store"), store_o, rtol=1e-14)
    rt.set_convergence_limit(0, float(c.rad_convergence_limit))
