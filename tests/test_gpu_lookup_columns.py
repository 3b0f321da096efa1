"""The (T, log10 P) table look-up over the COLUMNS of a batch, and against the commit before.

The two kernel templates of csrc/tp_lookup.h (k_tp_scalar, k_tp_spectral) serve the stage API with one column and the device loop with
all of them: per-column strides of temperatures, pressures and outputs, per-column table sets, and the choice of which columns
a launch covers.  lookup_cases.column_batch has three columns that differ in all of these, at L = 2 and L = 65 (one level past
a 64-thread block).  Byte for byte means exactly that: the batch launches and the single-column stage calls run the same
statements on the same numbers.

What the routes of tests/lookup_cases.py gave on the commit before (cf4ceda), recorded twice with equal bits on an MI355X by
tests/golden/make_lookup_golden.py from that commit's library, is tests/golden/lookup/parent_bits.npz: routes() below is held to it byte for byte."""
import contextlib
import hashlib
import os

import numpy as np
import pytest

import lines_cases
import lookup_cases as lc
import lookup_reference as lk
import test_gpu_lookup_edges as le

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lookup", "parent_bits.npz")
LOOP_NAMES = ("T_lay", "c_p_lay", "kappa_lay", "F_net", "abort")


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    c = Context(0)
    yield c


@contextlib.contextmanager
def _columns(ctx, c, which=(0, 1, 2)):
    """the column batch of `c`, or a batch of some of its columns, before its first refresh"""
    from helios_amd.rt import batch_from_case
    with le._knobs(c.env):
        rt = batch_from_case(ctx, c, ncol=len(which), columns=[c.columns[col] for col in which])
        try:
            second = rt.add_premixed_tables(*c.second_set)
            for k, col in enumerate(which):
                rt.set_column_table(k, second if c.col_set[col] else 0)
                rt.set_temperatures(k, c.T_cols[col])
            rt.set_kappa_table(c.entr_temp, c.entr_press, c.entr_kappa, c.entr_c_p)
            rt.build_planck_table(1)
            yield rt
        finally:
            rt.close()


def _kappa_cp(ctx, L):
    """kappa_lay, kappa_int, c_p_lay and T_int of every column after hx_rt_kappa_cp_refresh"""
    c = lc.column_batch(L)
    with _columns(ctx, c) as rt:
        rt.kappa_cp_refresh()
        return {n: np.array([rt.get(n, col) for col in range(3)]) for n in ("kappa_lay", "kappa_int", "c_p_lay", "T_int")}


def _other_T(c, col):
    return c.T_cols[(col + 1) % 3]


def _mmm_of_conv_adjust(ctx, L):
    """meanmolmass_lay after a refresh, NEW temperatures and hx_rt_conv_adjust(rt, 10): the refresh's own values would not do"""
    c = lc.column_batch(L)
    with _columns(ctx, c) as rt:
        rt.refresh()
        for col in range(3):
            rt.set_temperatures(col, _other_T(c, col))
        rt.conv_adjust(10)
        return np.array([rt.get("meanmolmass_lay", col) for col in range(3)])


def _stage(ctx):
    """the stage API on the free levels"""
    from impls import HipBackend
    raw = HipBackend(ctx)
    c = lc.ladder()
    T, P = lc.free_levels()[:2]
    n, X, Y = len(T), c.nbin, c.ny
    out = dict(opac=np.zeros(n * X * Y), scat=np.zeros(n * X), mmm=np.zeros(n), spec=np.zeros(n * X * Y), kappa=np.zeros(n),
               cp=np.zeros(n))
    raw.opac_interpol(T, c.ktemp, P, c.kpress, c.opac_k, out["opac"], c.opac_scat_cross, out["scat"], c.npress, c.ntemp, Y, X, n)
    raw.meanmolmass_interpol(T, c.ktemp, out["mmm"], c.opac_meanmass, P, c.kpress, c.npress, c.ntemp, n)
    raw.opac_species_interpol(T, c.ktemp, P, c.kpress, c.opac_k, out["spec"], c.npress, c.ntemp, Y, X, n)
    raw.kappa_interpol(T, c.ktemp, P, c.kpress, out["kappa"], c.opac_meanmass, c.npress, c.ntemp, n)
    raw.cp_interpol(T, c.ktemp, P, c.kpress, out["cp"], c.opac_meanmass, c.npress, c.ntemp, n)       # (log10 T)
    return out


def routes(ctx):
    """every array the fixture holds, by name"""
    out = {"stage " + k: v for k, v in _stage(ctx).items()}
    for name in ("ladder", "L2", "L17_k8", "L33"):
        for tag, env in (("unfused", le.UNFUSED), ("default", None)):
            run = le._run(ctx, name, env)
            for key, v in run.items():
                if key not in ("tiling", "bytes", "T_int"):
                    out["%s %s %s" % (name, tag, key)] = v
    for L in lc.COLUMN_LAYERS:
        for key, v in _kappa_cp(ctx, L).items():
            if key != "T_int":
                out["columns L%d %s" % (L, key)] = v
        out["columns L%d meanmolmass_lay" % L] = _mmm_of_conv_adjust(ctx, L)
    return out


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), np.uint8)


# ---- the commit before ---------------------------------------------------------------------------------------------------

def test_routes_equal_the_parent_commit_byte_for_byte(ctx):
    with np.load(GOLDEN) as f:
        want = {k: f[k] for k in f.files}
    got = routes(ctx)
    assert {k[len("sha256 "):] if k.startswith("sha256 ") else k for k in want} == set(got)
    for key, w in want.items():
        if key.startswith("sha256 "):
            g = got[key[len("sha256 "):]]
            assert np.array_equal(digest(g), w), "%s: another SHA-256 than on the parent commit" % key
        else:
            le._same_bytes(got[key], w, key + " against the parent commit")


# ---- columns and strides -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", lc.COLUMN_LAYERS)
def test_kappa_cp_refresh_equals_the_stage_api_per_column(ctx, L):
    """hx_rt_kappa_cp_refresh, three launches for the batch, against hx_kappa_interpol / hx_cp_interpol on each column's arrays
    alone (byte for byte) and against the long-double restatement (check_rule)"""
    from impls import HipBackend
    raw = HipBackend(ctx)
    c = lc.column_batch(L)
    got = _kappa_cp(ctx, L)
    nt, npr = len(c.entr_temp), len(c.entr_press)
    for col in range(3):
        want_T_int = lk.interface_T(c.T_cols[col], L)
        assert np.array_equal(got["T_int"][col].view(np.uint64), want_T_int.view(np.uint64))
        for name, T, P, table, log_t in (("kappa_lay", c.T_cols[col][:L], c.p_lay, c.entr_kappa, False),
                                         ("kappa_int", got["T_int"][col], c.p_int, c.entr_kappa, False),
                                         ("c_p_lay", c.T_cols[col][:L], c.p_lay, c.entr_c_p, True)):
            alone = np.zeros(len(T))
            call = raw.cp_interpol if log_t else raw.kappa_interpol
            call(np.ascontiguousarray(T), c.entr_temp, P, c.entr_press, alone, table, npr, nt, len(T))
            le._same_bytes(got[name][col], alone, "L = %d column %d %s against the stage call" % (L, col, name))
            args = (np.asarray(table).reshape(nt, npr), T, P, c.entr_temp, c.entr_press)
            lines_cases.check_rule(got[name][col], lk.look_up(lk.LD, *args, log_t=log_t), lk.look_up(np.float64, *args, log_t=log_t),
                                   "L = %d column %d %s" % (L, col, name))
    assert np.abs(got["kappa_lay"][0] / got["kappa_lay"][1] - 1).max() > 1e-3       # the columns do differ


@pytest.mark.parametrize("L", lc.COLUMN_LAYERS)
def test_conv_adjust_mean_mass_equals_the_stage_api_per_column(ctx, L):
    """the mean molecular mass hx_rt_conv_adjust(rt, 10) takes from each column's CURRENT table set at the current layer
    temperatures, against hx_meanmolmass_interpol on that column with its own set"""
    from impls import HipBackend
    raw = HipBackend(ctx)
    c = lc.column_batch(L)
    got = _mmm_of_conv_adjust(ctx, L)
    for col in range(3):
        table = c.second_set[2] if c.col_set[col] else c.opac_meanmass
        alone = np.zeros(L)
        raw.meanmolmass_interpol(np.ascontiguousarray(_other_T(c, col)[:L]), c.ktemp, alone, table, c.p_lay, c.kpress, c.npress,
                                 c.ntemp, L)
        le._same_bytes(got[col], alone, "L = %d column %d meanmolmass_lay" % (L, col))
    assert np.abs(got[0] / got[1] - 1).max() > 1e-3


def _ten_steps(rt, c, which):
    L = c.nlayer
    for k in range(len(which)):
        rt.set_state(k, "delta_t_prefactor", np.full(L + 1, 0.5))
    given = [rt.get("c_p_lay", k) for k in range(len(which))]
    for it in range(10, 20):
        rt.step(it)
    return given, [{n: rt.get(n, k) for n in LOOP_NAMES} for k in range(len(which))]


@pytest.mark.parametrize("L", lc.COLUMN_LAYERS)
def test_time_stepped_kappa_refresh_covers_the_time_stepped_columns_alone(ctx, L):
    """ten hx_rt_step calls from iteration 10 (the refresh of kappa and c_p for the time-stepped columns, computation.py:921-923,
    runs at iteration 10): column 1, not time-stepped, keeps the c_p it was given bit for bit; every column equals its
    single-column batch"""
    c = lc.column_batch(L)
    with _columns(ctx, c) as rt:
        given, batch = _ten_steps(rt, c, (0, 1, 2))
    np.testing.assert_array_equal(batch[1]["c_p_lay"].view(np.uint64), given[1].view(np.uint64))
    for col in range(3):
        with _columns(ctx, c, (col,)) as rt1:
            g1, single = _ten_steps(rt1, c, (col,))
        np.testing.assert_array_equal(g1[0], given[col])
        for n in LOOP_NAMES:
            np.testing.assert_array_equal(batch[col][n], single[0][n], err_msg="L = %d column %d, %s" % (L, col, n))
        assert np.abs(single[0]["T_lay"] - c.T_cols[col]).max() > 1e-6                      # temperatures that move
        if col != 1:
            assert np.abs(batch[col]["c_p_lay"] / given[col] - 1).max() > 1e-3              # refreshed from the table


@pytest.mark.parametrize("L", lc.COLUMN_LAYERS)
def test_opacities_of_a_finished_column_are_those_of_its_last_real_refresh(ctx, L):
    """opac_wg_* are rebuilt on demand from what each column's last real refresh used: column 1, finished after the first
    refresh, then given other temperatures and another table set, reads as it does in a batch of its own after one refresh"""
    c = lc.column_batch(L)
    names = ("opac_wg_lay", "opac_wg_int", "scat_cross_lay", "scat_cross_int")
    with _columns(ctx, c) as rt:
        rt.refresh()
        rt.set_state(1, "done", np.array([1], np.int32))
        rt.set_temperatures(1, _other_T(c, 1))
        rt.set_column_table(1, 0)
        rt.refresh()
        batch = [{n: rt.get(n, col) for n in names} for col in range(3)]
    for col in range(3):
        with _columns(ctx, c, (col,)) as rt1:
            rt1.refresh()
            for n in names:
                le._same_bytes(batch[col][n], rt1.get(n, 0), "L = %d column %d %s" % (L, col, n))
    assert np.abs(batch[0]["opac_wg_lay"][:20] / batch[1]["opac_wg_lay"][:20] - 1).max() > 1e-3
