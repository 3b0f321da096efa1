"""The radiative half of an iteration at its edges: the wavelength totals (k_rt_totals_a, k_rt_totals_b in
csrc/rt_kernels.h; k_band_quadrature, k_band_totals in csrc/stage_flux.hip) against long-double sums of the same terms, and
the temperature step (rad_temp_step, smoothing_flux in csrc/temp_step.h) against the CPU oracle and the long-double
restatement of tests/rad_cases.py on IDENTICAL inputs -- directly through hx_rad_temp_iter on crafted columns, and inside
the device loop on what the device really saw: every chunking of the bins (tails, empty chunks, fewer chunks than the four
segments of the second level), 2 I on both sides of the 256-wide stride, L + 1 on both sides of 1024 threads, the latch of
`done`, the foreplay, the iteration index on the device, and batches whose columns differ in everything the step reads.
tests/test_rad_cases.py proves without a GPU that each case takes the branches it is named for; every run in the device
loop asserts again, on the device's own fluxes, that no discrete comparison is closer than 1e-10 to its limit.

Bounds (none is taken from a measurement).  Flags, T_store, F_net_diff, the prefactor, clamped temperatures, everything
a call must not touch, and F_net = F_up_tot - F_down_tot: bit for bit.  T_lay: rtol 1e-12, the bound of
test_gpu_reference.py for conv_temp_iter (pow differs by an ulp or two, delta_T is added to a larger T).  F_smooth: 8 ulp;
F_smooth_sum: (L + 2) 2^-53 sum|F_smooth|.  Band values: (ny + 2) 2^-53 sum|term|.  Totals: (nbin + 16) 2^-52 sum|term|, the
shape of the bound test_gpu_conv_edges.py derives for the same kind of tree.

With the environment variable RAD_EDGES_JSON set, the largest deviations per layer count go into the file it names."""
import contextlib
import json
import os

import numpy as np
import pytest

import cases
import rad_cases as rc
from helios_amd import phys_const as pc

pytestmark = pytest.mark.gpu
LD = np.longdouble
SIZE = dict(ny=4, ntemp=6, npress=5)


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


@pytest.fixture(scope="module")
def hip(ctx):
    from impls import hip_impl
    return hip_impl(ctx)


def record(L, what, value):
    print("L = %d  %s: %.3e" % (L, what, value))
    path = os.environ.get("RAD_EDGES_JSON")
    if path:
        have = json.load(open(path)) if os.path.exists(path) else {}
        key = "%d %s" % (L, what)
        have[key] = max(float(value), have.get(key, 0.0))
        json.dump(have, open(path, "w"), indent=1, sort_keys=True)


def against_port(got, want, case, out):
    """the device against the CPU oracle on the same inputs, by the bounds of the module's text"""
    L = case.L
    for k in ("abort", "T_store", "pref"):
        np.testing.assert_array_equal(got[k], want[k], err_msg="%s against the oracle, %s" % (k, case.name))
    np.testing.assert_array_equal(got["F_net_diff"][:L], want["F_net_diff"][:L], err_msg=case.name)
    np.testing.assert_allclose(got["T"], want["T"], rtol=1e-12, atol=0, err_msg="T_lay against the oracle, " + case.name)
    exact = sorted(set(out["clamp_lo"]) | set(out["clamp_hi"]) | (set(range(L)) if case.no_atmo == 1 else set()))
    np.testing.assert_array_equal(got["T"][exact], want["T"][exact], err_msg=case.name)
    if case.smooth == 1:
        total = np.abs(want["F_smooth"]).sum()
        if "F_smooth" in got:
            assert (np.abs(got["F_smooth"] - want["F_smooth"]) <= 8 * np.spacing(np.abs(want["F_smooth"]))).all(), case.name
        assert (np.abs(got["F_smooth_sum"] - want["F_smooth_sum"]) <= (2 * (L + 2) + 16) * 2.0 ** -53 * total).all(), case.name


# ---- 1. hx_rad_temp_iter on the crafted columns ------------------------------------------------------------------------
@pytest.mark.parametrize("case", rc.all_cases(), ids=lambda c: c.name)
def test_rad_temp_iter_on_crafted_columns(hip, port, case):
    out, _margins = rc.restate(case)
    got = rc.run_impl(hip, case)
    dev = rc.check_against(got, case, out, "device")
    against_port(got, rc.run_impl(port, case), case, out)
    np.testing.assert_array_equal(got["abort"], case.expect["abort"])
    for k, v in dev.items():
        record(case.L, "direct " + k, v)


# ---- 2. hx_integrate_flux ----------------------------------------------------------------------------------------------
def long_double_totals(up_band, down_band, dir_band, dl, I, X):
    """the wavelength sums of the band values as they stand, and the sums of the terms' magnitudes"""
    dl = np.asarray(dl, np.float64).astype(LD)[None, :]
    u, d, f = (np.asarray(a, np.float64).reshape(I, X).astype(LD) for a in (up_band, down_band, dir_band))
    return (u * dl).sum(axis=1), ((f + d) * dl).sum(axis=1), (np.abs(u) * dl).sum(axis=1), ((np.abs(f) + np.abs(d)) * dl).sum(axis=1)


def check_totals(L, X, up_tot, down_tot, net, bands, dl, what):
    I = len(up_tot)
    up, down, up_abs, down_abs = long_double_totals(bands[0], bands[1], bands[2], dl, I, X)
    bound = (X + 16) * 2.0 ** -52
    for name, tot, want, mag in (("F_up_tot", up_tot, up, up_abs), ("F_down_tot", down_tot, down, down_abs)):
        err = np.abs(np.asarray(tot, np.float64).astype(LD) - want)
        assert (mag > 0).all(), name + ": a total without terms"
        record(L, "%s %s / sum|term|" % (what, name), float((err / mag).max()))
        assert (err <= bound * mag).all(), "%s %s: %.3e of %.3e" % (what, name, float((err / mag).max()), bound)
    np.testing.assert_array_equal(net, np.asarray(up_tot) - np.asarray(down_tot), err_msg=what + " F_net")


@pytest.mark.parametrize("ni", (3, 129))
@pytest.mark.parametrize("ny", (1, 20, 64))
@pytest.mark.parametrize("nbin", (1, 31, 32, 33, 1023, 1024, 1025))
def test_integrate_flux_against_long_double_sums(hip, nbin, ny, ni):
    """k_band_quadrature (32 bins a workgroup) and k_band_totals (1024 threads): fluxes of mixed sign, the beam flux ten
    decades above the diffuse flux so that a dropped or doubled F_dir shows"""
    rng = np.random.default_rng(100000 * ni + 100 * nbin + ny)
    n = ny * nbin * ni
    gw = rng.uniform(0.1, 1.0, ny)
    dl = rng.uniform(1e-6, 1e-4, nbin)
    F_up, F_down = rng.uniform(-1e5, 1e5, n), rng.uniform(-1e5, 1e5, n)
    F_dir = -rng.uniform(0.5e15, 1e15, n)
    tot = [np.full(ni, rc.POISON) for _ in range(3)]
    band = [np.full(nbin * ni, rc.POISON) for _ in range(3)]           # down, up, dir
    hip.integrate_flux(dl, tot[0], tot[1], tot[2], F_down, F_up, F_dir, band[0], band[1], band[2], gw, nbin, ni, ny)
    w = (0.5 * gw).astype(LD)[None, None, :]
    for name, got, F in (("F_down_band", band[0], F_down), ("F_up_band", band[1], F_up), ("F_dir_band", band[2], F_dir)):
        term = F.reshape(ni, nbin, ny).astype(LD) * w
        want, mag = term.sum(axis=2).reshape(-1), np.abs(term).sum(axis=2).reshape(-1)
        err = np.abs(got.astype(LD) - want)
        record(ni - 1, "integrate_flux %s / sum|term|" % name, float((err / mag).max()))
        assert (err <= (ny + 2) * 2.0 ** -53 * mag).all(), name
    check_totals(ni - 1, nbin, tot[1], tot[0], tot[2], (band[1], band[0], band[2]), dl, "integrate_flux")
    assert (np.abs(tot[0]) > 1e9 * np.abs(tot[1])).all()               # the beam flux is in the down total, once


def test_integrate_flux_refuses_65_gauss_points(hip):
    from helios_amd._lib import HeliosHipError
    nbin, ni, ny = 3, 3, 65
    z = lambda n: np.zeros(n)
    with pytest.raises(HeliosHipError, match="status 3"):               # HX_E_UNSUPPORTED
        hip.integrate_flux(z(nbin), z(ni), z(ni), z(ni), z(ny * nbin * ni), z(ny * nbin * ni), z(ny * nbin * ni),
                           z(nbin * ni), z(nbin * ni), z(nbin * ni), z(ny), nbin, ni, ny)


# ---- 3. the device loop -------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _knob(nchunk):
    """HELIOS_RT_NCHUNK while a batch is created (hx_rt_create reads it), unset otherwise"""
    saved = os.environ.pop("HELIOS_RT_NCHUNK", None)
    try:
        if nchunk is not None:
            os.environ["HELIOS_RT_NCHUNK"] = str(nchunk)
        yield
    finally:
        os.environ.pop("HELIOS_RT_NCHUNK", None)
        if saved is not None:
            os.environ["HELIOS_RT_NCHUNK"] = saved


def loop_case(X, L, scat=0, smooth=0):
    c = cases.make_case(nbin=X, nlayer=L, scat=scat, dir_beam=1, p_boa=1e11 if L <= 4 else 1e9, **SIZE)
    c.smooth = smooth
    c.T_lay = rc.default_T(L + 1)
    return c


@pytest.fixture(scope="module")
def batches(ctx):
    """one batch per (bins, layers, chunks, scattering, smoothing, columns), shared by the tests on it: every test sets all
    the state it reads"""
    from helios_amd.rt import batch_from_case
    have = {}

    def get(X, L, nchunk=None, scat=0, smooth=0, columns=None, tag=""):
        key = (X, L, nchunk, scat, smooth, tag)
        if key not in have:
            c = loop_case(X, L, scat, smooth)
            with _knob(nchunk):
                rt = batch_from_case(ctx, c, ncol=len(columns) if columns else 1, columns=columns)
            rt.build_planck_table(1)
            have[key] = (rt, c)
        return have[key]
    yield get
    for rt, _c in have.values():
        rt.close()


def formula_chunks(X):
    """rt_fused.hip, hx_rt_create: `bin chunks of the totals reduction`"""
    return max(1, min(512, max((X + 47) // 48, min(32, (X + 7) // 8))))


def device_totals(rt, c, col, what):
    L, X = c.nlayer, c.nbin
    check_totals(L, X, rt.get("F_up_tot", col), rt.get("F_down_tot", col), rt.get("F_net", col),
                 (rt.get("F_up_band", col), rt.get("F_down_band", col), rt.get("F_dir_band", col)), c.opac_deltawave, what)


CHUNKINGS = [(1, None, 1), (9, None, 2), (17, None, 3), (250, None, 32), (257, None, 32),      # chosen by the bin count
             (17, 1, 1), (17, 3, 3), (17, 5, 5), (9, 64, 64)]                                     # forced


@pytest.mark.parametrize("L", (2, 127, 128, 1024))
@pytest.mark.parametrize("X,forced,want", CHUNKINGS, ids=["X%d_%s" % (x, f or "auto") for x, f, _w in CHUNKINGS])
def test_totals_of_every_chunking(batches, X, forced, want, L):
    """tails of 5 + 4 and 6 + 6 + 5 bins, chunks of exactly 8, three empty chunks (257 bins: 32 chunks of 9), fewer
    chunks than segments, a segment tail (5 chunks), more chunks than bins; 2 I = 256 at L = 127, 258 at L = 128"""
    rt, c = batches(X, L, forced, scat=1)
    if forced is None:
        assert formula_chunks(X) == want        # a retuned formula must say so here, not silently stop testing the edge
        per = -(-X // want)
        assert {1: per == 1, 9: (per, X - per) == (5, 4), 17: (per, X - 2 * per) == (6, 5), 250: per == 8 and 31 * per < X,
                257: per == 9 and 29 * per >= X > 28 * per}[X]
    assert rt.totals_chunks() == want
    rt.set_state(0, "done", np.zeros(1, np.int32))
    rt.step(0, step_temperature=False)
    assert np.abs(rt.get("F_dir_band")).max() > 0
    device_totals(rt, c, 0, "device loop")


COLUMN_DEFAULT = dict(foreplay=0, adapt=20, tstep=0.0, no_atmo=0)


def step_on_what_the_device_saw(rt, c, port, it, name, col=0, colpar=None, restore_T=True, **design):
    """totals without a step; T_store, prefactor, heating and limit chosen from the F_net just read for the branches
    wanted; the step; then the oracle and the restatement on exactly the arrays read back"""
    L = c.nlayer
    cp = dict(COLUMN_DEFAULT, g=float(c.g), F_intern=float(c.F_intern), **(colpar or {}))
    rt.set_state(col, "done", np.zeros(1, np.int32))
    if restore_T:
        rt.set_temperatures(col, rc.default_T(L + 1))
    rt.step(it, step_temperature=False)
    T0, F_net0, F_down0 = rt.get("T_lay", col), rt.get("F_net", col), rt.get("F_down_tot", col)
    given = dict(F_net=F_net0, F_down_tot=F_down0, p_lay=c.p_lay, p_int=c.p_int, T=T0, F_intern=cp["F_intern"], g=cp["g"],
                 c_p=rt.get("c_p_lay", col), mmm=rt.get("meanmolmass_lay", col), tstep=cp["tstep"])
    base = 0.1 if it == 10000 else 1.0 if it == cp["foreplay"] else "keep"
    case = rc.RadCase(name, L, name, it=it, foreplay=cp["foreplay"], adapt=cp["adapt"], limit=None, tstep=cp["tstep"] != 0,
                      no_atmo=cp["no_atmo"], smooth=int(c.smooth), base=base, given=given, **design)
    rt.set_state(col, "T_store", case.T_store)
    rt.set_state(col, "delta_t_prefactor", case.pref)
    rt.set_column_heating(col, case.heat_lay, case.heat_sum)
    rt.set_convergence_limit(col, case.limit)
    rt.step(it, step_temperature=True)
    np.testing.assert_array_equal(rt.get("F_net", col), F_net0, err_msg="the same temperatures, another F_net: " + name)
    np.testing.assert_array_equal(rt.get("F_down_tot", col), F_down0)
    np.testing.assert_array_equal(rt.get("F_add_heat_lay", col), case.heat_lay)
    case.mmm = rt.get("meanmolmass_lay", col)                 # what the step saw
    got = dict(T=rt.get("T_lay", col), T_store=rt.get("T_store", col), pref=rt.get("delta_t_prefactor", col),
               F_net_diff=rt.get("F_net_diff", col), abort=rt.get("abort", col), F_smooth_sum=rt.get("F_smooth_sum", col))
    out, margins = rc.restate(case)
    worst = min(margins, key=lambda t: t[2])
    assert worst[2] >= rc.MARGIN_MIN, "%s at entry %d: %.3e from its limit on the device's values" % worst
    dev = rc.check_against(got, case, out, "device loop")
    against_port(got, rc.run_impl(port, case), case, out)
    np.testing.assert_array_equal(got["abort"], case.expect["abort"], err_msg=name)
    for k in ("clamp500", "shrink", "grow"):
        assert out[k] == case.expect[k], (name, k)
    for k, v in dev.items():
        record(L, "device loop " + k, v)
    return case, got, out


LATCH = [(2, 0), (127, 0), (128, 0), (1024, 0), (1024, 1)]


@pytest.mark.parametrize("L,smooth", LATCH, ids=["L%d_smooth%d" % t for t in LATCH])
def test_step_and_latch_on_what_the_device_saw(batches, port, L, smooth):
    """every flag set: done, iters_done = it + 1, and the column is left alone from then on; one flag short: not done, L
    flags counted.  L = 1024: the ghost layer, entry 1024, is thread 0's second stride -- it is stepped and counted"""
    rt, c = batches(17, L, smooth=smooth)
    it = 19
    ok = rc.alt(L, 0.5, -0.5)
    case, got, out = step_on_what_the_device_saw(rt, c, port, it, "latch_all_L%d" % L, e=ok, e_ghost=0.25)
    assert got["abort"].all() and int(rt.converged_layers()[0]) == L + 1
    assert got["T"][L] != case.T[L] and out["shrink"] and out["grow"]
    assert int(rt.get("done")[0]) == 1 and int(rt.get("iters_done")[0]) == it + 1
    names = ("T_lay", "T_store", "delta_t_prefactor", "abort", "F_net", "F_up_tot", "F_down_tot", "F_net_diff", "F_up_band")
    before = {n: rt.get(n) for n in names}
    rt.step(it + 1)
    for n, v in before.items():
        np.testing.assert_array_equal(rt.get(n), v, err_msg="a finished column: " + n)
    assert int(rt.get("iters_done")[0]) == it + 1
    short = ok.copy()
    short[L // 2] = 2.0
    case, got, out = step_on_what_the_device_saw(rt, c, port, it, "latch_one_short_L%d" % L, e=short, e_ghost=0.25)
    assert int(rt.get("done")[0]) == 0 and int(rt.converged_layers()[0]) == L and got["abort"][L // 2] == 0
    # the ghost layer alone short of its limit
    case, got, out = step_on_what_the_device_saw(rt, c, port, it, "latch_ghost_short_L%d" % L, e=ok, e_ghost=2.0)
    assert int(rt.get("done")[0]) == 0 and int(rt.converged_layers()[0]) == L and got["abort"][L] == 0


def test_foreplay_in_the_device_loop(batches, port):
    """foreplay = 5: iteration 4 writes the totals and nothing else (no flags, no latch even with every layer inside the
    limit); iteration 5 sets the prefactor to 1"""
    X, L = 17, 8
    rt, c = batches(X, L, columns=[dict(foreplay=5)], tag="foreplay5")
    short = rc.alt(L, 0.5, -0.5)
    short[3] = 2.0
    case, got, out = step_on_what_the_device_saw(rt, c, port, 5, "foreplay_it5", colpar=dict(foreplay=5), e=short)
    assert (got["pref"] == 1.0).all() and (case.pref != 1.0).all() and int(rt.get("done")[0]) == 0
    rt.set_convergence_limit(0, 1e30)                      # with this limit a step sets every flag
    rt.set_state(0, "delta_t_prefactor", case.pref)
    names = ("T_lay", "T_store", "delta_t_prefactor", "abort", "F_net_diff", "F_smooth_sum")
    before = {n: rt.get(n) for n in names}
    assert not before["abort"].all()
    rt.step(4)
    for n, v in before.items():
        np.testing.assert_array_equal(rt.get(n), v, err_msg="before the foreplay's end: " + n)
    assert int(rt.get("done")[0]) == 0
    device_totals(rt, c, 0, "foreplay")
    rt.step(5)
    assert rt.get("abort").all() and int(rt.get("done")[0]) == 1 and int(rt.get("iters_done")[0]) == 6
    rt.set_convergence_limit(0, float(c.rad_convergence_limit))


@pytest.mark.parametrize("start,nsteps", [(9998, 3), (9991, 10)])
def test_iteration_index_from_the_device(batches, start, nsteps):
    """hx_rt_run (the index read on the device; from 9991 nine iterations replayed as a graph) against hx_rt_step calls
    (the host's value) from the same state: bit for bit, and iteration 10000 resets the prefactor in both"""
    X, L = 17, 8
    rt, c = batches(X, L, scat=1, tag="run")
    names = ("T_lay", "T_store", "delta_t_prefactor", "abort", "F_net", "F_net_diff")
    res = []
    for how in ("run", "steps"):
        rt.set_state(-1, "restart", np.ones(1, np.int32))
        rt.set_convergence_limit(0, 1e-12)
        rt.set_temperatures(0, rc.default_T(L + 1))
        rt.set_state(0, "delta_t_prefactor", np.linspace(0.3, 0.9, L + 1))
        rt.set_state(0, "T_store", rc.default_T(L + 1) + 0.01)
        rt.step(start - 1)                                     # refreshed, as a loop arriving here is
        replays = rt.get("graph_replays")
        if how == "run":
            rt.run(start, nsteps)
            after = rt.get("graph_replays")
            if start % 10 == 1 and after[2] == 1:
                assert after[0] == replays[0] + 1
        else:
            for it in range(start, start + nsteps):
                rt.step(it)
        res.append({n: rt.get(n) for n in names})
        assert int(rt.get("done")[0]) == 0
    for n in names:
        np.testing.assert_array_equal(res[0][n], res[1][n], err_msg=n)
    assert (res[0]["delta_t_prefactor"] == 0.1).all()            # 10000 % 20 == 0: reset, stored, no adapt test
    rt.set_convergence_limit(0, float(c.rad_convergence_limit))


SIGMA_T4 = lambda T: pc.SIGMA_SB * T ** 4
OUTER = [dict(foreplay=2, adapt_interval=2, F_intern=SIGMA_T4(250.0), rad_convergence_limit=1e-6, physical_tstep=0.0,
              no_atmo=1, g=800.0),
         dict(foreplay=1, adapt_interval=3, F_intern=SIGMA_T4(400.0), rad_convergence_limit=1e-4, physical_tstep=2e-3,
              no_atmo=0, g=1500.0)]
STATE = ("T_lay", "T_store", "delta_t_prefactor", "abort", "F_net", "F_up_tot", "F_down_tot", "F_net_diff", "done", "iters_done")


def test_three_column_batch_with_a_finished_column(batches):
    """L = 9, strides L, L + 1 and I; the middle column is done and comes back bit for bit; the outer two differ in every
    hx_rt_column field the step reads (one has no_atmo = 1, one is time-stepped) and equal their single-column runs"""
    X, L = 17, 9
    assert all(OUTER[0][k] != OUTER[1][k] for k in OUTER[0])
    T = [rc.default_T(L + 1), rc.default_T(L + 1) + 50.0, rc.default_T(L + 1)[::-1] - 30.0]
    pref = [np.linspace(0.2, 0.6, L + 1), np.full(L + 1, 0.5), np.linspace(0.9, 0.4, L + 1)]

    def run(rt, cols):
        for k, col in enumerate(cols):
            rt.set_temperatures(k, T[col])
            rt.set_state(k, "delta_t_prefactor", pref[col])
            rt.set_state(k, "T_store", T[col] - 0.02)
            rt.set_state(k, "done", np.array([1 if col == 1 else 0], np.int32))
        before = [{n: rt.get(n, k) for n in STATE} for k in range(len(cols))]
        for it in range(0, 4):
            rt.step(it)
        return before, [{n: rt.get(n, k) for n in STATE} for k in range(len(cols))]

    rt3, _c = batches(X, L, scat=1, columns=[OUTER[0], {}, OUTER[1]], tag="three")
    before, after = run(rt3, [0, 1, 2])
    for n in STATE:
        np.testing.assert_array_equal(after[1][n], before[1][n], err_msg="finished column: " + n)
    for k, col in ((0, 0), (1, 2)):
        rt1, _c = batches(X, L, scat=1, columns=[OUTER[k]], tag="single%d" % k)
        _b, single = run(rt1, [col])
        assert np.abs(single[0]["T_lay"] - T[col]).max() > 0
        for n in STATE:
            np.testing.assert_array_equal(after[col][n], single[0][n], err_msg="column %d of the batch, %s" % (col, n))
    assert (after[0]["T_lay"][:L] == 1.001).all() and after[0]["T_lay"][L] != 1.001          # no_atmo
    # each column's count of converged layers in its own slot: the last column inside any limit, the first as it was
    assert int(after[2]["done"][0]) == 0 and after[0]["abort"].sum() < L + 1
    rt3.set_convergence_limit(2, 1e30)
    rt3.step(4)
    count = rt3.converged_layers()
    assert int(count[2]) == L + 1 and int(rt3.get("done", 2)[0]) == 1 and int(rt3.get("iters_done", 2)[0]) == 5
    assert int(count[0]) == int(rt3.get("abort", 0).sum()) < L + 1 and int(count[1]) == 0
    for n in STATE:
        np.testing.assert_array_equal(rt3.get(n, 1), before[1][n], err_msg="finished column: " + n)


def test_time_stepped_column_behind_one_that_is_not(batches):
    """kappa and c_p of a time-stepped column are refreshed from the table every 10th iteration (computation.py:921-923)
    whatever column 0 is: column 1 of (not time-stepped, time-stepped) equals its single-column run bit for bit through
    iteration 10, and so does column 0, which keeps the c_p it was given"""
    X, L = 17, 9
    cols = [dict(physical_tstep=0.0), dict(physical_tstep=2e-3)]
    entr_temp, entr_press = np.linspace(100.0, 4000.0, 8), np.logspace(0, 11, 7)
    tt, pp = np.meshgrid(entr_temp, entr_press, indexing="ij")
    kappa = (0.2 + 0.1 * tt / 4000.0 + 0.005 * np.log10(pp)).reshape(-1)
    c_p = (3.5 * pc.R_UNIV * (1.0 + 0.5 * tt / 4000.0 + 0.005 * np.log10(pp))).reshape(-1)
    T = [rc.default_T(L + 1), rc.default_T(L + 1)[::-1] + 20.0]
    names = ("T_lay", "c_p_lay", "kappa_lay", "F_net", "abort")

    def run(rt, which):
        rt.set_kappa_table(entr_temp, entr_press, kappa, c_p)
        for k, col in enumerate(which):
            rt.set_temperatures(k, T[col])
            rt.set_state(k, "delta_t_prefactor", np.full(L + 1, 0.5))
        given = [rt.get("c_p_lay", k) for k in range(len(which))]
        mid = None
        for it in range(0, 11):
            rt.step(it)
            if it == 5:
                mid = [rt.get("c_p_lay", k) for k in range(len(which))]
        return given, mid, [{n: rt.get(n, k) for n in names} for k in range(len(which))]

    rt2, _c = batches(X, L, scat=1, columns=cols, tag="tstep_pair")
    given, mid, pair = run(rt2, [0, 1])
    for col in (0, 1):
        rt1, _c = batches(X, L, scat=1, columns=[cols[col]], tag="tstep_single%d" % col)
        g1, m1, single = run(rt1, [col])
        for n in names:
            np.testing.assert_array_equal(pair[col][n], single[0][n], err_msg="column %d of the pair, %s" % (col, n))
        assert np.abs(single[0]["T_lay"] - T[col]).max() > 1e-6                    # temperatures that move
    np.testing.assert_array_equal(pair[0]["c_p_lay"], given[0])                    # not time-stepped: no refresh
    assert np.abs(mid[1] / given[1] - 1).max() > 1e-3                              # refreshed at iteration 0 ...
    assert np.abs(pair[1]["c_p_lay"] / mid[1] - 1).max() > 0                       # ... and again at 10, T having moved
