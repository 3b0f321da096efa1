"""The iteration sweeps of k_rt_flux<ROWS, K> (csrc/rt_flux_kernel.inc, the non-MATRIX branch) alone, at every tiling:
three refresh-free steps of a batch, each held to tests/sweep_reference.py's long-double restatement of that one step on the
device's own planes, Planck nodes and up-flux state -- the refresh, the Planck table and the quadrature are not in the
comparison.  The rule: |got - ref| <= max(FLOOR, R 2^-53) m with the count of roundings R derived there and the companion
magnitude m of the restatement; the four spectral arrays at every step, every entry.

(a) the tilings of tests/test_sweep_reference.py's case list, whose table is asserted against hx_rt_flux_geometry here;
(b) tests/coef_cases.py's columns, whose planes hold the edges (opaque, transparent, w0 at its limits, thin);
(c) the band fluxes against the quadrature of the device's own spectral fluxes, in every case of (a) and (b);
(d) boa_source_factor against coef_reference's w0 and E;
(e) a two-column batch under the serpentine launch order with part of the state kept cached, and a finished column.

The figures -- largest err / bound per case -- go to profiles/flux_sweeps_parity.json."""
import contextlib
import json
import os

import numpy as np
import pytest

import coef_cases as cc
import lines_cases
import sweep_reference as sr
import test_sweep_reference as tsr
from test_gpu_precision_tilings import _knobs, _make, _selected_ranges, _geometry
from test_gpu_rt_names import column_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BANDS = ("F_up_band", "F_down_band")
EDGE_COLUMNS = [(f, s) for f in cc.FLAG_SETS if not f.startswith("matrix") for s in cc.SHAPES]


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    c = Context(0)
    yield c


def _record_parity(case, ratio):
    path = os.path.join(ROOT, "profiles", "flux_sweeps_parity.json")
    try:
        held = json.load(open(path)) if os.path.exists(path) else {}
        held.setdefault("largest err / bound per case", {})[case] = float("%.3e" % ratio)
        with open(path, "w") as f:
            json.dump(held, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass        # a read-only tree: the assertions have been made


@contextlib.contextmanager
def _env(extra):
    saved = {k: os.environ.get(k) for k in extra}
    try:
        for k, v in extra.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


# ---- one step against its restatement ------------------------------------------------------------------------------------

def _valid(c, key):
    """the entries of a spectral flux array the batch computes: the centre arrays are as long as the interface ones"""
    n = c.ny * c.nbin
    return n * (c.nlayer if key.startswith("Fc_") else c.nlayer + 1)


def _cancelled_share(c, want, mags):
    return max(sr.cancelled_fraction(want[k][:_valid(c, k)], mags[k][:_valid(c, k)]) for k in sr.FLUX_KEYS
               if not (int(c.iso) and k.startswith("Fc_")))


def _hold_step(rt, c, it, bound, label, col=0, column=None, derived_vp_apart=False):
    """state read, step `it` run by the caller in between (a generator: next() before the step, next() after), the step
    restated from that state; returns the largest err / bound over the four spectral arrays"""
    inp = sr.inputs_from_batch(rt, c, col, column)
    before = [rt.get(k, col) for k in ("planckband_lay", "planckband_int")]
    yield None
    assert int(rt.get("done", col)[0]) == 0, label
    for k, b in zip(("planckband_lay", "planckband_int"), before):        # same temperatures: the same nodes
        np.testing.assert_array_equal(rt.get(k, col).view(np.uint64), b.view(np.uint64), err_msg=label)
    iso = int(c.iso)
    res = sr.restate(inp, tsr.NSWEEP if c.scat else 1, 1)
    want = sr.to_wg(res["U"][0], res["D"][0], iso, c.nlayer)
    mags = sr.to_wg(res["mU"][0], res["mD"][0], iso, c.nlayer)
    worst, fails, got = 0.0, [], {}
    for key in sr.FLUX_KEYS:
        got[key] = rt.get(key, col)
        if iso and key.startswith("Fc_"):
            assert not got[key].any()
            continue
        n = _valid(c, key)
        ratio, _, bad = sr.check(got[key][:n], want[key][:n], mags[key][:n], bound, "%s step %d %s" % (label, it, key))
        worst = max(worst, ratio)
        if bad.size:
            nc = c.ny * c.nbin
            fails.append((key, ratio, [(int(i) // nc, (int(i) % nc) // c.ny, int(i) % c.ny) for i in bad[:4]], int(bad.size)))
    assert not fails, (label, it, fails)
    share = _cancelled_share(c, want, mags)
    if derived_vp_apart and inp["vp"] is None and share > 0.01:
        # v' = Kconst ((1 - alpha) - beta) - u' of a thick or nearly conservative half-layer is the small difference of
        # rounded terms, in the kernel as in the magnitude: with v' handed over as a plane the recurrences themselves cancel nowhere
        al, be, up = (np.asarray(inp[k], sr.LD) for k in ("alpha", "beta", "up"))
        given = sr.restate(dict(inp, vp=sr.LD(inp["Kconst"]) * ((1 - al) - be) - up), tsr.NSWEEP if c.scat else 1, 1)
        print("%-44s entries with m > 100 |value|: %.4f, all of them from the derived v'" % (label, share))
        share = _cancelled_share(c, sr.to_wg(given["U"][0], given["D"][0], iso, c.nlayer),
                                 sr.to_wg(given["mU"][0], given["mD"][0], iso, c.nlayer))
    assert share <= 0.01, (label, "entries with m > 100 |value|", share)
    _hold_bands(rt, c, got, label, col)
    yield worst


def _hold_bands(rt, c, spectral, label, col=0):
    """(c) F_up_band and F_down_band against sum_y 0.5 w_y F of the device's own spectral fluxes in long double: at most
    (ny + 2) 2^-53 of sum |terms|, floored at FLOOR of it"""
    X, Y, I = c.nbin, c.ny, c.nlayer + 1
    w = 0.5 * np.asarray(c.gauss_weight, sr.LD)
    bound = max(lines_cases.FLOOR, (Y + 2) * 2.0 ** -53)
    for band, key in zip(BANDS, ("F_up_wg", "F_down_wg")):
        terms = np.asarray(spectral[key], sr.LD).reshape(I, X, Y) * w
        want, mag = terms.sum(axis=2), np.abs(terms).sum(axis=2)
        got = rt.get(band, col).reshape(I, X)
        err = np.abs(got - want).astype(np.float64)
        ratio = float(np.max(np.where(err == 0.0, 0.0, err / np.maximum(mag.astype(np.float64), 1e-300)))) / bound
        print("%-44s largest err / bound %.3f" % (label + " " + band, ratio))
        assert np.all(np.isfinite(got)) and ratio <= 1.0, (label, band, ratio)


def _run_case(ctx, c, env, want, label, extra_env=None, derived_vp_apart=False):
    """a batch of one column: the tiling that ran is `want`, then three refresh-free steps, each held; returns (largest
    err / bound, tiling, planes)"""
    from helios_amd.rt import batch_from_case
    with _knobs(env), _env(extra_env or {}):
        rt = batch_from_case(ctx, c)
    try:
        t = rt.flux_tiling()
        assert (t["ROWS"], t["k"], t["generic_scans"], t["coef_bytes"]) == tuple(want) + (8,), (label, t)
        bound = sr.rel_bound(t["ROWS"], t["k"], tsr.NSWEEP if c.scat else 1)
        rt.keep_down_fluxes(True)
        rt.build_planck_table(1 if c.T_star > 10 else 0)
        rt.refresh()
        planes = rt.coef_planes(0)
        worst = 0.0
        for it in (1, 2, 3):
            held = _hold_step(rt, c, it, bound, label, derived_vp_apart=derived_vp_apart)
            next(held)
            rt.step(it, step_temperature=False)            # (it % 10 != 0: no refresh)
            worst = max(worst, next(held))
        assert np.array_equal(rt.coef_planes(0).view(np.uint64), planes.view(np.uint64)), "the steps refreshed"
        _record_parity(label, worst)
        return worst, t, planes
    finally:
        rt.close()


# ---- (a) the tilings -----------------------------------------------------------------------------------------------------

def test_the_table_of_tilings_is_the_librarys():
    assert _selected_ranges() == tsr.SELECTED
    for (L, iso), want in tsr.DEEP.items():
        assert _geometry(L, iso) == want, (L, iso)


@pytest.mark.parametrize("case", tsr.CASES, ids=[c[0] for c in tsr.CASES])
def test_three_steps_at_every_tiling(ctx, case):
    """the tiling the case names ran (flux_tiling), and steps 1, 2, 3 each hold the rule in the four spectral arrays and (c)
    in the two band arrays"""
    name, L, iso, env, kw, want = case
    c = _make(L, iso, kw, "double")
    _run_case(ctx, c, env, want, name)


def test_bands_across_workgroups_and_gauss_point_parts(ctx):
    """(c)'s quadrature crosses both here: three bins of twenty Gauss points on 64 lanes each -- one bin per workgroup, its
    Gauss points in four passes of five"""
    c = _make(209, 0, dict(nbin=3, dir_beam=1, albedo=0.2), "double")
    assert c.ny == 20
    _, t, _ = _run_case(ctx, c, {}, (7, 64, 0), "bands_3bins_20points_k64")
    assert t["nparts"] >= 2 and -(-c.nbin // t["nxb"]) >= 2, t


# ---- (b) edges in the plane values -----------------------------------------------------------------------------------

@pytest.mark.parametrize("flagset,shape", EDGE_COLUMNS)
def test_three_steps_on_the_crafted_columns(ctx, flagset, shape):
    """tests/coef_cases.py's columns without the matrix method: the rule at every step, and the planes that ran hold opaque
    half-layers (alpha = 0), thin ones (1 - alpha < 1e-9), w0 at w_0_limit and -- where the column has such bins: a clouded
    bin always scatters -- transparent half-layers (alpha = 1, beta = 0) and w0 = 0 (beta = 0).  The magnitude exceeds 100
    |value| in at most 1 % of the entries once the derived v' of the thick and the nearly conservative bins is set apart"""
    c = cc.make(flagset, shape)
    L, iso = cc.SHAPES[shape]
    worst, t, p = _run_case(ctx, c, {}, tsr.selected(L, iso) + (0,), "%s_%s" % (flagset, shape), derived_vp_apart=True)
    H = L if iso else 2 * L
    x, _, _, pad = sr.slots(t, c.nbin, c.ny, H)
    alpha, beta, bins = p[:, 0][~pad], p[:, 1][~pad], x[~pad]
    groups = np.array([b["group"] for b in c.bins])[bins]
    rest = (1.0 - alpha) - beta
    assert np.any(alpha[groups == "thick"] == 0.0), "opaque half-layers"
    assert np.any((alpha < 1.0) & (alpha > 1.0 - 1e-9) & (groups == "tiny")), "thin half-layers"
    # w0 at w_0_limit: without the I2S correction nearly all that is not transmitted is scattered back
    conservative = (groups == "w0_limit") & (beta > 0.0) & ((rest <= 1e-3 * (1.0 - alpha)) | bool(c.scat_corr))
    assert np.any(conservative), "w0 at w_0_limit"
    if any(b["group"] == "vacuum" for b in c.bins):              # (not with clouds: a clouded bin always scatters)
        assert np.all(alpha[groups == "vacuum"] == 1.0) and np.all(beta[groups == "vacuum"] == 0.0), "transparent half-layers"
        w0_zero = np.array([b["R"] == 0.0 and b["csc"] == 0.0 and b["group"] != "vacuum" for b in c.bins])[bins]
        assert w0_zero.any() and np.all(beta[w0_zero] == 0.0), "w0 = 0"


# ---- (d) boa_source_factor -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flagset,shape", [(f, s) for f in cc.FLAG_SETS for s in cc.SHAPES])
def test_boa_source_factor_against_the_restatement(ctx, flagset, shape):
    """(1 - w0) / (E - w0) of the bottom half-layer against coef_reference's long double under test_gpu_coef_edges.py's
    rule -- absolute on the scale 1, bound max(FLOOR, MARGIN eps) with eps the fp64 twin's largest deviation in the bin's
    group --, exactly 1 where the point does not scatter (w0 = 0, or the matrix method's pure-absorption vote)"""
    from helios_amd.rt import batch_from_case
    c = cc.make(flagset, shape)
    with _knobs({}):
        rt = batch_from_case(ctx, c)
    try:
        rt.build_planck_table(1 if c.T_star > 10 else 0)
        rt.refresh()
        keys = ["opac_wg_lay", "scat_cross_lay", "meanmolmass_lay"] + (["g_0_tot_lay"] if c.clouds else []) \
            + (["F_dir_wg"] if c.dir_beam else [])
        if not c.iso:
            keys += ["opac_wg_int", "scat_cross_int", "meanmolmass_int"] + (["g_0_tot_int"] if c.clouds else []) \
                + (["Fc_dir_wg"] if c.dir_beam else [])
        src = {k: rt.get(k) for k in keys}
        got = rt.get("boa_source_factor")
    finally:
        rt.close()
    ld, f64, idx, _, scatters = cc.restated(c, src)
    X, Y = c.nbin, c.ny
    H = idx[0].max() + 1
    bottom = lambda a: np.asarray(a).reshape(H, X * Y)[0]
    sc = bottom(scatters)
    want = np.where(sc, bottom(ld["boaK"]), 1)
    twin = np.where(sc, bottom(f64["boaK"]), 1.0)
    groups = bottom(cc.group_of_slots(c, idx))
    assert got.shape == want.shape and np.all(np.isfinite(got))
    fails = []
    for g in sorted(set(groups)):
        sel = groups == g
        eps = float(np.max(np.abs(twin[sel].astype(sr.LD) - want[sel])))
        bound = max(lines_cases.FLOOR, lines_cases.MARGIN * eps)
        dev = float(np.max(np.abs(got[sel] - want[sel])))
        print("%-12s worst %.2e bound %.2e" % (g, dev, bound))
        if not dev <= bound:
            fails.append((g, dev, bound))
    assert not fails, fails
    no_scattering = ~sc | (bottom(ld["w0"]) == 0)
    assert np.all(got[no_scattering] == 1.0)
    if flagset in ("plain", "matrix"):
        assert no_scattering.any()
    if c.scat_corr:
        assert np.any(got < 1.0), "no point with E != 1"


# ---- (e) launch policy and finished columns --------------------------------------------------------------------------

def test_two_columns_serpentine_with_part_of_the_state_cached_and_a_finished_column(ctx):
    """two columns with different profiles and albedos, HELIOS_RT_SERPENTINE = 1 (every other launch walks the grid from its
    far end) and a HELIOS_RT_STATE_CACHE_MB that keeps the state of three of the six workgroups cached: both columns hold
    the rule over three steps; then column 1 is marked done and its state, U[0], down-fluxes and band fluxes keep their bits
    over a step in which column 0 moves"""
    from helios_amd.rt import batch_from_case
    L = 50
    c = _make(L, 0, dict(nbin=3, dir_beam=1, albedo=0.2, clouds=1, scat_corr=1, g_0=0.2), "double")
    rows, k = tsr.selected(L, 0)
    with _knobs({}):
        probe = batch_from_case(ctx, c, ncol=2)
    try:
        t = probe.flux_tiling()
    finally:
        probe.close()
    per_wg = t["nparts"] * t["NW"] * t["ROWS"] * 64 * 8
    total = -(-c.nbin // t["nxb"]) * 2
    assert total >= 4, t
    mb = (total // 2 + 0.5) * per_wg / 1048576.0
    with _knobs({}), _env(dict(HELIOS_RT_SERPENTINE=1, HELIOS_RT_STATE_CACHE_MB=repr(mb))):
        rt = batch_from_case(ctx, c, ncol=2)
    try:
        assert rt.flux_tiling() == t and (t["ROWS"], t["k"]) == (rows, k)
        policy = rt.get("flux_launch_policy")
        assert policy[0] == 1.0 and abs(policy[1] - mb) <= 1e-12 * mb
        assert 0 < int(policy[1] * 1048576.0 / per_wg) < total, "part of the grid, not all of it"
        p_lay, p_int, T_lay, albedo = column_inputs(c, 1)
        rt.set_column_profile(1, p_lay, p_int, T_lay, albedo, c.starflux)
        columns = [None, dict(surf_albedo=albedo)]
        bound = sr.rel_bound(rows, k, tsr.NSWEEP)
        rt.keep_down_fluxes(True)
        rt.build_planck_table(1)
        rt.refresh()
        assert not np.array_equal(rt.coef_planes(0), rt.coef_planes(1))
        worst = 0.0
        for it in (1, 2, 3):
            held = [_hold_step(rt, c, it, bound, "serpentine column %d" % col, col, columns[col]) for col in (0, 1)]
            for h in held:
                next(h)
            rt.step(it, step_temperature=False)
            worst = max([worst] + [next(h) for h in held])
        _record_parity("serpentine_two_columns", worst)
        rt.set_state(1, "done", np.array([1], np.int32))
        keys = sr.FLUX_KEYS + BANDS
        before = [{key: rt.get(key, col) for key in keys} for col in (0, 1)]
        rt.step(4, step_temperature=False)
        for key in keys:
            np.testing.assert_array_equal(rt.get(key, 1).view(np.uint64), before[1][key].view(np.uint64), err_msg=key)
        assert any(not np.array_equal(rt.get(key, 0), before[0][key]) for key in sr.FLUX_KEYS), "column 0 did not move"
        assert [int(rt.get("done", col)[0]) for col in (0, 1)] == [0, 1]
    finally:
        rt.close()
