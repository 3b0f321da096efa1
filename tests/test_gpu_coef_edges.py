"""The coefficient refresh (k_rt_coef / k_rt_coef_f32, slab_coeffs, the matrix method's vote; the stage kernels
calc_trans_iso / calc_trans_noniso) on the crafted columns of tests/coef_cases.py, held to the long-double restatement of
tests/coef_reference.py.

The tolerance rule is lines_cases.check_rule's with two changes the cancellations of the formulas force: deviations are
ABSOLUTE, on the scale 1 for alpha and beta and 2 pi epsi for u', v', dd, du (the beam planes also over the largest
|beam| of the spectral point), and eps is the fp64 twin's largest deviation over the slots of the same GROUP and plane.
Bound = max(lines_cases.FLOOR, lines_cases.MARGIN eps); tests/test_coef_cases.py caps it on the CPU.  The group
thin_exact sits ON delta_tau_limit, where a rounding picks the branch: its sources are held to the twin's branch."""
import contextlib
import os

import numpy as np
import pytest

import cases
import coef_cases as cc
import coef_reference as cr
import fused_helpers as fh
import lines_cases
from plane_coding import decode_slot, encode_planes
from sweep_reference import planes_of as _planes_of, slots as _slots

pytestmark = pytest.mark.gpu
KNOBS = ("HELIOS_RT_K", "HELIOS_RT_GENERIC_SCANS", "HELIOS_RT_MAXTHREADS", "HELIOS_RT_COEF_TPB", "HELIOS_RT_CLOUD_LDS")
ALL = [(f, s) for f in cc.FLAG_SETS for s in cc.SHAPES]
_kept = {}


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    c = Context(0)
    yield c


@contextlib.contextmanager
def _knobs(env):
    """exactly these tuning knobs while a batch is created (hx_rt_create reads them), the others unset"""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in env.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _refresh(ctx, c, env=None, debug=0):
    """one refresh and no iteration: the tiling, the planes, the arrays the refresh consumed and, with debug = 1, the count
    of limited G+-"""
    from helios_amd.rt import batch_from_case
    c = c.copy()
    c.debug = debug
    with _knobs(env or {}):
        rt = batch_from_case(ctx, c)
    try:
        rt.keep_down_fluxes(True)
        rt.build_planck_table(1 if c.T_star > 10 else 0)
        ctx.diag_reset()
        rt.refresh()
        keys = ["opac_wg_lay", "scat_cross_lay", "meanmolmass_lay"] + (["g_0_tot_lay"] if c.clouds else []) \
            + (["F_dir_wg"] if c.dir_beam else [])
        if not c.iso:
            keys += ["opac_wg_int", "scat_cross_int", "meanmolmass_int"] + (["g_0_tot_int"] if c.clouds else []) \
                + (["Fc_dir_wg"] if c.dir_beam else [])
        return dict(tiling=rt.flux_tiling(), planes=rt.coef_planes(0), src={k: rt.get(k) for k in keys},
                    g_limited=ctx.diag()["g_limited"])
    finally:
        rt.close()


def _base(ctx, flagset, shape):
    """the default fp64 run of a case with its restatements (once per module)"""
    key = (flagset, shape)
    if key not in _kept:
        c = cc.make(flagset, shape)
        run = _refresh(ctx, c)
        _kept[key] = (c, run) + cc.restated(c, run["src"])
    return _kept[key]


def _stored(c, run):
    """the stored planes by (plane, half-layer, bin, Gauss point): what two tilings of one column must agree on bit for bit"""
    t, p = run["tiling"], run["planes"]
    H = c.nlayer if c.iso else 2 * c.nlayer
    x, y, h, pad = _slots(t, c.nbin, c.ny, H)
    out = np.zeros((t["nplane"], H * c.nbin * c.ny), p.dtype)
    out[:, ((h * c.nbin + x) * c.ny + y)[~pad]] = p.transpose(1, 0, 2, 3)[:, ~pad]
    return out


def _check_planes(c, run, ld, f64, idx, beam_max, scatters):
    t, p64 = run["tiling"], run["planes"]
    X, Y = c.nbin, c.ny
    H = c.nlayer if c.iso else 2 * c.nlayer
    assert p64.dtype == np.float64 and t["coef_bytes"] == 8
    assert t["nplane"] == 3 + int(c.scat_corr) + 2 * int(c.dir_beam) and t["has_vp"] == int(c.scat_corr), t
    assert np.all(np.isfinite(p64)), "%d NaN or inf in the planes, first at %s" % (
        np.sum(~np.isfinite(p64)), decode_slot(t, np.nonzero(~np.isfinite(p64.ravel()))[0][0], X))
    x, y, h, pad = _slots(t, X, Y, H)
    assert p64.shape == (x.shape[0], t["nplane"], x.shape[1], 64)
    j = ((h * X + x) * Y + y)[~pad]
    assert np.array_equal(np.sort(j), np.arange(H * X * Y)), "every half-layer of every spectral point has one slot"
    # padding: alpha = 1, beta = 0, zeros
    pp = p64.transpose(1, 0, 2, 3)[:, pad]
    assert np.all(pp[0] == 1.0) and np.all(pp[1:] == 0.0)
    got = {p: v[~pad] for p, v in _planes_of(c, t, p64).items()}
    want, twin = cr.planes(ld, scatters), cc.twin_planes(c, f64, scatters)
    groups = cc.group_of_slots(c, idx)
    flat = np.nonzero(~pad.ravel())[0]
    fails, lines, alts = [], [], None
    for p in got:
        scale = np.broadcast_to(cr.plane_scale(p, c.epsi, np.maximum(beam_max, 1e-300)), beam_max.shape)
        dev = (np.abs(got[p] - want[p][j]) / scale[j]).astype(np.float64)
        eps_slot = (np.abs(twin[p].astype(cr.LD) - want[p]) / scale).astype(np.float64)
        for g in sorted(set(groups)):
            sel = groups[j] == g
            if g == cc.EXACT_GROUP and p in ("up", "vp") and not c.iso:
                # the twin's branch; the bound is a hundredth of what taking the other branch would change
                if alts is None:
                    inp, fl = cc.slot_inputs(c, run["src"])[0], cr.flags_of_case(c)
                    alts = [cr.planes(cr.restate(inp, cr.Flags(**dict(fl, delta_tau_limit=lim))), scatters) for lim in (0.0, 1.0)]
                other = max(float(np.max(np.abs(want[p] - alt[p])[groups == g] / scale[groups == g])) for alt in alts)
                d = (np.abs(got[p] - twin[p][j]) / scale[j])[sel]
                bound = other / 100.0
            else:
                d, bound = dev[sel], max(lines_cases.FLOOR, lines_cases.MARGIN * float(eps_slot[groups == g].max()))
            worst = int(np.argmax(d))
            lines.append("%-12s %-5s worst %.2e bound %.2e" % (g, p, d[worst], bound))
            if not d[worst] <= bound:
                s = flat[sel][worst]          # the slot's flat (tile, row, lane); plane 0 for the address
                tile, rem = divmod(int(s), t["ROWS"] * 64)
                fails.append((g, p, float(d[worst]), bound, decode_slot(t, tile * t["nplane"] * t["ROWS"] * 64 + rem, X)))
    print("\n%s %s rows %d k %d:\n  " % (c.flagset, c.shape_name, t["ROWS"], t["k"]) + "\n  ".join(lines))
    assert not fails, fails
    # exact where the design says exact
    cube = {p: np.empty(H * X * Y) for p in got}
    for p in got:
        cube[p][j] = got[p]
        cube[p] = cube[p].reshape(H, X, Y)
    sc = scatters.reshape(H, X, Y)[0]
    for xb, b in enumerate(c.bins):
        if b["expect"].get("alpha0"):
            assert np.all(cube["alpha"][:, xb, :] == 0.0), (b["group"], b["name"], "alpha == 0")
        if b["expect"].get("nan_beam"):
            assert np.all(cube["dd"][:, xb, :] == 0.0) and np.all(cube["du"][:, xb, :] == 0.0), (b["name"], "NaN beam terms are 0")
    beta0 = np.all(cube["beta"] == 0.0, axis=0)
    twin_beta0 = np.all(np.where(scatters, f64["beta"], 0.0).reshape(H, X, Y) == 0.0, axis=0)
    assert np.all(beta0[~sc]), "a pure-absorption point has beta == 0 in every half-layer"
    assert np.array_equal(beta0[sc], twin_beta0[sc]), "and no scattering point, unless N itself is 0 (trans = 1: the vacuum)"
    return cube


# ---- (a) the fp64 planes against the restatement ------------------------------------------------------------------------

@pytest.mark.parametrize("flagset,shape", ALL)
def test_planes_against_the_restatement(ctx, flagset, shape):
    """alpha, beta, u', v' (as k_rt_flux forms it), dd, du of every slot under the rule; padding, thick slots, the votes of
    the matrix method and NaN beam terms exactly; no NaN or inf in a plane; the count of limited G+- with debug = 1; and
    the same bits in both workgroup shapes and, with clouds, with the cloud terms in LDS or read from the bin-major rows"""
    c, run, ld, f64, idx, beam_max, scatters = _base(ctx, flagset, shape)
    _check_planes(c, run, ld, f64, idx, beam_max, scatters)
    if not c.iso:
        exact = cc.group_of_slots(c, idx) == cc.EXACT_GROUP
        assert np.any(f64["dtau"][exact] == c.delta_tau_limit), "no half-layer sits on delta_tau_limit exactly"
    variants = [dict(HELIOS_RT_MAXTHREADS=64)]
    if c.clouds:
        variants += [dict(HELIOS_RT_CLOUD_LDS=0), dict(HELIOS_RT_CLOUD_LDS=1), dict(HELIOS_RT_CLOUD_LDS=0, HELIOS_RT_MAXTHREADS=64)]
    for env in variants:
        other = _refresh(ctx, c, env)
        assert other["tiling"]["threads"] == 64 or "HELIOS_RT_MAXTHREADS" not in env, other["tiling"]
        np.testing.assert_array_equal(_stored(c, other).view(np.uint64), _stored(c, run).view(np.uint64), err_msg=str(env))
    if c.dir_beam:
        dbg = _refresh(ctx, c, debug=1)
        np.testing.assert_array_equal(_stored(c, dbg).view(np.uint64), _stored(c, run).view(np.uint64))
        want = int(ld["g_limited"].sum())
        print("limited G+-: %d counted, %d restated (fp64 twin %d)" % (dbg["g_limited"], want, int(f64["g_limited"].sum())))
        assert dbg["g_limited"] == want == int(f64["g_limited"].sum())
        if flagset in ("beam_glimit", "beam_nan"):
            assert want > 0
        assert run["g_limited"] == 0        # debug = 0: not counted


# ---- (b) the fp32 planes ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("flagset,shape", ALL)
def test_fp32_planes_are_the_fp64_planes_coded_once_at_the_edges(ctx, flagset, shape):
    """precision = single on the same columns: the fp32 image is plane_coding.encode_planes of the fp64 image, bit for bit
    (-0.0 rest, a rest slightly negative at w0_limit, zeros, beam terms with G+- at 1e8).  The matrix method keeps fp64 planes: there
    the batch says so and the planes are the fp64 run's"""
    c, run = _base(ctx, flagset, shape)[:2]
    s = _refresh(ctx, cc.make(flagset, shape, prec="single"))
    t = s["tiling"]
    if c.get("flux_calc_method", "iteration") == "matrix":     # the direct solve reads fp64 planes whatever the precision asked
        assert t == run["tiling"] and t["coef_bytes"] == 8
        np.testing.assert_array_equal(s["planes"].view(np.uint64), run["planes"].view(np.uint64))
        return
    assert t["coef_bytes"] == 4 and s["planes"].dtype == np.float32
    assert {k: v for k, v in t.items() if k != "coef_bytes"} == {k: v for k, v in run["tiling"].items() if k != "coef_bytes"}
    enc = encode_planes(run["planes"], t)
    assert np.all(np.isfinite(enc)) and np.all(np.isfinite(s["planes"]))
    bad = np.nonzero(enc.view(np.uint32).ravel() != s["planes"].view(np.uint32).ravel())[0]
    assert bad.size == 0, "%d of %d slots differ; first at %s: fp64 %r, coded %r, stored %r" % (
        bad.size, enc.size, decode_slot(t, bad[0], c.nbin), float(run["planes"].ravel()[bad[0]]), float(enc.ravel()[bad[0]]),
        float(s["planes"].ravel()[bad[0]]))


# ---- (c) the stage kernels, thresholds hit exactly ----------------------------------------------------------------------

def _stage_problem(iso):
    """arrays handed to calc_trans_* directly.  The limits are powers of two and the inputs small whole numbers, so the
    quotients are exact in fp64 and in long double alike and the comparisons (all strict) see EQUAL operands:
    w0 == i2s_transition = 1/8, w0 == w_0_scat_limit = 2^-10, dtau == 2^-13; g0 == -0.0 (>= 0: the fit is on); 0/0"""
    X, Y, L = 9, 2, 3
    #        ray  kap          g0      what
    rows = [(1.0, 7.0, 0.3),                    # w0 == i2s_transition: the fit stays off
            (1.0, 7.0 * (1 - 1e-6), 0.3),       # just above: on
            (1.0, 1023.0, 0.3),                 # w0 == w_0_scat_limit: no vote
            (1.0, 1023.0 * (1 - 1e-6), 0.3),    # just above: votes
            (0.5, 0.5, -0.0),                   # g0 == -0.0: on (and dtau = dcol exactly)
            (0.5, 0.5, -1e-300),                # g0 < 0: off
            (0.0, 0.0, 0.2),                    # 0 / 0: w0 = w_0_limit, dtau = 0
            (0.0, 3.0, 0.2),                    # no scattering at all
            (1.0, 1.0, 0.85)]
    ray, kap, g0 = (np.array([r[i] for r in rows]) for i in range(3))
    nlev = L if iso else L + 1
    src = dict(opac_wg_lay=np.tile(np.repeat(kap, Y), L), opac_wg_int=np.tile(np.repeat(kap, Y), L + 1),
               scat_cross_lay=np.tile(ray, L), scat_cross_int=np.tile(ray, L + 1), meanmolmass_lay=np.ones(L),
               meanmolmass_int=np.ones(L + 1), g_0_tot_lay=np.tile(g0, L), g_0_tot_int=np.tile(g0, L + 1))
    c = cases.Case(nbin=X, ny=Y, nlayer=L, iso=iso, clouds=1, scat=1, dir_beam=0, scat_corr=1, g_0=0.0, epsi=0.5, epsi2=0.5,
                   mu_star=-0.6, i2s_transition=0.125, w_0_limit=1.0 - 1e-10, w_0_scat_limit=2.0 ** -10,
                   delta_tau_limit=2.0 ** -13)
    for nm, n in (("lay", L), ("int", L + 1)):
        c["abs_cross_all_clouds_" + nm] = np.zeros(n * X)
        c["scat_cross_all_clouds_" + nm] = np.zeros(n * X)
    c.delta_colmass = np.full(L, 2.0 ** -13)
    c.delta_col_upper, c.delta_col_lower = np.full(L, 2.0 ** -13), np.full(L, 2.0 ** -13)
    c.bins = [dict(group="stage")] * X
    return c, src, nlev


@pytest.mark.parametrize("iso", [0, 1])
def test_stage_kernels_on_exact_thresholds(ctx, iso):
    """calc_trans_iso / calc_trans_noniso through the hip stage backend against the restatement under the rule (scale
    max(1, |value|), one group); equality takes the "not" side of every strict comparison, in the kernel, the twin and the
    long double alike; scat_trigger and the count of limited G+- exactly"""
    from impls import HipBackend
    raw = HipBackend(ctx)
    c, src, nlev = _stage_problem(iso)
    X, Y, L = c.nbin, c.ny, c.nlayer
    inp, idx, _ = cc.slot_inputs(c, src)
    fl = cr.flags_of_case(c, need_G=True)
    ld, f64 = cr.restate(inp, fl, cr.LD), cr.restate(inp, fl, np.float64)
    H = L if iso else 2 * L
    for key in ("i2s_on", "vote", "clamped", "g_limited"):
        assert np.array_equal(ld[key], f64[key]), key
    on, vote = ld["i2s_on"].reshape(H, X, Y)[0, :, 0], ld["vote"].reshape(H, X, Y)[0, :, 0]
    assert on.tolist() == [False, True, False, False, True, False, True, False, True], on.tolist()
    assert vote.tolist() == [True, True, False, True, True, True, True, False, True], vote.tolist()
    assert np.all(ld["w0"].reshape(H, X, Y)[:, 0] == 0.125) and np.all(f64["dtau"].reshape(H, X, Y)[:, 4] == 2.0 ** -13)
    n = Y * X * (L + 1)
    trig = np.zeros(Y * X, np.int32)
    ctx.diag_reset()
    if iso:
        o = {k: np.zeros(n) for k in ("trans", "dtau_gas", "M", "N", "P", "Gp", "Gm", "w0")}
        raw.calc_trans_iso(o["trans"], o["dtau_gas"], o["M"], o["N"], o["P"], o["Gp"], o["Gm"], c.delta_colmass,
                           src["opac_wg_lay"], src["meanmolmass_lay"], src["scat_cross_lay"], c.abs_cross_all_clouds_lay,
                           c.scat_cross_all_clouds_lay, np.zeros(X * L), o["w0"], src["g_0_tot_lay"], trig, c.g_0, c.epsi,
                           c.epsi2, c.mu_star, c.w_0_limit, c.w_0_scat_limit, c.scat, X, Y, L, c.clouds, c.scat_corr, 1,
                           c.i2s_transition)
        got = {k: v[:Y * X * L] for k, v in o.items()}
    else:
        o = {k + sfx: np.zeros(n) for k in ("trans", "dtau_gas", "M", "N", "P", "Gp", "Gm", "w0") for sfx in ("_u", "_l")}
        raw.calc_trans_noniso(o["trans_u"], o["trans_l"], o["dtau_gas_u"], o["dtau_gas_l"], o["M_u"], o["M_l"], o["N_u"],
                              o["N_l"], o["P_u"], o["P_l"], o["Gp_u"], o["Gp_l"], o["Gm_u"], o["Gm_l"], c.delta_col_upper,
                              c.delta_col_lower, src["opac_wg_lay"], src["opac_wg_int"], src["meanmolmass_lay"],
                              src["meanmolmass_int"], src["scat_cross_lay"], src["scat_cross_int"],
                              c.abs_cross_all_clouds_lay, c.abs_cross_all_clouds_int, c.scat_cross_all_clouds_lay,
                              c.scat_cross_all_clouds_int, np.zeros(X * L), np.zeros(X * L), o["w0_u"], o["w0_l"],
                              src["g_0_tot_lay"], src["g_0_tot_int"], trig, c.g_0, c.epsi, c.epsi2, c.mu_star, c.w_0_limit,
                              c.w_0_scat_limit, c.scat, X, Y, L, c.clouds, c.scat_corr, 1, c.i2s_transition)
        got = {k: np.stack([o[k + "_l"][:Y * X * L].reshape(L, -1), o[k + "_u"][:Y * X * L].reshape(L, -1)], axis=1).reshape(-1)
               for k in ("trans", "dtau_gas", "M", "N", "P", "Gp", "Gm", "w0")}
    for key, v in got.items():
        want, twin = ld[key], f64[key]
        assert np.all(np.isfinite(v)), key
        scale = np.maximum(1.0, np.abs(want))
        dev = float(np.max(np.abs(v - want) / scale))
        bound = max(lines_cases.FLOOR, lines_cases.MARGIN * float(np.max(np.abs(twin - want) / scale)))
        print("%s: worst %.2e bound %.2e" % (key, dev, bound))
        assert dev <= bound, (key, dev, bound)
    assert np.array_equal(trig.reshape(X, Y), ld["vote"].reshape(H, X, Y).any(axis=0).astype(np.int32))
    assert ctx.diag()["g_limited"] == int(ld["g_limited"].sum())


# ---- (d) one flux solve -------------------------------------------------------------------------------------------------

FLUX_KEYS = ["F_up_wg", "F_down_wg", "Fc_up_wg", "Fc_down_wg"]
SWAP = dict(w0="w_0", trans="trans_wg", M="M", N="N", P="P", Gp="G_plus", Gm="G_minus")


def _oracle_solves(port, c0, grid):
    """the oracle's first flux solve twice: on its own coefficient arrays, and with them replaced by the long-double
    restatement rounded to double -- how much of the reference's own coefficient noise reaches the fluxes"""
    outs = []
    for swap in (False, True):
        c = c0.copy()
        s = cases.alloc_state(c)
        s.planck_grid[:] = grid
        cases.interpolate_temperatures_and_planck(port, c, s)
        cases.refresh_premixed(port, c, s)
        if swap:
            inp, idx, _ = cc.slot_inputs(c, dict(s))
            ld = cr.restate(inp, cr.flags_of_case(c, need_G=True), cr.LD)
            X, Y, L = c.nbin, c.ny, c.nlayer
            for key, nm in SWAP.items():
                v = np.asarray(ld[key], np.float64)
                if c.iso:
                    s[nm if nm in ("w_0", "trans_wg", "G_plus", "G_minus") else nm + "_term"][:Y * X * L] = v
                else:
                    v = v.reshape(L, 2, X * Y)
                    s[nm + "_lower"][:Y * X * L] = v[:, 0].reshape(-1)
                    s[nm + "_upper"][:Y * X * L] = v[:, 1].reshape(-1)
        cases.flux_sweeps(port, c, s)
        outs.append({k: np.array(s[k]) for k in FLUX_KEYS})
    return outs


@pytest.mark.parametrize("flagset,shape", [(f, s) for f in cc.FLAG_SETS for s in ("L9", "iso20")] + [("plain", "L100"),
                                                                                                       ("matrix_clouds", "L100")])
def test_one_flux_solve_against_the_oracle(ctx, port, flagset, shape):
    """F_up_wg, F_down_wg and the layer-centre fluxes after one iteration against the oracle on the device's Planck table,
    bin by bin: 1e-9 |oracle| + 1e-13 of the largest flux (fused_helpers.compare's rule) where the group's plane bounds are
    at the floor; elsewhere the larger of that and MARGIN times what the reference's own coefficient noise moves the bin's
    fluxes (measured on the CPU), which must stay under 1e-5 of the bin's largest flux.

    [matrix_clouds-L100], bin w0_limit t700 (pure scatterers clamped at w_0_limit, 200 half-layers of dtau = 700) is the
    case that found the direct solve composing the reflectivity's Moebius map in rho itself: nine digits of rho lost in
    the product, the fluxes 5.5e-5 (272 bounds) off the oracle, which sits on tests/matrix_referee.py's extended solve."""
    c = cc.make(flagset, shape)
    f, grid = fh.run_fused(ctx, c, 1, keys=FLUX_KEYS + ["F_dir_wg"], with_planck_grid=True)
    own, swapped = _oracle_solves(port, c, grid)
    _, _, ld, f64, idx, beam_max, scatters = _base(ctx, flagset, shape)
    want, twin = cr.planes(ld, scatters), cc.twin_planes(c, f64, scatters)
    groups = cc.group_of_slots(c, idx)
    noisy = set()
    for p in want:
        if p in ("dd", "du") and not c.dir_beam:
            continue
        scale = cr.plane_scale(p, c.epsi, np.maximum(beam_max, 1e-300))
        dev = (np.abs(twin[p].astype(cr.LD) - want[p]) / scale).astype(np.float64)
        noisy |= {g for g in set(groups) if lines_cases.MARGIN * dev[groups == g].max() > lines_cases.FLOOR}
    X, Y, L = c.nbin, c.ny, c.nlayer
    scale_all = max(np.abs(own["F_down_wg"]).max(), np.abs(f["F_dir_wg"]).max(), np.abs(own["F_up_wg"]).max())
    keys = [k for k in FLUX_KEYS if not (c.iso and k.startswith("Fc_"))]
    fails, lines = [], []
    for x, b in enumerate(c.bins):
        worst = 0.0
        largest = max(float(np.abs(np.asarray(own[k])[:Y * X * L].reshape(L, X, Y)[:, x]).max()) for k in keys)
        for k in keys:
            nlev = L if k.startswith("Fc_") else L + 1
            a, o, o2 = (np.asarray(v)[:Y * X * nlev].reshape(nlev, X, Y)[:, x] for v in (f[k], own[k], swapped[k]))
            assert np.all(np.isfinite(a)), (k, b["group"], b["name"])
            bound = 1e-9 * np.abs(o) + 1e-90 + 1e-13 * scale_all
            if b["group"] in noisy:
                moved = float(np.max(np.abs(o - o2)))
                assert lines_cases.MARGIN * moved <= 1e-5 * largest, (k, b["group"], b["name"], moved, largest)
                bound = np.maximum(bound, lines_cases.MARGIN * moved)
            ratio = float(np.max(np.abs(a - o) / bound))
            worst = max(worst, ratio)
            if ratio > 1.0:
                fails.append((k, b["group"], b["name"], ratio))
        lines.append("%-12s %-12s %s worst deviation %.3f of its bound" % (b["group"], b["name"], "noisy" if b["group"] in noisy else "floor",
                                                                          worst))
    print("\n%s %s\n  " % (flagset, shape) + "\n  ".join(lines))
    assert not fails, fails
