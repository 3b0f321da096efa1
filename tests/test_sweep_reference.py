"""tests/sweep_reference.py on the CPU: its restatement of the flux sweeps is the reference's physics (the CPU oracle on
crafted columns), the rule holds for a twin that rounds where k_rt_flux rounds at every tiling of the GPU case list
(tests/test_gpu_flux_sweeps.py), every mutant of the twin breaks it, and the companion magnitude hides nothing.

The tilings are the table below -- which (rows, k) the library selects for which layer counts; the GPU module asserts it
against hx_rt_flux_geometry.  The planes of (2) - (4) are synthetic (no refresh runs here): drawn per half-layer with
0 <= alpha, 0 <= beta, alpha + beta <= 1 and sources of the size Kconst (1 - alpha - beta) B, with opaque half-layers
(alpha = 0), transparent ones (alpha = 1, beta = 0, no sources), thin tops, a pure absorber and a point at w0 = 1 - 1e-10."""
import numpy as np
import pytest

import cases
import coef_cases as cc
import coef_reference as cr
import sweep_reference as sr
from helios_amd import phys_const as pc
from test_gpu_precision_tilings import KNOB_CASES, _flags

# {(rows, k, isothermal): (smallest, largest layer count)} of the selection over 1-416 layers and 1-832 isothermal ones
SELECTED = {
    (1, 8, 0): (1, 4), (3, 8, 0): (9, 12), (1, 16, 0): (5, 8), (2, 16, 0): (13, 16), (3, 16, 0): (17, 24), (4, 16, 0): (25, 32),
    (5, 16, 0): (33, 40), (6, 16, 0): (41, 48), (7, 16, 0): (49, 56), (8, 16, 0): (57, 64), (9, 16, 0): (65, 72),
    (10, 16, 0): (73, 80), (11, 16, 0): (81, 88), (12, 16, 0): (89, 96), (13, 16, 0): (97, 104), (14, 16, 0): (105, 112),
    (8, 32, 0): (113, 128), (9, 32, 0): (129, 144), (10, 32, 0): (145, 160), (11, 32, 0): (161, 176), (12, 32, 0): (177, 192),
    (13, 32, 0): (193, 208), (7, 64, 0): (209, 224), (8, 64, 0): (225, 256), (9, 64, 0): (257, 288), (10, 64, 0): (289, 320),
    (11, 64, 0): (321, 352), (12, 64, 0): (353, 384), (13, 64, 0): (385, 416),
    (1, 8, 1): (1, 8), (3, 8, 1): (17, 24), (1, 16, 1): (9, 16), (2, 16, 1): (25, 32), (3, 16, 1): (33, 48), (4, 16, 1): (49, 64),
    (5, 16, 1): (65, 80), (6, 16, 1): (81, 96), (7, 16, 1): (97, 112), (8, 16, 1): (113, 128), (9, 16, 1): (129, 144),
    (10, 16, 1): (145, 160), (11, 16, 1): (161, 176), (12, 16, 1): (177, 192), (13, 16, 1): (193, 208), (14, 16, 1): (209, 224),
    (8, 32, 1): (225, 256), (9, 32, 1): (257, 288), (10, 32, 1): (289, 320), (11, 32, 1): (321, 352), (12, 32, 1): (353, 384),
    (13, 32, 1): (385, 416), (7, 64, 1): (417, 448), (8, 64, 1): (449, 512), (9, 64, 1): (513, 576), (10, 64, 1): (577, 640),
    (11, 64, 1): (641, 704), (12, 64, 1): (705, 768), (13, 64, 1): (769, 832)}
# (layers, isothermal) -> (rows, k) beyond 16 rows: 20, 24 and 32 rows on 64 lanes
DEEP = {(600, 0): (20, 64), (1024, 0): (32, 64), (1500, 1): (24, 64)}
# tests/test_gpu_fused.py's "L3" and "L2_beam": six and four half-layers on eight lanes, lanes without a row
SHALLOW = [("L3", 3, dict(nbin=3, albedo=0.3)), ("L2_beam", 2, dict(nbin=3, albedo=0.2, dir_beam=1))]


def selected(nlayer, iso):
    for (rows, k, i), (lo, hi) in SELECTED.items():
        if i == iso and lo <= nlayer <= hi:
            return rows, k
    return DEEP[(nlayer, iso)]


def sweep_cases():
    """[(name, layers, isothermal, knobs, make_case keywords, (rows, k, generic scans))]: both ends of every selected range
    (one layer left out: the synthetic column needs two for its heights), the knob cases of
    tests/test_gpu_precision_tilings.py, the deep columns and the shallow ones; the flags rotate as _flags(i) there"""
    out = []
    for (r, k, iso), (lo, hi) in sorted(SELECTED.items(), key=lambda kv: (kv[0][2], kv[0][1], kv[0][0])):
        for L in sorted({max(2, lo), hi}):
            out.append(("%srows%d_k%d_L%d" % ("iso_" if iso else "", r, k, L), L, iso, {}, None, (r, k, 0)))
    for name, L, env in KNOB_CASES:
        H = 2 * L
        if "HELIOS_RT_K" in env:
            want = (-(-H // env["HELIOS_RT_K"]), env["HELIOS_RT_K"], 0)
        else:
            want = selected(L, 0) + (int(env.get("HELIOS_RT_GENERIC_SCANS", 0)),)
        out.append((name, L, 0, env, None, want))
    for (L, iso), (r, k) in sorted(DEEP.items()):
        out.append(("%sdeep_rows%d_L%d" % ("iso_" if iso else "", r, L), L, iso, {}, None, (r, k, 0)))
    out = [(n, L, iso, env, _flags(i), want) for i, (n, L, iso, env, _, want) in enumerate(out)]
    for name, L, kw in SHALLOW:
        out.append((name, L, 0, {}, kw, selected(L, 0) + (0,)))
    return out


CASES = sweep_cases()
NSWEEP = 4          # 3 scat + 1 (hx_rt_create): every case here scatters


# ---- synthetic planes ------------------------------------------------------------------------------------------------

def synthetic(H, iso, beam, has_vp, seed, kind="generic", nbin=2, ny=3):
    """inputs of restate / scan_twin for nbin x ny points over H half-layers (see the module's docstring).  kind "thin": no
    opaque half-layer and a beam that reaches the surface.  kind "underflow": every flux below 1e-100 -- Planck values and a beam of 1e-120 -- in a purely absorbing column with an up-source of
    -20 B in a few half-layers below a layer centre, large enough to make the up-flux there negative, and one of +40 B in
    the half-layer above, which makes it positive again at the interface; alpha = 0.1 in both, so that neither value is the
    small difference of large terms.  The reference leaves the negative value at the centre alone and tiny() has nothing to
    turn at the interface; with the parity swapped the centre's value is turned and the interface's moves by 0.1 of it
    -- and, since beta = 0.05 in the half-layer above, the next sweep's down-flux at the centre by 0.05 of it: at one row per
    lane a turned value never reaches another row of the same sweep, and that is where the swap still shows.
    (A flux that tiny() DOES turn is kept out of these columns on purpose: the kernel turns it in the replay of its own
    lane only -- the lanes' compositions are affine -- so lanes above it would see it unturned, 1e-100 away from the
    reference.  No column produces one: u', v' and the beam sources min(0, .) / M are not negative.)"""
    rng = np.random.default_rng(seed)
    n = nbin * ny
    Kconst = np.pi
    w0 = rng.uniform(0.05, 0.95, n)
    w0[0], w0[-1] = 0.0, 1.0 - 1e-10
    dtau = 10.0 ** rng.uniform(-3.0, 1.0, (H, n))
    scale = 1.0
    turned = np.array([h for h in sorted({2, 2 * (H // 4), 2 * (H // 3)}) if h + 1 < H])    # even half-layers: odd top nodes
    if kind == "underflow":
        w0[:] = 0.0
        scale = 1e-120
        dtau[turned], dtau[turned + 1] = -0.5 * np.log(0.1), -0.5 * np.log(0.1)          # alpha = 0.1 in both
    elif kind == "thin":                                    # the whole column a few tenths deep: the beam reaches the surface
        dtau = 10.0 ** rng.uniform(-4.0, -2.0, (H, n))
    else:
        dtau[H - max(1, H // 8):] *= 1e-6                   # thin top
    alpha = np.exp(-2.0 * dtau * np.sqrt(1.0 - w0))
    beta = (1.0 - alpha) * 0.9 * w0
    opaque = rng.choice(H, max(1, H // 16), replace=False)
    clear = np.setdiff1d(rng.choice(H, max(1, H // 16), replace=False), opaque)
    if kind != "generic":
        opaque, clear = opaque[:0], clear[:0]
    if kind == "underflow":
        beta[turned + 1] = 0.05
    alpha[opaque], beta[opaque] = 0.0, 0.3 * w0
    alpha[clear], beta[clear] = 1.0, 0.0
    rest = (1.0 - alpha) - beta
    f = rng.uniform(0.35, 0.5, (H, n))
    up = Kconst * rest * f
    vp = Kconst * rest * (1.0 - f) * rng.uniform(0.9, 1.1, (H, n)) if has_vp else None
    B0 = np.repeat(rng.uniform(0.5, 2.0, nbin) * 1e3, ny) * scale
    B = B0 * np.exp(-2.0 * np.arange(H + 1)[:, None] / H) * np.repeat(rng.uniform(0.95, 1.05, (H + 1, nbin)), ny, axis=1)
    inp = dict(alpha=alpha, beta=beta, up=up, vp=vp, B=B, Bstar=50.0 * B0, Bsurf=1.3 * B[0], iso=int(iso), dir_beam=int(beam),
               Kconst=Kconst, albedo=np.repeat(np.linspace(0.2, 0.35, nbin), ny), boaK=(1.0 - w0) / (1.1 - w0),
               f_factor=0.5, R_star=pc.R_SUN, a=0.05 * pc.AU, U=B * rng.uniform(0.5, 1.5, (H + 1, n)))
    if beam:
        F = np.empty((H + 1, n))
        F[H] = 3.0 * B0
        for h in range(H - 1, -1, -1):
            F[h] = F[h + 1] * np.exp(-dtau[h] / 0.5)
        absorbed = F[1:] - F[:-1]
        inp["dd"], inp["du"], inp["Fdir0"] = 0.3 * np.maximum(w0, 0.1) * absorbed, 0.2 * np.maximum(w0, 0.1) * absorbed, F[0]
        if kind == "underflow":
            inp["du"][turned], inp["du"][turned + 1] = -20.0 * B[turned], 40.0 * B[turned]
        inp["dd"][clear], inp["du"][clear] = 0.0, 0.0
    else:
        inp["Fdir0"] = np.zeros(n)
    return inp


def _flat(res, step):
    """U and D of a step side by side, [2][H + 1][points]"""
    return np.array([res["U"][step], res["D"][step]])


# ---- (1) the restatement is the reference's physics ----------------------------------------------------------------

# the restatement's coefficient names -> the oracle's arrays (test_gpu_coef_edges.py swaps the same)
SWAP = dict(w0="w_0", trans="trans_wg", M="M", N="N", P="P", Gp="G_plus", Gm="G_minus")
PHYSICS = [(f, s) for f in ("plain", "clouds", "beam_glimit", "beam_nan", "beam_graze") for s in ("L9", "iso20")]


@pytest.mark.parametrize("flagset,shape", PHYSICS)
def test_the_restatement_is_the_oracles_flux_solve(port, flagset, shape):
    """planes from coef_reference.restate in long double on the arrays of the oracle's own refresh, Planck nodes, beam and
    albedo from the oracle's state; one iteration from a zero state against the oracle's F_up_wg, F_down_wg, Fc_up_wg,
    Fc_down_wg under fused_helpers.compare's rule (1e-8 |oracle| + 1e-90 + 1e-13 of the largest flux).  The oracle solves
    on its coefficient arrays replaced by the same restatement rounded to double, as
    test_gpu_coef_edges.py::test_one_flux_solve_against_the_oracle does for the groups whose fp64 coefficients are noise
    (thick, w0_limit, thin_exact): the sweeps are compared here, not the refresh.  And the magnitude hides nothing: at most
    1 % of the entries have m > 100 |value|."""
    c, s = cc.oracle_state(port, cc.make(flagset, shape))
    X, Y, L, iso = c.nbin, c.ny, c.nlayer, int(c.iso)
    H = L if iso else 2 * L
    slot_in, idx, _ = cc.slot_inputs(c, dict(s))
    ld = cr.restate(slot_in, cr.flags_of_case(c, need_G=True), cr.LD)
    for key, nm in SWAP.items():
        v = np.asarray(ld[key], np.float64)
        if iso:
            s[nm if nm in ("w_0", "trans_wg", "G_plus", "G_minus") else nm + "_term"][:Y * X * L] = v
        else:
            v = v.reshape(L, 2, X * Y)
            s[nm + "_lower"][:Y * X * L] = v[:, 0].reshape(-1)
            s[nm + "_upper"][:Y * X * L] = v[:, 1].reshape(-1)
    cases.flux_sweeps(port, c, s)
    planes = cr.planes(cr.restate(slot_in, cr.flags_of_case(c), cr.LD), np.ones(idx.shape[1], bool))
    inp = {p: planes[p].reshape(H, X * Y) for p in ("alpha", "beta", "up", "vp")}
    if c.dir_beam:
        inp.update(dd=planes["dd"].reshape(H, X * Y), du=planes["du"].reshape(H, X * Y))
    inp["B"], inp["Bstar"], inp["Bsurf"] = sr.planck_nodes(s.planckband_lay, s.planckband_int, iso, X, Y, L)
    inp.update(iso=iso, dir_beam=int(c.dir_beam), Kconst=2.0 * np.pi * c.epsi, albedo=np.repeat(c.surf_albedo, Y),
               boaK=ld["boaK"].reshape(H, X * Y)[0], Fdir0=np.asarray(s.F_dir_wg)[:X * Y], f_factor=c.f_factor,
               R_star=c.R_star, a=c.a, U=np.zeros((H + 1, X * Y)))
    res = sr.restate(inp, 3 * c.scat + 1, 1)
    got = sr.to_wg(res["U"][0], res["D"][0], iso, L)
    scale = max(np.abs(s.F_down_wg).max(), np.abs(s.F_dir_wg).max(), np.abs(s.F_up_wg).max())
    for k in sr.FLUX_KEYS:
        if iso and k.startswith("Fc_"):
            continue
        n = Y * X * (L if k.startswith("Fc_") else L + 1)
        a, o = got[k][:n].astype(np.float64), np.asarray(s[k])[:n]
        ratio = np.abs(a - o) / (1e-8 * np.abs(o) + 1e-90 + 1e-13 * scale)
        print("%s %s %s: largest deviation %.3f of its bound" % (flagset, shape, k, ratio.max()))
        assert np.all(np.isfinite(a)) and ratio.max() <= 1.0, (k, float(ratio.max()), int(np.argmax(ratio)))
    share = sr.cancelled_fraction(_flat(res, 0), np.array([res["mU"][0], res["mD"][0]]))
    print("entries with m > 100 |value|: %.4f" % share)
    assert share <= 0.01


# ---- (2) the bound holds for the honest twin -----------------------------------------------------------------------

def test_the_bound_is_at_most_2e_13_for_every_tiling():
    bounds = {(want[0], want[1]): sr.rel_bound(want[0], want[1], NSWEEP) for _, _, _, _, _, want in CASES}
    worst = max(bounds, key=bounds.get)
    print("largest bound %.4e at rows %d, k %d; R there %d" % (bounds[worst], worst[0], worst[1],
                                                             sr.rounding_count(worst[0], worst[1], NSWEEP)))
    assert max(bounds.values()) <= 2e-13
    assert sr.rounding_count(13, 64, 4) == 2 * 4 * (39 + 12 + 4) + 8
    # the table is complete and without overlap
    for iso, top in ((0, 416), (1, 832)):
        covered = sorted((lo, hi) for (r, k, i), (lo, hi) in SELECTED.items() if i == iso)
        assert covered[0][0] == 1 and covered[-1][1] == top
        assert all(a[1] + 1 == b[0] for a, b in zip(covered, covered[1:]))
    for (r, k, iso), (lo, hi) in SELECTED.items():
        for L in (lo, hi):
            H = L if iso else 2 * L
            assert (k * (r - 1) < H <= k * r) or (r == 1 and H <= k), (r, k, iso, L)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_the_honest_twin_keeps_the_rule(case):
    """scan_twin at the case's (rows, k) on synthetic planes of the case's half-layers, beam and v' plane as the case's
    flags have them: every entry of U and D within the rule of the long-double restatement, one step from a non-zero state;
    and at most 1 % of the entries with m > 100 |value|"""
    name, L, iso, env, kw, (rows, k, _) = case
    H = L if iso else 2 * L
    inp = synthetic(H, iso, kw.get("dir_beam", 0), kw.get("scat_corr", 0), seed=1000 + CASES.index(case))
    ref = sr.restate(inp, NSWEEP, 1)
    twin = sr.scan_twin(inp, rows, k, NSWEEP, 1)
    m = np.array([ref["mU"][0], ref["mD"][0]])
    ratio, _, bad = sr.check(_flat(twin, 0), _flat(ref, 0), m, sr.rel_bound(rows, k, NSWEEP), name)
    assert bad.size == 0, (name, ratio, bad[:5])
    assert sr.cancelled_fraction(_flat(ref, 0), m) <= 0.01


# ---- (3) the rule is sharp -------------------------------------------------------------------------------------------

# (rows, k, half-layers): a partly filled last lane (34 half-layers: lane 11 holds one row of three, lanes 12-15 none),
# fewer half-layers than lanes, and 64 lanes (418 half-layers of 448)
MUTANT_TILINGS = [(3, 16, 34), (1, 8, 6), (7, 64, 418)]
# (beam, v' plane, kind): with the beam D at the top is 0 and Fdir0 is not; without it the reverse
MUTANT_COLUMNS = [(1, 1, "generic"), (0, 0, "generic"), (1, 0, "thin"), (1, 0, "underflow")]


@pytest.mark.parametrize("rows,k,H", MUTANT_TILINGS)
def test_every_mutant_breaks_the_rule(rows, k, H):
    """two steps on four columns per tiling; the honest twin holds the rule on each, and every fault of
    sweep_reference.FAULTS breaks it at some entry of some column -- the swapped parity of tiny() on the column whose fluxes
    underflow"""
    bound = sr.rel_bound(rows, k, NSWEEP, 2)
    broke = {f: [] for f in sr.FAULTS}
    for i, (beam, has_vp, kind) in enumerate(MUTANT_COLUMNS):
        inp = synthetic(H, 0, beam, has_vp, seed=77 + i, kind=kind)
        ref = sr.restate(inp, NSWEEP, 2)
        want = np.array([_flat(ref, 0), _flat(ref, 1)])
        m = np.array([[ref["mU"][s], ref["mD"][s]] for s in (0, 1)])
        if kind == "underflow":
            assert np.abs(want).max() < sr.TINY and (want < 0).any() and (want > 0).any()
        assert sr.cancelled_fraction(want, m) <= 0.01
        for fault in (None,) + sr.FAULTS:
            twin = sr.scan_twin(inp, rows, k, NSWEEP, 2, fault=fault)
            got = np.array([_flat(twin, 0), _flat(twin, 1)])
            ok = sr.holds(got, want, m, bound)
            if fault is None:
                assert ok.all(), (kind, beam, int((~ok).sum()))
            elif not ok.all():
                broke[fault].append((beam, kind, int((~ok).sum())))
    print("rows %d k %d H %d: entries that break the rule per mutant (beam, column, count): %s" % (rows, k, H, broke))
    assert all(broke.values()), [f for f, b in broke.items() if not b]
    assert any(kind == "underflow" for _, kind, _ in broke["tiny_parity"])
