"""CPU: the crafted columns of tests/coef_cases.py take the branches they are named for, the rounding noise of the
coefficient formulas stays under its caps, and the restatement of tests/coef_reference.py restates the reference (the
CPU oracle's calc_trans_iso / calc_trans_noniso).  Nothing here runs an implementation under test."""
import numpy as np
import pytest

import coef_cases as cc
import coef_reference as cr
import lines_cases

ALL = [(f, s) for f in cc.FLAG_SETS for s in cc.SHAPES]
# The largest bound max(FLOOR, MARGIN eps) a group may reach (eps: the fp64 twin's largest deviation from the long double
# over the group's slots, per plane).  1e-9 and, for w0_limit, 1e-6: eight times the worst CPU figures of the formulas
# (u' at w0 = 0.999 and at w0 = w_0_limit, just above delta_tau_limit).  beam_glimit's beam planes are the one addition:
# G+- limited at 1e8 multiply values of order one that each carry a rounding of 2^-53, so dd and du of such a slot are
# uncertain by about 1e8 x 2^-53 ~ 1e-8 of the beam whatever the order of the operations; eight times that and a sum of
# four such terms give 1e-6.
CAP, CAP_LOOSE = 1e-9, 1e-6


def cap_of(group, plane):
    if group == "w0_limit" or (group == "beam_glimit" and plane in ("dd", "du")):
        return CAP_LOOSE
    return CAP


_kept = {}


def column(port, flagset, shape):
    if (flagset, shape) not in _kept:
        c = cc.make(flagset, shape)
        c2, s = cc.oracle_state(port, c)
        src = dict(s)
        _kept[(flagset, shape)] = (c, c2, s) + cc.restated(c, src)
    return _kept[(flagset, shape)]


def group_eps(c, ld, f64, idx, beam_max, scatters):
    """{(group, plane): (eps, bound)}: the fp64 twin's largest absolute deviation from the long double on the plane's
    scale over the group's slots, and the bound of the tolerance rule that follows from it"""
    want, twin = cr.planes(ld, scatters), cc.twin_planes(c, f64, scatters)
    groups = cc.group_of_slots(c, idx)
    out = {}
    for p in cr.PLANES:
        if p in ("dd", "du") and not c.dir_beam:
            continue
        scale = cr.plane_scale(p, c.epsi, np.maximum(beam_max, 1e-300))
        dev = (np.abs(twin[p].astype(cr.LD) - want[p]) / scale).astype(np.float64)
        assert np.all(np.isfinite(dev)), (p, "the restatements hold no NaN or inf in a plane")
        for g in sorted(set(groups)):
            if g == cc.EXACT_GROUP and p in ("up", "vp") and not c.iso:
                continue        # (a rounding decides the branch there: held to the twin's branch, not to this rule)
            eps = float(dev[groups == g].max())
            out[(g, p)] = (eps, max(lines_cases.FLOOR, lines_cases.MARGIN * eps))
    return out


@pytest.mark.parametrize("flagset,shape", ALL)
def test_cases_take_their_branches_with_margin(port, flagset, shape):
    """every bin's designed outcomes (thin / clamped / I2S on / E floored / limited G / NaN beam / cut beam terms / the
    votes of the matrix method) as the restatement decides them in long double AND in fp64, every discrete comparison with a
    margin >= 1e-10; every half-layer of the column carries its bin's variant, so each group sits on lower and upper
    halves, on half-layer 0 and on the last one"""
    c, c2, s, ld, f64, idx, beam_max, scatters = column(port, flagset, shape)
    worst = cc.check_margins(c, ld, idx)
    print("\n%s %s: %d bins, %d slots; smallest margins %s" % (flagset, shape, c.nbin, idx.shape[1],
                                                               ", ".join("%s %.2e" % kv for kv in sorted(worst.items()))))
    cc.check_expectations(c, ld, f64, idx, scatters)
    H = c.nlayer if c.iso else 2 * c.nlayer
    assert idx[0].max() == H - 1 and set(cc.group_of_slots(c, idx)) == {b["group"] for b in c.bins}
    exact = cc.group_of_slots(c, idx) == cc.EXACT_GROUP
    for key in ("thin", "clamped", "i2s_on", "E_floored", "vote", "g_limited"):       # the twin decides as the long double
        assert np.array_equal(ld[key][~exact], f64[key][~exact]), key
    if not c.iso:       # the group on the limit itself: some half-layers AT it (not thin), and both branches taken
        at = f64["dtau"][exact] == c.delta_tau_limit
        print("thin_exact: %d of %d slots have dtau == delta_tau_limit, %d are thin" % (at.sum(), exact.sum(), f64["thin"][exact].sum()))
        assert at.any() and not np.any(f64["thin"][exact][at]) and f64["thin"][exact].any()
    if flagset.startswith("matrix"):
        assert scatters.any() and not scatters.all()


@pytest.mark.parametrize("flagset,shape", ALL)
def test_the_formulas_own_noise_stays_under_its_caps(port, flagset, shape):
    c, c2, s, ld, f64, idx, beam_max, scatters = column(port, flagset, shape)
    eps = group_eps(c, ld, f64, idx, beam_max, scatters)
    print("\n%s %s: fp64 twin's largest deviation from long double -> bound, per group and plane" % (flagset, shape))
    for g in sorted({g for g, _ in eps}):
        print("  %-12s " % g + "  ".join("%s %.1e -> %.1e" % (p, eps[(g, p)][0], eps[(g, p)][1]) for p in cr.PLANES if (g, p) in eps))
    over = [(g, p, e, b) for (g, p), (e, b) in eps.items() if b > cap_of(g, p)]
    assert not over, over


@pytest.mark.parametrize("flagset,shape", ALL)
def test_restatement_restates_the_oracle(port, flagset, shape):
    """w0, dtau, trans, M, N, P, G+- of the CPU oracle's calc_trans_* on the same inputs against the long double under the
    tolerance rule (absolute deviations on the scale max(1, |value|), eps the twin's largest of the group), scat_trigger
    exactly"""
    c, c2, s, _, _, idx, _, _ = column(port, flagset, shape)
    inp, idx, _ = cc.slot_inputs(c, dict(s))
    fl = cr.flags_of_case(c, need_G=True)
    ld, f64 = cr.restate(inp, fl, cr.LD), cr.restate(inp, fl, np.float64)
    X, Y, L = c.nbin, c.ny, c.nlayer
    H = L if c.iso else 2 * L
    groups = cc.group_of_slots(c, idx)

    def halves(name):
        if c.iso:
            return np.asarray(s[name]).reshape(-1, X, Y)[:L].reshape(-1)
        lo, up = (np.asarray(s[name + sfx]).reshape(-1, X, Y)[:L] for sfx in ("_lower", "_upper"))
        return np.stack([lo, up], axis=1).reshape(-1)
    names = dict(w0="w_0", dtau_gas="delta_tau_wg", trans="trans_wg", M="M", N="N", P="P", Gp="G_plus", Gm="G_minus")
    if c.iso:
        names.update(M="M_term", N="N_term", P="P_term")
    for key, nm in names.items():
        got, want, twin = halves(nm), ld[key], f64[key]
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(np.isnan(twin), nan), key
        scale = np.maximum(1.0, np.abs(np.where(nan, 0, want)))
        dev = np.where(nan, 0, np.abs(got - want) / scale).astype(np.float64)
        eps = np.where(nan, 0, np.abs(twin - want) / scale).astype(np.float64)
        for g in sorted(set(groups)):
            sel = groups == g
            bound = max(lines_cases.FLOOR, lines_cases.MARGIN * eps[sel].max())
            assert dev[sel].max() <= bound, (key, g, float(dev[sel].max()), bound)
    trig = ld["vote"].reshape(H, X, Y).any(axis=0).astype(np.int32)
    assert np.array_equal(np.asarray(s.scat_trigger).reshape(X, Y), trig)


def test_limited_G_is_not_always_1e8_in_magnitude():
    """1e8 G / |G| rounds twice: the limited value is 1e8 (1 - 2^-53) for about one G in twenty, so "limited" cannot be
    read off |G| >= 1e8 afterwards -- the restatement (and the kernels) count where they limit"""
    G = 10.0 ** np.random.default_rng(1).uniform(8.0, 300.0, 100000)
    lim = 1e8 * G / np.abs(G)
    assert np.all(np.abs(lim - 1e8) <= 1e8 * 2.0 ** -52) and np.any(lim < 1e8)
