"""tests/beam_reference.py and tests/beam_cases.py without a GPU: the bound is anchored to the reference and not to the code
under test (the CPU oracle, the reference's own kernels where oracle/_ref is built, and the restatement's fp64 mode lie
within it of the long-double restatement, entry by entry), every wrong variant leaves it by a factor of ten or more on the
cases named for it, and the cases reach what they are named for."""
import itertools

import numpy as np
import pytest

import beam_cases as bc
import beam_reference as br

CRAFTED = bc.all_crafted()
FORM_NAME = {(0, 1): "plane iso", (0, 0): "plane noniso", (1, 1): "sphere iso", (1, 0): "sphere noniso"}


def hold(b, F, Fc, label):
    """every entry of F_dir_wg (and Fc_dir_wg below its top slab) within its bound of the restatement b; returns the ratios"""
    L1, nc = b.F.shape
    rF = b.ratio("F", np.asarray(F)[:L1 * nc])
    assert rF.max() <= 1.0, "%s F_dir_wg: %.3f of its bound at %r" % (label, rF.max(), np.unravel_index(rF.argmax(), rF.shape))
    rc = 0.0
    if b.Fc is not None:
        rFc = b.ratio("Fc", np.asarray(Fc)[:(L1 - 1) * nc])
        assert rFc.max() <= 1.0, "%s Fc_dir_wg: %.3f of its bound at %r" % (label, rFc.max(), np.unravel_index(rFc.argmax(), rFc.shape))
        rc = float(rFc.max()) if rFc.size else 0.0
    return float(rF.max()), rc


def _all_pairs(rows, names):
    for a, b in itertools.combinations(range(len(names)), 2):
        need = set(itertools.product({r[a] for r in rows}, {r[b] for r in rows}))
        assert need == {(r[a], r[b]) for r in rows}, (names[a], names[b])


def test_case_lists_hold_every_pair_of_values():
    for form in bc.FORMS:
        rows = [(c.profile, c.L, (c.nbin, c.ny), c.zenith, c.planet) for c in CRAFTED if (c.sphere, c.iso) == form]
        assert len(rows) == 25 and {r[0] for r in rows} == set(bc.PROFILES) and {r[1] for r in rows} == set(bc.LAYERS)
        assert {r[2] for r in rows} == set(bc.SIZES) and {r[3] for r in rows} == set(bc.ZENITHS)
        _all_pairs(rows, ("profile", "layers", "size", "zenith", "planet"))
    assert len(bc.LOOP_TABLE) <= 12 and sum(r[7] for r in bc.LOOP_TABLE) == 1
    rows = [r[:7] for r in bc.LOOP_TABLE]
    assert {r[0] for r in rows} == {31, 32, 33} and {r[1] for r in rows} == {31, 32} and {r[2] for r in rows} == {20, 4}
    _all_pairs(rows, bc.LOOP_FACTORS)
    assert len({c.name for c in CRAFTED}) == len(CRAFTED)


def _held_by(impl, what):
    worst = {}
    for c in CRAFTED:
        F, Fc = bc.run_stage(impl, c)
        rF, rFc = hold(bc.restated(c), F, Fc, "%s, %s" % (what, c.name))
        key = FORM_NAME[(c.sphere, c.iso)]
        worst[key] = max(worst.get(key, 0.0), rF)
        worst["Fc_dir"] = max(worst.get("Fc_dir", 0.0), rFc)
        n = c.nc * (c.L + 1)
        assert (F[n:] == bc.SENTINEL).all() and (Fc is None or (Fc[n - c.nc:] == bc.SENTINEL).all()), c.name
    for k, v in sorted(worst.items()):
        print("%-18s %-14s largest err / bound %.3f" % (what, k, v))


def test_oracle_within_the_bound(port):
    _held_by(port, "the CPU oracle")


def test_reference_kernels_within_the_bound(ref):
    _held_by(ref, "the reference")


def test_fp64_restatement_within_the_bound():
    worst = 0.0
    for c in CRAFTED:
        d = bc.restate(c, np.float64)
        worst = max((worst,) + hold(bc.restated(c), d.F, d.Fc, "fp64 mode, " + c.name))
    print("the restatement in fp64: largest err / bound %.3f" % worst)


CRAFTED_VARIANTS = ("q_exchanged", "mu_star_in_sphere", "centre_lower_half", "centre_layer_off", "product_slab_off")


def _leaves(b, w):
    r = b.ratio("F", w.F).max()
    return max(r, b.ratio("Fc", w.Fc).max()) if b.Fc is not None else r


@pytest.mark.parametrize("variant", CRAFTED_VARIANTS)
def test_wrong_variant_leaves_the_bound_on_crafted_cases(variant):
    named = [c for c in CRAFTED if bc.applies(variant, c)]
    assert len(named) >= 10, br.WRONG[variant]
    least = min((_leaves(bc.restated(c), bc.restate(c, br.LD, variant)), c.name) for c in named)
    print("%s: least departure %.3e bounds (%s), %d cases" % (br.WRONG[variant], least[0], least[1], len(named)))
    assert least[0] >= 10.0, (br.WRONG[variant], least)


def test_crafted_inputs_reach_what_they_are_named_for():
    for c in CRAFTED:
        b = bc.restated(c)
        vals = [b.F] + ([b.Fc] if b.Fc is not None else [])
        if c.profile == "span":
            assert min(float(np.abs(v).min()) for v in vals) >= 1e-290, c.name       # the relative rule decides every entry
            if c.nc > 1:
                assert b.slant.max(axis=0).min() < 1.1e-6 and 590.0 < b.slant.max() < 610.0, c.name
        if c.profile == "subnormal":
            bottom = np.abs(b.F[0]).astype(np.float64)
            assert (bottom >= 2.0 ** -1074).all() and (bottom < 2.0 ** -1022).all(), c.name
            assert 710.0 <= b.slant[0].min() and b.slant[0].max() <= 744.0, c.name
        if c.profile == "opaque_layer":
            d, m = bc.restate(c, np.float64), c.opaque
            assert (d.F[:m + 1] == 0.0).all() and (b.F[m + 1:] != 0).all(), c.name
            if d.Fc is not None:
                assert (d.Fc[:m] == 0.0).all(), c.name
            tu = c.tau_u.copy()
            tu[m] = 0.0
            tl = None if c.tau_l is None else c.tau_l.copy()
            if tl is not None:
                tl[m] = 0.0
            for T, have in ((np.float64, d), (br.LD, b)):
                without = br.beam(tu, tl, c.B_star, c.z, c.mu_star, c.R_planet, c.R_star, c.a, 1, c.sphere, c.ny, T)
                assert (without.F[m + 1:] == have.F[m + 1:]).all(), c.name
                if have.Fc is not None:
                    assert (without.Fc[m + 1:] == have.Fc[m + 1:]).all(), c.name
        if c.profile == "empty":
            assert (b.F == b.F0[None, :]).all() and (b.F0 != 0).all()
        if c.profile == "dir0":
            assert not b.F.any()
    assert bc.mu_of_zenith(0.0) == -1.0


# ---- the columns of the device loop, through the oracle's own refresh -------------------------------------------------------
@pytest.fixture(scope="module")
def refreshed(port):
    """(case as the oracle left it, oracle state) per LOOP_TABLE row, computed once"""
    return {c.name: bc.oracle_refresh(port, c) for c in bc.loop_cases()}


def test_loop_columns_span_the_optical_depths_and_hold_the_oracle(refreshed):
    worst = 0.0
    for name, (c, s) in refreshed.items():
        g = bc.tau_inputs(c, s)
        tau_u, tau_l = br.half_layer_tau(g)
        n = c.ny * c.nbin * c.nlayer
        if c.iso:           # the restated optical depths are the oracle's, bit for bit
            np.testing.assert_array_equal(tau_u.reshape(-1), s.delta_tau_wg[:n], err_msg=name)
        else:
            np.testing.assert_array_equal(tau_u.reshape(-1), s.delta_tau_wg_upper[:n], err_msg=name)
            np.testing.assert_array_equal(tau_l.reshape(-1), s.delta_tau_wg_lower[:n], err_msg=name)
        b = bc.restate_column(g, s.planckband_lay[c.nlayer::c.nlayer + 2], c.z_lay, c)
        assert b.slant[0].min() < 1e-3 and b.slant[0].max() > 745.0, (name, b.slant[0].min(), b.slant[0].max())
        if c.geom_zenith_corr:
            assert abs((c.R_planet + c.z_lay[0]) / (c.R_planet + c.z_lay[-1]) - 1.0) > 0.02, name
        worst = max((worst,) + hold(b, s.F_dir_wg, s.Fc_dir_wg, "the oracle's refresh, " + name))
    print("the oracle's refresh of the loop columns: largest err / bound %.3f" % worst)


TAU_NAMED = {"clouds_added": lambda c: c.clouds == 1, "rayleigh_flipped": lambda c: True,
             "upper_with_interface_i": lambda c: c.iso == 0}


@pytest.mark.parametrize("variant", br.TAU_VARIANTS)
def test_wrong_optical_depths_leave_the_bound_on_loop_columns(refreshed, variant):
    named = [(c, s) for c, s in refreshed.values() if TAU_NAMED[variant](c)]
    assert named
    for c, s in named:
        g, B = bc.tau_inputs(c, s), s.planckband_lay[c.nlayer::c.nlayer + 2]
        r = _leaves(bc.restate_column(g, B, c.z_lay, c), bc.restate_column(g, B, c.z_lay, c, variant=variant))
        print("%s on %s: %.3e bounds" % (br.WRONG[variant], c.name, r))
        assert r >= 10.0, (br.WRONG[variant], c.name, r)


def test_batch_columns_differ_in_what_the_beam_reads(port):
    """(i): a column restated with column 0's mu_star, R_star, a and R_planet leaves its own bound"""
    c0 = bc.batch_case()
    for k in ("mu_star", "a", "R_star", "R_planet", "g", "T_star"):
        assert len({col[k] for col in bc.BATCH_COLUMNS}) == 3, k
    for col in bc.BATCH_COLUMNS[1:]:
        c, s = bc.oracle_refresh(port, bc.column_case(c0, col))
        g, B = bc.tau_inputs(c, s), s.planckband_lay[c.nlayer::c.nlayer + 2]
        own = bc.restate_column(g, B, c.z_lay, c)
        assert 1.0 < own.slant.max() < bc.BATCH_SLANT_LIMIT
        hold(own, s.F_dir_wg, s.Fc_dir_wg, "the oracle on a batch column")
        lent = bc.restate_column(g, B, c.z_lay, c, column={k: bc.BATCH_COLUMNS[0][k] for k in ("mu_star", "R_star", "a", "R_planet")})
        r = _leaves(own, lent)
        print("%s: %.3e bounds" % (br.WRONG["column_0_parameters"], r))
        assert r >= 10.0
