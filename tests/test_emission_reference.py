"""The angular-emission contract (tests/emission_reference.py) held to what is known in closed form: an enclosure, the
absorbing slab, the invariance under splitting shells, and the plain fp64 statement at the edges of its two branches."""
import numpy as np
import pytest
from scipy.special import expn

import emission_reference as er

LD = np.longdouble
TS = np.float64(er.T_SWITCH)
# optical depths of a shell: nothing, the smallest numbers, both sides of the switch along every angle, an opaque shell
DEPTHS = [0.0, 1e-300, 1e-12, 1e-3, float(np.nextafter(TS, 0)), float(TS), float(np.nextafter(TS, 1)), 0.3, 1.0, 30.0, 800.0]


def _enclosure(B, omega):
    """a column of len(DEPTHS) shells per bin inside a cavity at B[x]: F_up = F_down = pi B at every boundary, in long double"""
    S, X, Y = len(DEPTHS), len(B), 3
    pi = LD(er.PI)
    dtau = np.empty((S, X, Y), LD)
    for s, d in enumerate(DEPTHS):
        dtau[s] = LD(d) * np.array([0.5, 1.0, 1.7], LD)[None, :]          # the switch is crossed along some angle in every y
    cloud = np.zeros((S, X), LD)
    cloud[1::3] = LD(1e-2)
    w0 = np.full((S, X, Y), LD(omega))
    Bx = np.asarray(B, LD)
    B_ends = np.broadcast_to(Bx, (S, X))
    F = np.broadcast_to((pi * Bx)[None, :, None], (S + 1, X, Y))
    return dtau, cloud, w0, B_ends, B_ends, F, F, None, np.array([0.4, 1.1, 0.5], LD)


@pytest.mark.parametrize("N", [1, 2, 8, 16])
@pytest.mark.parametrize("omega", [0.0, 0.37, 1.0 - 1e-10])
def test_enclosure_returns_its_own_planck_value(omega, N):
    """B constant, F_up = F_down = pi B, no beam: every intensity is B, whatever the albedo and the optical depths"""
    B = np.array([1.0, 3.3e-7, 2.5e11])
    args = _enclosure(B, omega)
    mu, w, mu_inv = er.angles(N)
    out = er.emission(*args, mu_inv, 0.0, mu=mu, mu_weight=w)
    dev = np.abs(out["I_wg"] / np.asarray(B, LD)[None, :, None] - 1)
    print("enclosure omega = %g, N = %d: max relative deviation %.2e" % (omega, N, float(dev.max())))
    assert float(dev.max()) <= 1e-15
    band = np.abs(out["I_band"] / np.asarray(B, LD)[None, :] - 1)          # the Gauss weights of the column sum to 2
    assert float(band.max()) <= 1e-15
    # and an isotropic intensity B gives the flux pi B:  2 pi sum_m w_m mu_m = pi up to the quadrature's rounding
    assert float(np.abs(out["F"] / (LD(er.PI) * np.asarray(B, LD)) - 1).max()) <= 1e-14


# the quadrature's own relative error for F / (pi B) of an absorbing slab,
# |2 sum_m w_m mu_m (1 - exp(-tau / mu_m)) / (1 - 2 E_3(tau)) - 1|
SLAB_ERROR = {(0.1, 8): 3.6e-4, (0.1, 16): 3.6e-6, (1.0, 8): 2.8e-6, (1.0, 16): 4.0e-9, (10.0, 8): 9.5e-12, (10.0, 16): 1e-16}


@pytest.mark.parametrize("tau,N", sorted(SLAB_ERROR))
def test_absorbing_slab_against_the_closed_form(tau, N):
    """one isothermal, purely absorbing slab over a cold lower boundary: F = pi B (1 - 2 E_3(tau))"""
    mu, w, mu_inv = er.angles(N)
    B = 2.75
    one, zero = np.full((1, 1), B), np.zeros((2, 1, 1))
    out = er.emission(np.full((1, 1, 1), tau), np.zeros((1, 1)), np.zeros((1, 1, 1)), one, one, zero, zero, None, [2.0],
                      mu_inv, 0.0, mu=mu, mu_weight=w, I_start=np.zeros((1, 1)))
    got = out["F"][0] / (LD(er.PI) * LD(B))
    want = LD(1.0 - 2.0 * expn(3, tau))
    err = float(abs(got / want - 1))
    print("slab tau = %g, N = %d: F / (pi B) = %.17g, closed form %.17g, relative error %.2e" % (tau, N, float(got), float(want), err))
    assert err <= max(2 * SLAB_ERROR[(tau, N)], 1e-15)
    if N == 8 and tau == 1.0:
        # the two-stream closure of the run (D = 2) is ten per cent off where the quadrature is not
        assert abs((1 - np.exp(-2.0)) / float(want) - 1) > 0.1


def _seeded_column(seed, S=7, X=4, Y=3):
    rng = np.random.default_rng(seed)
    dtau = 10.0 ** rng.uniform(-8, 1.7, (S, X, Y))
    cloud = 10.0 ** rng.uniform(-6, 0, (S, X)) * (rng.uniform(size=(S, X)) < 0.5)
    w0 = rng.uniform(0, 1, (S, X, Y))
    Bk = rng.uniform(1.0, 3.0, (S + 1, X))
    F_up = np.pi * Bk[:, :, None] * rng.uniform(0.5, 1.5, (S + 1, X, Y))
    F_down = np.pi * Bk[:, :, None] * rng.uniform(0.5, 1.5, (S + 1, X, Y))
    F_dir = 10.0 * rng.uniform(0.0, 1.0, (S + 1, X, Y))
    w = np.polynomial.legendre.leggauss(Y)[1]
    return dtau, cloud, w0, Bk[:-1], Bk[1:], F_up, F_down, F_dir, w


def test_splitting_every_shell_in_three_leaves_the_intensities_alone():
    """a source linear in tau is integrated exactly: dividing every shell in three, with B and the fluxes interpolated
    linearly in tau and the albedo kept, changes nothing but rounding.  Measured: 5.4e-19 relative in long double."""
    dtau, cloud, w0, B_bot, B_top, F_up, F_down, F_dir, w = [np.asarray(v, LD) for v in _seeded_column(5)]
    mu, mw, mu_inv = er.angles(8)
    beta = 1.0 / (4.0 * np.pi * 0.6)
    whole = er.emission(dtau, cloud, w0, B_bot, B_top, F_up, F_down, F_dir, w, mu_inv, beta)
    S = dtau.shape[0]
    third = lambda v: np.repeat(v / LD(3), 3, axis=0)
    f = [LD(k) / LD(3) for k in range(4)]
    Bb = np.concatenate([np.stack([B_bot[s] + f[k] * (B_top[s] - B_bot[s]) for k in range(3)]) for s in range(S)])
    Bt = np.concatenate([np.stack([B_bot[s] + f[k + 1] * (B_top[s] - B_bot[s]) for k in range(3)]) for s in range(S)])
    between = lambda F: np.concatenate([np.stack([F[s] + f[k] * (F[s + 1] - F[s]) for k in range(3)]) for s in range(S)]
                                       + [F[S:]])
    split = er.emission(third(dtau), third(cloud), np.repeat(w0, 3, axis=0), Bb, Bt, between(F_up), between(F_down),
                        between(F_dir), w, mu_inv, beta)
    dev = float(np.abs(split["I_wg"] / whole["I_wg"] - 1).max())
    print("splitting in three: max relative change of I %.2e" % dev)
    assert dev <= 1e-14
    assert float(np.abs(split["I_band"] / whole["I_band"] - 1).max()) <= 1e-14


def test_plain_fp64_at_the_edges_of_its_branches():
    """the weights (e, a, b) in fp64 against long double: one ulp on either side of the switch, at 0, at 1e-300, at 800.
    Bounds from the statements themselves: above the switch 1 - u / t and u / t - e cancel to 0.025 of their operands, each
    known to about an ulp -- 2e-14 relative; below it ten terms that fall by t / 3 each, a few ulp -- 1e-15."""
    t = np.array([np.nextafter(TS, 0), TS, np.nextafter(TS, 1), 0.0, 1e-300, 800.0])
    ref = er.weights(t, LD)
    plain = er.weights(t, np.float64)
    for name, r, p in zip("eab", ref, plain):
        rel = np.abs(np.asarray(p, LD) - r) / np.where(r != 0, np.abs(r), 1)
        print(name, " ".join("%.2e" % float(v) for v in rel))
    e, a, b = plain
    assert e[3] == 1 and a[3] == 0 and b[3] == 0                      # an empty shell leaves the intensity alone
    assert e[4] == 1 and a[4] == 5e-301 and b[4] == 5e-301
    assert e[5] == 0 and a[5] == 1 - 1 / 800 and b[5] == 1 / 800
    for k in (0, 1, 2):
        lim = 1e-15 if k == 0 else 2e-14
        for r, p in zip(ref, plain):
            assert abs(LD(p[k]) - r[k]) <= lim * abs(r[k]), (k, float(p[k]), float(r[k]))
    # the two branches agree across the switch: the series is complete there (its next term is 1e-23 of the sum)
    for r in ref[1:]:
        assert abs(r[0] / r[1] - 1) < 1e-15


def test_measured_deviation_of_the_plain_statement():
    """the figures the README quotes for t_s = 0.05 and ten terms: plain fp64 against long double over each branch"""
    above = np.geomspace(TS, 800.0, 20001)
    below = np.geomspace(1e-12, np.nextafter(TS, 0), 20001)
    worst = {}
    for name, tt in (("above", above), ("below", below)):
        ref, plain = er.weights(tt, LD), er.weights(tt, np.float64)
        worst[name] = [float((np.abs(np.asarray(p, LD) - r) / np.abs(r)).max()) for r, p in list(zip(ref, plain))[1:]]
        print(name, "a %.2e b %.2e" % tuple(worst[name]))
    assert max(worst["above"]) <= 2e-14 and max(worst["below"]) <= 1e-15


def test_a_thick_isothermal_column_emits_its_planck_value():
    """no scattering, every shell opaque: the intensity is the top layer's B along every angle"""
    S, X, Y = 3, 2, 2
    B = np.array([[3.0, 5.0], [2.0, 4.0], [1.5, 2.5]])
    z = np.ones((S + 1, X, Y))
    mu, mw, mu_inv = er.angles(4)
    out = er.emission(np.full((S, X, Y), 800.0), np.zeros((S, X)), np.zeros((S, X, Y)), B, B, z, z, None, [1.0, 1.0], mu_inv, 0.0)
    assert float(np.abs(out["I_band"] - B[-1][None, :]).max()) < 1e-18


def test_layouts_of_the_two_layer_modes():
    lay = np.arange(6.0).reshape(3, 2)
    inter = 10 + np.arange(8.0).reshape(4, 2)
    bot, top = er.planck_ends(lay)
    assert bot is top or np.array_equal(bot, top)
    bot, top = er.planck_ends(lay, inter)
    assert bot[:, 0].tolist() == [10, 0, 12, 2, 14, 4] and top[:, 0].tolist() == [0, 12, 2, 14, 4, 16]
    F = er.boundaries_of(np.arange(4.0).reshape(4, 1, 1), 100 + np.arange(4.0).reshape(4, 1, 1))     # centres over-allocated
    assert F.ravel().tolist() == [0, 100, 1, 101, 2, 102, 3]
    assert er.shells_of_layers(np.array([1, 2]), np.array([5, 6])).tolist() == [1, 5, 2, 6]


def test_angles_are_gauss_legendre_on_the_unit_interval():
    for N in (1, 2, 8, 16):
        mu, w, mu_inv = er.angles(N)
        assert np.all(np.diff(mu) > 0) and mu[0] > 0 and mu[-1] < 1 and abs(w.sum() - 1) < 1e-15
        assert abs((w * mu).sum() - 0.5) < 1e-15 and np.array_equal(mu_inv, 1.0 / mu)
    assert er.angles(1)[0][0] == 0.5
