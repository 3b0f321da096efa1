"""The direct stellar beam restated in numpy, in a type the caller chooses (np.longdouble for the reference, np.float64
for the formula's own rounding), with a bound for every entry computed alongside it.  The contract is the oracle's
(orc_fdir_iso, orc_fdir_noniso in oracle/helios_oracle.c; kernels.cu:1265-1362); the kernels held to it are k_fdir_plane and
k_fdir_sphere (csrc/stage_trans.hip), k_rt_dtau_halves and k_rt_fdir_band (csrc/rt_kernels.h).

Contract.  With c = y + ny x a spectral point, L layers and interfaces 0 ... L (L is the top of the atmosphere):

    F0[c]        = -dir_beam * mu_star * (((R_star / a) * (R_star / a)) * PI * B_star[x])
    F_dir[c, i]  = F0 * prod_{j = L-1 ... i} exp(a_ij),     a_ij = tau_j / mu_ij,        F_dir[c, L] = F0
    Fc_dir[c, i] = F0 * prod_{j = L-1 ... i+1} exp(a_ij) * exp(tau_u,i / mu_ii)          (the top slab is never written)

tau_j is the optical depth of layer j (of half-layers: tau_u + tau_l, summed first); mu_ij = mu_star in plane geometry and
-sqrt(1 - q^2 (1 - mu_star^2)), q = (R_planet + z[i]) / (R_planet + z[j]), with the spherical correction.

The optical depths of the half-layers (half_layer_tau) follow k_rt_dtau_halves and calc_trans_*: always in fp64 and in the
kernel's order of operations.  Only + * / occur and contraction is off in csrc/Makefile, so these are the device's bits;
everything after them is evaluated in the chosen type.  Cloud optical depth does not enter the beam.

Bound.  With u = 2^-53, an fp64 evaluation of the contract lies within

    u (8 + sum_j (3 + kappa_ij |a_ij|)) |value|  +  (n_factors + 2) 2^-1074

of the exact value.  The 8 is F0's five roundings and the constant PI.  Per factor: the exponential of the device and of
glibc, each documented at <= 1 ulp, taken as 2 u, and the multiplication: 3 u; and the argument's own relative error kappa u
moves the factor by |a| times its size.  Plane geometry: kappa = 2, one rounding from the sum of the halves and one from the
division.  Sphere: kappa = 3 + 5 / mu_ij^2 -- q carries 3 u and q^2 7 u; q^2 (1 - mu_star^2) has an absolute error of at most
9 u because both factors are <= 1; the difference from 1 has 10 u absolute against a value >= mu_ij^2; the square root halves
that and adds u; then the sum of the halves and the division.  The absolute term is one subnormal spacing per
multiplication: every factor is <= 1, so no earlier error grows.  Fc_dir: the same, with its own last factor.

On the CPU (33 layers x 40 points, vertical totals 1e-6 ... 600 |mu_star|, zenith 0, 60, 80, 89 and 89.9 degrees, both
geometries) the plain fp64 evaluation reaches 0.22 ... 0.32 of this bound everywhere, the sphere at 89.9 degrees included,
where the error itself is 7e5 u: the bound is neither slack nor violated by the formula's own rounding.  On the cases of
tests/beam_cases.py, which add half-layers, one and two layers, subnormal values and an opaque layer, the fp64 mode and the
CPU oracle reach 0.63 at most (plane, half-layers, 89.9 degrees).  tests/test_beam_reference.py holds the oracle and the
fp64 mode of this module to the bound; tests/test_gpu_beam_edges.py the device, whose figures are in that module's text.

WRONG names restatements that are wrong on purpose; tests/test_beam_reference.py shows that each leaves the bound by a
factor of ten or more on the cases that are named for it."""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
TINY = 2.0 ** -1074
PI = 3.141592653589793                      # HX_PI (csrc/hx_common.h), PI of the oracle

WRONG = {
    "q_exchanged": "(a) i and j exchanged in q",
    "mu_star_in_sphere": "(b) mu_star for every j while the sphere is on",
    "centre_lower_half": "(c) Fc_dir with the lower half in place of the upper",
    "centre_layer_off": "(d) Fc_dir taken one layer off",
    "clouds_added": "(e) cloud optical depth added",
    "rayleigh_flipped": "(f) Rayleigh kept at scat = 0, dropped at scat = 1",
    "upper_with_interface_i": "(g) the upper half averaged with interface i in place of i + 1",
    "product_slab_off": "(h) the running product started one slab off",
    "column_0_parameters": "(i) column 0's mu_star, R_star, a, R_planet used for another column",
}
TAU_VARIANTS = ("clouds_added", "rayleigh_flipped", "upper_with_interface_i")


def half_layer_tau(g, variant=None):
    """(tau_u, tau_l), each [L][ny nbin] in fp64, as k_rt_dtau_halves forms them; isothermal layers: (tau, None).
    g: nbin, ny, nlayer, iso, scat, g, p_int, delta_col_upper/lower, opac_wg_lay/int, scat_cross_lay/int,
    meanmolmass_lay/int (flat, the reference's layouts; longer arrays are read from their start) -- and, for the wrong
    variant that adds them, abs/scat_cross_all_clouds_lay/int."""
    X, Y, L = int(g["nbin"]), int(g["ny"]), int(g["nlayer"])
    I = L + 1
    f8 = lambda k, n: np.asarray(g[k], np.float64)[:n]
    opl = f8("opac_wg_lay", Y * X * L).reshape(L, X, Y)
    scl = f8("scat_cross_lay", X * L).reshape(L, X, 1)
    mml = f8("meanmolmass_lay", L).reshape(L, 1, 1)
    scat = int(g["scat"]) == 1
    if variant == "rayleigh_flipped":
        scat = not scat
    zero = np.zeros((L, X, 1))
    if int(g["iso"]) == 1:
        p = f8("p_int", I)
        dcol = ((p[:-1] - p[1:]) / float(g["g"])).reshape(L, 1, 1)
        ray = scl if scat else zero
        tau = dcol * (opl + ray / mml)
        if variant == "clouds_added":
            cl = f8("abs_cross_all_clouds_lay", X * L).reshape(L, X, 1) + (f8("scat_cross_all_clouds_lay", X * L).reshape(L, X, 1) if scat else 0.0)
            tau = tau + dcol * cl / mml
        return tau.reshape(L, X * Y), None
    opi = f8("opac_wg_int", Y * X * I).reshape(I, X, Y)
    sci = f8("scat_cross_int", X * I).reshape(I, X, 1)
    mmi = f8("meanmolmass_int", I).reshape(I, 1, 1)
    du, dl = f8("delta_col_upper", L).reshape(L, 1, 1), f8("delta_col_lower", L).reshape(L, 1, 1)
    up = slice(0, L) if variant == "upper_with_interface_i" else slice(1, I)
    ray_up = (scl + sci[up]) / 2.0 if scat else zero
    ray_low = (sci[:L] + scl) / 2.0 if scat else zero
    kap_up, kap_low = (opl + opi[up]) / 2.0, (opi[:L] + opl) / 2.0
    mu_up, mu_low = (mml + mmi[up]) / 2.0, (mmi[:L] + mml) / 2.0
    tau_u = du * (kap_up + ray_up / mu_up)
    tau_l = dl * (kap_low + ray_low / mu_low)
    if variant == "clouds_added":
        cab_l, cab_i = (f8("abs_cross_all_clouds_" + s, X * n).reshape(n, X, 1) for s, n in (("lay", L), ("int", I)))
        csc_l, csc_i = (f8("scat_cross_all_clouds_" + s, X * n).reshape(n, X, 1) for s, n in (("lay", L), ("int", I)))
        csc_up, csc_low = ((csc_l + csc_i[1:]) / 2.0, (csc_i[:L] + csc_l) / 2.0) if scat else (0.0, 0.0)
        tau_u = tau_u + du * ((cab_l + cab_i[1:]) / 2.0 + csc_up) / mu_up
        tau_l = tau_l + dl * ((cab_i[:L] + cab_l) / 2.0 + csc_low) / mu_low
    return tau_u.reshape(L, X * Y), tau_l.reshape(L, X * Y)


class Beam(object):
    """F [L + 1][nc] and Fc [L][nc] (None with isothermal layers) in the chosen type, F0 [nc], and for each value its
    relative bound in units of u and its absolute bound; slant [L + 1][nc]: sum_j |a_ij|, the slant optical depth down to
    interface i"""

    def bound(self, key):
        v, rel, ab = {"F": (self.F, self.rel_F, self.abs_F), "Fc": (self.Fc, self.rel_Fc, self.abs_Fc)}[key]
        return rel * U * np.abs(v).astype(LD) + ab

    def ratio(self, key, got):
        """|got - value| / bound per entry; anything that is not a number counts as outside"""
        want = self.F if key == "F" else self.Fc
        got = np.asarray(got).reshape(want.shape)
        with np.errstate(invalid="ignore"):
            r = np.abs(got.astype(LD) - want.astype(LD)) / self.bound(key)
        return np.where(np.isfinite(r) & (r < 1e300), r, np.inf).astype(np.float64)


def slant_mu(T, mu_star, R_planet, z, i, j, sphere):
    if not sphere:
        return T(mu_star)
    q = (T(R_planet) + T(z[i])) / (T(R_planet) + T(z[j]))
    with np.errstate(invalid="ignore"):
        return -np.sqrt(T(1.0) - (q * q) * (T(1.0) - T(mu_star) * T(mu_star)))


def beam(tau_u, tau_l, B_star, z_lay, mu_star, R_planet, R_star, a, dir_beam, sphere, ny, dtype=LD, variant=None):
    """the contract of the module's text on tau_u, tau_l [L][nc] (fp64; tau_l None: isothermal layers), B_star [nbin]"""
    T = dtype
    tau_u = np.asarray(tau_u, np.float64)
    L, nc = tau_u.shape
    noniso = tau_l is not None
    tu = tau_u.astype(T)
    tl = np.asarray(tau_l, np.float64).astype(T) if noniso else None
    tau = tu + tl if noniso else tu
    rs = T(R_star) / T(a)
    I_dir = ((rs * rs) * T(PI)) * np.asarray(B_star, np.float64).astype(T)
    F0 = np.repeat((T(-int(dir_beam)) * T(mu_star)) * I_dir, ny)
    assert F0.shape == (nc,)
    sph = bool(sphere) and variant != "mu_star_in_sphere"

    def mu_of(i, j):
        return slant_mu(T, mu_star, R_planet, z_lay, j, i, sph) if variant == "q_exchanged" else \
            slant_mu(T, mu_star, R_planet, z_lay, i, j, sph)

    def kappa_of(mu):
        return 3.0 + 5.0 / float(mu) ** 2 if sphere else 2.0

    b = Beam()
    b.F0 = F0
    b.F, b.rel_F, b.abs_F = np.zeros((L + 1, nc), T), np.zeros((L + 1, nc)), np.zeros((L + 1, nc))
    b.Fc = b.rel_Fc = b.abs_Fc = None
    b.slant = np.zeros((L + 1, nc))
    if noniso:
        b.Fc, b.rel_Fc, b.abs_Fc = np.zeros((L, nc), T), np.zeros((L, nc)), np.zeros((L, nc))
    top = L - 2 if variant == "product_slab_off" else L - 1
    with np.errstate(under="ignore", invalid="ignore"):
        for i in range(L + 1):
            F, rel, n = F0.copy(), np.full(nc, 8.0), 0
            slant = np.zeros(nc)
            for j in range(top, i - 1, -1):
                mu = mu_of(i, j)
                kap = kappa_of(mu)
                if noniso and j == i:
                    half = tl[i] if variant == "centre_lower_half" else tu[i]
                    au = half / mu
                    b.Fc[i] = F * np.exp(au)
                    b.rel_Fc[i] = rel + 3.0 + kap * np.abs(au).astype(np.float64)
                    b.abs_Fc[i] = (n + 3) * TINY
                aij = tau[j] / mu
                F = F * np.exp(aij)
                mag = np.abs(aij).astype(np.float64)
                rel = rel + 3.0 + kap * mag
                slant = slant + mag
                n += 1
            if noniso and i < L and top < i:          # (the wrong start of the product: no factor left for this centre)
                b.Fc[i], b.rel_Fc[i], b.abs_Fc[i] = F0, 8.0, 2 * TINY
            b.F[i], b.rel_F[i], b.abs_F[i] = F, rel, (n + 2) * TINY
            b.slant[i] = slant
    if noniso and variant == "centre_layer_off":
        b.Fc = np.concatenate([b.Fc[1:], F0[None, :]])
    return b


def band_of(F_dir_wg, gauss_weight, nbin, ny, ninterface):
    """the Gauss sum of k_rt_fdir_band in long double on a given F_dir_wg: (sum_y w_y / 2 F, sum_y |term|), [I][nbin]"""
    term = np.asarray(F_dir_wg, np.float64)[:ny * nbin * ninterface].reshape(ninterface, nbin, ny).astype(LD) * \
        (LD(0.5) * np.asarray(gauss_weight, np.float64).astype(LD))[None, None, :]
    return term.sum(axis=2), np.abs(term).sum(axis=2)
