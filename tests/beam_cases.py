"""Inputs of the direct-beam tests (tests/test_beam_reference.py without a GPU, tests/test_gpu_beam_edges.py with one):
seeded, small, each case named for what it reaches.

crafted(): optical depths for the per-stage entries hx_fdir_iso and hx_fdir_noniso -- 1, 2 and 33 layers; 1, 255, 256, 260
and 257 spectral points around one 256-thread workgroup; zenith 0 (mu_star = -1 exactly), 60 and 89.9 degrees; plane and
sphere; a rocky column (z > 0, R_planet = 6.4e8) and a gas column (z < 0 in the lowest layers, R_planet = 7e9), both spanning
4e8 cm so that q leaves 1 by 5 % and more.  The profiles: `empty` (all zero), `span` (the largest slant total of any
interface log-uniform from 1e-6 to 600 over the spectral points, the vertical optical depth falling by 1e5 from the bottom
layer to the top), `opaque_layer` (one mid layer with a <= -800 for every interface below it), `subnormal` (slant totals down
to the bottom interface in [710.5, 743.5] under |F0| in [0.9, 1]) and `dir0` (span with dir_beam = 0).  Per kernel form (geometry x half-layers) the list holds every
(profile, size) pair once, with layers, zenith and planet chosen so that every pair of values of any two factors occurs.

loop_cases(): columns for the device loop from cases.make_case(dir_beam=1, ...), opac_k and the Rayleigh table scaled per
bin so that the slant totals of the column run from below 1e-3 to above 745 across its bins; LOOP_TABLE holds at most twelve
combinations in which every pair of values of nbin, nlayer, ny, iso, geom_zenith_corr, scat and planet type occurs, one of
them with clouds.  BATCH_COLUMNS: three columns that differ in everything the beam reads per column."""
import functools
import zlib

import numpy as np

import beam_reference as br
import cases
from helios_amd import phys_const as pc

PROFILES = ("empty", "span", "opaque_layer", "subnormal", "dir0")
LAYERS = (1, 2, 33)
SIZES = ((1, 1), (51, 5), (64, 4), (13, 20), (257, 1))         # (nbin, ny): 1, 255, 256, 260, 257 spectral points
ZENITHS = (0.0, 60.0, 89.9)
PLANETS = ("rocky", "gas")
FORMS = ((0, 1), (0, 0), (1, 1), (1, 0))                       # (sphere, iso): k_fdir_plane<false>, <true>, k_fdir_sphere<false>, <true>
GUARD = 64
SENTINEL = -7.0e77


def mu_of_zenith(deg):
    return -1.0 if deg == 0.0 else float(np.cos(np.pi - deg * np.pi / 180.0))       # cases.make_case's


class BeamCase(object):
    def __repr__(self):
        return self.name


def heights(planet, L, rng):
    """layer-centre heights that rise through 4e8 cm: above a rocky surface, or around a gas planet's reference level"""
    frac = (np.arange(L) + 0.5 + (rng.uniform(-0.3, 0.3, L) if L > 1 else 0.0)) / L
    if planet == "rocky":
        return 6.4e8, 2.0e6 + 4.0e8 * frac
    return 7.0e9, 4.0e8 * (frac - 0.6)


def crafted(profile, L, size, zenith, sphere, planet, iso, seed=0):
    nbin, ny = size
    c = BeamCase()
    c.name = "%s_L%d_%dx%d_zen%g_%s_%s_%s" % (profile, L, nbin, ny, zenith, "sphere" if sphere else "plane", planet,
                                              "iso" if iso else "noniso")
    rng = np.random.default_rng([seed, PROFILES.index(profile), L, nbin, ny, int(zenith * 10), sphere, PLANETS.index(planet), iso])
    c.profile, c.L, c.nbin, c.ny, c.zenith, c.sphere, c.planet, c.iso = profile, L, nbin, ny, zenith, int(sphere), planet, int(iso)
    c.dir_beam = 0 if profile == "dir0" else 1
    nc = c.nc = nbin * ny
    c.mu_star = mu_of_zenith(zenith)
    c.R_star = pc.R_SUN * float(rng.uniform(0.7, 1.3))
    c.a = 0.05 * pc.AU * float(rng.uniform(0.7, 1.3))
    c.R_planet, c.z = heights(planet, L, rng)
    geo = abs(c.mu_star) * (c.R_star / c.a) ** 2 * br.PI
    c.B_star = rng.uniform(0.9, 1.0, nbin) / geo if profile == "subnormal" else 10.0 ** rng.uniform(-6.0, -3.0, nbin)
    c.planck = rng.uniform(1e-8, 1e-5, nbin * (L + 2))                 # planckband_lay: the stellar row is entry L of each bin
    c.planck[L::L + 2] = c.B_star
    # |mu_0j|: the slant factors down to the bottom interface, the largest of every layer; deepest(w): the largest slant
    # total of any interface for layer weights w |mu_0j| (at grazing incidence on a sphere the paths to higher interfaces
    # are the longer ones)
    mu = np.array([[abs(float(br.slant_mu(np.float64, c.mu_star, c.R_planet, c.z, i, j, sphere))) if j >= i else np.inf
                    for j in range(L)] for i in range(L)])
    mu0 = mu[0]
    deepest = lambda w: float((w * mu0 / mu).sum(axis=1).max())
    if profile == "empty":
        tau = np.zeros((L, nc))
    elif profile in ("span", "dir0"):
        total = rng.permutation(np.geomspace(1e-6, 600.0, nc)) if nc > 1 else np.array([30.0])
        w = 10.0 ** (-5.0 * np.arange(L) / max(L - 1, 1))
        tau = total[None, :] * (w / deepest(w) * mu0)[:, None]
    elif profile == "subnormal":
        total = rng.uniform(710.5, 743.5, nc)
        w = rng.uniform(0.5, 1.5, L)
        tau = total[None, :] * (w / w.sum() * mu0)[:, None]
    else:
        assert profile == "opaque_layer"
        total = 10.0 ** rng.uniform(-3.0, 0.5, nc)
        w = rng.uniform(0.5, 1.5, L)
        tau = total[None, :] * (w / deepest(w) * mu0)[:, None]
        c.opaque = L // 2
        tau[c.opaque] = 800.0 * 1.001 * mu0[c.opaque]
    if iso:
        c.tau_u, c.tau_l = tau, None
    else:
        f = rng.uniform(0.3, 0.7, (L, nc))
        c.tau_u, c.tau_l = tau * f, tau * (1.0 - f)
    return c


def crafted_cases():
    """per kernel form every (profile, size) pair; layers, zenith and planet run through their values along both"""
    out = []
    for f, (sphere, iso) in enumerate(FORMS):
        for p, profile in enumerate(PROFILES):
            for s, size in enumerate(SIZES):
                out.append(crafted(profile, LAYERS[(p + s) % 3], size, ZENITHS[(p + 2 * s + f) % 3], sphere,
                                   PLANETS[(p + s // 3 + s + f) % 2], iso))
    return out


@functools.lru_cache(maxsize=None)
def all_crafted():
    return tuple(crafted_cases())


def restate(c, dtype=br.LD, variant=None):
    return br.beam(c.tau_u, c.tau_l, c.B_star, c.z, c.mu_star, c.R_planet, c.R_star, c.a, c.dir_beam, c.sphere, c.ny, dtype, variant)


_RESTATED = {}


def restated(c):
    """the long-double restatement of a crafted case, computed once and left unchanged"""
    if c.name not in _RESTATED:
        _RESTATED[c.name] = restate(c)
    return _RESTATED[c.name]


def run_stage(impl, c, guard=GUARD):
    """hx_fdir_iso / hx_fdir_noniso (or the oracle's) on a crafted case: (F_dir_wg, Fc_dir_wg or None), each with `guard`
    sentinel cells behind it, the sentinel everywhere before the call"""
    I = c.L + 1
    n = c.nc * I
    F = np.full(n + guard, SENTINEL)
    z = np.ascontiguousarray(c.z, np.float64)
    args = (z, c.mu_star, c.R_planet, c.R_star, c.a, c.dir_beam, c.sphere, I, c.nbin, c.ny)
    if c.iso:
        impl.fdir_iso(F, c.planck.copy(), np.ascontiguousarray(c.tau_u.reshape(-1)), *args)
        return F, None
    Fc = np.full(n + guard, SENTINEL)
    impl.fdir_noniso(F, Fc, c.planck.copy(), np.ascontiguousarray(c.tau_u.reshape(-1)), np.ascontiguousarray(c.tau_l.reshape(-1)), *args)
    return F, Fc


def applies(variant, c):
    """whether a crafted case is named for a wrong variant: the variant changes what the case computes"""
    if c.profile in ("empty", "dir0"):
        return False
    if variant == "q_exchanged" or variant == "mu_star_in_sphere":
        # mu_ij leaves mu_star only for i < j and off the zenith; under an opaque layer nothing is left to see it with
        return bool(c.sphere) and c.zenith != 0.0 and c.L > 1 and not (c.profile == "opaque_layer" and c.L < c.opaque + 3)
    if variant == "centre_lower_half":
        return not c.iso
    if variant == "centre_layer_off":
        return not c.iso and c.L > 1
    return variant == "product_slab_off"


# ---- the device loop ---------------------------------------------------------------------------------------------------------
# nbin, nlayer, ny, iso, geom_zenith_corr, scat, planet type, clouds, zenith
LOOP_TABLE = [
    (31, 31, 20, 0, 0, 0, "gas", 0, 60.0),
    (31, 32, 4, 1, 1, 1, "rocky", 0, 80.0),
    (32, 31, 4, 0, 1, 1, "gas", 1, 85.0),
    (32, 32, 20, 1, 0, 0, "rocky", 0, 60.0),
    (33, 31, 20, 1, 1, 0, "gas", 0, 80.0),
    (33, 32, 4, 0, 0, 1, "rocky", 0, 85.0),
    (31, 31, 4, 1, 0, 1, "rocky", 0, 85.0),
    (32, 32, 20, 0, 1, 1, "gas", 0, 80.0),
    (33, 31, 20, 0, 1, 0, "rocky", 0, 60.0),
    (31, 32, 20, 1, 1, 1, "gas", 0, 60.0),
    (32, 31, 4, 1, 0, 0, "gas", 0, 80.0),
    (33, 32, 4, 0, 0, 0, "gas", 0, 85.0),
]
LOOP_FACTORS = ("nbin", "nlayer", "ny", "iso", "geom_zenith_corr", "scat", "planet_type")
SMALL = dict(ntemp=6, npress=5)


def loop_name(row):
    return "X%d_L%d_ny%d_iso%d_sphere%d_scat%d_%s_clouds%d" % row[:8]


def oracle_refresh(port, c):
    """the oracle's own first refresh of a column: its state (opacities, heights, beam) and the case as it left it"""
    c = c.copy()
    s = cases.alloc_state(c)
    cases.setup_planck(port, c, s)
    cases.interpolate_temperatures_and_planck(port, c, s)
    cases.refresh_premixed(port, c, s)
    return c, s


def tau_inputs(c, s, column=None):
    """half_layer_tau's inputs from a case and an oracle state"""
    g = dict(nbin=c.nbin, ny=c.ny, nlayer=c.nlayer, iso=c.iso, scat=c.scat, g=(column or {}).get("g", c.g), p_int=c.p_int,
             delta_col_upper=c.delta_col_upper, delta_col_lower=c.delta_col_lower)
    for k in ("opac_wg_lay", "opac_wg_int", "scat_cross_lay", "scat_cross_int", "meanmolmass_lay", "meanmolmass_int"):
        g[k] = s[k]
    for k in ("abs_cross_all_clouds_lay", "abs_cross_all_clouds_int", "scat_cross_all_clouds_lay", "scat_cross_all_clouds_int"):
        g[k] = c[k]
    return g


def restate_column(g, B_star, z_lay, c, column=None, dtype=br.LD, variant=None):
    """the beam of one column of the loop from half_layer_tau's inputs g, the stellar row and the heights"""
    col = dict(mu_star=c.mu_star, R_planet=c.R_planet, R_star=c.R_star, a=c.a)
    col.update({k: v for k, v in (column or {}).items() if k in col})
    tau_u, tau_l = br.half_layer_tau(g, variant if variant in br.TAU_VARIANTS else None)
    return br.beam(tau_u, tau_l, B_star, z_lay, col["mu_star"], col["R_planet"], col["R_star"], col["a"], c.dir_beam,
                   c.geom_zenith_corr, c.ny, dtype, None if variant in br.TAU_VARIANTS else variant)


@functools.lru_cache(maxsize=None)
def loop_case(row, top=3e3):
    """the column of a LOOP_TABLE row: opac_k (70 % of a bin's target) and the Rayleigh table (30 %) scaled per bin so that
    the largest slant total of bin x, down to the bottom interface, is 3e-4 (top / 3e-4)^(x / (nbin - 1)) -- measured with
    the oracle's refresh and this module's restatement, before and after"""
    import oracle
    nbin, nlayer, ny, iso, sphere, scat, planet, clouds, zenith = row
    c = cases.make_case(nbin=nbin, nlayer=nlayer, ny=ny, iso=iso, geom_zenith_corr=sphere, scat=scat, dir_beam=1,
                        clouds=clouds, zenith_deg=zenith, seed=zlib.crc32(repr(row).encode()), **SMALL)
    c.planet_type = planet
    c.name = loop_name(row)
    c1, s = oracle_refresh(oracle.port, c)
    g = tau_inputs(c1, s)
    B = s.planckband_lay[nlayer::nlayer + 2]
    gas = restate_column(dict(g, scat=0), B, c1.z_lay, c1, dtype=np.float64).slant[0].reshape(nbin, ny)
    ray = (restate_column(dict(g, scat=1), B, c1.z_lay, c1, dtype=np.float64).slant[0].reshape(nbin, ny) - gas).max(axis=1)
    gas = gas.max(axis=1)
    target = np.geomspace(3e-4, top, nbin)
    c.opac_k = (c.opac_k.reshape(-1, nbin, ny) * (0.7 * target / gas)[None, :, None]).reshape(-1)
    c.opac_scat_cross = (c.opac_scat_cross.reshape(-1, nbin) * (0.3 * target / ray)[None, :]).reshape(-1)
    return c


def loop_cases():
    return [loop_case(row) for row in LOOP_TABLE]


# three columns of one batch: zenith 30, 75 and 88 degrees, and a, R_star, R_planet, g, T_star all different
BATCH_ROW = (33, 31, 4, 0, 1, 1, "gas", 0, 30.0)
BATCH_COLUMNS = [
    dict(mu_star=mu_of_zenith(30.0), a=0.05 * pc.AU, R_star=1.0 * pc.R_SUN, R_planet=1.0 * pc.R_JUP, g=1000.0, T_star=5000.0),
    dict(mu_star=mu_of_zenith(75.0), a=0.03 * pc.AU, R_star=0.6 * pc.R_SUN, R_planet=0.5 * pc.R_JUP, g=1800.0, T_star=3800.0),
    dict(mu_star=mu_of_zenith(88.0), a=0.08 * pc.AU, R_star=1.4 * pc.R_SUN, R_planet=1.6 * pc.R_JUP, g=600.0, T_star=6500.0),
]


BATCH_SLANT_LIMIT = 700.0


def batch_case():
    """the case of the three-column batch: a LOOP_TABLE column's scaling made for column 0, up to a slant total of 10 -- at
    88 degrees and the smallest g that is some 400, and every beam value of the batch stays a normal number.  (Where all
    Gauss points of an entry are subnormal, the products w_y / 2 F of k_rt_fdir_band round to the subnormal spacing, in the
    kernel as in any fp64 evaluation, and the bound (ny + 2) 2^-53 sum |term| of the Gauss sum has no term for that: the
    same columns scaled up to 3e3 miss it by 1.8e5 at one entry of the third column, on the device and in numpy's fp64
    alike, bit for bit.)"""
    return loop_case(BATCH_ROW, 10.0)


def column_case(c, column):
    """the single-column case that a batch column stands for (the oracle's chain takes its parameters from the case)"""
    cc = c.copy()
    for k, v in column.items():
        cc[k] = v
    cc.delta_colmass = (cc.p_int[:-1] - cc.p_int[1:]) / cc.g
    cc.delta_col_upper = (cc.p_lay - cc.p_int[1:]) / cc.g
    cc.delta_col_lower = (cc.p_int[:-1] - cc.p_lay) / cc.g
    return cc
