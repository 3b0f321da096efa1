"""TEST INFRASTRUCTURE: crafted columns for the two convection half-steps of the device loop (csrc/conv_adjust.h,
k_rt_conv_adjust and k_rt_totals_c in csrc/rt_kernels.h), and the `quant` object helios_amd/host_functions.py takes.
No GPU here: tests/test_conv_cases.py proves on the host functions alone that every case has the structure it is named
for, tests/test_gpu_conv_edges.py runs the same cases on the device.

How a profile is crafted.  T_lay is piecewise a power of p: exponent G_RAD = 0.05 in the radiative stretches, and
KAPPA + eps inside a zone of n layers with eps = min(0.05, 0.05 / (n - 1)).  The adjustment conserves enthalpy with
weights ~ p, so a zone's bottom cools and its top warms by about eps * ln(p_bottom / p_top) at the most; with this eps
that is a quarter of the distance (KAPPA - G_RAD) * ln(p_i / p_i+1) which keeps the pair across a zone's edge stable.
A zone therefore ends where it was put (an exponent "well above kappa" makes it entrain its neighbours one by one, and
where it stops is then anybody's guess), while every comparison of an unstable pair still has a margin of eps * dlnp
>= 8e-6, far from the 1e-10 below.  Once on the adiabat, neighbours are 1e-6 * kappa * dlnp >= 1e-8 from the limits
with kappa * (1 +- 1e-6).

The surface: conv_check and mark_convective_layers flag the surface entry together with layer 0, always both.  A zone
that starts at -1 therefore always holds layer 0; `ends = -1` cannot come out of the flags.  "Surface zone alone" is
{-1, 0}, "merged" is {-1, 0, ..., k} with the layers 0..k super-adiabatic themselves.
"""
import contextlib

import numpy as np

import cases
from helios_amd import host_functions as hs
from helios_amd import phys_const as pc
from helios_amd import synthetic as syn

KAPPA = 0.25
G_RAD = 0.05
MARGIN_MIN = 1e-10
SIZE = dict(nbin=5, ny=4, ntemp=6, npress=5, plancktable_dim=800, plancktable_step=10)


# ---- pressures ------------------------------------------------------------------------------------------------------
def pressures(L, regime="high", k=None):
    """p_lay, p_int of the three regimes of the `p_lay <= 10` break of conv_check / mark_convective_layers:
    high: every p_lay > 10 (the loops run to L - 1); low: every p_lay <= 10 (they end at once);
    break: p_lay[k - 1] > 10 >= p_lay[k] for the interior index k"""
    if regime == "high":
        return syn.pressure_levels(1e9, 1e2, L)
    if regime == "low":
        return syn.pressure_levels(9.0, 1e-3, L)
    if regime == "break":
        p_boa = 1e9
        ratio = (10.0 / p_boa) ** ((2 * L - 1) / (2.0 * k))       # interface k at 10
        return syn.pressure_levels(p_boa, p_boa * ratio, L)
    raise KeyError(regime)


def conv_smem_bytes(L):
    """dynamic LDS of the two convection kernels (conv_adjust.h): 17 double and 5 int arrays of L + 2"""
    return 156 * (L + 2)


def find_lim(p_lay):
    """index at which the loops of conv_check / mark_convective_layers stop (L - 1 without a break)"""
    L = len(p_lay)
    for i in range(L - 1):
        if p_lay[i] <= 1e1:
            return i
    return L - 1


def base_case(L, regime="high", k=None, T_star=5000.0):
    """a small column on the chosen pressure grid, every array that depends on the pressures recomputed, with a plain
    radiative profile (what the first conv_advance sees)"""
    c = cases.make_case(nlayer=L, T_star=T_star, T_intern=300.0, **SIZE)
    c.p_lay, c.p_int = pressures(L, regime, k)
    c.delta_colmass = (c.p_int[:-1] - c.p_int[1:]) / c.g
    c.delta_col_upper = (c.p_lay - c.p_int[1:]) / c.g
    c.delta_col_lower = (c.p_int[:-1] - c.p_lay) / c.g
    c.c_p_lay = np.full(L, pc.R_UNIV / KAPPA)
    c.T_lay = profile(c.p_lay, c.p_int, [], surface=False)
    return c


# ---- profiles -------------------------------------------------------------------------------------------------------
def zone_exponent(n):
    return KAPPA + (0.05 if n < 2 else min(0.05, 0.05 / (n - 1)))


def profile(p_lay, p_int, zones, surface=False, steep=(), T0=1500.0):
    """T_lay[L + 1] (surface last): zones = [(first, last)] super-adiabatic stretches that become one zone each;
    steep = [(first, last)] stretches with the exponent 0.5 (for layers the loops must NOT look at); surface: the
    surface entry super-adiabatic against layer 0 or not"""
    L = len(p_lay)
    expo = np.full(L, G_RAD)                  # expo[i]: between layers i - 1 and i
    for a, b in zones:
        expo[a + 1:b + 1] = zone_exponent(b - a + 1)
    for a, b in steep:
        expo[a + 1:b + 1] = 0.5
    T = np.empty(L + 1)
    T[0] = T0
    for i in range(1, L):
        T[i] = T[i - 1] * (p_lay[i] / p_lay[i - 1]) ** expo[i]
    T[L] = T[0] * (p_int[0] / p_lay[0]) ** (KAPPA + 0.05 if surface else G_RAD)
    return T


def comb(first, last, period=3):
    """two-layer zones every `period` layers: (first, first + 1), (first + period, ...), none beyond `last`"""
    return [(a, a + 1) for a in range(first, last, period) if a + 1 <= last]


# ---- the cases ------------------------------------------------------------------------------------------------------
class ConvCase(object):
    """one crafted column: inputs of a conv_adjust call and the structure it is named for"""

    def __init__(self, name, L, zones=(), surface=False, regime="high", k=None, T_star=5000.0, it=7, steep=(),
                 stale=(), dampara=-1.0, fluxes=None, heat_sum=None, expect=None, expect_zones=None):
        self.name, self.L, self.regime, self.k, self.T_star, self.it = name, L, regime, k, T_star, it
        self.zones, self.surface, self.steep, self.stale = list(zones), surface, list(steep), list(stale)
        self.dampara = float(dampara)                 # what the device gets: <= 0 is automatic
        self.input_dampara = "automatic" if dampara <= 0 else float(dampara)
        self.fluxes = fluxes                          # {interface index: (numerator - F_intern - heat, F_up)} see set_fluxes
        self.heat_sum = heat_sum                      # F_add_heat_sum [L] or None
        self.expect = dict(expect or {})
        want = [((-1 if (surface and a == 0) else a), b) for a, b in self.zones]
        if surface and not any(a == 0 for a, _b in self.zones):
            want = [(-1, 0)] + want
        self.expect_zones = want if expect_zones is None else list(expect_zones)
        self.p_lay, self.p_int = pressures(L, regime, k)
        self.T = profile(self.p_lay, self.p_int, self.zones, surface, self.steep)
        self.conv_layer0 = np.zeros(L + 1, np.int32)
        for j in self.stale:
            self.conv_layer0[j] = 1
        self.conv_unstable0 = np.zeros(L + 1, np.int32)
        n = [b - max(a, 0) + 1 for a, b in self.expect_zones]
        self.n_max = max(n) if n else 0

    @property
    def rtol(self):
        """both sides do the same operations in the same order and differ in pow alone (each within 1 ulp); theta and
        fac[i] are products over at most 2 n such powers for a zone of n layers"""
        return max(1e-13, 4.0 * (self.n_max + 2) * 2.0 ** -53)

    def batch_key(self):
        return (self.L, self.regime, self.k, self.T_star)

    def __repr__(self):
        return self.name


def default_fluxes(L, F_intern):
    """fluxes for the host-only runs of cases that take theirs from the device: ratio = 1 at every interface"""
    F_down = np.linspace(2.0, 1.0, L + 1) * F_intern
    F_up = F_down + F_intern
    return F_up, F_down


def make_quant(case, c, T, F_up, F_down, F_net, mmm, conv_layer=None, conv_unstable=None, F_smooth_sum=None,
               kappa=KAPPA, rad_convergence_limit=None):
    """the attributes of the reference's Store that its host functions touch in the convection loop (the model is
    loop_driver.conv_quant), on copies of the given arrays"""
    L = case.L
    q = cases.Case()
    q.nlayer, q.ninterface = L, L + 1
    q.p_lay, q.p_int = np.asarray(case.p_lay, float), np.asarray(case.p_int, float)
    q.T_lay = np.array(T, np.float64)
    q.kappa_lay, q.kappa_int = np.full(L, float(kappa)), np.full(L + 1, float(kappa))
    q.c_p_lay = np.asarray(c.c_p_lay, np.float64).copy()
    q.meanmolmass_lay = np.array(mmm, np.float64)
    q.F_net, q.F_up_tot, q.F_down_tot = (np.array(v, np.float64) for v in (F_net, F_up, F_down))
    q.F_add_heat_sum = np.zeros(L) if case.heat_sum is None else np.array(case.heat_sum, np.float64)
    q.F_smooth_sum = np.zeros(L) if F_smooth_sum is None else np.array(F_smooth_sum, np.float64)
    q.F_intern, q.T_star = float(c.F_intern), float(case.T_star)
    q.rad_convergence_limit = float(c.rad_convergence_limit if rad_convergence_limit is None else rad_convergence_limit)
    q.input_dampara = case.input_dampara
    q.conv_unstable = np.array(case.conv_unstable0 if conv_unstable is None else conv_unstable, np.int32)
    q.conv_layer = np.array(case.conv_layer0 if conv_layer is None else conv_layer, np.int32)
    q.marked_red = np.zeros(L + 1, np.int32)
    q.converged = np.zeros(L + 1, np.int32)
    q.iter_value = int(case.it)
    return q


# ---- the margin recorder -------------------------------------------------------------------------------------------
class _Logged(np.ndarray):
    """an array that notes the scalar indices it is read at"""

    def __getitem__(self, i):
        if isinstance(i, (int, np.integer)) and getattr(self, "log", None) is not None:
            self.log.append(int(i))
        return np.ndarray.__getitem__(self, i)


def _logged(a):
    v = np.array(a, np.float64).view(_Logged)
    v.log = []
    return v


class Record(object):
    def __init__(self):
        self.margin = np.inf      # smallest |T / limit - 1| of every adiabat and surface comparison made
        self.kink = np.inf        # smallest |T[i+1] / T[i] - 1| the kink rule of mark_convective_layers looked at
        self.zones = []           # (starts, ends) of every conv_correct, in order
        self.layers = []          # conv_layer after every mark_convective_layers: (stitching, before stitching, after)
        self.n_compare = 0


@contextlib.contextmanager
def recording(q):
    """wraps hs._adiabat_limit, the two surface comparisons, the kink rule and hs._zones while host functions run on q"""
    rec = Record()
    orig = dict(limit=hs._adiabat_limit, zones=hs._zones, check=hs.conv_check, mark=hs.mark_convective_layers,
                stitch=hs.stitching_convective_zone_holes)

    def limit(quant, i, sign):
        v = orig["limit"](quant, i, sign)
        rec.margin = min(rec.margin, abs(quant.T_lay[i + 1] / v - 1.0))
        rec.n_compare += 1
        return v

    def surface(quant, sign):
        L = int(quant.nlayer)
        T_ad = quant.T_lay[L] * (quant.p_lay[0] / quant.p_int[0]) ** (quant.kappa_int[0] * (1 + sign * 1e-6))
        rec.margin = min(rec.margin, abs(quant.T_lay[0] / T_ad - 1.0))
        rec.n_compare += 1

    def check(quant):
        surface(quant, +1)
        return orig["check"](quant)

    def stitch(quant):
        rec.before_stitch = np.array(quant.conv_layer, np.int32)
        return orig["stitch"](quant)

    def mark(quant, stitching):
        surface(quant, -1)
        L = int(quant.nlayer)
        T = np.asarray(quant.T_lay, float)
        if L >= 2:
            rec.kink = min(rec.kink, float(np.abs(T[1:L] / T[:L - 1] - 1.0).min()))
        rec.before_stitch = None
        out = orig["mark"](quant, stitching)
        after = np.array(quant.conv_layer, np.int32)
        rec.layers.append((stitching, after if rec.before_stitch is None else rec.before_stitch, after))
        return out

    def zones(flags, L):
        s, e = orig["zones"](flags, L)
        rec.zones.append((list(s), list(e)))
        return s, e

    hs._adiabat_limit, hs._zones, hs.conv_check, hs.mark_convective_layers = limit, zones, check, mark
    hs.stitching_convective_zone_holes = stitch
    try:
        yield rec
    finally:
        hs._adiabat_limit, hs._zones, hs.conv_check, hs.mark_convective_layers = (orig["limit"], orig["zones"],
                                                                                 orig["check"], orig["mark"])
        hs.stitching_convective_zone_holes = orig["stitch"]


def run_host(q):
    """hs.convective_adjustment(q) under the recorder; returns the record, with the flux-test indices of the last
    (fudging) conv_correct and the fudge factors they give"""
    q.F_up_tot = _logged(q.F_up_tot)
    q.F_add_heat_sum = _logged(q.F_add_heat_sum)
    with recording(q) as rec, np.errstate(invalid="ignore"):
        hs.convective_adjustment(q)
    rec.tests = list(q.F_up_tot.log)
    rec.below = list(q.F_add_heat_sum.log)
    q.F_up_tot, q.F_add_heat_sum = np.asarray(q.F_up_tot).copy(), np.asarray(q.F_add_heat_sum).copy()
    nz = len(rec.tests)
    rec.fudge, rec.ratio, rec.dampara = [], [], []
    for n, (test, below) in enumerate(zip(rec.tests, rec.below)):
        if q.input_dampara == "automatic":
            dp = (0.5 if n < nz - 1 else 4.0) if q.T_star > 10 else 8.0
        else:
            dp = float(q.input_dampara)
        ratio = (q.F_intern + q.F_add_heat_sum[below] + q.F_smooth_sum[below] + q.F_down_tot[test]) / q.F_up_tot[test]
        with np.errstate(invalid="ignore"):
            f = np.float64(ratio) ** (1.0 / dp)
        rec.ratio.append(float(ratio))
        rec.dampara.append(dp)
        rec.fudge.append(min(1.01, max(0.99, f)))
        rec.nan = getattr(rec, "nan", []) + [bool(np.isnan(f))]
    return rec


def host_inputs(case, c=None):
    """what a host-only run of the case uses where the device run reads its own state back: the fluxes (ratio 1
    everywhere unless the case chooses them) and the mean molecular mass of the premixed table at the crafted profile"""
    import oracle
    c = base_case(case.L, case.regime, case.k, case.T_star) if c is None else c
    F_up, F_down = default_fluxes(case.L, c.F_intern)
    F_up, F_down = apply_fluxes(case, F_up, F_down, c.F_intern)
    mmm = np.zeros(case.L)
    oracle.port.meanmolmass_interpol(np.ascontiguousarray(case.T), c.ktemp, mmm, c.opac_meanmass,
                                     np.ascontiguousarray(case.p_lay), c.kpress, c.npress, c.ntemp, case.L)
    return c, F_up, F_down, F_up - F_down, mmm


# ---- the list -------------------------------------------------------------------------------------------------------
def boundary_cases():
    """zone starts and ends at the last lane of one ballot round and the first of the next (the walk starts at layer -1:
    lane 63 of round 0 is layer 62), for L on both sides"""
    out = []
    for L in (63, 64, 65, 66):
        for b in (62, 63, 64):
            if b + 1 <= L - 1:
                out.append(ConvCase("L%d_start%d" % (L, b), L, zones=[(10, 14), (b, L - 1)], expect=dict(start=b)))
            if b <= L - 1:
                out.append(ConvCase("L%d_end%d" % (L, b), L, zones=[(10, 14), (b - 5, b)], expect=dict(end=b)))
    out.append(ConvCase("L127_end126", 127, zones=[(30, 40), (125, 126)], expect=dict(end=126)))
    out.append(ConvCase("L127_surface_end126", 127, zones=[(30, 40), (120, 126)], surface=True, expect=dict(end=126)))
    out.append(ConvCase("L128_start126", 128, zones=[(30, 40), (126, 127)], expect=dict(start=126, end=127)))
    out.append(ConvCase("L128_end126", 128, zones=[(30, 40), (120, 126)], expect=dict(end=126)))
    out.append(ConvCase("L129_start126", 129, zones=[(30, 40), (126, 128)], expect=dict(start=126, end=128)))
    out.append(ConvCase("L129_start127", 129, zones=[(30, 40), (127, 128)], surface=True, expect=dict(start=127)))
    out.append(ConvCase("L129_end126", 129, zones=[(30, 40), (120, 126)], expect=dict(end=126)))
    return out


def size_cases():
    out = []
    out.append(ConvCase("L2_surface", 2, surface=True, expect=dict(start=-1, end=0)))
    out.append(ConvCase("L2_pair", 2, zones=[(0, 1)], expect=dict(start=0, end=1)))
    out.append(ConvCase("L3_surface", 3, surface=True, expect=dict(start=-1, end=0)))
    out.append(ConvCase("L3_pair", 3, zones=[(1, 2)], expect=dict(start=1, end=2)))
    out.append(ConvCase("L8_surface", 8, surface=True, expect=dict(start=-1, end=0)))
    out.append(ConvCase("L8_two", 8, zones=[(1, 2), (5, 6)], expect=dict(nzones=2)))
    for L in (255, 256, 257):
        out.append(ConvCase("L%d_comb_top" % L, L, zones=comb(1, L - 5) + [(L - 2, L - 1)],
                            expect=dict(start=L - 2, end=L - 1, min_zones=65)))
    out.append(ConvCase("L256_comb_start254", 256, zones=comb(2, 250) + [(254, 255)], surface=True,
                        expect=dict(start=254, end=255, min_zones=65)))
    out.append(ConvCase("L257_comb_end255", 257, zones=comb(1, 245) + [(250, 255)], expect=dict(end=255, min_zones=65)))
    for L in (313, 314):
        out.append(ConvCase("L%d_comb" % L, L, zones=comb(1, L - 1), expect=dict(min_zones=100)))
        out.append(ConvCase("L%d_long" % L, L, zones=[(5, L - 5)], expect=dict(nzones=1, min_longest=300)))
    return out


STITCH_ZONES = [(5, 10), (13, 18), (30, 35)]


def special_cases():
    """at L = 64"""
    L = 64
    out = [ConvCase("none", L, expect=dict(nzones=0, untouched=True))]
    out.append(ConvCase("surface_alone", L, zones=[(20, 25)], surface=True, expect=dict(start=-1, end=0, nzones=2)))
    out.append(ConvCase("surface_merged", L, zones=[(0, 6), (20, 25)], surface=True, expect=dict(start=-1, end=6, nzones=2)))
    # stale flags above the break.  They make zones of radiative layers; where the adjustment runs twice (a column that
    # also has an instability) the first pass puts 46..48 on the adiabat, steeper than what was there, so that layer 48
    # ends up colder than 49 and the kink rule of the second marking clears it: kept = what is left at the end
    stale, kept = [46, 47, 48, 55], [46, 47, 55]
    out.append(ConvCase("press_high", L, zones=[(10, 14), (50, 60)], regime="high", expect=dict(lim=L - 1, nzones=2)))
    # every p_lay <= 10: the loops look at nothing, the super-adiabatic stretches stay, the stale flags make zones
    out.append(ConvCase("press_low", L, regime="low", steep=[(10, 14), (30, 33)], stale=stale,
                        expect=dict(lim=0, stale=stale), expect_zones=[(46, 48), (55, 55)]))
    out.append(ConvCase("press_low_surface", L, regime="low", surface=True, steep=[(10, 14)], stale=stale,
                        expect=dict(lim=0, stale=kept, start=-1), expect_zones=[(-1, 0), (46, 47), (55, 55)]))
    # break at 40: zones below, a super-adiabatic stretch above that must be ignored, stale flags above
    out.append(ConvCase("press_break", L, regime="break", k=40, zones=[(10, 14), (36, 39)], steep=[(50, 53)], stale=stale,
                        expect=dict(lim=40, stale=kept, ignored=(50, 53)),
                        expect_zones=[(10, 14), (36, 39), (46, 47), (55, 55)]))
    out.append(ConvCase("press_break_at_zone", L, regime="break", k=40, zones=[(10, 14), (36, 40)], steep=[(41, 44)],
                        stale=stale, expect=dict(lim=40, stale=kept, ignored=(41, 44)),
                        expect_zones=[(10, 14), (36, 40), (46, 47), (55, 55)]))
    out.append(ConvCase("stitch_5000", L, zones=STITCH_ZONES, it=5000, expect=dict(nzones=3, stitch=False)))
    out.append(ConvCase("stitch_5001", L, zones=STITCH_ZONES, it=5001, expect=dict(nzones=2, stitch=True),
                        expect_zones=[(5, 18), (30, 35)]))
    out.append(ConvCase("it_7", L, zones=[(10, 14), (40, 50)], it=7, expect=dict(nzones=2)))
    out.append(ConvCase("it_10", L, zones=[(10, 14), (40, 50)], it=10, expect=dict(nzones=2)))
    return out


# ratio of (F_intern + heating + F_down) / F_up at the flux-test interface, per outcome of the fudge factor:
# `lo`: clamps to 0.99 for every damping parameter used (0.5 ... 8); `hi`: to 1.01; `mid`: strictly between; `nan`: a
# negative ratio under a fractional power (the heating sum below the test interface is set strongly negative)
FUDGE_RATIO = dict(lo=0.5, hi=2.0, mid=1.002, nan=None)
DAMPARA = dict(auto_star=(-1.0, 5000.0), auto_nostar=(-1.0, 5.0), explicit=(2.5, 5000.0), zero=(0.0, 5000.0))


def fudge_cases():
    """two zones with a gap wider than a scale height: zone 0 takes its test interface from the gap, zone 1 (the top
    zone) from 0.8 end + 0.2 L; and a surface-only zone at L = 3, whose test index is 0, so that the heating sum is
    read at the wrapped index L - 1"""
    out = []
    L = 64
    zones = [(8, 14), (30, 40)]
    t0, t1 = int((14 + 30) / 2), int(0.8 * 40 + 0.2 * L)
    for dname, (dampara, T_star) in DAMPARA.items():
        for o0, o1 in (("lo", "hi"), ("hi", "mid"), ("mid", "nan"), ("nan", "lo")):
            if o0 == "nan" and dampara <= 0 and T_star > 10:
                continue          # the lower zone's automatic damping is 0.5: a square, no NaN from a negative ratio
            heat = np.linspace(0.01, 0.02, L) * pc.SIGMA_SB * 300.0 ** 4
            fl = {}
            for t, o in ((t0, o0), (t1, o1)):
                if o == "nan":
                    heat[t - 1] = -50.0 * pc.SIGMA_SB * 300.0 ** 4
                    fl[t] = None
                else:
                    fl[t] = FUDGE_RATIO[o]
            out.append(ConvCase("fudge_%s_%s_%s" % (dname, o0, o1), L, zones=zones, T_star=T_star, dampara=dampara,
                                fluxes=fl, heat_sum=heat,
                                expect=dict(tests=[t0, t1], outcomes=[o0, o1], branches=["gap", "top"])))
    L = 3
    for dname, (dampara, T_star) in DAMPARA.items():
        for o in ("mid", "nan", "lo", "hi"):
            heat = np.array([0.01, 0.02, 0.3]) * pc.SIGMA_SB * 300.0 ** 4
            if o == "nan":
                heat[L - 1] = -50.0 * pc.SIGMA_SB * 300.0 ** 4
            out.append(ConvCase("fudge_wrap_%s_%s" % (dname, o), L, surface=True, T_star=T_star, dampara=dampara,
                                fluxes={0: FUDGE_RATIO[o]}, heat_sum=heat,
                                expect=dict(tests=[0], outcomes=[o], branches=["wrap"], start=-1, end=0)))
    return out


def apply_fluxes(case, F_up, F_down, F_intern):
    """the chosen ratios of a fudge case written into copies of F_up_tot / F_down_tot: case.fluxes = {test index: ratio
    wanted for (F_intern + heat[test - 1] + F_down[test]) / F_up[test]}; None: the (negative) heating sum decides"""
    F_up, F_down = np.array(F_up, np.float64), np.array(F_down, np.float64)
    L = case.L
    heat = case.heat_sum if case.heat_sum is not None else np.zeros(L)
    for test, ratio in (case.fluxes or {}).items():
        below = test - 1 if test - 1 >= 0 else test - 1 + L
        F_down[test] = 3.0 * F_intern
        F_up[test] = 4.0 * F_intern if ratio is None else (F_intern + heat[below] + F_down[test]) / ratio
    return F_up, F_down


def batch_columns():
    """the three-column batch at L = 65: three different profiles; column 1 is `done`"""
    L = 65
    return [ConvCase("col0_two_zones", L, zones=[(10, 14), (58, 64)], expect=dict(nzones=2)),
            ConvCase("col1_done", L, zones=[(3, 9), (40, 45)], surface=True, expect=dict(nzones=3)),
            ConvCase("col2_surface_merged", L, zones=[(0, 4), (20, 30), (61, 63)], surface=True, expect=dict(nzones=3))]


ADVANCE_L = (127, 128, 129, 257, 313, 314)


def advance_case(L):
    """the column of the advance half at L layers: a comb where L is large enough for five ballot rounds"""
    if L >= 257:
        return ConvCase("adv_L%d_comb" % L, L, zones=comb(1, L - 5) + [(L - 2, L - 1)], expect=dict(min_zones=65))
    return ConvCase("adv_L%d" % L, L, zones=[(30, 40), (120, 126)], expect=dict(nzones=2))


def adjust_cases():
    return size_cases() + boundary_cases() + special_cases() + fudge_cases()


def all_cases():
    return adjust_cases() + batch_columns() + [advance_case(L) for L in ADVANCE_L]
