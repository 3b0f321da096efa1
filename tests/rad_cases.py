"""TEST INFRASTRUCTURE: crafted inputs for the radiative temperature step (rad_temp_step and smoothing_flux in
csrc/temp_step.h, k_rad_temp_iter in csrc/stage_flux.hip, the tail of k_rt_totals_b in csrc/rt_kernels.h) and a
long-double restatement of orc_rad_temp_iter (oracle/helios_oracle.c) that also returns the MARGIN of every discrete
comparison it makes.  No GPU here: tests/test_rad_cases.py proves on the restatement and the CPU oracle that every case
takes the branches it is named for, tests/test_gpu_rad_edges.py runs the same cases on the device.

How a case is crafted.  Every entry i of a column (layers 0 .. L - 1, the ghost layer L) gets its branch by design
numbers, and the inputs follow from them in plain double arithmetic:
  e[i]    the convergence quantity |F_intern + heat_sum + smooth_sum - F_net[i + 1]| / (F_toa + F_intern) in units of
          local_limit, signed; |e| < 1 sets the flag.  F_net[i + 1] is placed accordingly, F_net[0] by e_ghost.
  ghost   |F_intern - F_net[1]| / (F_toa + F_intern) is |e[0] - 0.1| local_limit (heat_sum[0] + smooth_sum[0] is
          0.1 (F_toa + F_intern) local_limit without smoothing): above 0.5 the ghost layer steps on F_net[1]
  sgn[i]  sign of dF of a layer; F_add_heat_lay[i] is what makes F_net[i] - F_net[i + 1] + heating (+ F_smooth) that
  dT[i]   |delta_T| wanted before the clamp at 500: the prefactor is chosen for it (where the iteration resets the
          prefactor the step is what it is)
  r[i]    |T - T_store| in units of adapt_interval / 2 |delta_T|: below 1 the prefactor shrinks, above it grows
  near[i] T placed half a step inside ("hi", "lo") or two steps away from ("hi_safe", "lo_safe") a temperature clamp
  zero    entries with dF == 0 exactly: heating = -(F_net[i] - F_net[i + 1]) as the kernel evaluates it
The expectations (flags, clamps, shrinking prefactors, the ghost layer's choice) are read off these design numbers, never
off an implementation.

Margins.  A comparison a <> b has the margin |a - b| / max(|a|, |b|); exact zeros on both sides (a == b == 0, reached
by exact arithmetic only) and an input compared as it stands (p_lay against 1e6) carry no rounding and count as inf.
"""
import numpy as np

from helios_amd import phys_const as pc
from helios_amd import synthetic as syn

LD = np.longdouble
MARGIN_MIN = 1e-10
DIM, STEP = 400, 10
T_MAX = DIM * STEP - 1.001
T_MIN = 1.001
G = 1000.0
F_TOA = 1.0e9
F_INTERN = pc.SIGMA_SB * 300.0 ** 4


def rel(a, b):
    a, b = LD(a), LD(b)
    m = max(abs(a), abs(b))
    return np.inf if m == 0 else float(abs(a - b) / m)


# ---- the restatement ------------------------------------------------------------------------------------------------
def restate(c):
    """orc_rad_temp_iter on the inputs of case `c` (its attributes are not changed).  What the kernel gets by one or two
    IEEE operations (F_net_diff, dF, the prefactor's update, T_store) is formed in double in the kernel's order, what
    passes through pow in long double.  Returns (out, margins): out = dict of T (long double), T64 (its double, clamped
    entries at the limits), T_store, pref, F_net_diff, abort, F_smooth, F_smooth_sum (long double), and the discrete
    outcomes clamp500 / clamp_lo / clamp_hi / shrink / grow / ghost / smoothed; margins = [(what, entry, margin)]"""
    L = c.L
    m = []
    T0 = np.array(c.T, np.float64)
    F_net = np.array(c.F_net, np.float64)
    F_smooth = np.array(c.F_smooth, np.float64).astype(LD)
    F_smooth_sum = np.array(c.F_smooth_sum, np.float64).astype(LD)
    smoothed = []
    if c.smooth == 1:
        for i in range(L):
            x = np.float64(0.0)
            if c.p_lay[i] != 1e6:
                m.append(("p_lay < 1e6", i, rel(c.p_lay[i], 1e6)))
            if c.p_lay[i] < 1e6 and i < L - 1 and i > 0:
                x = (T0[i - 1] + T0[i + 1]) / np.float64(2.0) - T0[i]
                smoothed.append(i)
            F_smooth[i] = LD(x) ** 7
        F_smooth_sum = np.cumsum(F_smooth)
    F_smooth64 = F_smooth.astype(np.float64)
    norm = LD(c.F_down_tot[L]) + LD(c.F_intern)
    T = np.zeros(L + 1, LD)
    T64 = np.zeros(L + 1)
    T_store, pref = np.array(c.T_store, np.float64), np.array(c.pref, np.float64)
    F_net_diff = np.zeros(L)
    abort = np.zeros(L + 1, np.int32)
    out = dict(clamp500=[], clamp_lo=[], clamp_hi=[], shrink=[], grow=[], ghost=0, smoothed=smoothed)
    for i in range(L + 1):
        if i < L:
            d = (F_net[i] - F_net[i + 1]) + np.float64(c.heat_lay[i])
            F_net_diff[i] = d
            dF = d + F_smooth64[i]
            if dF != 0:
                # against the terms it is the sum of; F_net is of order 1e9 and dF of order 1e5, so this is >= 1e-5
                m.append(("dF != 0", i, float(abs(dF) / (abs(F_net[i]) + abs(F_net[i + 1]) + abs(c.heat_lay[i])
                                                          + abs(F_smooth64[i])))))
        else:
            dF = np.float64(c.F_intern) - F_net[0]
            q = abs(LD(c.F_intern) - LD(F_net[1])) / norm
            m.append(("ghost > 0.5 local_limit", i, rel(q, LD(0.5) * LD(c.limit))))
            if q > LD(0.5) * LD(c.limit):
                dF = np.float64(c.F_intern) - F_net[1]
                out["ghost"] = 1
        delta_T = LD(0)
        if c.tstep == 0:
            if c.it == c.foreplay:
                pref[i] = 1e0
            if c.it == 10000:
                pref[i] = 1e-1
            if dF != 0:
                delta_t = LD(pref[i]) * LD(c.p_lay[0]) / LD(abs(dF)) ** LD(0.9)
                delta_T = LD(dF) / (LD(c.p_int[0]) - LD(c.p_int[1])) * delta_t
            m.append(("|delta_T| > 500", i, rel(abs(delta_T), 500)))
            if abs(delta_T) > 500:
                delta_T = LD(500.0) * np.sign(dF)
                out["clamp500"].append(i)
            if c.it % c.adapt == 0:
                T_store[i] = T0[i]
            if c.it % c.adapt == c.adapt - 1:
                a, b = abs(T0[i] - T_store[i]), LD(c.adapt) / 2 * abs(delta_T)
                m.append(("adaptive <", i, rel(a, b)))
                if a < b:
                    pref[i] = pref[i] / np.float64(1.5)
                    out["shrink"].append(i)
                else:
                    pref[i] = pref[i] * np.float64(1.1)
                    out["grow"].append(i)
        else:
            j = i if i < L else 0
            delta_T = (LD(c.g) / (LD(c.c_p[j]) / (LD(c.mmm[j]) / LD(pc.AMU))) * LD(dF)
                       / (LD(c.p_int[j]) - LD(c.p_int[j + 1])) * LD(c.tstep))
        t = LD(T0[i]) + delta_T
        exact = False
        if c.no_atmo == 1 and i != L:
            t, exact = LD(T_MIN), True
        else:
            m.append(("T < 1.001", i, rel(t, T_MIN)))
            m.append(("T > dim step - 1.001", i, rel(t, T_MAX)))
        if t < T_MIN:
            t, exact = LD(T_MIN), True
            out["clamp_lo"].append(i)
        if t > T_MAX:
            t, exact = LD(T_MAX), True
            out["clamp_hi"].append(i)
        T[i] = t
        T64[i] = (T_MIN if t == LD(T_MIN) else T_MAX) if exact else np.float64(t)
        if i < L:
            q = abs(LD(c.F_intern) + LD(c.heat_sum[i]) + F_smooth_sum[i] - LD(F_net[i + 1])) / norm
        else:
            q = abs(LD(c.F_intern) - LD(F_net[0])) / norm
        m.append(("ok", i, rel(q, c.limit)))
        abort[i] = 1 if q < LD(c.limit) else 0
    out.update(T=T, T64=T64, T_store=T_store, pref=pref, F_net_diff=F_net_diff, abort=abort, F_smooth=F_smooth,
               F_smooth_sum=F_smooth_sum)
    return out, m


def min_margin(margins):
    return min([v for _w, _i, v in margins] or [np.inf])


def run_impl(impl, c):
    """the stage function of `impl` (oracle.port, the reference, the HIP library) on copies of the case's inputs, with
    F_net_diff one entry longer than the kernel may write and a marker in it"""
    L = c.L
    d = dict(T=np.array(c.T, np.float64), T_store=np.array(c.T_store, np.float64), pref=np.array(c.pref, np.float64),
             F_net_diff=np.full(L + 1, POISON), abort=np.full(L + 1, -7, np.int32),
             F_smooth=np.array(c.F_smooth, np.float64), F_smooth_sum=np.array(c.F_smooth_sum, np.float64))
    impl.rad_temp_iter(np.array(c.F_down_tot, np.float64), np.zeros(L + 1), np.array(c.F_net, np.float64),
                       d["F_net_diff"], d["T"], np.array(c.p_lay, np.float64), np.array(c.p_int, np.float64), d["abort"],
                       d["T_store"], d["pref"], np.array(c.heat_lay, np.float64), np.array(c.heat_sum, np.float64),
                       d["F_smooth"], d["F_smooth_sum"], np.array(c.c_p, np.float64), np.array(c.mmm, np.float64),
                       int(c.it), int(c.foreplay), float(c.g), L, float(c.tstep), float(c.limit), int(c.adapt),
                       int(c.smooth), DIM, STEP, float(c.F_intern), int(c.no_atmo))
    return d


POISON = -1.25e300


# ---- the cases ------------------------------------------------------------------------------------------------------
def alt(n, a, b):
    return np.array([a if i % 2 == 0 else b for i in range(n)], float)


def default_T(n):
    """smooth in the large, kinks of a few K of both signs (the smoothing flux is their 7th power)"""
    return 1500.0 + 400.0 * np.sin(0.02 * np.arange(n)) + np.array([(3.0, -2.0, 4.0, 0.0, -5.0)[i % 5] for i in range(n)])


class RadCase(object):
    """one crafted column; see the module's text for the design numbers"""

    def __init__(self, name, L, branch, it=5, foreplay=0, adapt=20, limit=1e-3, e=None, e_ghost=0.25, sgn=None, dT=3.14159,
                 r=None, near=None, zero=(), tstep=False, no_atmo=0, smooth=0, p=(1e9, 1e2), p_exact=None, base="keep",
                 given=None):
        """given: dict(F_net, F_down_tot, p_lay, p_int, T, F_intern, g, c_p, mmm) read back from a batch.  The fluxes are
        what they are then: the convergence quantity is steered by F_add_heat_sum instead of F_net, local_limit is
        chosen so that the ghost layer's quantity is e_ghost of it (limit = None), and which flux the ghost layer steps
        on is left to the fluxes (its margin is asserted all the same)"""
        self.name, self.L, self.branch = name, L, branch
        self.it, self.foreplay, self.adapt = int(it), int(foreplay), int(adapt)
        self.smooth, self.no_atmo, self.g, self.F_intern = int(smooth), int(no_atmo), G, F_INTERN
        self.base = base                                  # "keep", 1.0 or 0.1: what the iteration makes of the prefactor
        assert base == (0.1 if it == 10000 else 1.0 if it == foreplay else "keep")     # by hand, and checked
        n = L + 1
        e = alt(L, 0.5, -0.5) if e is None else np.asarray(e, float)
        sgn = alt(L, 1.0, -1.0) if sgn is None else np.asarray(sgn, float)
        dT = np.full(n, float(dT)) if np.isscalar(dT) else np.asarray(dT, float)
        r = alt(n, 0.5, 2.0) if r is None else np.asarray(r, float)
        near = dict(near or {})
        self.zero = sorted(zero)
        i_ = np.arange(L)
        if given is None:
            self.limit = float(limit)
            self.p_lay, self.p_int = syn.pressure_levels(p[0], p[1], L)
            for k, v in (p_exact or {}).items():
                self.p_lay[k] = v
            self.F_down_tot = np.linspace(0.2, 1.0, n) * F_TOA
            self.c_p = 3.5 * pc.R_UNIV * (1.0 + 0.3 * i_ / float(L))
            self.mmm = 2.3 * pc.AMU * (1.0 + 0.2 * (i_ % 4))
            T = default_T(n)
        else:
            assert not near and not zero
            self.p_lay, self.p_int, self.F_down_tot, self.c_p, self.mmm, T = (
                np.array(given[k], np.float64) for k in ("p_lay", "p_int", "F_down_tot", "c_p", "mmm", "T"))
            self.g, self.F_intern = float(given["g"]), float(given["F_intern"])
            self.F_net = np.array(given["F_net"], np.float64)
        F_INT = self.F_intern
        norm = self.F_down_tot[L] + F_INT
        if given is not None:
            self.limit = float(limit) if limit is not None else float(abs(F_INT - self.F_net[0]) / norm / abs(e_ghost))
        nl = norm * self.limit
        if self.smooth == 1 or given is not None:
            self.F_smooth, self.F_smooth_sum = np.zeros(L), np.zeros(L)     # (a batch holds zeros while smooth = 0)
        else:        # inputs of the step then, read at [i]: different everywhere so that a wrong index shows
            self.F_smooth = 10.0 * ((i_ % 5) - 2.0)
            self.F_smooth_sum = -0.2 * nl * (1.0 + 0.07 * i_)
            self.F_smooth_sum[0] = -0.2 * nl
        self.T = T                                        # temperature clamps move entries below, never the neighbours
        fs, fss = self.smoothing(T)                       # of a smoothed layer: `near` is not used with smooth = 1
        assert not (near and self.smooth == 1)
        if given is None:
            self.heat_sum = 0.3 * nl * (1.0 + i_ / float(L))
            self.heat_sum[0] = 0.3 * nl
            self.F_net = np.zeros(n)
            self.F_net[0] = F_INT - e_ghost * nl
            self.F_net[1:] = F_INT + self.heat_sum + fss - e * nl
        else:
            self.heat_sum = self.F_net[1:] - F_INT - fss + e * nl
        mag = 1e5 * (1.0 + 0.1 * (i_ % 7))
        diff = self.F_net[:-1] - self.F_net[1:]
        self.heat_lay = sgn * mag - diff - fs
        for i in self.zero:
            if i < L:
                assert self.smooth == 0
                self.F_smooth[i] = 0.0
                self.heat_lay[i] = -diff[i]
        dF = np.append((diff + self.heat_lay) + fs, 0.0)
        ghost_q = abs(F_INT - self.F_net[1]) / norm
        dF[L] = F_INT - (self.F_net[1] if ghost_q > 0.5 * self.limit else self.F_net[0])
        assert all(dF[i] == 0 for i in self.zero) and np.count_nonzero(dF == 0) == len(self.zero)
        K = self.p_lay[0] / (self.p_int[0] - self.p_int[1])
        self.pref = np.full(n, 0.7)
        if tstep:
            j = np.append(i_, 0)
            coef = self.g / (self.c_p[j] / (self.mmm[j] / pc.AMU)) * dF / (self.p_int[j] - self.p_int[j + 1])
            self.tstep = float(dT.max() / np.abs(coef).max()) if given is None else float(given["tstep"])
            step = coef * self.tstep
        else:
            self.tstep = 0.0
            nz = dF != 0
            if base == "keep":
                self.pref[nz] = dT[nz] / (K * np.abs(dF[nz]) ** 0.1)
            eff = self.pref if base == "keep" else np.full(n, float(base))
            step = np.zeros(n)
            step[nz] = np.sign(dF[nz]) * np.minimum(eff[nz] * K * np.abs(dF[nz]) ** 0.1, 500.0)
        self.step = step
        for i, where in near.items():
            s = abs(step[i])
            T[i] = dict(hi=T_MAX - 0.5 * s, hi_safe=T_MAX - 2.0 * s, lo=T_MIN + 0.5 * s, lo_safe=T_MIN + 2.0 * s)[where]
            assert step[i] > 0 if where.startswith("hi") else step[i] < 0
        self.T_store = T + np.where(step != 0, r * self.adapt / 2.0 * np.abs(step), 1.0)
        # ---- what the design says must come out ----
        store = self.tstep == 0 and self.it % self.adapt == 0
        adapts = self.tstep == 0 and self.it % self.adapt == self.adapt - 1
        idx = np.arange(n)
        shrink = (step != 0) & ((r < 1) | store) if adapts else np.zeros(n, bool)
        self.expect = dict(
            abort=(np.abs(np.append(e, e_ghost)) < 1).astype(np.int32),
            # heat_sum[0] + smooth_sum[0] is (0.3 - 0.2) nl without smoothing, 0.3 nl with it (layer 0 is never smoothed)
            ghost=(1 if abs(e[0] - (0.1 if self.smooth == 0 else 0.3)) > 0.5 else 0) if given is None else None,
            clamp500=[int(i) for i in idx if self.tstep == 0 and base == "keep" and dT[i] > 500 and dF[i] != 0],
            clamp_hi=sorted(i for i, w in near.items() if w == "hi"),
            clamp_lo=sorted(i for i, w in near.items() if w == "lo"),
            shrink=[int(i) for i in idx[shrink]], grow=[int(i) for i in idx[~shrink]] if adapts else [],
            stores=bool(store))

    def smoothing(self, T):
        """the smoothing flux and its prefix sum as the design places F_net by them (plain double)"""
        L = self.L
        fs = np.zeros(L)
        if self.smooth == 1:
            for i in range(1, L - 1):
                if self.p_lay[i] < 1e6:
                    fs[i] = ((T[i - 1] + T[i + 1]) / 2.0 - T[i]) ** 7
            return fs, np.cumsum(fs)
        return self.F_smooth, self.F_smooth_sum

    def __repr__(self):
        return self.name


def iteration_cases():
    out = []
    for it in (0, 6, 7, 19, 20, 39, 9999, 10000, 10019):
        base = 0.1 if it == 10000 else 1.0 if it == 7 else "keep"
        out.append(RadCase("it%d_adapt20_foreplay7" % it, 5, "iteration %d" % it, it=it, foreplay=7, base=base))
    out.append(RadCase("it0_foreplay0", 5, "iteration 0 is the foreplay's end and stores", it=0, foreplay=0, base=1.0))
    out.append(RadCase("it10000_foreplay10000", 5, "the second assignment wins", it=10000, foreplay=10000, base=0.1))
    out.append(RadCase("it5_adapt1", 5, "store and adapt test in one call", it=5, adapt=1))
    out.append(RadCase("it10000_adapt1", 5, "reset, store and adapt test in one call", it=10000, adapt=1, base=0.1))
    out.append(RadCase("it4_adapt2", 5, "stores", it=4, adapt=2))
    out.append(RadCase("it5_adapt2", 5, "adapt test", it=5, adapt=2))
    return out


def branch_cases():
    out = []
    zero = (0, 1, 2, 4)
    for it in (5, 19):       # three layers and the ghost layer without a flux divergence; at 19 the adapt test runs
        out.append(RadCase("dF_zero_it%d" % it, 4, "dF == 0", it=it, zero=zero, e_ghost=0.0, r=[0.5] * 5))
    for sg in (1.0, -1.0):   # |delta_T| at 499 and 501 for either sign of dF, the ghost layer on both sides too
        for gh in (499.0, 501.0):
            out.append(RadCase("clamp500_%s_ghost%d" % ("up" if sg > 0 else "down", gh), 4, "clamp at 500",
                               dT=[499.0, 501.0, 499.0, 501.0, gh], sgn=[sg, sg, -sg, -sg], e_ghost=0.25 * sg))
    out.append(RadCase("clamp500_it19", 4, "clamped step in the adapt test", it=19, dT=[499.0, 501.0, 499.0, 501.0, 501.0],
                       sgn=[1, -1, -1, 1]))
    out.append(RadCase("T_clamps", 4, "both temperature clamps", sgn=[1, 1, -1, -1], e_ghost=0.25,
                       near={0: "hi", 1: "hi_safe", 2: "lo", 3: "lo_safe", 4: "hi"}))
    out.append(RadCase("T_clamps_ghost_low", 4, "the ghost layer at the lower clamp", sgn=[1, 1, -1, -1], e_ghost=-0.25,
                       near={0: "hi_safe", 2: "lo_safe", 3: "lo", 4: "lo"}))
    out.append(RadCase("T_clamps_tstep", 4, "both temperature clamps, time-stepped", sgn=[1, 1, -1, -1], tstep=True,
                       near={0: "hi", 1: "hi_safe", 2: "lo", 3: "lo_safe", 4: "hi"}))
    # the ghost layer: |e[0] - 0.1| = 0.4 / 0.65 / 0.6 against 0.5
    out.append(RadCase("ghost_F_net0", 3, "ghost layer below 0.5 local_limit", e=[0.5, -0.5, 0.5], e_ghost=-0.3))
    out.append(RadCase("ghost_F_net1", 3, "ghost layer between 0.5 and 1 local_limit", e=[0.75, -0.5, 0.5], e_ghost=-0.3))
    out.append(RadCase("ghost_F_net1_negative", 3, "ghost layer above 0.5 local_limit, other sign", e=[-0.5, -0.5, 0.5]))
    L = 6
    ok = alt(L, 0.5, -0.5)
    out.append(RadCase("conv_all", L, "every flag set", e=ok, e_ghost=0.25))
    first, last = ok.copy(), ok.copy()
    first[0], last[L - 1] = 2.0, -2.0
    out.append(RadCase("conv_but_first", L, "all but the first layer", e=first))
    out.append(RadCase("conv_but_last", L, "all but the last layer", e=last))
    out.append(RadCase("conv_but_ghost", L, "all but the ghost layer", e=ok, e_ghost=2.0))
    out.append(RadCase("conv_none", L, "no flag set", e=alt(L, 2.0, -2.0), e_ghost=-2.0))
    out.append(RadCase("tstep", 5, "physical timestep", tstep=True, it=19))
    out.append(RadCase("tstep_F_net1", 5, "physical timestep, ghost layer on F_net[1]", tstep=True, e=[0.75, -0.5, 0.5, 2, 0.5]))
    out.append(RadCase("no_atmo", 5, "no_atmo", no_atmo=1, it=19))
    out.append(RadCase("no_atmo_tstep", 5, "no_atmo, time-stepped", no_atmo=1, tstep=True))
    return out


# p_lay of pressure_levels(1e9, 1e2, 8): 10^(8.53, 7.6, 6.67, 5.73, 4.8, 3.87, 2.93, 2): layer 3 is put AT 1e6
SMOOTH8 = dict(p=(1e9, 1e2), p_exact={3: 1e6})


def smooth_cases():
    out = []
    out.append(RadCase("smooth_straddle", 8, "p_lay on both sides of 1e6 and at it", smooth=1, it=19, **SMOOTH8))
    out.append(RadCase("smooth_all_low", 8, "every p_lay below 1e6: the guards 0 < i < L - 1 decide", smooth=1,
                       p=(1e5, 1e-1), e=[0.5, -0.5, 2, 0.5, -0.5, -2, 0.5, 0.5]))
    out.append(RadCase("smooth_tstep", 8, "smoothing, time-stepped", smooth=1, tstep=True, **SMOOTH8))
    return out


SIZES = (2, 3, 127, 128, 1023, 1024)


def size_case(L, smooth):
    """every kind of entry at every stride: flags missing at the first, a middle and the last layer, the adapt test"""
    e = alt(L, 0.5, -0.5)
    e[[0, L // 2, L - 1]] = (0.75, -2.0, 2.0)
    return RadCase("L%d_smooth%d" % (L, smooth), L, "layer count %d" % L, it=19, smooth=smooth, e=e, e_ghost=0.25)


def size_cases():
    return [size_case(L, s) for L in SIZES for s in (0, 1)]


EXPECT_SMOOTHED = {"smooth_straddle": [4, 5, 6], "smooth_all_low": [1, 2, 3, 4, 5, 6], "smooth_tstep": [4, 5, 6]}


def all_cases():
    return iteration_cases() + branch_cases() + smooth_cases() + size_cases()


# ---- the bounds of the direct comparison ----------------------------------------------------------------------------
def check_against(got, c, out=None, who=""):
    """`got` (run_impl's dict, or the same arrays read back from a batch; F_smooth may be missing there) against the
    restatement of case `c`.  Bit for bit: flags, T_store, F_net_diff, the prefactor (assignments and one IEEE division
    or product), clamped and no_atmo temperatures, and everything the call must not touch.  T_lay: rtol 1e-12 (pow
    within an ulp or two, delta_T added to a larger T).  F_smooth: 8 ulp (pow); F_smooth_sum: (L + 2) 2^-53 sum|F_smooth|
    against the long-double prefix sum of the F_smooth it was formed from (+ 16 2^-53 sum|F_smooth| where only the
    restatement's F_smooth, 8 ulp from the device's, is at hand).  Returns the largest deviations"""
    L = c.L
    out = restate(c)[0] if out is None else out
    msg = "%s %s" % (who, c.name)
    dev = {}
    np.testing.assert_array_equal(got["abort"], out["abort"], err_msg="abort, " + msg)
    np.testing.assert_array_equal(got["T_store"], out["T_store"], err_msg="T_store, " + msg)
    np.testing.assert_array_equal(got["pref"], out["pref"], err_msg="prefactor, " + msg)
    np.testing.assert_array_equal(got["F_net_diff"][:L], out["F_net_diff"], err_msg="F_net_diff, " + msg)
    if len(got["F_net_diff"]) > L:
        assert got["F_net_diff"][L] == POISON, "F_net_diff[L] written, " + msg
    T = np.asarray(got["T"], np.float64)
    dev["T_lay"] = float(np.abs(T.astype(LD) / out["T"] - 1).max())
    assert dev["T_lay"] <= 1e-12, "T_lay %.3e, %s" % (dev["T_lay"], msg)
    exact = sorted(set(out["clamp_lo"]) | set(out["clamp_hi"]) | (set(range(L)) if c.no_atmo == 1 else set()))
    np.testing.assert_array_equal(T[exact], out["T64"][exact], err_msg="clamped T_lay, " + msg)
    if c.smooth == 1:
        want = out["F_smooth"]
        total = float(np.abs(want).sum())
        bound = (L + 2) * 2.0 ** -53 * total
        if "F_smooth" in got:
            fs = np.asarray(got["F_smooth"], np.float64)
            ulp = np.spacing(np.abs(want.astype(np.float64)))
            dev["F_smooth_ulp"] = float((np.abs(fs.astype(LD) - want) / np.where(ulp > 0, ulp, 1)).max())
            assert (np.abs(fs.astype(LD) - want) <= 8 * ulp).all(), "F_smooth, " + msg
            prefix = np.cumsum(fs.astype(LD))
        else:
            prefix, bound = out["F_smooth_sum"], bound + 16 * 2.0 ** -53 * total
        err = np.abs(np.asarray(got["F_smooth_sum"], np.float64).astype(LD) - prefix)
        dev["F_smooth_sum"] = float(err.max() / total) if total > 0 else 0.0
        assert (err <= bound).all(), "F_smooth_sum %.3e of %.3e, %s" % (err.max(), bound, msg)
    else:
        if "F_smooth" in got:
            np.testing.assert_array_equal(got["F_smooth"], c.F_smooth, err_msg="F_smooth touched, " + msg)
        np.testing.assert_array_equal(got["F_smooth_sum"], c.F_smooth_sum, err_msg="F_smooth_sum touched, " + msg)
    return dev
