"""TEST INFRASTRUCTURE: what the coefficient refresh (k_rt_coef in csrc/rt_coef_kernel.inc, slab_coeffs in
csrc/two_stream.h; the stage kernels calc_trans_iso / calc_trans_noniso) computes for ONE half-layer, restated in numpy,
vectorised over slots and written once with the dtype as a parameter: np.longdouble is the reference, np.float64 the plain
twin in the kernel's own operation order (its deviation from the long double is the rounding noise of the formulas
themselves, the scale of tests/test_gpu_coef_edges.py's tolerance rule).  No GPU here.

Inputs are the fp64 values the kernel consumes at the two nodes of the half-layer -- `lay` the layer centre, `int` the
interface (lower half: interface i and centre i, upper half: centre i and interface i + 1; isothermal layers take the
centre values alone) -- and the flags and limits of hx_rt_flags.  Every discrete comparison comes back with its MARGIN in
tests/rad_cases.py's sense, |a - b| / max(|a|, |b|), inf where both sides are exact.

NaN.  fmin / fmax return the other operand where one is NaN; min(w0, w_0_limit) therefore turns 0 / 0 into w_0_limit,
and min(0, NaN) discards a NaN beam term.  `_fmin` and `_fmax` spell that out.  A comparison with NaN is false:
|G| < 1e8 fails for a NaN, which is then "limited" to NaN (1e8 NaN / NaN) and counted, as G_limiter's warning is.
"""
import numpy as np

LD = np.longdouble
PLANES = ("alpha", "beta", "up", "vp", "dd", "du")
G_LIMIT = 1e8
E_FIT = (1.225, 0.1582, 0.1777, 0.07465, 0.2351, 0.05582)
INPUTS = ("kap_lay", "kap_int", "ray_lay", "ray_int", "cab_lay", "cab_int", "csc_lay", "csc_int", "g0_lay", "g0_int",
          "mu_lay", "mu_int", "dcol", "Fbot", "Ftop")


class Flags(dict):
    """the flags and limits of hx_rt_flags the refresh reads, with mu_star of the column"""
    __getattr__ = dict.__getitem__

    def __init__(self, **kw):
        d = dict(iso=0, scat=1, clouds=0, scat_corr=0, dir_beam=0, need_G=None, g_0=0.0, epsi=0.5, epsi2=0.5,
                 mu_star=-0.5, i2s_transition=0.1, w_0_limit=1.0 - 1e-10, w_0_scat_limit=1e-3, delta_tau_limit=1e-4)
        d.update(kw)
        dict.__init__(self, d)


def flags_of_case(c, **kw):
    return Flags(**dict({k: c[k] for k in ("iso", "scat", "clouds", "scat_corr", "dir_beam", "g_0", "epsi", "epsi2", "mu_star",
                                           "i2s_transition", "w_0_limit", "w_0_scat_limit", "delta_tau_limit")}, **kw))


def _fmin(a, b):
    """C's fmin: the other operand where one is NaN"""
    a, b = np.broadcast_arrays(a, b)
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(b < a, b, a)))


def _fmax(a, b):
    a, b = np.broadcast_arrays(a, b)
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(b > a, b, a)))


def margin(a, b):
    """|a - b| / max(|a|, |b|) in long double; inf where both are 0 or either is NaN (decided by exact arithmetic alone)"""
    a, b = np.broadcast_arrays(np.asarray(a, LD), np.asarray(b, LD))
    m = np.maximum(np.abs(a), np.abs(b))
    with np.errstate(all="ignore"):
        out = np.where(m == 0, np.inf, np.abs(a - b) / np.where(m == 0, 1, m))
    return np.where(np.isnan(a) | np.isnan(b), np.inf, out).astype(np.float64)


def _sum_margin(total, *terms):
    """a sum against 0: |sum| over the sum of |terms| (rad_cases' "dF != 0"); inf where every term is 0 or one is NaN"""
    s = sum(np.abs(np.asarray(t, LD)) for t in terms)
    with np.errstate(all="ignore"):
        out = np.where(s == 0, np.inf, np.abs(np.asarray(total, LD)) / np.where(s == 0, 1, s))
    return np.where(np.isnan(s) | np.isnan(total), np.inf, out).astype(np.float64)


def restate(inp, fl, T=LD):
    """dict of per-slot arrays of dtype T: w0, dtau, E, trans, M, N, P, Gp, Gm, boaK and boaK_abs, the planes of the
    scattering form (alpha, beta, up, vp, dd, du) and of the matrix method's pure-absorption form (*_abs); the integers
    g_limited (0, 1 or 2), vote (w0 > w_0_scat_limit), thin, clamped, i2s_on, E_floored, dn_cut, up_cut, dn_pos, up_pos; and `margins`,
    {comparison: float64 array}.  `inp` maps INPUTS to float64 arrays (ray, cab, csc, g0 may be left out: zeros, and the
    flags' g_0); Fbot / Ftop are the beam at the half-layer's bottom and top node."""
    n = len(np.atleast_1d(inp["kap_lay"]))

    def c(v):
        return np.broadcast_to(np.asarray(v, np.float64), (n,)).astype(T)

    def get(name):
        return c(inp.get(name, 0.0))
    one, two, half, zero = T(1), T(2), T(0.5), T(0)
    iso = int(fl.iso) == 1

    def avg(nm):  # half_bands' and the kernel's own average: (interface + centre) / 2, a commutative sum
        return get(nm + "_lay") if iso else (get(nm + "_int") + get(nm + "_lay")) / two
    epsi, epsi2, mu_star = T(fl.epsi), T(fl.epsi2), T(fl.mu_star)
    out, m = {}, {}
    with np.errstate(all="ignore"):
        kap, mu, dcol = avg("kap"), avg("mu"), get("dcol")
        ray = avg("ray") if int(fl.scat) == 1 else c(0.0)
        csc = avg("csc") if int(fl.scat) == 1 and int(fl.clouds) == 1 else c(0.0)
        cab = avg("cab") if int(fl.clouds) == 1 else c(0.0)
        g0 = avg("g0") if int(fl.clouds) == 1 else c(fl.g_0)
        sc, ab = ray + csc, kap * mu + cab
        w0raw = sc / (sc + ab)
        w0 = _fmin(w0raw, T(fl.w_0_limit)).astype(T)
        m["w0 clamp"] = margin(w0raw, fl.w_0_limit)
        out["clamped"] = ~(w0raw < T(fl.w_0_limit))          # (NaN: clamped)
        dtau = dcol * (kap + ray / mu) + dcol * (cab + csc) / mu
        # E (Heng, Malik & Kitzmann 2018 fit)
        E = np.full(n, one, T)
        out["i2s_on"] = np.zeros(n, bool)
        out["E_floored"] = np.zeros(n, bool)
        if int(fl.scat_corr) == 1:
            e = [T(v) for v in E_FIT]
            fit = e[0] - e[1] * g0 - e[2] * w0 - e[3] * (g0 * g0) + e[4] * w0 * g0 - e[5] * (w0 * w0)
            on = (w0 > T(fl.i2s_transition)) & (g0 >= zero)
            E = np.where(on, _fmax(one, fit), one).astype(T)
            m["w0 > i2s_transition"] = margin(w0, fl.i2s_transition)
            m["g0 >= 0"] = margin(g0, 0.0) if int(fl.clouds) == 1 else np.full(n, np.inf)
            m["E floor"] = np.where(on, margin(fit, 1.0), np.inf)
            out["i2s_on"], out["E_floored"] = on, on & ~(fit > one)
        omg = one - w0 * g0
        trans = np.exp(-one / epsi * np.sqrt(E * omg * (E - w0)) * dtau)
        r = np.sqrt((E - w0) / (E * omg))
        zm, zp = half * (one - r), half * (one + r)
        t2 = trans * trans
        M = (zm * zm) * t2 - (zp * zp)
        N = zp * zm * (one - t2)
        P = ((zm * zm) - (zp * zp)) * trans
        # G+-
        need_G = int(fl.dir_beam) == 1 if fl.need_G is None else bool(fl.need_G)
        Gp, Gm = np.zeros(n, T), np.zeros(n, T)
        out["g_limited"] = np.zeros(n, np.int64)
        m["|G| < 1e8"] = np.full(n, np.inf)
        if need_G:
            num = w0 * (E * omg + g0 * epsi / epsi2)
            den = E * (one / (epsi * epsi)) * (E - w0) * omg - one / (mu_star * mu_star)
            third = epsi * w0 * g0 * mu_star / (epsi2 * E * omg)
            inv = one / (mu_star * E * omg)
            raw = [half * (num / den * (one / epsi + inv) + third), half * (num / den * (one / epsi - inv) - third)]
            lim = [~(np.abs(G) < T(G_LIMIT)) for G in raw]
            Gp, Gm = [np.where(l, T(G_LIMIT) * G / np.abs(G), G).astype(T) for G, l in zip(raw, lim)]
            out["g_limited"] = lim[0].astype(np.int64) + lim[1].astype(np.int64)
            m["|G| < 1e8"] = np.minimum(margin(np.abs(raw[0]), G_LIMIT), margin(np.abs(raw[1]), G_LIMIT))
        thin = (dtau < T(fl.delta_tau_limit)) | iso
        m["dtau < delta_tau_limit"] = np.full(n, np.inf) if iso else margin(dtau, fl.delta_tau_limit)
        m["w0 > w_0_scat_limit"] = margin(w0, fl.w_0_scat_limit)
        out["vote"], out["thin"] = w0 > T(fl.w_0_scat_limit), thin
        # the planes, scattering form
        invM = one / M
        pi2e = two * T(np.pi) * epsi
        K = pi2e * (one - w0) / (E - w0)
        qq = epsi / (E * omg) * (P - M + N) / dtau
        u = np.where(thin, (N + M - P) / two, (M + N) + qq)
        v = np.where(thin, (N + M - P) / two, -P - qq)
        out.update(alpha=P * invM, beta=-N * invM, up=K * u * invM, vp=K * v * invM, boaK=(one - w0) / (E - w0))
        dd, du = np.zeros(n, T), np.zeros(n, T)
        out["dn_cut"], out["up_cut"] = np.zeros(n, bool), np.zeros(n, bool)
        out["dn_pos"], out["up_pos"] = np.zeros(n, bool), np.zeros(n, bool)
        m["dn < 0"], m["upw < 0"] = np.full(n, np.inf), np.full(n, np.inf)
        if int(fl.dir_beam) == 1:
            nmu, Fb, Ft = -mu_star, get("Fbot"), get("Ftop")
            a1, a2 = Fb / nmu * (Gm * M + Gp * N), Ft / nmu * Gm * P
            b1, b2 = Ft / nmu * (Gm * N + Gp * M), Fb / nmu * P * Gp
            dn, upw = a1 - a2, b1 - b2
            dd, du = _fmin(zero, dn).astype(T) * invM, _fmin(zero, upw).astype(T) * invM
            m["dn < 0"] = _sum_margin(dn, Fb / nmu * Gm * M, Fb / nmu * Gp * N, a2)
            m["upw < 0"] = _sum_margin(upw, Ft / nmu * Gm * N, Ft / nmu * Gp * M, b2)
            out["dn_cut"], out["up_cut"] = ~(dn < zero), ~(upw < zero)     # (NaN and 0: the term is 0)
            out["dn_pos"], out["up_pos"] = dn > zero, upw > zero
        out.update(dd=dd, du=du)
        # the matrix method's pure-absorption form: alpha = T, beta = 0, F_out = T F_in + 2 pi eps P'
        gq = epsi * (trans - one) / dtau
        ua = np.where(thin, (one - trans) / two, one + gq)
        va = np.where(thin, (one - trans) / two, -trans - gq)
        out.update(alpha_abs=trans, beta_abs=np.zeros(n, T), up_abs=pi2e * ua * one, vp_abs=pi2e * va * one,
                   dd_abs=np.zeros(n, T), du_abs=np.zeros(n, T), boaK_abs=np.ones(n, T))
    out.update(w0=w0, dtau=dtau, dtau_gas=dcol * (kap + ray / mu), E=E, trans=trans, M=M, N=N, P=P, Gp=Gp, Gm=Gm,
               g0=g0, margins=m)
    return out


def planes(res, scatters):
    """the six plane values per slot where `scatters` (bool per slot: the vote of the slot's spectral point) picks the form"""
    return {p: np.where(scatters, res[p], res[p + "_abs"]) for p in PLANES}


def plane_scale(plane, epsi=0.5, beam_max=1.0):
    """the scale of the tolerance rule's absolute deviations: 1 for alpha and beta, 2 pi epsi for the sources, times the
    largest |beam| of the spectral point for the beam planes"""
    if plane in ("alpha", "beta"):
        return 1.0
    s = 2.0 * np.pi * epsi
    return s * beam_max if plane in ("dd", "du") else s
