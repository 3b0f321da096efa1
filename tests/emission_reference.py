"""The angular-emission contract (README, "Angular emission spectrum") restated one spectral point at a time.

`emission(...)` evaluates it in `np.longdouble`, `plain_fp64(...)` runs the very same statements in fp64: the difference of
the two at an entry is the rounding error a straightforward fp64 evaluation has there, which is what the HIP kernel is
held against (tests/test_gpu_emission_angles.py).  Nothing here is shared with helios_amd: the module imports numpy only.

Shell-major arrays, S shells and S + 1 boundaries (boundary 0 = BOA interface, boundary S = TOA interface):
dtau[s, x, y] gas + Rayleigh optical depth of shell s, cloud[s, x] the clouds', w0[s, x, y] the shell's single-scattering
albedo, B_bot[s, x] / B_top[s, x] the Planck value at the shell's lower / upper end, F_up / F_down / F_dir[k, x, y] the
run's spectral fluxes at boundary k, w[y] Gauss weights of the bin (they sum to 2), mu[m] the emission angles' cosines.
"""
import numpy as np

T_SWITCH = 0.05          # below it the weights of the source come from their series
N_TERMS = 10
PI = np.float64(np.pi)   # the contract's pi is the fp64 one, in either evaluation: the inputs are fp64 numbers
FACTORIALS = [2, 6, 24, 120, 720, 5040, 40320, 362880, 3628800, 39916800]      # (n + 1)!, n = 1 ... 10


def angles(N):
    """Gauss-Legendre nodes and weights on [0, 1] in ascending mu, fp64, and 1 / mu rounded to fp64"""
    x, w = np.polynomial.legendre.leggauss(N)
    mu = (x + 1.0) / 2.0
    return mu, w / 2.0, 1.0 / mu


def series_constants(dtype):
    """c_n = (-1)^(n+1) / (n+1)!  and  d_n = (-1)^(n+1) n / (n+1)!,  n = 1 ... 10, each one division in `dtype`"""
    t = np.dtype(dtype).type
    c = [t(1 if n % 2 else -1) / t(FACTORIALS[n - 1]) for n in range(1, N_TERMS + 1)]
    d = [t(n if n % 2 else -n) / t(FACTORIALS[n - 1]) for n in range(1, N_TERMS + 1)]
    return c, d


def weights(tt, dtype=np.longdouble):
    """(e, a, b) of the formal solution with a source linear in tau, for the slant optical depths tt (any shape)"""
    t = np.dtype(dtype).type
    tt = np.asarray(tt, dtype)
    big = tt >= t(T_SWITCH)
    # t >= t_s
    with np.errstate(divide="ignore", invalid="ignore"):
        u = -np.expm1(-tt)
        e1 = t(1) - u
        q = u / tt
        a1 = t(1) - q
        b1 = q - e1
    # t < t_s: every term formed and added in ascending n
    c, d = series_constants(dtype)
    p = tt.copy()
    a2 = p * c[0]
    b2 = p * d[0]
    for n in range(1, N_TERMS):
        p = p * tt
        a2 = a2 + p * c[n]
        b2 = b2 + p * d[n]
    e2 = np.exp(-tt)
    return np.where(big, e1, e2), np.where(big, a1, a2), np.where(big, b1, b2)


def shells_of_layers(lower, upper=None):
    """shell-major array from per-layer arrays [layer, ...]: the layers themselves, or lower/upper halves interleaved"""
    lower = np.asarray(lower)
    if upper is None:
        return lower
    out = np.empty((2 * lower.shape[0],) + lower.shape[1:], lower.dtype)
    out[0::2] = lower
    out[1::2] = np.asarray(upper)
    return out


def planck_ends(planck_lay, planck_int=None):
    """(B_bot, B_top)[s, x] from planck_lay[i, x] (layer centres) and, with non-isothermal layers, planck_int[i, x]
    (interfaces): an isothermal layer has its own value at both ends; otherwise the boundaries alternate between
    interface i (k = 2i) and the centre of layer i (k = 2i + 1)"""
    planck_lay = np.asarray(planck_lay)
    if planck_int is None:
        return planck_lay, planck_lay
    L = planck_lay.shape[0]
    Bk = np.empty((2 * L + 1,) + planck_lay.shape[1:], planck_lay.dtype)
    Bk[0::2] = np.asarray(planck_int)
    Bk[1::2] = planck_lay
    return Bk[:-1], Bk[1:]


def boundaries_of(interfaces, centres=None):
    """flux array [k, x, y] from the interface array [i, x, y] and, with non-isothermal layers, the centres' array"""
    interfaces = np.asarray(interfaces)
    if centres is None:
        return interfaces
    L = interfaces.shape[0] - 1
    out = np.empty((2 * L + 1,) + interfaces.shape[1:], interfaces.dtype)
    out[0::2] = interfaces
    out[1::2] = np.asarray(centres)[:L]
    return out


def emission(dtau, cloud, w0, B_bot, B_top, F_up, F_down, F_dir, w, mu_inv, beta, mu=None, mu_weight=None,
             dtype=np.longdouble, I_start=None):
    """the whole contract in `dtype`.  Returns a dict: I_wg[m, x, y], I_band[m, x] and, given mu and mu_weight, the disc
    sum F[x].  F_dir None: the beam is off and the term is absent.  `I_start`[x, y]: the intensity at boundary 0 instead of
    F_up[0] / pi (the closed-form tests start from 0)."""
    t = np.dtype(dtype).type
    cast = lambda v: np.asarray(v).astype(dtype)      # fp64 inputs as they are; a test may hand over long doubles
    dtau, cloud, w0, B_bot, B_top, F_up, F_down, w, mu_inv = [cast(v) for v in (dtau, cloud, w0, B_bot, B_top, F_up, F_down,
                                                                                w, mu_inv)]
    S, X, Y = dtau.shape
    N = len(mu_inv)
    assert cloud.shape == (S, X) and w0.shape == dtau.shape and B_bot.shape == (S, X) and B_top.shape == (S, X)
    assert F_up.shape == (S + 1, X, Y) and F_down.shape == F_up.shape and w.shape == (Y,)
    pi = t(PI)
    J = (F_up + F_down) / (t(2) * pi)
    if F_dir is not None:
        J = J + t(beta) * np.abs(cast(F_dir))
    I = np.empty((N, X, Y), dtype)
    start = F_up[0] / pi if I_start is None else cast(I_start)
    for m in range(N):
        I[m] = start
    for s in range(S):
        dt = dtau[s] + cloud[s][:, None]
        om = w0[s]
        S_bot = (t(1) - om) * B_bot[s][:, None] + om * J[s]
        S_top = (t(1) - om) * B_top[s][:, None] + om * J[s + 1]
        for m in range(N):
            e, a, b = weights(dt * mu_inv[m], dtype)
            I[m] = (I[m] * e + S_top * a) + S_bot * b
    I_band = np.zeros((N, X), dtype)
    for y in range(Y):
        I_band = I_band + (t(0.5) * w[y]) * I[:, :, y]
    out = {"I_wg": I, "I_band": I_band}
    if mu is not None:
        out["F"] = disc_flux(I_band, mu, mu_weight, dtype)
    return out


def disc_flux(I_band, mu, mu_weight, dtype=np.longdouble):
    """F[x] = 2 pi sum_m w_m mu_m I[m, x], in ascending m"""
    t = np.dtype(dtype).type
    I_band = np.asarray(I_band).astype(dtype)
    acc = np.zeros(I_band.shape[1], dtype)
    for m in range(I_band.shape[0]):
        acc = acc + (t(np.float64(mu_weight[m])) * t(np.float64(mu[m]))) * I_band[m]
    return (t(2) * t(PI)) * acc


def plain_fp64(*args, **kw):
    """the same statements in fp64"""
    kw["dtype"] = np.float64
    return emission(*args, **kw)


def bound(ref, plain, floor=1e-13):
    """the project's rule for holding an fp64 kernel to the restatement, relative: per entry max(floor |ref|, 8 eps), eps
    being the deviation of the plain fp64 evaluation from the extended one at that entry"""
    ref = np.asarray(ref, np.longdouble)
    return np.maximum(np.longdouble(floor) * np.abs(ref), 8 * np.abs(np.asarray(plain, np.longdouble) - ref))
