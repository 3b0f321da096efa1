"""The transit-depth contract (README, "Transit depth spectrum") restated one chord at a time.

`transit(...)` evaluates it in `np.longdouble`, `plain_fp64(...)` runs the very same statements in fp64: the difference of
the two at an entry is the rounding error a straightforward fp64 evaluation has there, which is what the HIP kernel is
held against (tests/test_gpu_transit.py).  Nothing here is shared with helios_amd: the module imports numpy only.

Arrays: dtau[s, x, y] gas + Rayleigh optical depth of shell s, cloud[s, x] the clouds' optical depth of the same shell,
zb[0..S] ascending shell boundaries (altitudes, z = 0 at radius R0), w[y] Gauss weights (they sum to 2).
"""
import numpy as np


def shell_boundaries(z_lay, delta_z_lay, iso, dtype=np.float64):
    """zb of a column: the interfaces built upward from the lowest one; with non-isothermal layers interleaved with the
    layer centres (shell 2i = lower half of layer i, shell 2i + 1 = upper half)"""
    z_lay = np.asarray(z_lay, dtype)
    dz = np.asarray(delta_z_lay, dtype)
    L = len(dz)
    z_int = np.empty(L + 1, dtype)
    z_int[0] = z_lay[0] - dz[0] / dtype(2)
    for i in range(L):
        z_int[i + 1] = z_int[i] + dz[i]
    if iso:
        return z_int
    zb = np.empty(2 * L + 1, dtype)
    zb[0::2] = z_int
    zb[1::2] = z_lay[:L]
    return zb


def shells_of_layers(lower, upper=None):
    """shell-major array from per-layer arrays [layer, ...]: the layers themselves, or lower/upper halves interleaved"""
    lower = np.asarray(lower)
    if upper is None:
        return lower
    out = np.empty((2 * lower.shape[0],) + lower.shape[1:], lower.dtype)
    out[0::2] = lower
    out[1::2] = np.asarray(upper)
    return out


def chord_tau(alpha, zb, R0, j):
    """tau[x, y] of the chord through the centre of shell j: sum over s >= j of alpha_s * l_{s,j}, from s = j upward.
    alpha[s, x, y], zb and R0 share one dtype, which is the dtype of every operation."""
    t = zb.dtype.type
    zj = (zb[j] + zb[j + 1]) / t(2)
    bj = R0 + zj
    z = zb[j + 1:]                                       # upper boundaries of the shells s = j ... S - 1
    q_up = np.sqrt((z - zj) * ((R0 + z) + bj))          # product form; z - z_j from altitudes, before any radius
    q_low = np.concatenate(([t(0)], q_up[:-1]))          # the term of the lower boundary is 0 for s = j
    ell = t(2) * (q_up - q_low)
    terms = alpha[j:] * ell[:, None, None]
    return np.add.accumulate(terms, axis=0)[-1]          # strictly one after the other, from s = j upward


def transit(dtau, cloud, zb, w, R0, R_star=None, dtype=np.longdouble, chords=None):
    """the whole contract in `dtype`.  Returns a dict: tau[j, x, y], T_band[j, x], A[x], T_floor[x], R_eff[x] and, given
    R_star, depth[x].  `chords`: evaluate these impact parameters only (tau and T_band then hold those rows; no area)."""
    t = np.dtype(dtype).type
    dtau = np.asarray(dtau, np.float64).astype(dtype)
    cloud = np.asarray(cloud, np.float64).astype(dtype)
    zb = np.asarray(zb, np.float64).astype(dtype)
    w = np.asarray(w, np.float64).astype(dtype)
    R0 = t(np.float64(R0))
    S = len(zb) - 1
    assert dtau.shape[0] == S and cloud.shape == dtau.shape[:2] and w.shape == dtau.shape[2:]
    alpha = (dtau + cloud[:, :, None]) / (zb[1:] - zb[:-1])[:, None, None]
    js = list(range(S)) if chords is None else list(chords)
    tau = np.empty((len(js),) + dtau.shape[1:], dtype)
    T_band = np.empty((len(js), dtau.shape[1]), dtype)
    for n, j in enumerate(js):
        tau[n] = chord_tau(alpha, zb, R0, j)
        acc = np.zeros(dtau.shape[1], dtype)
        for y in range(len(w)):
            acc = acc + (t(0.5) * w[y]) * np.exp(-tau[n][:, y])
        T_band[n] = acc
    out = {"tau": tau, "T_band": T_band}
    if chords is not None:
        return out
    A = np.zeros(dtau.shape[1], dtype)
    for j in range(S):
        A = A + ((t(1) - T_band[j]) * (zb[j + 1] - zb[j])) * ((t(2) * R0 + zb[j + 1]) + zb[j])
    out["A"] = A
    out["T_floor"] = T_band[0].copy()
    out["R_eff"] = np.sqrt((R0 + zb[0]) * (R0 + zb[0]) + A)
    if R_star is not None:
        r = out["R_eff"] / t(np.float64(R_star))
        out["depth"] = r * r
    return out


def plain_fp64(dtau, cloud, zb, w, R0, R_star=None, chords=None):
    """the same statements in fp64"""
    return transit(dtau, cloud, zb, w, R0, R_star, dtype=np.float64, chords=chords)


def bound(ref, plain, floor=1e-13):
    """the project's rule for holding an fp64 kernel to the restatement: per entry max(floor, 8 eps), eps being the deviation
    of the plain fp64 evaluation from the extended one at that entry (absolute; divide by |ref| for a relative check)"""
    return np.maximum(np.longdouble(floor), 8 * np.abs(np.asarray(plain, np.longdouble) - ref))
