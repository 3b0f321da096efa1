"""The contract of helios_amd/cia.py restated in plain statements, one (nu, T, P) at a time: `long_double(...)` in np.longdouble
(the checker of the numpy backend), `plain_fp64(...)` the same statements in fp64 (the yardstick of what fp64 can hold).  The
constants are restated; tests/test_cia.py holds them to the module's.

The contract is one of fp64 numbers, so what it DECIDES -- the band that holds nu, the interval of a block, the blocks around T
and whether a value lies outside them -- is decided on the fp64 values in both restatements; what it COMPUTES is computed in the
number format asked for.  nu is an input: the grid's nu_i = nu_first + i * dnu are fp64 numbers.

`bands`: [(numin, numax, [(T, nu[], k[]), ...])], a band's blocks in ascending T, the bands apart from each other.
    block   0 for nu < nu_b[0] or nu > nu_b[n-1]; else i = the last index with nu_b[i] <= nu, at most n - 2,
            d = nu_b[i+1] - nu_b[i], u = (nu - nu_b[i]) / d, u' = (nu_b[i+1] - nu) / d, v = u' * k[i] + u * k[i+1]
    band    block 0 for T <= T_0, block m-1 for T >= T_{m-1}; else j = the last index with T_j <= T, D = T_{j+1} - T_j,
            w = (T - T_j) / D, w' = (T_{j+1} - T) / D, sigma = w' * v_j + w * v_{j+1}
    sigma   of the one band with numin <= nu <= numax, 0 outside every band
    kappa   sigma * (P / (K_B * T)) * N_A / M
"""
import numpy as np

# helios_amd/phys_const.py
K_B = 1.380649e-16
N_A = 6.02214076e23


def block_value(nu_b, k_b, nu, T):
    nu_b, k_b = np.asarray(nu_b, np.float64), np.asarray(k_b, np.float64)
    n = len(nu_b)
    if nu < nu_b[0] or nu > nu_b[n - 1]:
        return T(0.0)
    i = min(int(np.searchsorted(nu_b, nu, side="right")) - 1, n - 2)         # the last index with nu_b[i] <= nu, at most n - 2
    x, a0, a1, k0, k1 = T(nu), T(nu_b[i]), T(nu_b[i + 1]), T(k_b[i]), T(k_b[i + 1])
    d = a1 - a0
    u, up = (x - a0) / d, (a1 - x) / d
    return up * k0 + u * k1


def band_value(blocks, nu, temp, T):
    m = len(blocks)
    if temp <= blocks[0][0]:
        return block_value(blocks[0][1], blocks[0][2], nu, T)
    if temp >= blocks[m - 1][0]:
        return block_value(blocks[m - 1][1], blocks[m - 1][2], nu, T)
    j = 0
    while blocks[j + 1][0] <= temp:
        j += 1
    t, t0, t1 = T(temp), T(blocks[j][0]), T(blocks[j + 1][0])
    big_d = t1 - t0
    w, wp = (t - t0) / big_d, (t1 - t) / big_d
    return wp * block_value(blocks[j][1], blocks[j][2], nu, T) + w * block_value(blocks[j + 1][1], blocks[j + 1][2], nu, T)


def sigma(bands, nu, temp, T):
    for numin, numax, blocks in bands:
        if numin <= nu <= numax:
            return band_value(blocks, nu, temp, T)
    return T(0.0)


def kappa(bands, nu, temp, press, partner_mass, T):
    """one (nu, T, P); nu, temp, press are fp64 numbers"""
    nu, temp, press = np.float64(nu), np.float64(temp), np.float64(press)
    return sigma(bands, nu, temp, T) * (T(press) / (T(K_B) * T(temp))) * T(N_A) / T(partner_mass)


def _over(bands, nus, temp, press, partner_mass, T):
    return np.array([kappa(bands, nu, temp, press, partner_mass, T) for nu in np.asarray(nus, np.float64).reshape(-1)], T)


def long_double(bands, nus, temp, press, partner_mass):
    return _over(bands, nus, temp, press, partner_mass, np.longdouble)


def plain_fp64(bands, nus, temp, press, partner_mass):
    return _over(bands, nus, temp, press, partner_mass, np.float64)
