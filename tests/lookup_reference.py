"""The bilinear (T, log10 P) table look-up of the device-resident loop -- locate_tp / blend_tp of helios_amd/csrc/two_stream.h,
interface_T of rt_kernels.h and the correlated-k species chain of rt_species.h / rt_mix_species_kernel.inc -- restated in plain
numpy, elementwise over the levels it is asked for: `long_double(...)` in np.longdouble (the checker of every copy of the
look-up), `plain_fp64(...)` the same statements in fp64 (the yardstick of what fp64 can hold).

The contract is one of fp64 numbers, so what it DECIDES -- the fractional indices t and p, their clamps ([0.001, n - 1.001] with
the margin of the premixed tables, [0, n - 1] without: the per-species tables) and floor / ceil of both -- is decided on fp64
values computed as the kernels compute them, in both restatements.  What it COMPUTES -- the weights (pup - p), (p - pdown),
(tup - t), (t - tdown) and the four-term, two-term or one-term blend, every statement left to right -- is computed in the
number format asked for.

    dt = (ktemp[n-1] - ktemp[0]) / (n - 1.0)                     t = (T - ktemp[0]) / dt
    dp = (log10 kpress[m-1] - log10 kpress[0]) / (m - 1.0)       p = (log10 P - log10 kpress[0]) / dp

The temperature axis uses IEEE operations only: t, tdown, tup are the device's bit for bit.  The pressure axis goes through
log10, taken from libm here (math.log10, one value at a time: numpy's vector log10 is another implementation); `log10p`
replaces it where a test moves it by a few ulp.
"""
import math

import numpy as np

LD = np.longdouble
AMU = 1.6605390666e-24     # helios_amd/phys_const.py; tests/test_lookup_cases.py holds it to the module's


def log10_libm(v):
    return np.array([math.log10(x) for x in np.asarray(v, np.float64).reshape(-1)])


def locate(temp, press, ktemp, kpress, margin=True, log10p=None, log_t=False):
    """locate_tp at arrays of levels, in fp64: dict of t, p (fp64) and tdown, tup, pdown, pup (int64); `log_t`: the temperature
    axis in log10 T too (the c_p and entropy tables)"""
    temp = np.asarray(temp, np.float64).reshape(-1)
    ktemp, kpress = np.asarray(ktemp, np.float64), np.asarray(kpress, np.float64)
    nt, npr = len(ktemp), len(kpress)
    if log_t:
        lt = log10_libm(ktemp)
        dt = (lt[nt - 1] - lt[0]) / (nt - 1.0)
        t = (log10_libm(temp) - lt[0]) / dt
    else:
        dt = (ktemp[nt - 1] - ktemp[0]) / (nt - 1.0)
        t = (temp - ktemp[0]) / dt
    lp = log10_libm(press) if log10p is None else np.asarray(log10p, np.float64).reshape(-1)
    lk = log10_libm(kpress)
    dp = (lk[npr - 1] - lk[0]) / (npr - 1.0)
    p = (lp - lk[0]) / dp
    if margin:
        t = np.minimum(nt - 1.001, np.maximum(0.001, t))
        p = np.minimum(npr - 1.001, np.maximum(0.001, p))
    else:
        t = np.minimum(nt - 1.0, np.maximum(0.0, t))
        p = np.minimum(npr - 1.0, np.maximum(0.0, p))
    return dict(t=t, p=p, tdown=np.floor(t).astype(np.int64), tup=np.ceil(t).astype(np.int64),
                pdown=np.floor(p).astype(np.int64), pup=np.ceil(p).astype(np.int64))


def branch(k):
    """blend_tp's case per level: 3 four terms, 1 two terms along P (tdown == tup), 2 two terms along T (pdown == pup), 0 one"""
    return (k["pdown"] != k["pup"]).astype(np.int64) + 2 * (k["tdown"] != k["tup"])


def blend(dd, ud, du, uu, k, fmt, species=False):
    """blend_tp: corners [level, ...] (dd = [tdown][pdown], ud = [tdown][pup], du = [tup][pdown], uu = [tup][pup]) in `fmt`"""
    dd, ud, du, uu = (np.asarray(v).astype(fmt) for v in (dd, ud, du, uu))
    shape = (-1,) + (1,) * (dd.ndim - 1)
    t, p = k["t"].astype(fmt).reshape(shape), k["p"].astype(fmt).reshape(shape)
    a = k["pup"].astype(fmt).reshape(shape) - p
    b = p - k["pdown"].astype(fmt).reshape(shape)
    c = k["tup"].astype(fmt).reshape(shape) - t
    d = t - k["tdown"].astype(fmt).reshape(shape)
    four = dd * a * c + ud * b * c + du * a * d + uu * b * d
    along_p = dd * a + ud * b
    along_t = (du * d + dd * c) if species else (dd * c + du * d)
    br = branch(k).reshape(shape)
    return np.where(br == 3, four, np.where(br == 1, along_p, np.where(br == 2, along_t, dd)))


def corners(table, k):
    """the four corners of every level from a table shaped [t][p][...]"""
    return (table[k["tdown"], k["pdown"]], table[k["tdown"], k["pup"]], table[k["tup"], k["pdown"]], table[k["tup"], k["pup"]])


def look_up(fmt, table, temp, press, ktemp, kpress, margin=True, species=False, log10p=None, log_t=False):
    """a table shaped [t][p][...] at arrays of levels: [level][...] in `fmt`"""
    k = locate(temp, press, ktemp, kpress, margin, log10p, log_t)
    return blend(*corners(np.asarray(table, np.float64), k), k, fmt, species)


def tables(fmt, c, temp, press, log10p=None):
    """the premixed tables of case `c` (reference layouts: k-table [t][p][x][y], Rayleigh [t][p][x], mean mass [t][p]) at
    arrays of levels: dict of opac [level][x * ny + y], scat [level][x], mmm [level]"""
    nt, npr, X, Y = c.ntemp, c.npress, c.nbin, c.ny
    k = locate(temp, press, c.ktemp, c.kpress, True, log10p)
    out = {}
    for name, tab, tail in (("opac", c.opac_k, (X * Y,)), ("scat", c.opac_scat_cross, (X,)), ("mmm", c.opac_meanmass, ())):
        out[name] = blend(*corners(np.asarray(tab, np.float64).reshape((nt, npr) + tail), k), k, fmt, False)
    return out


def long_double(c, temp, press, log10p=None):
    return tables(LD, c, temp, press, log10p)


def plain_fp64(c, temp, press, log10p=None):
    return tables(np.float64, c, temp, press, log10p)


def interface_T(T_lay, nlayer):
    """interface_T (rt_kernels.h) of the layer temperatures T_lay[0 .. nlayer - 1], in fp64: its three cases"""
    T = np.asarray(T_lay, np.float64)
    L = int(nlayer)
    out = np.empty(L + 1)
    out[0] = T[0] - 0.5 * (T[1] - T[0])
    out[L] = T[L - 1] + 0.5 * (T[L - 1] - T[L - 2])
    out[1:L] = T[0:L - 1] + 0.5 * (T[1:L] - T[0:L - 1])
    return out


def species_mix(fmt, c, temp, press, vmr, log10p=None):
    """the species chain of case `c` (c.species as tests/cases.py lays it out, every absorber correlated-k) at arrays of levels
    with the mixing ratios vmr [species][level]: dict of
        mmm  [level]             num / tot * AMU over the species counted in mu, as k_rt_species_prep sums them
        fac  [species][level]    vmr * (weight * AMU) / mmm
        raw  [absorber][level][x * ny + y]   blend_tp(..., species = true) without the margin
        opac [level][x * ny + y]             0.0 + fac_0 * raw_0 + fac_1 * raw_1 ..., absorbers in the order of the list
        scat [level][x]                      0.0 + vmr * sigma over the scatterers
    and the indices (key "k")"""
    nt, npr, X, Y = c.ntemp, c.npress, c.nbin, c.ny
    vmr = np.asarray(vmr, np.float64)
    k = locate(temp, press, c.ktemp, c.kpress, False, log10p)
    n = len(k["t"])
    num, tot = np.zeros(n, fmt), np.zeros(n, fmt)
    for s, sp in enumerate(c.species):
        if not sp["is_cia"]:
            num = num + vmr[s].astype(fmt) * fmt(sp["weight"])
            tot = tot + vmr[s].astype(fmt)
    mmm = num / tot * fmt(AMU)
    fac = [vmr[s].astype(fmt) * (fmt(sp["weight"]) * fmt(AMU)) / mmm for s, sp in enumerate(c.species)]
    opac, scat, raw = np.zeros((n, X * Y), fmt), np.zeros((n, X), fmt), []
    for s, sp in enumerate(c.species):
        if sp["absorbing"]:
            tab = np.asarray(sp["pretab"], np.float64).reshape(nt, npr, X * Y)
            raw.append(blend(*corners(tab, k), k, fmt, True))
            opac = opac + fac[s][:, None] * raw[-1]
        if sp["scattering"]:
            scat = scat + vmr[s].astype(fmt)[:, None] * np.asarray(sp["scat"]).astype(fmt)[None, :]
    return dict(mmm=mmm, fac=np.array(fac), raw=raw, opac=opac, scat=scat, k=k)
