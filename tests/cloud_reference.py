"""One cloud deck's three spectra restated plainly in np.longdouble -- the weighted sums over the radii and the re-binning
contract of helios_amd.tools.convert_spectrum with int_lambda given -- next to a plain sequential fp64 evaluation of the host's
own formulas, synthetic LX-MIE directories, and the bin grids of the edge tests (tests/test_cloud_decks.py on the CPU,
tests/test_gpu_cloud_decks.py on the device).  Of the project it takes the radius grid, nothing else.

The tolerance rule is that of tests/ktable_reference.py: a value is held to the restatement within max(1e-13, 8 * eps), eps the
relative deviation of the comparison evaluation (plain fp64 for the host path, the host path for the device) from the
restatement AT THAT ENTRY; an exact zero of the restatement must be an exact zero."""
import os

import numpy as np

from helios_amd.clouds import DELTA_R, R_VALUES

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
FLOOR = 1e-13
NW_EDGE = 37              # the non-uniform Mie grid of the edge cases
NW_BEYOND_CHUNK = 2500    # more Mie wavelengths inside one workgroup's bins than k_cloud_deck_spectra stages per pass (1024 + 1)


def require_extended_precision():
    assert EPS_LD <= 1.1e-19, "np.longdouble has eps %.3e here: no 64-bit mantissa to hold the kernels to" % EPS_LD


# ---- the restatement ------------------------------------------------------------------------------------------------------------
def reference_weighted(table, weight):
    """sum over the radii of cross-section times weight at every Mie wavelength, in long double: (absorption, scattering)"""
    w = np.asarray(weight, np.float64).astype(LD)[:, None]
    return (table["absorb"].astype(LD) * w).sum(axis=0), (table["scat"].astype(LD) * w).sum(axis=0)


def _ld_log(v):
    with np.errstate(divide="ignore"):
        return np.log(v)


def reference_rebin(lam, flux, inter, log):
    """convert_spectrum(lam, flux, ., int_lambda=inter, type=log|linear) in long double.  Which case a bin falls under is decided
    on the doubles, as the contract has it; the log mode is the mean of ln(flux) over the bin, exponentiated"""
    require_extended_precision()
    lam = np.asarray(lam, np.float64)
    L, f, nw = lam.astype(LD), np.asarray(flux, LD), len(lam)
    lf = _ld_log(f)

    def edge(x):
        """(value, ln value); value 0 marks an interface outside the table"""
        if x < lam[0] or x > lam[-1]:
            return LD(0), LD(-np.inf)
        p = int(np.searchsorted(lam, x, side="left")) - 1       # -1, an interface ON the first point, wraps as the host's index does
        q = p + 1
        xl = LD(x)
        d_hi, d_lo, width = L[q] - xl, xl - L[p], L[q] - L[p]
        if log:
            ln = ((LD(0) if d_hi == 0 else d_hi * lf[p]) + d_lo * lf[q]) / width
            return np.exp(ln), ln
        return (f[p] * d_hi + f[q] * d_lo) / width, None
    edges = [edge(x) for x in inter]
    out = np.zeros(len(inter) - 1, LD)
    for i in range(len(out)):
        (e0, l0), (e1, l1) = edges[i], edges[i + 1]
        if e0 == 0 or e1 == 0:
            continue
        lo, hi = inter[i], inter[i + 1]
        first = int(np.searchsorted(lam, lo, side="left"))
        if not lam[first] < hi:
            out[i] = np.exp((l0 + l1) / 2) if log else (e0 + e1) / 2
            continue
        last = int(np.searchsorted(lam, hi, side="left"))
        if last >= nw:
            continue
        x = np.concatenate(([LD(lo)], L[first:last], [LD(hi)]))
        dx = np.diff(x)
        if log:
            ly = np.concatenate(([l0], lf[first:last], [l1]))
            terms = np.where(dx == 0, LD(0), dx * (ly[:-1] + ly[1:]) / 2)
            out[i] = np.exp(terms.sum() / (LD(hi) - LD(lo)))
        else:
            y = np.concatenate(([e0], f[first:last], [e1]))
            out[i] = (dx * (y[:-1] + y[1:]) / 2).sum() / (LD(hi) - LD(lo))
    return out


def reference_spectra(table, weight, inter):
    """[3][nbin] in long double: absorption and scattering (log), the scattering-weighted third spectrum (linear)"""
    a, s = reference_weighted(table, weight)
    return np.stack([reference_rebin(table["lamda_mie"], a, inter, True), reference_rebin(table["lamda_mie"], s, inter, True),
                     reference_rebin(table["lamda_mie"], s, inter, False)])


# ---- the host's formulas, evaluated plainly and sequentially in fp64 ----------------------------------------------------------------
def plain_rebin(lam, flux, inter, log):
    lam, flux, nw = [float(v) for v in lam], [float(v) for v in flux], len(lam)

    def edge(x):
        if x < lam[0] or x > lam[-1]:
            return 0.0
        p = int(np.searchsorted(lam, x, side="left")) - 1
        d_hi, d_lo, width = lam[p + 1] - x, x - lam[p], lam[p + 1] - lam[p]
        if log:
            return (flux[p] ** d_hi * flux[p + 1] ** d_lo) ** (1 / width)
        return (flux[p] * d_hi + flux[p + 1] * d_lo) / width
    e = [edge(float(x)) for x in inter]
    out = []
    for i in range(len(inter) - 1):
        lo, hi = float(inter[i]), float(inter[i + 1])
        if e[i] == 0 or e[i + 1] == 0:
            out.append(0.0)
            continue
        first = int(np.searchsorted(lam, lo, side="left"))
        if not lam[first] < hi:
            out.append((e[i] * e[i + 1]) ** 0.5 if log else (e[i] + e[i + 1]) / 2.0)
            continue
        last = int(np.searchsorted(lam, hi, side="left"))
        if last >= nw:
            out.append(0.0)
            continue
        x = [lo] + lam[first:last] + [hi]
        y = [e[i]] + flux[first:last] + [e[i + 1]]
        acc = 1.0 if log else 0.0
        for k in range(len(x) - 1):
            if log:
                acc *= (y[k] * y[k + 1]) ** (0.5 * (x[k + 1] - x[k]))
            else:
                acc += (y[k] + y[k + 1]) / 2.0 * (x[k + 1] - x[k])
        out.append(acc ** (1 / (hi - lo)) if log else acc / (hi - lo))
    return np.array(out, np.float64)


def plain_spectra(table, weight, inter):
    nr, nw = table["scat"].shape
    a, s = [0.0] * nw, [0.0] * nw
    for r in range(nr):
        for j in range(nw):
            a[j] += float(table["absorb"][r, j]) * float(weight[r])
            s[j] += float(table["scat"][r, j]) * float(weight[r])
    lam = table["lamda_mie"]
    return np.stack([plain_rebin(lam, a, inter, True), plain_rebin(lam, s, inter, True), plain_rebin(lam, s, inter, False)])


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def relative_deviation(values, ref):
    """|values / ref - 1| per entry in long double; 0 where both are exactly 0, inf where only one is"""
    v, r = np.asarray(values, np.float64).astype(LD), np.asarray(ref, LD)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.abs(v - r) / np.abs(r)
    d = np.where((r == 0) & (v == 0), LD(0), d)
    return np.where((r == 0) & (v != 0), LD(np.inf), d).astype(np.float64)


def hold(values, ref, comparison, what):
    """assert the rule for every entry; returns the largest ratio deviation / tolerance.  `comparison`: the evaluation whose
    own deviation from the restatement sets the tolerance"""
    ref = np.asarray(ref, LD)
    zero = ref == 0
    assert np.all(np.asarray(values)[zero] == 0.0), "%s: a zero of the restatement is not an exact zero" % what
    dev, eps = relative_deviation(values, ref), relative_deviation(comparison, ref)
    tol = np.maximum(FLOOR, 8.0 * eps)
    ratio = float((dev / tol).max())
    worst = int(np.argmax(dev / tol))
    print("%s: largest deviation / tolerance = %.3e (entry %d: deviation %.3e, tolerance %.3e)"
          % (what, ratio, worst, dev.reshape(-1)[worst], tol.reshape(-1)[worst]))
    assert ratio <= 1.0, "%s: entry %d deviates by %.3e, the tolerance there is %.3e" % (
        what, worst, dev.reshape(-1)[worst], tol.reshape(-1)[worst])
    return ratio


# ---- synthetic LX-MIE directories ---------------------------------------------------------------------------------------------------
def synthetic_mie(nw, seed):
    """a Mie table on a non-uniform grid of nw wavelengths: micron as the files hold them, cross-sections [radius][wavelength]"""
    rng = np.random.default_rng(seed)
    steps = rng.uniform(0.4, 1.6, nw - 1) * (np.log(80.0) / (nw - 1))
    lam_um = 0.3 * np.exp(np.concatenate(([0.0], np.cumsum(steps))))
    r = R_VALUES[:, None]
    size = 2 * np.pi * r / lam_um[None, :]
    geo = np.pi * (r * 1e-4) ** 2
    scat = geo * np.minimum(size ** 4, 2.0 + np.cos(size)) * rng.uniform(0.7, 1.3, (len(R_VALUES), nw))
    absorb = geo * np.minimum(size, 1.0) * rng.uniform(0.2, 0.6, (len(R_VALUES), nw))
    g = rng.uniform(0.0, 0.9, (len(R_VALUES), nw))
    return lam_um, scat, absorb, g


def write_mie_directory(path, lam_um, scat, absorb, g):
    """51 files r{radius:.6f}.dat: one header line, 7 columns of which 0 (wavelength, micron), 3 (scattering), 4 (absorption) and
    6 (g_0) are read; every number with 17 significant digits, so that the reader gets these doubles back"""
    os.makedirs(path, exist_ok=True)
    for k, r in enumerate(R_VALUES):
        with open(os.path.join(path, "r{:.6f}.dat".format(r)), "w") as f:
            f.write("#wavelength size_parameter extinction scattering absorption albedo asymmetry\n")
            for j in range(len(lam_um)):
                f.write("%.17e %.17e %.17e %.17e %.17e %.17e %.17e\n" % (
                    lam_um[j], 2 * np.pi * r / lam_um[j], scat[k, j] + absorb[k, j], scat[k, j], absorb[k, j],
                    scat[k, j] / (scat[k, j] + absorb[k, j]), g[k, j]))
    return path + os.sep


def table_of(lam_um, scat, absorb):
    """the table as the reader builds it from the files"""
    return dict(lamda_mie=np.asarray(lam_um, np.float64) * 1e-4, scat=np.asarray(scat, np.float64),
                absorb=np.asarray(absorb, np.float64))


def radius_weight(r_mode, sigma):
    from helios_amd.clouds import Cloud
    return Cloud.lognorm_pdf(R_VALUES, r_mode, sigma) * DELTA_R


# ---- bin grids ----------------------------------------------------------------------------------------------------------------------
def bin_grid(lam, nbin):
    """nbin + 1 interfaces [cm] around a Mie grid `lam`: from half its first to twice its last wavelength, so that bins lie below
    and above the table; three interfaces moved onto tabulated wavelengths -- the first one, an inner one and the last one (the
    bin below it has the last tabulated wavelength as its upper interface); with few bins (1: one bin well inside) some hold ten
    points and more, with many most hold none"""
    lam = np.asarray(lam, np.float64)
    n = len(lam)
    if nbin == 1:
        return np.array([0.5 * (lam[2] + lam[3]), 0.5 * (lam[n - 3] + lam[n - 2])])
    if nbin == 65:
        # 40 fine bins up to the table's 6th point, one wide bin to its 6th point from the end, 24 bins to beyond its end
        inter = np.concatenate((np.geomspace(0.5 * lam[0], lam[5], 41), np.geomspace(lam[n - 6], 2.0 * lam[-1], 25)))
    else:
        inter = np.geomspace(0.5 * lam[0], 2.0 * lam[-1], nbin + 1)
    for target in (lam[0], lam[n // 3], lam[-1]):
        k = int(np.argmin(np.abs(np.log(inter / target))))
        inter[k] = target
    assert len(inter) == nbin + 1 and np.all(np.diff(inter) > 0)
    return inter


def grid_features(lam, inter):
    """which of the contract's cases the bins of a grid contain"""
    lam, inter = np.asarray(lam), np.asarray(inter)
    inside = np.array([np.count_nonzero((lam >= inter[i]) & (lam < inter[i + 1])) for i in range(len(inter) - 1)])
    within = (inter[:-1] >= lam[0]) & (inter[1:] <= lam[-1])
    return dict(below=bool(np.any(inter[:-1] < lam[0])), above=bool(np.any(inter[1:] > lam[-1])),
                empty=bool(np.any(within & (inside == 0))), ten=bool(np.any(within & (inside >= 10))),
                on_point=bool(np.any(np.isin(inter, lam))), ends_on_last=bool(np.any(inter[1:] == lam[-1])),
                on_first=bool(np.any(inter[:-1] == lam[0])), most_points=int(inside[within].max()) if within.any() else 0)


class Quant(object):
    """what the host's Cloud methods read of a Store"""

    def __init__(self, inter, nlayer=1, iso=0, p_boa=1e6, p_toa=1.0):
        self.opac_interwave = np.asarray(inter, np.float64)
        self.opac_wave = 0.5 * (self.opac_interwave[1:] + self.opac_interwave[:-1])
        self.nbin, self.nlayer, self.ninterface, self.iso, self.clouds = len(self.opac_wave), nlayer, nlayer + 1, iso, 1
        self.p_int = np.geomspace(p_boa, p_toa, nlayer + 1)
        self.p_lay = np.sqrt(self.p_int[:-1] * self.p_int[1:])


def host_cloud(mie_paths, r_mode, sigma, p_bot=(1e4,), f_bot=(1e-12,), ratio=(0.5,)):
    from helios_amd.clouds import Cloud
    c = Cloud()
    c.nr_cloud_decks = len(mie_paths)
    c.mie_path, c.cloud_r_mode, c.cloud_r_std_dev = list(mie_paths), list(r_mode), list(sigma)
    c.cloud_mixing_ratio_setting = "manual"
    c.p_cloud_bot, c.f_cloud_bot, c.cloud_to_gas_scale_height = list(p_bot), list(f_bot), list(ratio)
    return c


def host_spectra(cloud, deck, quant):
    """[3][nbin] of one deck by the host's Cloud path (reads the directory)"""
    cloud.calc_weighted_cross_sections_with_pdf_and_interpolate_wavelengths(deck, quant)
    return np.array([cloud.abs_cross_one_cloud, cloud.scat_cross_one_cloud, cloud.g_0_one_cloud], np.float64)
