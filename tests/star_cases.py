"""What the star tool's CPU and GPU tests share: the committed fixtures (tests/golden/star/, made by make_star_golden.py from the
reference's own functions), the tolerance rule, and synthetic spectra whose bins hold exactly the numbers of points a test
asks for."""
import os

import numpy as np

import star_reference as sr
from helios_amd import fits_lite, star

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "star")
PHOENIX = os.path.join(GOLD, "phoenix")
GRID_R50 = os.path.join(GOLD, "grid_r50.h5")
GRID_CENTRES = os.path.join(GOLD, "grid_centres.h5")

_cache = {}


def golden():
    if "ref" not in _cache:
        _cache["ref"] = dict(np.load(os.path.join(GOLD, "reference.npz")))
    return _cache["ref"]


def blend_cases():
    g = golden()
    return {k[len("blend_"):-len("_par")]: tuple(g[k]) for k in g if k.startswith("blend_") and k.endswith("_par")}


def phoenix_lambda():
    if "lam" not in _cache:
        _cache["lam"] = fits_lite.getdata(os.path.join(PHOENIX, star.PHOENIX_WAVE_FILE), 0, force_lite=True).astype(np.float64) * 1e-8
    return _cache["lam"]


def corner(t, g, m):
    """the fp32 corner spectrum at a node, whichever way its file spells a zero [M/H]"""
    key = ("corner", int(t), float(g), float(m) + 0.0)
    if key not in _cache:
        d = star.PhoenixDirectory(PHOENIX)
        _cache[key] = fits_lite.getdata(d._find(star.corner_name(int(t), g, m)), 0, force_lite=True)
    return _cache[key]


def restated_blend(name):
    key = ("restated", name)
    if key not in _cache:
        t, g, m = blend_cases()[name]
        _cache[key] = sr.reference_blend(corner, int(t) if float(t).is_integer() else t, g, m)
    return _cache[key]


def grids():
    if "grids" not in _cache:
        c, i = star.read_lambda_grid(GRID_R50)
        c2, i2 = star.read_lambda_grid(GRID_CENTRES)
        _cache["grids"] = {"r50": (c, i), "centres": (c2, i2)}
    return _cache["grids"]


def bound(eps_ref):
    """the project's rule: within max(1e-13, 8 eps_ref) relative, eps_ref the checker's own deviation from the restatement"""
    return np.maximum(1e-13, 8 * np.asarray(eps_ref, np.float64))


def hold(value, restated, eps_source, what):
    """`value` against the restatement under the rule, `eps_source` being what measures eps (the reference's results for the
    numpy backend, the numpy backend's for the device); entries that are exactly 0 in the restatement are 0"""
    value, restated, eps_source = np.asarray(value), np.asarray(restated), np.asarray(eps_source)
    zero = eps_source.astype(np.float64) == 0            # exactly 0 in the checker (an underflow of fp64 included): 0 here
    assert np.all(value[zero] == 0), what
    if zero.all():
        return
    dev, eps = sr.rel_dev(value[~zero], restated[~zero]), sr.rel_dev(eps_source[~zero], restated[~zero])
    worst = int(np.argmax(dev - bound(eps)))
    print("%s: largest deviation %.3e, eps of the checker at most %.3e" % (what, dev.max(), eps.max()))
    assert np.all(dev <= bound(eps)), "%s: entry %d of the non-zero ones deviates by %.3e, allowed %.3e (%d entries beyond)" % (
        what, worst, dev[worst], bound(eps)[worst], int(np.sum(dev > bound(eps))))


def counted_spectrum(counts, seed=0, lead=2, tail=2):
    """(lamda, flux, interfaces): a spectrum with `lead` points before the first interface, counts[k] points strictly inside
    bin k, and `tail` points beyond the last interface; widths and fluxes vary, all numbers are plain doubles"""
    rng = np.random.default_rng(seed)
    lam, inter, x = [], [], 1.0e-4
    for _ in range(lead):
        lam.append(x)
        x += 1e-8 * (1 + rng.random())
    for c in counts:
        inter.append(x)
        x += 1e-8 * (1 + rng.random())
        for _ in range(int(c)):
            lam.append(x)
            x += 1e-8 * (1 + rng.random())
    inter.append(x)
    for _ in range(tail):
        x += 1e-8 * (1 + rng.random())
        lam.append(x)
    lam, inter = np.asarray(lam, np.float64), np.asarray(inter, np.float64)
    flux = 1e14 * (0.2 + rng.random(len(lam)))
    return lam, flux, inter
