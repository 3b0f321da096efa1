"""The k-table contract (include/helios_hip.h section 6) restated plainly in np.longdouble, one bin at a time, and the
re-gridding formula likewise; synthetic spectral axes whose bins hold exactly the numbers of points a test asks for; the
slabs and Gauss sets of the edge tests (tests/test_ktable_reference.py on the CPU, tests/test_gpu_ktable_edges.py on the
device).  Of the project it takes the floor's value and the spectral axis, nothing else: no sort, no scan, no plan."""
import numpy as np

from helios_amd.ktable import K_FLOOR, spectral_axis

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)


def require_extended_precision():
    """the reference is worth nothing in a long double that is a double: fail, do not skip"""
    assert EPS_LD <= 1.1e-19, "np.longdouble has eps %.3e here: no 64-bit mantissa to hold the kernels to" % EPS_LD


# ---- one bin ------------------------------------------------------------------------------------------------------------------
def reference_weights(lam, inter, x, s, e):
    """w of the points s .. e-1 of bin x (at least two): the wavelength interval each stands for over the bin's width"""
    lb = np.asarray(lam[s:e], np.float64).astype(LD)             # double -> long double is exact
    lo, hi = LD(np.float64(inter[x])), LD(np.float64(inter[x + 1]))
    w = np.empty(e - s, LD)
    w[0] = (lb[0] - lo) + (lb[1] - lb[0]) / 2
    w[1:-1] = (lb[2:] - lb[:-2]) / 2
    w[-1] = (hi - lb[-1]) + (lb[-1] - lb[-2]) / 2
    return w / (hi - lo)


def reference_floored(k32):
    """fp32 -> fp64 -> floor: NaN, zero, negatives and everything not above 1e-15 go to 1e-15; then exactly to long double"""
    k = np.asarray(k32, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        k = np.where(k > K_FLOOR, k, K_FLOOR)
    return k.astype(LD)


def reference_curve(lam, inter, x, s, e, opac_rev):
    """(y, log10 k) of the sorted points of a bin of at least two points; `opac_rev` in ascending wavelength"""
    require_extended_precision()
    w = reference_weights(lam, inter, x, s, e)
    k = reference_floored(opac_rev[s:e])
    order = np.lexsort((w, k))
    w, k = w[order], k[order]
    mid = np.empty(e - s, LD)
    mid[0] = w[0] / 2
    mid[1:] = (w[:-1] + w[1:]) / 2
    return np.cumsum(mid, dtype=LD), np.log10(k)


def reference_interp(y, logk, yg):
    """log10 k at the abscissae: linear in y between the two points around each, the end values outside [y_0, y_{n-1}]"""
    yg = np.asarray(yg, np.float64).astype(LD)
    hi = np.clip(np.searchsorted(y, yg, side="left"), 1, len(y) - 1)
    lo = hi - 1
    out = logk[lo] + (logk[hi] - logk[lo]) * ((yg - y[lo]) / (y[hi] - y[lo]))
    out = np.where(yg <= y[0], logk[0], out)
    return np.where(yg >= y[-1], logk[-1], out)


def reference_bin(lam, inter, x, s, e, opac_rev, yg):
    """log10 k (long double) of one bin of one (T, P) point at the abscissae yg"""
    require_extended_precision()
    n = e - s
    if n == 0:
        return np.full(len(yg), np.log10(LD(K_FLOOR)), LD)
    if n == 1:
        return np.full(len(yg), np.log10(reference_floored(opac_rev[s:e])[0]), LD)
    y, logk = reference_curve(lam, inter, x, s, e, opac_rev)
    return reference_interp(y, logk, yg)


def perturbed(y):
    """y with every point moved by one ulp of a double, neighbours in opposite directions"""
    ulp = np.spacing(y.astype(np.float64)).astype(LD)
    sign = np.where(np.arange(len(y)) % 2 == 0, LD(1), LD(-1))
    return y + sign * ulp


# ---- re-gridding ----------------------------------------------------------------------------------------------------------------
def reference_plan(old, new):
    """per target node the left source node -- the last one <= v -- and whether the axis is clamped: at or below the first
    source node and at (or beyond) the last"""
    old, new = np.asarray(old, np.float64), np.asarray(new, np.float64)
    left = np.maximum(np.searchsorted(old, new, side="right") - 1, 0).astype(np.int32)
    clamped = ((new <= old[0]) | (left == len(old) - 1)).astype(np.int32)
    return left, clamped


def reference_regrid(temp_old, press_old, k_old, temp_new, press_new, nc, rows=None):
    """k[rows of temp_new][press_new][nc] in long double: bilinear in T and log10 P as a product of two one-dimensional
    blends, the source's edge value where an axis is clamped.  log10 P is taken in long double."""
    require_extended_precision()
    T, Tn = np.asarray(temp_old, np.float64).astype(LD), np.asarray(temp_new, np.float64).astype(LD)
    lp = np.log10(np.asarray(press_old, np.float64).astype(LD))
    lpn = np.log10(np.asarray(press_new, np.float64).astype(LD))
    k = np.asarray(k_old, np.float64).reshape(len(T), len(lp), nc)
    tl, tc = reference_plan(temp_old, temp_new)
    pl, pc = reference_plan(press_old, press_new)
    rows = range(len(Tn)) if rows is None else rows
    out = np.empty((len(rows), len(lpn), nc), LD)
    for a, i in enumerate(rows):
        t0 = tl[i]
        t1 = t0 if tc[i] else t0 + 1
        ft = LD(0) if tc[i] else (Tn[i] - T[t0]) / (T[t1] - T[t0])
        for j in range(len(lpn)):
            p0 = pl[j]
            p1 = p0 if pc[j] else p0 + 1
            fp = LD(0) if pc[j] else (lpn[j] - lp[p0]) / (lp[p1] - lp[p0])
            lower = k[t0, p0].astype(LD) * (1 - fp) + k[t0, p1].astype(LD) * fp
            upper = k[t1, p0].astype(LD) * (1 - fp) + k[t1, p1].astype(LD) * fp
            out[a, j] = lower * (1 - ft) + upper * ft
    return out


# sources of 1 x 1, 1 x 3, 3 x 1 and 3 x 4 nodes (T, P); targets below, on, between and above them
REGRID_SOURCES = [([300.0], [1e4]), ([300.0], [1e2, 1e4, 1e7]), ([200.0, 450.0, 900.0], [1e5]),
                  ([200.0, 450.0, 900.0], [1e1, 1e3, 10 ** 4.33333333, 1e8])]
REGRID_T = [100.0, 200.0, 201.0, 450.0, 700.0, 900.0, 2500.0]              # below, on, between and above the nodes
REGRID_P = [1e-2, 1e1, 50.0, 1e3, 1e4, 10 ** 4.33333333, 3e6, 1e8, 1e10]


def regrid_source(temps, press, nc=35, seed=3):
    return 10.0 ** np.random.default_rng(seed).uniform(-15, 3, len(temps) * len(press) * nc)


# ---- synthetic axes ---------------------------------------------------------------------------------------------------------------
ON_POINT = "on a point"


def synthetic_grid(sizes, numax, res, place, first=1):
    """(lam, start, end, inter): the axis of `spectral_axis(0, numax, res)` and consecutive bins from point `first` on that hold
    exactly `sizes` points.  Every interface lies in the gap below the first point of the bin above it: at the fraction
    `place` of the gap, or -- ON_POINT -- on that point itself, which then belongs to the upper bin while the lower bin's last
    weight takes the whole gap.  Interfaces of empty bins share a gap, at equal steps up to that place."""
    lam = spectral_axis(0, numax, res)
    n = len(lam)
    start = first + np.concatenate(([0], np.cumsum(sizes)[:-1])).astype(np.int64)
    end = start + np.asarray(sizes, np.int64)
    assert first >= 1 and end[-1] <= n, "the bins need %d points from %d on, the axis has %d" % (sum(sizes), first, n)
    frac = 1.0 if place == ON_POINT else float(place)
    assert 0.0 < frac <= 1.0
    at = np.concatenate((start, end[-1:]))                # interface x lies in the gap below point at[x]
    inter = np.empty(len(at), np.float64)
    for b in np.unique(at):
        idx = np.nonzero(at == b)[0]
        below = lam[b - 1]
        above = lam[b] if b < n else lam[n - 1] + (lam[n - 1] - lam[n - 2])       # beyond the axis: one more gap of the last
        for q, xi in enumerate(idx):
            f = frac * (q + 1) / len(idx)
            inter[xi] = above if f == 1.0 else below + f * (above - below)
    assert np.all(np.diff(inter) > 0)
    # membership as the contract states it: inter[x] <= lam < inter[x + 1]
    for x in range(len(sizes)):
        inside = np.nonzero((inter[x] <= lam) & (lam < inter[x + 1]))[0]
        assert np.array_equal(inside, np.arange(start[x], end[x])), (x, sizes[x])
    # the kernel's key orders interior points by their index: their weights must rise strictly with it
    lo, hi = int(start[0]), int(end[-1])
    interior = (lam[lo + 2:hi] - lam[lo:hi - 2]) / 2
    assert np.all(np.diff(interior) > 0), "interior weights do not rise strictly on this axis"
    return lam, start.astype(np.int32), end.astype(np.int32), inter


# ---- the edge matrix ----------------------------------------------------------------------------------------------------------------
# where the kernel changes its path: the special cases n < 3, a wavefront, the scan's run length 1 -> 2 -> 3 -> 5, the hand-over
# from the LDS sort to the scratch at 16384 (one merge level up to 32768, three at 70001)
MAIN_SIZES = [0, 1, 2, 3, 4, 5, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4097, 16383, 16384, 16385, 32769, 70001]
SORT_SIZES = [3, 5, 7, 8, 9, 17, 31, 33, 100, 257, 1025, 2049]
NU0_SIZES = [4, 1, 37, 0, 2, 130, 3]               # the last bin holds nu = 0, which the axis puts at 10000 cm

F32_MAX = np.finfo(np.float32).max
F32_FLOOR_UP = np.float32(1e-15)                   # 1.00000000362e-15: above the double floor, not floored
F32_FLOOR_DOWN = np.nextafter(np.float32(1e-15), np.float32(0))
F32_SUBNORMAL = np.float32(1e-41)
assert float(F32_FLOOR_UP) > K_FLOOR >= float(F32_FLOOR_DOWN)


def main_grid(place):
    """171 000 points at 0.01 cm^-1, the bins from the short-wavelength end on"""
    return synthetic_grid(MAIN_SIZES, 1710, 0.01, place)


def sort_grid(place):
    return synthetic_grid(SORT_SIZES, 40, 0.01, place, first=3)


def nu0_grid(place):
    lam = spectral_axis(0, 3, 0.01)
    return synthetic_grid(NU0_SIZES, 3, 0.01, place, first=len(lam) - sum(NU0_SIZES))


def edge_slabs(n, seed):
    """five (T, P) slabs of n points, fp32 as the files hold them.  No inf: the contract does not define it."""
    rng = np.random.default_rng(seed)

    def sprinkle(a, values, every):
        for v in values:
            a[rng.choice(n, max(1, n // every), replace=False)] = v
        return a

    uniform = (10.0 ** rng.uniform(-20, 3, n)).astype(np.float32)
    sprinkle(uniform, [F32_MAX, F32_FLOOR_UP, F32_FLOOR_DOWN, F32_SUBNORMAL, np.float32(1.4e-45)], 150)
    ties = (rng.integers(10, 100, n) * 1e-13).astype(np.float32)              # two significant digits x 1e-12
    sprinkle(ties, [np.float32(0), np.float32(-3e-12), np.float32(np.nan), np.float32(-0.0), F32_FLOOR_UP, F32_MAX,
                    F32_SUBNORMAL], 40)
    equal = np.full(n, 3.5e-7, np.float32)
    floored = rng.choice(np.array([0, 1e-16, 1e-30, -1.0, F32_FLOOR_DOWN, F32_SUBNORMAL, np.nan], np.float32), n)
    slabs = np.stack([uniform, ties, equal, floored, uniform.copy()])
    assert np.all(~np.isinf(slabs)) and slabs[0].tobytes() == slabs[4].tobytes()
    return slabs


def gauss_sets(extra):
    """name -> abscissae: 1, 20 and 1100 Gauss points on (0, 1), then 1e-9, 1 - 1e-9 and `extra`"""
    out = {}
    for ng in (1, 20, 1100):
        y = 0.5 * np.polynomial.legendre.leggauss(ng)[0] + 0.5
        out["ng%d" % ng] = np.concatenate((y, [1e-9, 1 - 1e-9], np.asarray(extra, np.float64)))
    return out


class EdgeCase(object):
    """one grid and its five slabs: the long-double curves of every bin, made once"""

    def __init__(self, name, grid, seed):
        self.name = name
        self.lam, self.start, self.end, self.inter = grid
        self.slabs = edge_slabs(len(self.lam), seed)
        self.curves = {}
        for t in range(len(self.slabs)):
            rev = self.slabs[t][::-1]
            for x in range(len(self.start)):
                s, e = int(self.start[x]), int(self.end[x])
                if e - s >= 2:
                    self.curves[t, x] = reference_curve(self.lam, self.inter, x, s, e, rev)
        # a few y_i of the largest bins as abscissae, rounded to double
        big = np.argsort(self.end - self.start)[-3:]
        self.extra = np.array([float(self.curves[t, x][0][i]) for t in (0, 1) for x in big if (t, x) in self.curves
                               for i in (0, len(self.curves[t, x][0]) // 3, len(self.curves[t, x][0]) - 1)])
        self.gauss = gauss_sets(self.extra)

    def reference(self, yg, y_of=None):
        """log10 k [slab][bin][abscissa] in long double; `y_of` changes every curve's y first"""
        out = np.empty((len(self.slabs), len(self.start), len(yg)), LD)
        for t in range(len(self.slabs)):
            rev = self.slabs[t][::-1]
            for x in range(len(self.start)):
                s, e = int(self.start[x]), int(self.end[x])
                if e - s < 2:
                    out[t, x] = reference_bin(self.lam, self.inter, x, s, e, rev, yg)
                else:
                    y, logk = self.curves[t, x]
                    out[t, x] = reference_interp(y if y_of is None else y_of(y), logk, yg)
        return out

    def fp64(self, fp64_bin, yg):
        """log10 of a plain fp64 evaluation (helios_amd.ktable.numpy_bin), same layout, in long double"""
        out = np.empty((len(self.slabs), len(self.start), len(yg)), LD)
        for t in range(len(self.slabs)):
            rev = self.slabs[t][::-1]
            for x in range(len(self.start)):
                out[t, x] = np.log10(fp64_bin(self.lam, self.inter, x, int(self.start[x]), int(self.end[x]), rev, yg).astype(LD))
        return out

    def eps64(self, fp64_bin, yg, ref):
        """per slab: the largest |delta log10 k| of the fp64 evaluation against the reference"""
        return np.abs(self.fp64(fp64_bin, yg) - ref).reshape(len(self.slabs), -1).max(axis=1).astype(np.float64)


GRIDS = {"main-0.3": (main_grid, 0.3, 11), "main-on-point": (main_grid, ON_POINT, 12), "nu0-0.3": (nu0_grid, 0.3, 13),
         "nu0-on-point": (nu0_grid, ON_POINT, 14), "sort-0.3": (sort_grid, 0.3, 15), "sort-on-point": (sort_grid, ON_POINT, 16)}
_cases = {}


def edge_case(name):
    """the edge matrix's grids by name, with their slabs and curves; built once per process"""
    if name not in _cases:
        make, place, seed = GRIDS[name]
        _cases[name] = EdgeCase(name, make(place), seed)
    return _cases[name]


REFERENCE_CASES = ["main-0.3", "main-on-point", "nu0-0.3", "nu0-on-point"]
