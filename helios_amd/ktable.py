"""Per-species k-tables from HELIOS-K output, built on the device (include/helios_hip.h section 6, csrc/ktable.hip).

Stage 1 of the reference's k-table tool (ktable/source_ktable/build_individual_opacities.py, k-distribution format) and the
(T, P) re-gridding of combination.py::interpolate_opacity_to_final_grid: a directory of `Out_[<name>_]<numin>_<numax>_<T>_
<pcode>.bin` files becomes `<name>_opac_kdistr.h5` on the files' own (T, P) nodes and `<name>_opac_ip_kdistr.h5` on the
target grid -- the container `Read.read_species_opacities` and premix.py take.

Per wavelength bin and (T, P) point: floor the opacities at 1e-15, weight every point by the wavelength interval it stands
for, sort by (log10 k, weight), accumulate the mid-points of the weights to y, and interpolate log10 k linearly in y at the
Gauss abscissae.  The host decides bin membership and the empty-bin rule once per species (fp64, the reference's own
comparisons); the sort, the scan and the interpolation run in k_ktable_bins, or -- `backend="numpy"` -- in numpy, which is the
checker of the device path and what a machine without a GPU gets when it asks for it.

Where the slabs come from is build_table's `source`: FileSlabs reads them from the directory (build_species, as ever);
lines.LineSlabs makes them from a line list and leaves them on the device, where KTableBuilder.run_device sorts them without an
upload (`lines.py -ktable yes`).
"""
import argparse
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from ._tool import DeviceObject, dp, ip, vp


K_FLOOR = 1e-15
MAX_READERS = 16          # threads that read files; never sized by the machine's CPU count
LDS_POINTS = 16384        # bins up to this many points are sorted in LDS (128 KiB of keys)

EMPTY_BIN_MESSAGE = ("k-distribution construction failed: the original wavelength grid must be finer than the table's. "
                     "Every wavelength bin needs at least one opacity point of the HELIOS-K grid (bin %d, %.6e - %.6e cm, has "
                     "none); use a finer original grid or a coarser table grid.")


# ---- names and grids (no device) ---------------------------------------------------------------------------------------
def pressure_table():
    """HELIOS-K's pressure code -> dyne cm^-2, the reference's table: thirds of a decade carry eight digits"""
    from fractions import Fraction
    part = {0: Fraction(0), 33: Fraction(1, 3), 50: Fraction(1, 2), 66: Fraction(2, 3)}
    digits = {Fraction(1, 3): "33333333", Fraction(1, 2): "5", Fraction(2, 3): "66666666"}
    table = {}
    for sign, letter in ((-1, "n"), (1, "p")):
        for whole in range(0, 9 if sign < 0 else 5):
            for hundredths in (0, 33, 50, 66):
                if (sign < 0 and whole == 0 and hundredths == 0) or (whole == (8 if sign < 0 else 4) and hundredths):
                    continue
                cgs = sign * (whole + part[hundredths]) + 6          # the code is log10 of bar; 1 bar = 1e6 dyne cm^-2
                if cgs.denominator == 1:
                    value = float("1e%d" % int(cgs))
                else:                                                # thirds are cut after eight digits, towards zero
                    mag = abs(cgs)
                    value = 10 ** float("%s%d.%s" % ("-" if cgs < 0 else "", int(mag), digits[mag - int(mag)]))
                table["%s%d%02d" % (letter, whole, hundredths)] = value
    return table


def parse_file_name(fname):
    """`Out_[<name>_]<numin>_<numax>_<T>_<pcode>.<ext>` -> (name or None, numin, numax, T, pcode); the last four
    underscores delimit the numbers, whatever the name holds"""
    parts = fname.split("_")
    if len(parts) < 5 or parts[0] != "Out":
        raise IOError("ktable: %r is not a HELIOS-K output name (Out_[<name>_]<numin>_<numax>_<T>_<pcode>.bin)" % fname)
    name = "_".join(parts[1:-4]) if len(parts) > 5 else None
    try:
        numin, numax, temp = int(parts[-4]), int(parts[-3]), int(parts[-2])
    except ValueError:
        raise IOError("ktable: cannot read wavenumbers and temperature from %r" % fname)
    return name, numin, numax, temp, parts[-1][:4]


def gen_fixed_res_grid(bot_limit, top_limit, resolution):
    """interfaces of a grid of constant R = lambda / delta lambda (the reference's recurrence, in its arithmetic)"""
    out, point = [], bot_limit
    while point < top_limit:
        out.append(point)
        point *= (resolution + 1) / resolution
    return out


def read_grid_file(path):
    out = []
    with open(path) as f:
        for line in f:
            col = line.split()
            if col:
                out.append(float(col[0]))
    return out


def wavelength_grid(grid_format, wavelength_grid=None, grid_file=None):
    """interfaces in cm.  `wavelength_grid`: (R, lo, hi) with the limits in micron"""
    if grid_format == "native_helios-k":
        raise IOError("ktable: the native_helios-k grid format works with the sampling format only, which is not built; "
                      "choose fixed_resolution or file")
    if grid_format == "fixed_resolution":
        res, lo, hi = [float(v) for v in wavelength_grid]
        inter = gen_fixed_res_grid(lo * 1e-4, hi * 1e-4, res)
    elif grid_format == "file":
        inter = read_grid_file(grid_file)
    else:
        raise IOError("ktable: unknown grid format %r (fixed_resolution or file)" % (grid_format,))
    inter = np.asarray(inter, np.float64)
    if len(inter) < 2 or np.any(np.diff(inter) <= 0):
        raise IOError("ktable: the wavelength grid needs at least two interfaces, in ascending order")
    return inter


def grid_datasets(inter, n_gauss):
    """centres, widths and Gauss abscissae on (0, 1) as the reference forms them"""
    inter = np.asarray(inter, np.float64)
    centre = (inter[:-1] + inter[1:]) / 2
    width = inter[1:] - inter[:-1]
    y = np.array([0.5 * v + 0.5 for v in np.polynomial.legendre.leggauss(int(n_gauss))[0]], np.float64)
    return centre, width, y


def spectral_axis(numin0, numax_last, resolution):
    """wavelengths of the HELIOS-K points in ascending order (cm); nu = 0 stands at 10000 cm"""
    nu = np.arange(numin0, numax_last, resolution)
    lam = np.empty(len(nu), np.float64)
    pos = nu > 0
    lam[pos] = 1 / nu[pos]
    lam[~pos] = 10000.0
    return np.ascontiguousarray(lam[::-1])


def bin_ranges(lam, inter):
    """[start, end) of every bin in the ascending wavelength array: inter[x] <= lambda < inter[x + 1]"""
    start = np.searchsorted(lam, inter[:-1], side="left")
    end = np.searchsorted(lam, inter[1:], side="left")
    return start.astype(np.int32), end.astype(np.int32)


def check_empty_bins(lam, inter, start, end):
    """the reference's scan state at every bin without points: filled with the floor while the scan has not passed a point
    (l_start == 0) or once the last matched point is the grid's last; an error otherwise.  Returns the bins to fill."""
    n, l_start, l_end, fill = len(lam), 0, 0, []
    for x in range(len(start)):
        if end[x] > start[x]:
            l_end = int(end[x]) - 1
        # the scan leaves l_start at the first point at or beyond the bin's upper interface; it stays if there is none
        first_beyond = int(np.searchsorted(lam[l_start:], inter[x + 1], side="left")) + l_start
        if first_beyond < n:
            l_start = first_beyond
        if end[x] == start[x]:
            if l_start == 0 or l_end == n - 1:
                fill.append(x)
            else:
                raise IndexError(EMPTY_BIN_MESSAGE % (x, inter[x], inter[x + 1]))
    return fill


# ---- the contract in numpy ----------------------------------------------------------------------------------------------
def bin_weights(lam, inter, x, s, e):
    """w of the points s .. e-1 of bin x (at least two), divided by the bin width"""
    lb = lam[s:e]
    w = np.empty(e - s, np.float64)
    w[0] = (lb[0] - inter[x]) + (lb[1] - lb[0]) / 2
    w[1:-1] = (lb[2:] - lb[:-2]) / 2
    w[-1] = (inter[x + 1] - lb[-1]) + (lb[-1] - lb[-2]) / 2
    return w / (inter[x + 1] - inter[x])


def floored_log10(k32):
    """log10 of max(1e-15, k): NaN and everything not above the floor land on it"""
    k = np.asarray(k32, np.float32).astype(np.float64)
    with np.errstate(invalid="ignore"):
        k = np.where(k > K_FLOOR, k, K_FLOOR)
    return np.log10(k)


def _interp_clamped(y, logk, yg):
    hi = np.clip(np.searchsorted(y, yg), 1, len(y) - 1)
    lo = hi - 1
    slope = (logk[hi] - logk[lo]) / (y[hi] - y[lo])
    out = slope * (yg - y[lo]) + logk[lo]
    out[yg < y[0]] = logk[0]
    out[yg > y[-1]] = logk[-1]
    return out


def _compensated_cumsum(a):
    """the reference's sequential running sum in fp64, and with it what every one of its additions rounded away (two-sum,
    exact in fp64), summed up alongside: over 7e4 points the plain sum drifts by tens of ulps of y, which the steep steps
    between tie groups turn into 1e-9 in log10 k; this one stays within an ulp or two"""
    s = np.cumsum(a)
    prev = np.concatenate(([0.0], s[:-1]))
    b = s - prev
    lost = (prev - (s - b)) + (a - b)
    return s + np.cumsum(lost)


def numpy_bin(lam, inter, x, s, e, opac_rev, yg, plain_sum=False):
    """one bin of one (T, P) point; `opac_rev` in ascending wavelength.  `plain_sum`: y by the reference's plain running sum,
    the fp64 noise of which is what the tests measure the device's bound from"""
    n = e - s
    if n == 0:
        return np.full(len(yg), K_FLOOR)
    if n == 1:
        k = float(np.float32(opac_rev[s]))
        return np.full(len(yg), k if k > K_FLOOR else K_FLOOR)
    w = bin_weights(lam, inter, x, s, e)
    logk = floored_log10(opac_rev[s:e])
    order = np.lexsort((w, logk))
    w, logk = w[order], logk[order]
    mid = np.empty(n, np.float64)
    mid[0] = 0.5 * w[0]
    mid[1:] = 0.5 * (w[:-1] + w[1:])
    y = np.cumsum(mid) if plain_sum else _compensated_cumsum(mid)
    return 10 ** _interp_clamped(y, logk, yg)


def numpy_slab(lam, inter, start, end, opac, yg):
    """kpoints[x][y] of one (T, P) point; `opac` as the files hold it (ascending wavenumber)"""
    rev = np.asarray(opac, np.float32)[::-1]
    out = np.empty((len(start), len(yg)), np.float64)
    for x in range(len(start)):
        out[x] = numpy_bin(lam, inter, x, int(start[x]), int(end[x]), rev, yg)
    return out


def regrid_plan(old, new):
    """per target node: the left source node and whether the axis is clamped there (the reference's branches)"""
    left, reduced = np.zeros(len(new), np.int32), np.zeros(len(new), np.int32)
    for i, v in enumerate(new):
        if old[0] < v:
            l = 0
            for x in range(len(old)):
                if old[x] <= v:
                    l = x
                else:
                    break
            left[i] = l
        else:
            reduced[i] = 1
        if left[i] == len(old) - 1:
            reduced[i] = 1
    return left, reduced


def numpy_regrid(press_old, temp_old, k_old, temp_new, press_new, nx, ny):
    """bilinear in T and log10 P, clamped outside the source nodes; term order of the reference's four branches"""
    nc = nx * ny
    k = np.asarray(k_old, np.float64).reshape(len(temp_old), len(press_old), nc)
    tl, tr = regrid_plan(temp_old, temp_new)
    pl, pr = regrid_plan(press_old, press_new)
    T, Tn = np.asarray(temp_old, np.float64), np.asarray(temp_new, np.float64)
    lp, lpn = np.log10(np.asarray(press_old, np.float64)), np.log10(np.asarray(press_new, np.float64))
    out = np.empty((len(Tn), len(lpn), nc), np.float64)
    for i in range(len(Tn)):
        t0 = tl[i]
        for j in range(len(lpn)):
            p0 = pl[j]
            if tr[i] and pr[j]:
                out[i, j] = k[t0, p0]
            elif tr[i]:
                out[i, j] = (k[t0, p0 + 1] * (lpn[j] - lp[p0]) + k[t0, p0] * (lp[p0 + 1] - lpn[j])) / (lp[p0 + 1] - lp[p0])
            elif pr[j]:
                out[i, j] = (k[t0 + 1, p0] * (Tn[i] - T[t0]) + k[t0, p0] * (T[t0 + 1] - Tn[i])) / (T[t0 + 1] - T[t0])
            else:
                a, b = Tn[i] - T[t0], T[t0 + 1] - Tn[i]
                c, d = lpn[j] - lp[p0], lp[p0 + 1] - lpn[j]
                out[i, j] = (k[t0 + 1, p0 + 1] * a * c + k[t0 + 1, p0] * a * d + k[t0, p0 + 1] * b * c
                             + k[t0, p0] * b * d) / ((T[t0 + 1] - T[t0]) * (lp[p0 + 1] - lp[p0]))
    return out.reshape(-1)


def default_target_grid():
    """the reference's hard-coded final grid: T = 50 ... 6000 step 50; 28 pressures, 1e0 ... 1e9 and the thirds between them
    (cut after eight digits, as in the pressure-code table)"""
    temp = np.arange(50, 6050, 50).astype(np.float64)
    press = [float(10 ** p) for p in range(10)]
    for first in (0.33333333, 0.66666666):
        press += [10 ** p for p in np.arange(first, first + 9, 1)]
    return temp, np.sort(np.asarray(press, np.float64))


def target_grid(temperature_grid=None, pressure_grid=None):
    """the hard-coded grid, or `first last step` (K) and `log10 first, log10 last, nodes` in its place.  premix.py takes tables
    whose nodes are uniform to 1e-9: the hard-coded pressures, thirds of a decade cut after eight digits, are not"""
    temp, press = default_target_grid()
    try:
        if temperature_grid is not None:
            a, b, step = [float(v) for v in str(temperature_grid).split()]
            temp = a + step * np.arange(int(round((b - a) / step)) + 1)
        if pressure_grid is not None:
            a, b, n = str(pressure_grid).split()
            press = 10.0 ** np.linspace(float(a), float(b), int(n))
    except ValueError:
        raise IOError("ktable: -temperature_grid takes 'first last step', -pressure_grid 'log10first log10last nodes'")
    if len(temp) < 1 or len(press) < 1 or np.any(np.diff(temp) <= 0) or np.any(np.diff(press) <= 0):
        raise IOError("ktable: the target grid's nodes must ascend")
    return temp, press


# ---- device -------------------------------------------------------------------------------------------------------------
def regrid_args(temp_old, press_old, temp_new, press_new):
    """the plan of a re-gridding as hx_ktable_regrid and hx_ktmix_set_species_native take it: t_left, t_reduced, p_left,
    p_reduced, temp_old, logp_old, temp_new, logp_new.  The pointers hold their arrays: keep the list until the call is over."""
    plan = regrid_plan(temp_old, temp_new) + regrid_plan(press_old, press_new)
    nodes = [np.ascontiguousarray(v, np.float64) for v in (temp_old, np.log10(np.asarray(press_old, np.float64)), temp_new,
                                                           np.log10(np.asarray(press_new, np.float64)))]
    return [ip(a) for a in plan] + [dp(a) for a in nodes]


class KTableBuilder(DeviceObject):
    """one species' spectral axis and bins on the device; (T, P) slabs go through in batches"""

    PREFIX = "hx_ktable"

    def __init__(self, ctx, n_points, n_bins, n_gauss, n_tp, max_tp_per_launch=4, lds_points=LDS_POINTS):
        self.n_points, self.n_bins, self.n_gauss, self.n_tp = int(n_points), int(n_bins), int(n_gauss), int(n_tp)
        self.max_tp = max(1, min(int(max_tp_per_launch), self.n_tp))
        self.ip_nodes = 0
        self._create(ctx, self.n_points, self.n_bins, self.n_gauss, self.n_tp, self.max_tp, int(lds_points))

    def set_grid(self, lam, start, end, inter, yg):
        a = [np.ascontiguousarray(lam, np.float64), np.ascontiguousarray(start, np.int32), np.ascontiguousarray(end, np.int32),
             np.ascontiguousarray(inter, np.float64), np.ascontiguousarray(yg, np.float64)]
        assert len(a[0]) == self.n_points and len(a[1]) == len(a[2]) == self.n_bins
        assert len(a[3]) == self.n_bins + 1 and len(a[4]) == self.n_gauss
        self._call("set_grid", dp(a[0]), ip(a[1]), ip(a[2]), dp(a[3]), dp(a[4]))

    def run(self, slabs, first):
        """`slabs`: fp32 [n][n_points] as the files hold them, n <= max_tp_per_launch; fills nodes first .. first + n - 1.
        Returns once the slabs are on the device; the kernel may still be running."""
        s = np.ascontiguousarray(slabs, np.float32).reshape(-1, self.n_points)
        self._call("run", vp(s), int(s.shape[0]), int(first))

    def run_device(self, slabs_dptr, n, first):
        """the same for n slabs [n][n_points] that stand on the device (LineOpacity.slab_pointer): no upload.  Queued on the
        context's stream behind the kernels that wrote the slabs; returns at once"""
        self.ctx.check(self._l.hx_kt_run_device(self.handle, slabs_dptr, int(n), int(first)), "hx_kt_run_device")

    def regrid(self, temp_old, press_old, temp_new, press_new):
        assert len(temp_old) * len(press_old) == self.n_tp
        plan = regrid_args(temp_old, press_old, temp_new, press_new)
        self._call("regrid", len(temp_old), len(press_old), len(temp_new), len(press_new), *plan)
        self.ip_nodes = len(temp_new) * len(press_new)

    def _results(self):
        nc = self.n_bins * self.n_gauss
        return {"kpoints": self.n_tp * nc, "kpoints_ip": self.ip_nodes * nc, "timing_ms": 4}


# ---- one species ----------------------------------------------------------------------------------------------------------
def read_text_file(path):
    """second column of a HELIOS-K text file, as the fp32 HELIOS-K computes in"""
    vals = []
    with open(path) as f:
        for line in f:
            col = line.split()
            if col:
                vals.append(float(col[1]))
    return np.asarray(vals, np.float32)


class SpeciesFiles(object):
    """what the file names of one directory say: chunk limits, temperatures, pressure codes in ascending pressure"""

    def __init__(self, path, heliosk_format="binary"):
        if heliosk_format in ("binary", "bin"):
            self.ending = ".bin"
        elif heliosk_format in ("text", "dat"):
            self.ending = ".dat"
        else:
            raise IOError("ktable: unknown HELIOS-K output format %r (binary or text)" % (heliosk_format,))
        self.path = path if path.endswith("/") else path + "/"
        files = sorted(f for f in os.listdir(self.path) if "Out_" in f and "_cbin" not in f and self.ending in f)
        if not files:
            raise TypeError("ktable: no %s files in %s; check the HELIOS-K output format" % (self.ending, self.path))
        table = pressure_table()
        parsed = [parse_file_name(f) for f in files]
        self.file_name = parsed[0][0]
        for f, p in zip(files, parsed):
            if p[4] not in table:
                raise IOError("ktable: pressure code %r of %s is not in the table (n800 ... p400)" % (p[4], f))
        self.numin = sorted(set(p[1] for p in parsed))
        self.numax = sorted(set(p[2] for p in parsed))
        self.temps = sorted(set(p[3] for p in parsed))
        self.press = sorted(set(table[p[4]] for p in parsed))
        code_of = {}
        for code, value in table.items():
            code_of.setdefault(value, code)
        self.codes = [code_of[p] for p in self.press]
        if self.numin[0] != 0:
            raise IOError("ktable: the first chunk starts at %d cm^-1, not at 0: the reference's wavelength axis and opacity "
                          "axis are then one point apart, and there is no result to be faithful to" % self.numin[0])
        if len(self.numin) != len(self.numax):
            raise IOError("ktable: chunk limits of %s do not pair up" % self.path)

    def chunk_path(self, n, temp, code):
        stem = "Out_" if self.file_name is None else "Out_%s_" % self.file_name
        return "%s%s%05d_%05d_%05d_%s%s" % (self.path, stem, self.numin[n], self.numax[n], temp, code, self.ending)

    def read_chunk(self, n, temp, code):
        p = self.chunk_path(n, temp, code)
        return np.fromfile(p, np.float32) if self.ending == ".bin" else read_text_file(p)

    def resolution(self):
        return (self.numax[0] - self.numin[0]) / len(self.read_chunk(0, self.temps[0], self.codes[0]))

    def read_point(self, temp, code, resolution):
        chunks = []
        for n in range(len(self.numin)):
            c = self.read_chunk(n, temp, code)
            if len(c) == 0 or (self.numax[n] - self.numin[n]) / len(c) != resolution:
                raise IOError("ktable: %s holds %d points, which is not the resolution %g cm^-1 of the first file"
                              % (self.chunk_path(n, temp, code), len(c), resolution))
            chunks.append(c)
        return np.concatenate(chunks)


class FileSlabs(object):
    """where build_table's slabs come from: the files of one directory.  A source has the nodes (`temps`, `press`, ascending,
    node = p + np * t), `axis()` = (numin of the first chunk, numax of the last, the step between points), `host_slabs` for the
    numpy backend, `feed` for the device and `close`"""

    def __init__(self, path, heliosk_format="binary"):
        self.files = SpeciesFiles(path, heliosk_format)
        self.temps, self.press = self.files.temps, self.files.press
        self.points = [(t, c) for t in self.files.temps for c in self.files.codes]          # node = p + np * t

    def axis(self):
        self.res = self.files.resolution()
        return self.files.numin[0], self.files.numax[-1], self.res

    def read(self, k, n_points):
        s = self.files.read_point(self.points[k][0], self.points[k][1], self.res)
        if len(s) != n_points:
            raise IOError("ktable: %d opacity points for %d wavenumbers at T = %d, %s" % (len(s), n_points, self.points[k][0],
                                                                                           self.points[k][1]))
        return s

    def host_slabs(self, pool, n_points):
        return pool.map(lambda k: self.read(k, n_points), range(len(self.points)))

    def feed(self, b, pool, n_points):
        # the files of batch n + 1 are read while the kernel of batch n runs; the upload itself is not overlapped
        ntp = len(self.points)
        batches = [range(f, min(f + b.max_tp, ntp)) for f in range(0, ntp, b.max_tp)]
        pending = pool.map(lambda r: np.stack([self.read(k, n_points) for k in r]), batches)
        for r, slabs in zip(batches, pending):
            b.run(slabs, r[0])

    def close(self):
        pass


def build_species(path, inter, n_gauss, heliosk_format="binary", backend="hip", ctx=None, tp_per_launch=4,
                  lds_points=LDS_POINTS, target=None, timing=None):
    """datasets of `<name>_opac_kdistr` and, with `target` = (temperatures, pressures), of `<name>_opac_ip_kdistr`"""
    if backend not in ("hip", "numpy"):
        raise IOError("ktable: backend is hip or numpy (got %r)" % (backend,))
    return build_table(FileSlabs(path, heliosk_format), inter, n_gauss, backend, ctx, tp_per_launch, lds_points, target, timing)


def build_table(source, inter, n_gauss, backend="hip", ctx=None, tp_per_launch=4, lds_points=LDS_POINTS, target=None, timing=None):
    """build_species with the slabs of `source`: FileSlabs, or a producer that leaves them on the device (lines.LineSlabs)"""
    inter = np.asarray(inter, np.float64)
    centre, width, yg = grid_datasets(inter, n_gauss)
    numin, numax, res = source.axis()
    lam = spectral_axis(numin, numax, res)
    start, end = bin_ranges(lam, inter)
    check_empty_bins(lam, inter, start, end)
    nx, ny, ntp = len(start), len(yg), len(source.temps) * len(source.press)
    t0 = time.time()

    ip = None
    with ThreadPoolExecutor(max_workers=min(MAX_READERS, max(1, tp_per_launch))) as pool:
        if backend == "numpy":
            k = np.concatenate([numpy_slab(lam, inter, start, end, s, yg).reshape(-1) for s in source.host_slabs(pool, len(lam))])
            if target is not None:
                ip = numpy_regrid(source.press, source.temps, k, target[0], target[1], nx, ny)
        else:
            own = ctx is None
            if own:
                from .device import Context
                ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
            b = None
            try:
                b = KTableBuilder(ctx, len(lam), nx, ny, ntp, tp_per_launch, lds_points)
                b.set_grid(lam, start, end, inter, yg)
                source.feed(b, pool, len(lam))
                k = b.get("kpoints")
                if target is not None:
                    b.regrid(source.temps, source.press, target[0], target[1])
                    ip = b.get("kpoints_ip")
                if timing is not None:
                    timing["device_ms"] = b.get("timing_ms")
            finally:
                if b is not None:
                    b.close()
                source.close()
                if own:
                    ctx.close()
    if timing is not None:
        timing["seconds"], timing["points"], timing["resolution"] = time.time() - t0, ntp, res
    grid = {"interface wavelengths": inter, "center wavelengths": centre, "wavelength width of bins": width, "ypoints": yg}
    native = dict(grid, pressures=np.asarray(source.press, np.float64), temperatures=np.asarray(source.temps, np.float64),
                  kpoints=k)
    if ip is None:
        return native, None
    return native, dict(grid, pressures=np.asarray(target[1], np.float64), temperatures=np.asarray(target[0], np.float64),
                        kpoints=ip)


def write_table(path, datasets):
    """`.npz` or HDF5, chosen as premix.write_premixed_table chooses; returns the path written"""
    from .premix import write_premixed_table
    return write_premixed_table(path, datasets)


# ---- the tool -------------------------------------------------------------------------------------------------------------
def read_species_list(path):
    """header line, then `name path` per species"""
    out = []
    with open(path) as f:
        next(f)
        for line in f:
            col = line.split()
            if col:
                out.append((col[0], col[1]))
    return out


def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="ktable.py", description="species k-tables from HELIOS-K output")
    p.add_argument("-path_to_individual_species_file", default=None)
    p.add_argument("-format", default="k-distribution")
    p.add_argument("-helios_k_output_format", default="binary")
    p.add_argument("-grid_format", default="fixed_resolution")
    p.add_argument("-wavelength_grid", default="50 0.34 200")
    p.add_argument("-path_to_grid_file", default=None)
    p.add_argument("-number_of_gaussian_points", type=int, default=20)
    p.add_argument("-directory_with_individual_files", default="./output/")
    p.add_argument("-interpolate", default="yes", choices=("yes", "no"))
    p.add_argument("-temperature_grid", default=None, help="'first last step' in K, in place of the hard-coded 50 ... 6000")
    p.add_argument("-pressure_grid", default=None, help="'log10 first, log10 last, nodes' in dyne cm^-2, uniform in log10 P")
    p.add_argument("-backend", default="hip", choices=("hip", "numpy"))
    p.add_argument("-points_per_launch", type=int, default=4)
    p.add_argument("-container", default="h5", choices=("h5", "npz"))
    p.add_argument("-continuum_species", default=None, help="analytic containers on the target grid: H- (H-_bf and H-_ff), He-")
    p.add_argument("-rayleigh_species", default=None, help="species of scat_cross_sections: H2, He, H, CO2, CO, O2, N2, e-")
    p.add_argument("-grid_like", default=None, help="an _opac_ip_kdistr container whose grid the analytic tables take")
    p.add_argument("-individual_species_calculation", default=None, choices=("yes", "no"),
                   help="stage 1; by default exactly when -path_to_individual_species_file is given")
    p.add_argument("-mixed_table_production", default="no", choices=("yes", "no"),
                   help="stage 2: mixed_opac_kdistr from the containers of -directory_with_individual_files (ktable_mix.py)")
    p.add_argument("-path_to_final_species_file", default=None)
    p.add_argument("-path_to_fastchem_output", default=None)
    p.add_argument("-mixed_table_output_directory", default="./output/")
    p.add_argument("-units_of_mixed_opacity_table", default="CGS", choices=("CGS", "MKS"))
    p.add_argument("-sweep", default=None, help="\"path_to_fastchem_output=a/,b/\": one mixed table per FastChem directory")
    opt = p.parse_args(argv)
    if opt.individual_species_calculation is None:
        opt.individual_species_calculation = "yes" if opt.path_to_individual_species_file is not None else "no"
    elif opt.individual_species_calculation == "yes" and opt.path_to_individual_species_file is None:
        p.error("-individual_species_calculation yes needs -path_to_individual_species_file")
    if (opt.individual_species_calculation == "no" and opt.continuum_species is None and opt.rayleigh_species is None
            and opt.mixed_table_production != "yes"):
        p.error("one of -path_to_individual_species_file, -continuum_species, -rayleigh_species, -mixed_table_production yes "
                "is required")
    if opt.sweep is not None and opt.mixed_table_production != "yes":
        p.error("-sweep goes with -mixed_table_production yes")
    if opt.format == "sampling":
        raise IOError("ktable: format = sampling is not built; this tool makes k-distribution tables")
    if opt.format != "k-distribution":
        raise IOError("ktable: unknown format %r" % (opt.format,))
    if opt.number_of_gaussian_points < 1:
        raise IOError("ktable: -number_of_gaussian_points is an integer >= 1")
    return opt


def analytic_tables(opt, inter, ctx):
    """-continuum_species and -rayleigh_species: the containers and the Rayleigh file on the grid of -grid_like, or on the
    grid the tool's options define; returns the paths written"""
    from . import continuum
    names = continuum.continuum_species(opt.continuum_species) if opt.continuum_species is not None else []
    rayleigh = continuum.rayleigh_species(opt.rayleigh_species) if opt.rayleigh_species is not None else []
    if opt.grid_like is not None:
        grid = continuum.grid_like(opt.grid_like)
    else:
        grid = continuum.grid_from(inter, opt.number_of_gaussian_points, *target_grid(opt.temperature_grid, opt.pressure_grid))
    out_dir, written, builder = opt.directory_with_individual_files, [], None
    try:
        for name in names:
            t0 = time.time()
            if ctx is not None and builder is None:
                builder = continuum.ContinuumBuilder(ctx, grid["center wavelengths"], len(grid["ypoints"]), grid["temperatures"],
                                                     grid["pressures"])
            data = continuum.build_continuum(name, grid, opt.backend, ctx, builder)
            written.append(write_table("%s_opac_ip_kdistr.%s" % (os.path.join(out_dir, name), opt.container), data))
            print("ktable: %s, %d x %d (T, P) nodes, %d bins x %d Gauss points in %.2f s -> %s"
                  % (name, len(grid["temperatures"]), len(grid["pressures"]), len(grid["center wavelengths"]),
                     len(grid["ypoints"]), time.time() - t0, written[-1]))
    finally:
        if builder is not None:
            builder.close()
    if rayleigh:
        # nbin numbers per species: made on the host whatever the backend, there is no device work in it worth a launch
        path, new, kept = continuum.write_rayleigh_file(out_dir, opt.container, grid["center wavelengths"], rayleigh)
        written.append(path)
        print("ktable: Rayleigh cross-sections of %s -> %s" % (", ".join(new) if new else "no new species", path))
        if kept:
            print("ktable: rayleigh_%s already there, left as %s" % (", rayleigh_".join(kept), "it is" if len(kept) == 1 else
                                                                      "they are"))
    return written


def main(argv=None):
    """ktable.py: one table per species of the list (and its re-gridded twin), then the analytic tables asked for, then the
    mixed table; returns the paths written"""
    opt = parse_args(argv)
    inter = wavelength_grid(opt.grid_format, opt.wavelength_grid.split(), opt.path_to_grid_file)
    target = target_grid(opt.temperature_grid, opt.pressure_grid) if opt.interpolate == "yes" else None
    ctx = None
    stage1, stage2 = opt.individual_species_calculation == "yes", opt.mixed_table_production == "yes"
    if opt.backend == "hip" and (stage1 or opt.continuum_species is not None or stage2):
        from .device import Context
        ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    written = []
    try:
        species = read_species_list(opt.path_to_individual_species_file) if stage1 else []
        for name, path in species:
            timing = {}
            native, ip = build_species(path, inter, opt.number_of_gaussian_points, opt.helios_k_output_format, opt.backend, ctx,
                                       opt.points_per_launch, target=target, timing=timing)
            stem = os.path.join(opt.directory_with_individual_files, name)
            written.append(write_table("%s_opac_kdistr.%s" % (stem, opt.container), native))
            if ip is not None:
                written.append(write_table("%s_opac_ip_kdistr.%s" % (stem, opt.container), ip))
            print("ktable: %s, %d (T, P) points at %g cm^-1 into %d bins x %d Gauss points in %.2f s -> %s"
                  % (name, timing["points"], timing["resolution"], len(inter) - 1, opt.number_of_gaussian_points,
                     timing["seconds"], written[-1]))
        if opt.continuum_species is not None or opt.rayleigh_species is not None:
            written += analytic_tables(opt, inter, ctx)
        if stage2:
            from . import ktable_mix
            written += ktable_mix.run(opt, inter, ctx)
    finally:
        if ctx is not None:
            ctx.close()
    return written
