"""Mie tables of an aerosol from its optical constants, on the device (include/helios_hip.h section 10, csrc/mie.hip).

A cloudy run reads one directory per aerosol: the 51 files `r{radius:.6f}.dat` on the radius grid `clouds.R_VALUES`, which the
reference takes from LX-MIE, a separate program.  This tool makes the directory from a table of n(lambda), k(lambda).

Input.  A text file with the columns wavelength [micron], n, k; lines that start with `#` and the first `-header_lines N` lines
are skipped.  The refractive index is m = n + i k with k >= 0 (Bohren & Huffman's convention).  Refused, with the offending line:
n <= 0 or k < 0, wavelengths that do not strictly ascend, fewer than two rows, numbers that are not finite.

Wavelengths.  The table takes the file's own wavelengths, or -- `-wavelength_grid "nw lo hi"` -- nw wavelengths spaced evenly in
log lambda between lo and hi micron, with n and k interpolated linearly in log10 lambda.  A wavelength outside the file is refused;
nothing is extrapolated.

Per (radius, wavelength) pair.  x = 2 pi r / lambda; the series of a_n, b_n is truncated at N = floor(x + 4.05 x^(1/3) + 2);
    Q_ext = 2/x^2 sum (2n+1) Re(a_n + b_n),      Q_sca = 2/x^2 sum (2n+1) (|a_n|^2 + |b_n|^2),
    g = 4/(x^2 Q_sca) sum [ n(n+2)/(n+1) Re(a_n a*_{n+1} + b_n b*_{n+1}) + (2n+1)/(n(n+1)) Re(a_n b*_n) ]     (a_{N+1} = b_{N+1} = 0),
    Q_abs = max(Q_ext - Q_sca, 0), and where k = 0 exactly Q_abs = 0 and Q_sca = Q_ext (the cloud path re-bins absorption in its log
    mode: a 0 stays a finite 0 there, a negative value becomes NaN).
Cross-sections are C = Q pi r^2 in cm^2 with r in cm.  D_n(m x), the logarithmic derivative of psi_n, starts at n = N from Lentz's
continued fraction and is taken downward; psi_n and chi_n go upward from sin x and cos x.  No sin, cos or exp of the complex m x is
taken (with k = 1 and x = 2e4 they overflow).

Small x.  psi_1 = sin x / x - cos x is the difference of two numbers near 1 and keeps 3 eps / x^2 of relative error, which Q_sca and
g inherit several times over (fp64: 2.4e-13 at x = 0.1, 1.9e-8 in Q_sca and g = -1.7e-8 at x = 1e-4).  Below X_SMALL = 0.5 every
psi_n, n >= 1, is therefore taken from its ascending series x^(n+1)/(2n+1)!! (1 - x^2/(2(2n+3)) + ...), SERIES_TERMS = 10 terms in
Horner form, which has no cancellation; chi_n, the dominant solution, keeps its recurrence.  The branch is taken on the double x.

Output.  `-output_directory DIR` receives the files `r{:.6f}.dat` of clouds.R_VALUES: one header line and the columns wavelength
[micron], size parameter, C_ext, C_sca, C_abs, single-scattering albedo (1 where C_ext is 0), g, each with 17 significant digits,
so that Cloud.read_mie_file returns the computed doubles.  The tool prints the wavelength range it covers: opacity bins with an
interface outside that range get no cloud opacity (tools.convert_spectrum's rule).

`backend="device"` runs k_mie: one thread per pair, the pairs sorted by N, descending, the D_n in a bounded device buffer
(SCRATCH_BYTES, 256 MB) that the sorted pairs pass through in as many launches as needed; a single pair whose D_n do not fit is
refused with its radius, wavelength and byte count before anything is launched.  `backend="numpy"` computes the same contract
vectorised over the pairs in fp64: the checker of the device path, and what a machine without a GPU gets when it asks for it.
"""
import argparse
import os
import time

import numpy as np

from ._tool import DeviceObject, dp, ip
from .clouds import R_VALUES

X_SMALL = 0.5
SERIES_TERMS = 10
LENTZ_TOL_EPS = 16
TINY = 1e-30
SCRATCH_BYTES = 256 << 20
ENTRY_BYTES = 16                      # one complex D_n
MIE_FILE = "r{:.6f}.dat"              # clouds.py reads this name per radius of R_VALUES
HEADER = "# wavelength[micron] size_parameter C_ext[cm^2] C_sca[cm^2] C_abs[cm^2] albedo g_0"


def n_terms(x):
    x = np.asarray(x, np.float64)
    return np.floor(x + 4.05 * x ** (1.0 / 3.0) + 2.0).astype(np.int64)


def _check_pairs(x, m_re, m_im):
    x, m_re, m_im = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (x, m_re, m_im))
    if not (len(x) == len(m_re) == len(m_im)) or len(x) == 0:
        raise ValueError("mie: x, m_re and m_im are arrays of one length >= 1")
    for name, a, ok in (("x", x, x > 0), ("m_re", m_re, m_re > 0), ("m_im", m_im, m_im >= 0)):
        bad = ~(ok & np.isfinite(a))
        if bad.any():
            p = int(np.argmax(bad))
            raise ValueError("mie: pair %d: %s = %r is not a finite number %s 0" % (p, name, float(a[p]), ">=" if name == "m_im" else ">"))
    return x, m_re, m_im


# ---- the contract in numpy ------------------------------------------------------------------------------------------------
def _crec(br, bi):
    d = br * br + bi * bi
    return br / d, -bi / d


def _cdiv(ar, ai, br, bi):
    d = br * br + bi * bi
    return (ar * br + ai * bi) / d, (ai * br - ar * bi) / d


def _psi_series(n, x):
    s = np.ones_like(x)
    x2 = x * x
    for k in range(SERIES_TERMS, 0, -1):
        s = 1.0 - x2 / float(2 * k * (2 * n + 2 * k + 1)) * s
    pref = x
    for j in range(1, n + 1):
        pref = pref * x / float(2 * j + 1)
    return pref * s


def _lentz_start(N, zinv_r, zinv_i, cap):
    """D_N(z) per pair: J_{nu-1}(z) / J_nu(z) = a_1 + 1 / (a_2 + 1 / (a_3 + ...)), nu = N + 1/2, a_k = (-1)^(k+1) (2N + 2k - 1) / z,
    by the modified Lentz algorithm; the pairs that have converged leave the arrays"""
    tol = LENTZ_TOL_EPS * np.finfo(np.float64).eps
    P = len(N)
    out_r, out_i = np.empty(P), np.empty(P)
    act = np.arange(P)
    n2 = 2.0 * N.astype(np.float64)
    zr, zi, kcap = zinv_r.copy(), zinv_i.copy(), cap.copy()
    fr, fi = (n2 + 1.0) * zr, (n2 + 1.0) * zi
    fr = np.where((fr == 0.0) & (fi == 0.0), TINY, fr)
    Cr, Ci, Dr, Di = fr.copy(), fi.copy(), np.zeros(P), np.zeros(P)
    k, sign = 2, -1.0
    while len(act):
        c = sign * (n2 + float(2 * k - 1))
        ar, ai = c * zr, c * zi
        Dr, Di = ar + Dr, ai + Di
        Dr = np.where((Dr == 0.0) & (Di == 0.0), TINY, Dr)
        Dr, Di = _crec(Dr, Di)
        tr, ti = _crec(Cr, Ci)
        Cr, Ci = ar + tr, ai + ti
        Cr = np.where((Cr == 0.0) & (Ci == 0.0), TINY, Cr)
        dr, di = Cr * Dr - Ci * Di, Cr * Di + Ci * Dr
        fr, fi = fr * dr - fi * di, fr * di + fi * dr
        done = (np.abs(dr - 1.0) + np.abs(di) < tol) | (k >= kcap)
        if done.any():
            out_r[act[done]], out_i[act[done]] = fr[done], fi[done]
            keep = ~done
            act, n2, zr, zi, kcap = act[keep], n2[keep], zr[keep], zi[keep], kcap[keep]
            fr, fi, Cr, Ci, Dr, Di = fr[keep], fi[keep], Cr[keep], Ci[keep], Dr[keep], Di[keep]
        k, sign = k + 1, -sign
    Nf = N.astype(np.float64)
    return out_r - Nf * zinv_r, out_i - Nf * zinv_i


def numpy_series(x, m_re, m_im):
    """(Q_ext, Q_sca, g) per pair, fp64, the statements of csrc/mie.hip vectorised over the pairs: they are sorted by N,
    descending, so that the pairs still in the loop at term n are a prefix"""
    x, m_re, m_im = _check_pairs(x, m_re, m_im)
    P = len(x)
    N_in = n_terms(x)
    order = np.argsort(-N_in, kind="stable")
    xs, mr, mi, N = x[order], m_re[order], m_im[order], N_in[order]
    zinv_r, zinv_i = _crec(mr * xs, mi * xs)
    minv_r, minv_i = _crec(mr, mi)
    zabs = np.sqrt(mr * mr + mi * mi) * xs
    cap = (zabs + 4.05 * zabs ** (1.0 / 3.0)).astype(np.int64) + 100
    cur_r, cur_i = _lentz_start(N, zinv_r, zinv_i, cap)
    n_max = int(N[0])
    count = np.searchsorted(-N, -np.arange(n_max + 2), side="right")       # count[n]: pairs with N >= n
    levels = [None] * (n_max + 1)
    for n in range(n_max, 1, -1):
        c = count[n]
        dr, di = cur_r[:c], cur_i[:c]
        levels[n] = (dr.copy(), di.copy())
        tr, ti = float(n) * zinv_r[:c], float(n) * zinv_i[:c]
        ir, ii = _crec(dr + tr, di + ti)
        cur_r[:c], cur_i[:c] = tr - ir, ti - ii
    levels[1] = (cur_r, cur_i)
    small = xs < X_SMALL
    n_small = int(N[small].max()) if small.any() else 0
    sx, cx = np.sin(xs), np.cos(xs)
    psi0, chi0 = sx.copy(), cx.copy()
    psi1 = sx / xs - cx
    psi1[small] = _psi_series(1, xs[small])
    chi1 = cx / xs + sx
    s_ext, s_sca, s_g = np.zeros(P), np.zeros(P), np.zeros(P)
    a_pr, a_pi, b_pr, b_pi = np.zeros(P), np.zeros(P), np.zeros(P), np.zeros(P)
    for n in range(1, n_max + 1):
        c = count[n]
        xc = xs[:c]
        if n >= 2:
            f = float(2 * n - 1) / xc
            psi = f * psi1[:c] - psi0[:c]
            if n <= n_small:
                sm = small[:c]
                psi[sm] = _psi_series(n, xc[sm])
            chi = f * chi1[:c] - chi0[:c]
            psi0[:c], chi0[:c] = psi1[:c], chi1[:c]
            psi1[:c], chi1[:c] = psi, chi
        p1, p0, c1, c0 = psi1[:c], psi0[:c], chi1[:c], chi0[:c]
        nx = float(n) / xc
        dr, di = levels[n]
        ur, ui = dr * minv_r[:c] - di * minv_i[:c] + nx, dr * minv_i[:c] + di * minv_r[:c]
        ar, ai = _cdiv(ur * p1 - p0, ui * p1, ur * p1 + ui * c1 - p0, ui * p1 - ur * c1 + c0)
        ur, ui = mr[:c] * dr - mi[:c] * di + nx, mr[:c] * di + mi[:c] * dr
        br, bi = _cdiv(ur * p1 - p0, ui * p1, ur * p1 + ui * c1 - p0, ui * p1 - ur * c1 + c0)
        f = float(2 * n + 1)
        s_ext[:c] = s_ext[:c] + f * (ar + br)
        s_sca[:c] = s_sca[:c] + f * ((ar * ar + ai * ai) + (br * br + bi * bi))
        if n >= 2:
            s_g[:c] = s_g[:c] + float((n - 1) * (n + 1)) / float(n) * ((a_pr[:c] * ar + a_pi[:c] * ai) + (b_pr[:c] * br + b_pi[:c] * bi))
        s_g[:c] = s_g[:c] + f / float(n * (n + 1)) * (ar * br + ai * bi)
        a_pr[:c], a_pi[:c], b_pr[:c], b_pi[:c] = ar, ai, br, bi
        levels[n] = None
    q = 2.0 / (xs * xs)
    out = [np.empty(P), np.empty(P), np.empty(P)]
    for o, v in zip(out, (q * s_ext, q * s_sca, 2.0 * s_g / s_sca)):
        o[order] = v
    return tuple(out)


# ---- device ---------------------------------------------------------------------------------------------------------------
class MieSeries(DeviceObject):
    """hx_mie: up to n_pairs_max pairs per run through a D buffer of scratch_bytes"""

    PREFIX = "hx_mie"
    GUARD = 0x7ff8dead0badbeef

    def __init__(self, ctx, n_pairs_max, scratch_bytes=None):
        self.n_pairs_max = int(n_pairs_max)
        self.scratch_bytes = SCRATCH_BYTES if scratch_bytes is None else int(scratch_bytes)
        self.n_pairs = 0
        self._create(ctx, self.n_pairs_max, self.scratch_bytes)

    def run(self, x, m_re, m_im, order=None):
        """`order`: the sequence in which the pairs are dealt to lanes; None: by N, descending"""
        x, m_re, m_im = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (x, m_re, m_im))
        assert len(x) == len(m_re) == len(m_im)
        if order is None:
            with np.errstate(invalid="ignore"):
                order = np.argsort(-n_terms(np.where(x > 0, x, 1.0)), kind="stable")
        order = np.ascontiguousarray(order, np.int32)
        assert len(order) == len(x)
        self._call("run", len(x), dp(x), dp(m_re), dp(m_im), ip(order))
        self.n_pairs = len(x)

    def _results(self):
        return {"guard": (5, np.uint64), "timing_ms": 2, "q_ext": self.n_pairs, "q_sca": self.n_pairs, "g": self.n_pairs}

    def guards_intact(self):
        return bool(np.all(self.get("guard") == np.uint64(self.GUARD)))

def device_series(x, m_re, m_im, ctx=None, scratch_bytes=None, order=None, timing=None):
    """(Q_ext, Q_sca, g) per pair from k_mie"""
    x, m_re, m_im = _check_pairs(x, m_re, m_im)
    own = ctx is None
    if own:
        from .device import Context
        ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    try:
        s = MieSeries(ctx, len(x), scratch_bytes)
        try:
            s.run(x, m_re, m_im, order)
            out = s.get("q_ext"), s.get("q_sca"), s.get("g")
            if not s.guards_intact():
                raise RuntimeError("mie: a guard word behind the device arrays was overwritten")
            if timing is not None:
                t = s.get("timing_ms")
                timing.update(kernel_ms=float(t[0]), launches=int(t[1]))
        finally:
            s.close()
    finally:
        if own:
            ctx.close()
    return out


# ---- the table ------------------------------------------------------------------------------------------------------------
def mie_table(lam_um, n, k, radii_um=R_VALUES, backend="device", ctx=None, scratch_bytes=None, timing=None):
    """the Mie table of one material: dict(size, ext, scat, absorb, g), each [radius][wavelength]; cross-sections in cm^2.
    `lam_um`, `n`, `k`: arrays of one length; `radii_um`: any radii, in any order"""
    if backend not in ("device", "numpy"):
        raise ValueError("mie: backend is device or numpy (got %r)" % (backend,))
    lam, n, k = (np.ascontiguousarray(a, np.float64).reshape(-1) for a in (lam_um, n, k))
    radii = np.ascontiguousarray(radii_um, np.float64).reshape(-1)
    if not (len(lam) == len(n) == len(k)) or len(lam) == 0 or len(radii) == 0:
        raise ValueError("mie: wavelengths, n and k are arrays of one length, and there is at least one radius")
    for name, a in (("wavelength", lam), ("radius", radii)):
        if not np.all(np.isfinite(a) & (a > 0)):
            raise ValueError("mie: every %s is a finite number > 0" % name)
    t0 = time.time()
    size = 2.0 * np.pi * radii[:, None] / lam[None, :]
    shape = size.shape
    x = size.reshape(-1)
    m_re, m_im = np.broadcast_to(n, shape).reshape(-1), np.broadcast_to(k, shape).reshape(-1)
    x, m_re, m_im = _check_pairs(x, m_re, m_im)
    if backend == "device":
        cap = SCRATCH_BYTES if scratch_bytes is None else int(scratch_bytes)
        need = (n_terms(x) + 1) * ENTRY_BYTES
        if need.max() > cap:
            p = int(np.argmax(need))
            raise ValueError("mie: the pair r = %.17g micron, lambda = %.17g micron (x = %.6g) needs %d bytes for its D_n, the "
                             "buffer holds %d; nothing was launched" % (radii[p // shape[1]], lam[p % shape[1]], x[p], need[p], cap))
        q_ext, q_sca, g = device_series(x, m_re, m_im, ctx, scratch_bytes, timing=timing)
    else:
        q_ext, q_sca, g = numpy_series(x, m_re, m_im)
    geo = (np.pi * (radii * 1e-4) ** 2)[:, None]
    lossless = (np.broadcast_to(k, shape) == 0.0)
    q_ext, q_sca, g = q_ext.reshape(shape), q_sca.reshape(shape), g.reshape(shape)
    q_sca = np.where(lossless, q_ext, q_sca)
    q_abs = np.where(lossless, 0.0, np.maximum(q_ext - q_sca, 0.0))
    if timing is not None:
        timing["seconds"] = time.time() - t0
    return dict(size=size, ext=q_ext * geo, scat=q_sca * geo, absorb=q_abs * geo, g=g)


# ---- files ----------------------------------------------------------------------------------------------------------------
def read_refractive_index_file(path, header_lines=0):
    """(wavelengths [micron], n, k) of a text file with these three columns"""
    lam, n, k = [], [], []
    with open(path) as f:
        for nr, line in enumerate(f, 1):
            if nr <= int(header_lines) or line.startswith("#") or not line.strip():
                continue
            where = "line %d of %s (%r)" % (nr, path, line.rstrip("\n"))
            col = line.split()
            try:
                v = [float(c) for c in col[:3]]
            except ValueError:
                v = []
            if len(v) < 3:
                raise IOError("mie: %s does not hold wavelength, n and k" % where)
            if not np.all(np.isfinite(v)):
                raise IOError("mie: %s holds a number that is not finite" % where)
            if v[1] <= 0 or v[2] < 0:
                raise IOError("mie: %s: n > 0 and k >= 0 are required (m = n + i k)" % where)
            if not v[0] > 0 or (lam and not v[0] > lam[-1]):
                raise IOError("mie: %s: the wavelengths are > 0 and strictly ascending" % where)
            lam.append(v[0]); n.append(v[1]); k.append(v[2])
    if len(lam) < 2:
        raise IOError("mie: %s holds fewer than two rows of wavelength, n and k" % path)
    return np.array(lam), np.array(n), np.array(k)


def wavelength_grid(spec, lam_file, n_file, k_file):
    """`spec` = "nw lo hi": nw wavelengths evenly spaced in log lambda from lo to hi micron, with n and k interpolated linearly in
    log10 lambda; a node outside the file is refused"""
    part = str(spec).split()
    try:
        nw, lo, hi = int(part[0]), float(part[1]), float(part[2])
        ok = len(part) == 3 and nw >= 2 and 0 < lo < hi and np.isfinite(hi)
    except (ValueError, IndexError):
        ok = False
    if not ok:
        raise IOError("mie: -wavelength_grid is \"nw lo hi\" with nw >= 2 and 0 < lo < hi micron (got %r)" % (spec,))
    lam = 10.0 ** (np.log10(lo) + np.arange(nw) * ((np.log10(hi) - np.log10(lo)) / (nw - 1)))
    lam[0], lam[-1] = lo, hi
    outside = (lam < lam_file[0]) | (lam > lam_file[-1])
    if outside.any():
        raise IOError("mie: the wavelength %.17g micron of -wavelength_grid lies outside the file's %.17g ... %.17g micron; nothing "
                      "is extrapolated" % (lam[int(np.argmax(outside))], lam_file[0], lam_file[-1]))
    log_file, log_new = np.log10(lam_file), np.log10(lam)
    n, k = np.interp(log_new, log_file, n_file), np.interp(log_new, log_file, k_file)
    for j in np.nonzero(np.isin(lam, lam_file))[0]:           # a node on a file wavelength takes the file's values as they are
        i = int(np.searchsorted(lam_file, lam[j]))
        n[j], k[j] = n_file[i], k_file[i]
    return lam, n, k


def write_mie_directory(directory, lam_um, radii_um, table):
    """one file per radius, named as clouds.py reads them; returns the paths"""
    os.makedirs(directory, exist_ok=True)
    paths = []
    for j, r in enumerate(radii_um):
        ext, scat, absorb = table["ext"][j], table["scat"][j], table["absorb"][j]
        with np.errstate(divide="ignore", invalid="ignore"):
            albedo = np.where(ext == 0.0, 1.0, scat / ext)
        rows = np.stack([lam_um, table["size"][j], ext, scat, absorb, albedo, table["g"][j]], 1)
        paths.append(os.path.join(directory, MIE_FILE.format(r)))
        with open(paths[-1], "w") as f:
            f.write(HEADER + "\n")
            for row in rows:
                f.write(" ".join("%.16e" % v for v in row) + "\n")
    return paths


# ---- the tool -------------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="mie.py", description="Mie tables of an aerosol from its optical constants")
    p.add_argument("-refractive_index_file", required=True)
    p.add_argument("-output_directory", required=True)
    p.add_argument("-header_lines", type=int, default=0)
    p.add_argument("-wavelength_grid", default=None)
    p.add_argument("-backend", default="device", choices=("device", "numpy"))
    p.add_argument("-scratch_bytes", type=int, default=None)
    return p.parse_args(argv)


def main(argv=None):
    """mie.py: the directory of one aerosol; returns its path"""
    opt = parse_args(argv)
    t0 = time.time()
    lam, n, k = read_refractive_index_file(opt.refractive_index_file, opt.header_lines)
    if opt.wavelength_grid is not None:
        lam, n, k = wavelength_grid(opt.wavelength_grid, lam, n, k)
    timing = {}
    table = mie_table(lam, n, k, R_VALUES, opt.backend, scratch_bytes=opt.scratch_bytes, timing=timing)
    directory = os.path.join(str(opt.output_directory), "")
    write_mie_directory(directory, lam, R_VALUES, table)
    how = "numpy" if opt.backend == "numpy" else "k_mie %.1f ms in %d launch%s" % (
        timing["kernel_ms"], timing["launches"], "" if timing["launches"] == 1 else "es")
    print("mie: %d radii x %d wavelengths, %d terms in all, %s, %.2f s -> %s" % (
        len(R_VALUES), len(lam), int(n_terms(table["size"]).sum()), how, time.time() - t0, directory))
    print("mie: the table covers %.6g ... %.6g micron.  WARNING: opacity bins with an interface outside this range get no cloud "
          "opacity" % (lam[0], lam[-1]))
    return directory
