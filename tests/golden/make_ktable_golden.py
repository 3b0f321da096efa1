"""HELIOS-K directories and what the REFERENCE's k-table tool makes of them (tests/golden/ktable/*.npz).

    /opt/conda/bin/python3.9 tests/golden/make_ktable_golden.py                  # build container only
    /opt/conda/bin/python3.9 tests/golden/make_ktable_golden.py --time-reference # profiles/ktable_reference_time.json

Under the interpreter that has h5py and scipy this script writes small seeded HELIOS-K directories to a temporary place,
imports the reference's `Production` (ktable/source_ktable/build_individual_opacities.py) and `Comb` (combination.py) at run
time -- `pycuda.*` as empty modules, `numba.njit` as the identity where numba does not import -- lets `big_loop` and
`interpolate_opacity_to_final_grid` produce the tables, and stores the fp32 inputs next to the expected outputs.  Data only.

Every case is also computed by a restatement below whose cumulative sums run in `np.longdouble` (64-bit mantissa) and are
rounded once; `eps_ref = max |log10 k_ref - log10 k_restated|` is the reference's own rounding noise, stored per case: the
tests' tolerance is max(1e-13, 8 * eps_ref).

What this measured: from BINARY files the reference takes log10 in SINGLE precision in every bin that holds no floored value.
Its list of opacities then holds numpy float32 scalars only and `log10` keeps their type; one floored value -- a Python float
-- makes the list, and the logarithm, double.  The restatement takes log10 in double everywhere (the contract), so in cases a
and b `eps_ref` is that single-precision noise, a few 1e-7 dex, and not the scan's.  `floored_bins` marks per (T, P) point
the bins where the reference worked in double, and `eps_ref_floored_bins` is eps_ref over those alone: there the tests hold
the product to the scan's noise.  Text files parse to Python floats, so the text twin is double throughout.

  a.npz  fixed-resolution grid (R = 20, 30 - 2000 micron) over two chunks 0 - 100 - 200 cm^-1 at 0.1 cm^-1, 2 x 2 (T, P),
         20 % zeros, a NaN and negative values; the grid starts below the data (fill bins) and ends inside it.  20 Gauss
         points, and 1 and 8.  Plus the re-gridding of the 20-point table onto 5 x 5 nodes below, on, between and above.
  b.npz  grid file with a one-point and a two-point bin, named files, opacities of two significant digits; a text-format
         twin; a grid with an interior empty bin (the expected result is the error)
  c.npz  one bin of 75 000 points and one of 18 000, 0.01 cm^-1 data, one (T, P) point
"""
import json
import os
import shutil
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "ktable")
REF = "/root/reference"
sys.dont_write_bytecode = True


def import_reference():
    for name in ("pycuda", "pycuda.driver", "pycuda.autoinit", "pycuda.gpuarray", "pycuda.compiler"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["pycuda.compiler"].SourceModule = object
    try:
        import numba  # noqa: F401
    except Exception:
        nb = types.ModuleType("numba")
        nb.njit = lambda f=None, **kw: f if f is not None else (lambda g: g)
        nb.jit = nb.njit
        nb.typed = types.SimpleNamespace(List=list)
        sys.modules["numba"] = nb
    # astropy 4.3.1 (the conda env's) lists two numpy functions by name at import time that the env's numpy 1.26 no longer
    # has; it never calls them here
    for gone, fn in (("asscalar", lambda a: a.item()), ("alen", len)):
        if not hasattr(np, gone):
            setattr(np, gone, fn)
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "ktable"))
    from source_ktable import build_individual_opacities as bio
    from source_ktable import combination as comb
    return bio, comb


class Param(object):
    pass


def write_dir(root, files, text=False):
    os.makedirs(root)
    for name, data in files.items():
        if text:
            numin = int(name.split("_")[-4])
            numax = int(name.split("_")[-3])
            nu = numin + (numax - numin) * np.arange(len(data)) / len(data)
            with open(os.path.join(root, name.replace(".bin", ".dat")), "w") as f:
                for n, k in zip(nu, data):
                    f.write("%.5f %.17e\n" % (n, float(k)))      # 17 digits: the fp64 the reference parses IS the fp32
        else:
            np.asarray(data, np.float32).tofile(os.path.join(root, name))


def run_reference(bio, tmp, files, n_gauss, grid=None, interfaces=None, text=False, timing=None):
    import h5py
    d = tempfile.mkdtemp(dir=tmp)
    write_dir(os.path.join(d, "hk"), files, text)
    with open(os.path.join(d, "species.dat"), "w") as f:
        f.write("species path\nXX %s\n" % os.path.join(d, "hk"))
    p = Param()
    p.individual_species_file_path = os.path.join(d, "species.dat")
    p.format, p.n_gauss = "k-distribution", n_gauss
    p.heliosk_format = "text" if text else "binary"
    p.individual_calc_path = os.path.join(d, "out") + "/"
    if grid is not None:
        p.grid_format, p.resolution, p.grid_limits = "fixed_resolution", grid[0], [grid[1], grid[2]]
    else:
        p.grid_format, p.grid_file_path = "file", os.path.join(d, "grid.dat")
        with open(p.grid_file_path, "w") as f:
            f.write("".join("%.17e\n" % v for v in interfaces))
    prod = bio.Production()
    prod.read_individual_species_file(p)
    prod.set_up_press_dict()
    prod.initialize_wavelength_grid(p)
    t0 = time.time()
    prod.big_loop(p)
    if timing is not None:
        timing.append(time.time() - t0)
    with h5py.File(p.individual_calc_path + "XX_opac_kdistr.h5", "r") as f:
        out = {k: np.asarray(f[k][:], np.float64) for k in f.keys()}
    return out, prod


# ---- the restatement: the contract with the scan in extended precision ----------------------------------------------------
def restated_table(chunks_per_point, numin0, numax_last, res, inter, yg):
    nu = np.arange(numin0, numax_last, res)
    lam = np.array([1 / n if n > 0 else 10000.0 for n in nu])[::-1]
    out, floored = [], []
    for chunks in chunks_per_point:
        k = np.concatenate(chunks).astype(np.float32)[::-1].astype(np.float64)
        k = np.array([max(1e-15, v) for v in k])
        for x in range(len(inter) - 1):
            sel = np.nonzero((inter[x] <= lam) & (lam < inter[x + 1]))[0]
            n = len(sel)
            floored.append(n < 2 or bool(np.any(k[sel] == 1e-15)))
            if n == 0:
                out.append(np.full(len(yg), 1e-15))
                continue
            if n == 1:
                out.append(np.full(len(yg), k[sel[0]]))
                continue
            lb, logk = lam[sel], np.log10(k[sel])
            w = np.empty(n)
            w[0] = (lb[0] - inter[x]) + (lb[1] - lb[0]) / 2
            w[1:-1] = (lb[2:] - lb[:-2]) / 2
            w[-1] = (inter[x + 1] - lb[-1]) + (lb[-1] - lb[-2]) / 2
            w /= inter[x + 1] - inter[x]
            order = np.lexsort((w, logk))
            w, logk = w[order], logk[order]
            wl = w.astype(np.longdouble)
            mid = np.empty(n, np.longdouble)
            mid[0] = wl[0] / 2
            mid[1:] = (wl[:-1] + wl[1:]) / 2
            y = np.cumsum(mid).astype(np.float64)
            hi = np.clip(np.searchsorted(y, yg), 1, n - 1)
            lo = hi - 1
            v = (logk[hi] - logk[lo]) / (y[hi] - y[lo]) * (yg - y[lo]) + logk[lo]
            v[yg < y[0]] = logk[0]
            v[yg > y[-1]] = logk[-1]
            out.append(10 ** v)
    return np.concatenate(out), np.array(floored)


def eps_against(ref_k, exact, what):
    """(eps_ref, eps_ref over the bins the reference computed in double, that mask).  Agreement: single-precision log10 of
    |log10 k| <= 15 is off by up to 15 * 2^-24 = 9e-7 at either end of an interval; a misplaced tie moves a value by > 1e-5"""
    exact_k, floored = exact if isinstance(exact, tuple) else (exact, None)
    assert ref_k.shape == exact_k.shape
    dev = np.abs(np.log10(ref_k) - np.log10(exact_k))
    eps = float(dev.max())
    assert eps < 2e-6, (what, eps)
    if floored is None:
        print("%-14s eps_ref = %.3e" % (what, eps))
        return eps
    eps_fl = float(dev.reshape(len(floored), -1)[floored].max())
    assert eps_fl < 1e-9, (what, eps_fl)
    print("%-14s eps_ref = %.3e, over the %d of %d bins computed in double %.3e" % (what, eps, floored.sum(), len(floored),
                                                                                    eps_fl))
    return eps, eps_fl, floored


def store(name, d):
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name)
    np.savez_compressed(path, **d)
    print("wrote %s, %d bytes" % (path, os.path.getsize(path)))


def inputs(files):
    names = sorted(files)
    d = {"files": np.array(names)}
    for i, n in enumerate(names):
        d["data_%d" % i] = np.asarray(files[n], np.float32)
    return d


def expected(d, out, tag=""):
    for k, v in out.items():
        d[k + tag] = v


def chunks_in_order(files, temps, codes, limits, stem="Out_"):
    return [[np.asarray(files["%s%05d_%05d_%05d_%s.bin" % (stem, lo, hi, t, c)], np.float32) for lo, hi in limits]
            for t in temps for c in codes]


def case_a(bio, comb, tmp):
    rng = np.random.default_rng(7101)
    temps, codes, limits = (300, 500), ("n100", "p000"), ((0, 100), (100, 200))       # n100 = 1e5, p000 = 1e6 dyne cm^-2
    files = {}
    for t in temps:
        for c in codes:
            for lo, hi in limits:
                k = (10.0 ** rng.uniform(-8, 2, 1000)).astype(np.float32)
                k[rng.random(1000) < 0.2] = 0.0
                k[rng.integers(0, 1000, 6)] = -1.0e-3
                files["Out_%05d_%05d_%05d_%s.bin" % (lo, hi, t, c)] = k
    files["Out_00100_00200_00300_p000.bin"][17] = np.nan
    grid = (20.0, 30.0, 2000.0)
    d = inputs(files)
    d["wavelength_grid"] = np.array(grid)
    eps = {}
    for ng in (20, 1, 8):
        out, prod = run_reference(bio, tmp, files, ng, grid=grid)
        tag = "" if ng == 20 else "_ng%d" % ng
        expected(d, out, tag)
        exact = restated_table(chunks_in_order(files, temps, codes, limits), 0, 200, 0.1, np.asarray(prod.lamda_int),
                               np.asarray(prod.y_gauss))
        eps["eps_ref" + tag], eps["eps_ref_floored_bins" + tag], eps["floored_bins"] = eps_against(out["kpoints"], exact,
                                                                                                   "a" + tag)
        if ng == 20:
            d["press_codes"] = np.array(sorted(prod.press_dict))
            d["press_values"] = np.array([prod.press_dict[c] for c in sorted(prod.press_dict)])
            k20, nx = out, len(prod.lamda)
    d.update(eps)
    # (g) the re-gridding: nodes below, on, between and above the source's in both axes
    t_new = np.array([200.0, 300.0, 400.0, 500.0, 700.0])
    p_new = np.array([1e4, 1e5, 3e5, 1e6, 1e8])
    ip = comb.Comb.interpolate_opacity_to_final_grid(list(k20["pressures"]), list(k20["temperatures"]), list(k20["kpoints"]),
                                                     t_new, p_new, len(t_new), len(p_new), nx, 20)
    d["regrid_temperatures"], d["regrid_pressures"], d["regrid_kpoints"] = t_new, p_new, np.asarray(ip, np.float64)
    # restated in extended precision
    L = np.longdouble
    k = k20["kpoints"].reshape(2, 2, -1).astype(L)
    T, lp = k20["temperatures"].astype(L), np.log10(k20["pressures"]).astype(L)
    ex = np.empty((5, 5, k.shape[2]), L)
    for i, tn in enumerate(t_new.astype(L)):
        ft = min(max((tn - T[0]) / (T[1] - T[0]), L(0)), L(1))
        for j, pn in enumerate(np.log10(p_new).astype(L)):
            fp = min(max((pn - lp[0]) / (lp[1] - lp[0]), L(0)), L(1))
            ex[i, j] = (k[0, 0] * (1 - ft) * (1 - fp) + k[0, 1] * (1 - ft) * fp + k[1, 0] * ft * (1 - fp) + k[1, 1] * ft * fp)
    d["eps_ref_regrid"] = eps_against(d["regrid_kpoints"], ex.reshape(-1).astype(np.float64), "a regrid")
    store("a.npz", d)


def two_digits(v):
    e = np.floor(np.log10(v))
    return np.round(v / 10 ** e, 1) * 10 ** e


def case_b(bio, tmp):
    rng = np.random.default_rng(7102)
    temps, codes, limits, stem = (300,), ("n100", "p100"), ((0, 50),), "Out_my_mol_01_"
    files = {}
    for c in codes:
        k = two_digits(10.0 ** rng.uniform(-3, 0, 1000)).astype(np.float32)
        k[rng.random(1000) < 0.05] = 0.0
        files["%s00000_00050_00300_%s.bin" % (stem, c)] = k
    # 0.05 cm^-1: nu = 10.00 alone in [1/10.02, 1/9.98), nu = 9.95 and 9.90 in [1/9.98, 1/9.88)
    inter = np.array([0.021, 0.05, 1 / 10.02, 1 / 9.98, 1 / 9.88, 0.5, 3.0])
    d = inputs(files)
    d["interfaces"] = inter
    out, prod = run_reference(bio, tmp, files, 20, interfaces=inter)
    expected(d, out)
    exact = restated_table(chunks_in_order(files, temps, codes, limits, stem), 0, 50, 0.05, inter, np.asarray(prod.y_gauss))
    d["eps_ref"], d["eps_ref_floored_bins"], d["floored_bins"] = eps_against(out["kpoints"], exact, "b")
    # (e) the text twin
    out_t, _ = run_reference(bio, tmp, files, 20, interfaces=inter, text=True)
    d["kpoints_text"] = out_t["kpoints"]
    d["eps_ref_text"] = eps_against(out_t["kpoints"], exact[0], "b text")
    # (d) an interior empty bin: nothing between nu = 10.05 (0.099502 cm) and nu = 10.00 (0.1 cm)
    bad = np.array([0.05, 0.0996, 0.0997, 0.2])
    try:
        run_reference(bio, tmp, files, 20, interfaces=bad)
        raised = "none"
    except IndexError as e:
        raised = "IndexError: " + str(e)
    assert raised.startswith("IndexError") and "finer" in raised, raised
    d["empty_bin_interfaces"], d["empty_bin_error"] = bad, np.array(raised)
    store("b.npz", d)


def case_c(bio, tmp):
    rng = np.random.default_rng(7103)
    k = (10.0 ** rng.uniform(-6, 1, 100000)).astype(np.float32)
    k[rng.random(100000) < 0.15] = 0.0
    files = {"Out_00000_01000_01000_p200.bin": k}
    inter = np.array([1 / 950.0, 1 / 200.0, 1 / 20.0, 0.5, 2.0])       # 75 000, 18 000, 1 800 and 150 points
    d = inputs(files)
    d["interfaces"] = inter
    out, prod = run_reference(bio, tmp, files, 20, interfaces=inter)
    expected(d, out)
    exact = restated_table([[k]], 0, 1000, 0.01, inter, np.asarray(prod.y_gauss))
    d["eps_ref"], d["eps_ref_floored_bins"], d["floored_bins"] = eps_against(out["kpoints"], exact, "c")
    store("c.npz", d)


def time_reference(bio, tmp):
    """big_loop on ONE (T, P) point of tools/ktable_bench.py's synthetic species (0 - 30 000 cm^-1 at 0.01 cm^-1, R = 50 over
    0.34 - 200 micron, 20 Gauss points), on this machine's CPU"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "tools"))
    import ktable_bench
    files = {n: v for n, v in ktable_bench.synthetic_species(1).items()}
    t = []
    run_reference(bio, tmp, files, 20, grid=ktable_bench.GRID, timing=t)
    rec = {"what": "reference big_loop, one (T, P) point of the bench species, incl. reading its files",
           "points": int(sum(len(v) for v in files.values())), "seconds_per_tp_point": t[0],
           "python": sys.version.split()[0], "numpy": np.__version__}
    path = os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "ktable_reference_time.json")
    with open(path, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(rec)


def main():
    bio, comb = import_reference()
    tmp = tempfile.mkdtemp()
    try:
        if "--time-reference" in sys.argv:
            time_reference(bio, tmp)
            return
        case_a(bio, comb, tmp)
        case_b(bio, tmp)
        case_c(bio, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
