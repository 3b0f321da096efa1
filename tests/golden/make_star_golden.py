"""Synthetic stellar inputs and what the REFERENCE's star tool makes of them (tests/golden/star/).

    /opt/conda/bin/python3.9 tests/golden/make_star_golden.py

Run once under the interpreter that has numpy 1.26, astropy and h5py.  The script writes small seeded inputs with astropy --
a PHOENIX-like directory (a wavelength file in Angstrom, fp32 corner files `TTTTT_G.GG_M.M.fits`), an ASCII spectrum, a
MUSCLES-like BINTABLE file and a BT-Settl-like two-row image -- and two opacity-grid containers, imports the reference's
`star_tool/functions.py` and `source/tools.py` at run time with `wget`, `matplotlib` and `pycuda` as empty stand-in modules (no
code path can download anything, and every file the reference looks for exists in the temporary working directory), calls
`interpol_phoenix_spectrum`, the three file readers, `convert_spectrum` and `calc_analyt_planck_in_interval` directly, and
lets `main_loop` run in its automatic mode with the plot and the question on the terminal answered by stand-ins; the
temperatures it hands to the Planck function are recorded, the last of which is the fitted one.  The reference's constants
lack the parsec its MUSCLES reader asks for; astropy's value is set on the module before the call.  Data only: inputs under
tests/golden/star/, results in tests/golden/star/reference.npz.

Blend cases: all eight branches, T_eff on and around the 7000 K change of spacing, [M/H] = -2 and 1, and [M/H] = -0.3, whose
upper node the reference spells `-0.0`.
"""
import builtins
import os
import shutil
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "star")
REF = "/root/reference"
WAVE = "WAVE_PHOENIX-ACES-AGSS-COND-2011.fits"
N = 1500
sys.dont_write_bytecode = True

BLEND_CASES = {            # name: (T_eff, log g, [M/H])
    "full": (3026, 4.944, 0.39), "all_nodes": (3000, 5.0, 0.5), "tg_nodes": (3000, 5.0, 0.39), "tm_nodes": (3000, 4.944, 0.5),
    "m_node": (3026, 4.944, 0.5), "g_node": (3026, 5.0, 0.39), "t_node": (3000, 4.944, 0.39),
    "t7000": (7000, 4.2, -0.3), "t6950": (6950, 4.2, -0.3), "t7100": (7100, 4.2, -0.3),
    "m_low": (3026, 4.944, -2.0), "m_high": (3026, 4.944, 1.0),
}


def numpy_names_for_astropy():
    # astropy 4.3.1 lists two numpy functions by name at import time that numpy 1.26 no longer has; it never calls them here
    for gone, fn in (("asscalar", lambda a: a.item()), ("alen", len)):
        if not hasattr(np, gone):
            setattr(np, gone, fn)


def import_reference():
    for name in ("wget", "matplotlib", "matplotlib.pyplot", "pycuda", "pycuda.driver", "pycuda.autoinit", "pycuda.gpuarray",
                 "pycuda.compiler"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.path.insert(0, REF)
    sys.path.insert(0, os.path.join(REF, "star_tool"))
    import functions as fc
    from source import tools as tls
    from source import phys_const
    if not hasattr(phys_const, "PC"):
        # the reference's MUSCLES reader asks its constants for a parsec that they do not define (it fails as it stands);
        # astropy's value stands in, in the units of the other constants
        from astropy import constants
        phys_const.PC = constants.pc.cgs.value
    return fc, tls


class _Anything(object):
    """stands in for a figure, an axis and a legend: takes every call"""
    legendHandles = ()

    def __getattr__(self, name):
        return lambda *a, **k: _Anything()


def nodes(teff, log_g, metal):
    step = 100 if teff < 7000 else 200
    t = sorted(set([int(step * np.floor(teff / step)), int(step * np.ceil(teff / step))]))
    g = sorted(set([0.5 * np.floor(log_g / 0.5), 0.5 * np.ceil(log_g / 0.5)]))
    m = [0.5 * np.floor(metal / 0.5), 0.5 * np.ceil(metal / 0.5)]
    return [(a, b, c) for a in t for b in g for c in m]


def corner_file_name(t, g, m):
    return "{:05d}_{:.2f}_{:.1f}.fits".format(t, g, m)


def corner_spectrum(lam_cm, t, g, m, rng):
    """a black body with lines: smooth in the parameters, rough in wavelength, fp32 as the PHOENIX files are"""
    x = 1.4387769 / (lam_cm * t)
    planck = 3.7417718e-5 / lam_cm ** 5 / np.expm1(np.minimum(x, 600.0))
    lines = 1.0 - 0.6 * rng.random(len(lam_cm)) ** 3 * (1.0 + 0.1 * m) * (1.0 + 0.02 * g)
    return (planck * lines).astype(np.float32)


def write_inputs():
    from astropy.io import fits
    if os.path.isdir(OUT):
        shutil.rmtree(OUT)
    os.makedirs(os.path.join(OUT, "phoenix"))
    rng = np.random.default_rng(20221018)
    lam_A = np.sort(500.0 * (55000.0 / 500.0) ** np.sort(rng.random(N)))
    lam_A[0], lam_A[-1] = 500.0, 55000.0
    fits.PrimaryHDU(lam_A.astype(np.float64)).writeto(os.path.join(OUT, "phoenix", WAVE))
    lam_cm = lam_A * 1e-8
    written = set()
    for t_eff, log_g, metal in BLEND_CASES.values():
        for t, g, m in nodes(t_eff, log_g, metal):
            name = corner_file_name(t, g, m)
            if name not in written:
                seed = abs(hash((t, round(g * 2), round(m * 2)))) % (2 ** 31)
                spec = corner_spectrum(lam_cm, t, g, float(m) + 0.0, np.random.default_rng(seed))
                fits.PrimaryHDU(spec).writeto(os.path.join(OUT, "phoenix", name))
                written.add(name)
    # ASCII: eight header lines, nm and W m^-2 nm^-1 at 1 au as the solar file of the reference's example has them
    lam_nm = np.linspace(280.0, 4000.0, 400)
    f_sun = 2.0 * np.exp(-((lam_nm - 500.0) / 900.0) ** 2) + 0.01
    with open(os.path.join(OUT, "sun_like.txt"), "w") as f:
        for k in range(8):
            f.write("# header line %d\n" % (k + 1))
        for l, v in zip(lam_nm, f_sun):
            f.write("%.4f  %.6e\n" % (l, v))
    # MUSCLES-like: a BINTABLE in HDU 1, Angstrom and erg s^-1 cm^-2 A^-1 at Earth; one flux value is exactly 0
    lam_m = np.linspace(1000.0, 54000.0, 600)
    f_m = (1e-14 * np.exp(-((lam_m - 9000.0) / 8000.0) ** 2) + 1e-17).astype(np.float64)
    f_m[300] = 0.0
    cols = [fits.Column(name="WAVELENGTH", format="D", array=lam_m), fits.Column(name="FLUX", format="D", array=f_m),
            fits.Column(name="ERROR", format="E", array=(0.1 * f_m).astype(np.float32)),
            fits.Column(name="EXPTIME", format="J", array=np.arange(600, dtype=np.int32))]
    fits.HDUList([fits.PrimaryHDU(), fits.BinTableHDU.from_columns(cols)]).writeto(os.path.join(OUT, "muscles_like.fits"))
    # BT-Settl-like: a two-row fp32 image, micron and erg s^-1 cm^-2 micron^-1
    lam_b = np.linspace(0.3, 20.0, 500)
    f_b = 1e10 * np.exp(-((lam_b - 1.2) / 2.0) ** 2) + 1e6
    fits.PrimaryHDU(np.stack([lam_b, f_b]).astype(np.float32)).writeto(os.path.join(OUT, "btsettl_like.fits"))
    # the grids: R = 50 from 0.03 to 30 micron (below, across and beyond every spectrum), and bin centres alone
    import h5py
    inter = [0.03e-4]
    while inter[-1] < 30e-4:
        inter.append(inter[-1] * 51.0 / 50.0)
    inter = np.asarray(inter)
    with h5py.File(os.path.join(OUT, "grid_r50.h5"), "w") as f:
        f.create_dataset("center wavelengths", data=(inter[1:] + inter[:-1]) / 2)
        f.create_dataset("interface wavelengths", data=inter)
    with h5py.File(os.path.join(OUT, "grid_centres.h5"), "w") as f:
        f.create_dataset("wavelengths", data=np.linspace(0.2e-4, 8e-4, 120))
    return lam_cm


def edge_case():
    """a hand-made spectrum and grid: interfaces on the first, an interior and the last tabulated wavelength, bins without a
    point and with one, straddling each end, wholly outside, and a tabulated 0 on an interface"""
    lam = np.array([1.0, 1.5, 2.0, 2.25, 2.5, 3.0, 3.5, 4.0, 5.0, 6.0, 7.0, 8.0]) * 1e-4
    flux = np.array([3.0, 4.0, 2.5, 2.0, 6.0, 0.0, 5.0, 7.0, 1.0, 2.0, 3.0, 4.0]) * 1e13
    inter = np.array([0.5, 0.8, 1.0, 1.2, 1.4, 2.0, 2.6, 3.0, 3.2, 3.3, 3.4, 4.5, 6.5, 8.0, 9.0, 10.0]) * 1e-4
    return lam, flux, inter


def main():
    numpy_names_for_astropy()
    lam_cm = write_inputs()
    fc, tls = import_reference()
    from astropy.io import fits  # noqa: F401
    import h5py
    res = {}
    work = tempfile.mkdtemp(prefix="star_golden_")
    here = os.getcwd()
    try:
        os.chdir(work)
        os.makedirs("input/phoenix")
        shutil.copy(os.path.join(OUT, "phoenix", WAVE), "input/phoenix/" + WAVE)
        for name, (t_eff, log_g, metal) in BLEND_CASES.items():
            shutil.copytree(os.path.join(OUT, "phoenix"), "input/phoenix/" + name)
            res["blend_" + name] = np.asarray(fc.interpol_phoenix_spectrum(name, t_eff, log_g, metal), np.float64)
            res["blend_" + name + "_par"] = np.array([t_eff, log_g, metal], np.float64)
        # the readers
        sun = {"data_format": "ascii", "source_file": os.path.join(OUT, "sun_like.txt"), "name": "sun_like",
               "w_conversion_factor": 1e-7, "flux_conversion_factor": 1e10, "temp": 5772}
        mus = {"data_format": "muscles", "name": "muscles_like", "source_file": os.path.join(OUT, "muscles_like.fits"),
               "w_conversion_factor": 1e-8, "flux_conversion_factor": 1e8, "distance_from_Earth": 4.67517,
               "R_star": 0.366999654557, "temp": 3293.7}
        bts = {"data_format": "btsettl", "name": "btsettl_like", "source_file": os.path.join(OUT, "btsettl_like.fits"),
               "w_conversion_factor": 1e-4, "flux_conversion_factor": 1e4, "temp": 2600}
        for star, reader in ((sun, fc.read_ascii_file), (mus, fc.read_muscles_file), (bts, fc.read_btsettl_file)):
            l, f = reader(star)
            res["read_%s_lambda" % star["name"]], res["read_%s_flux" % star["name"]] = np.asarray(l, np.float64), \
                np.asarray(f, np.float64)
        # the re-binning, directly
        with h5py.File(os.path.join(OUT, "grid_r50.h5"), "r") as f:
            centre, inter = f["center wavelengths"][:], f["interface wavelengths"][:]
        with h5py.File(os.path.join(OUT, "grid_centres.h5"), "r") as f:
            centres_only = f["wavelengths"][:]
        full = res["blend_full"]
        for tag, temp in (("none", 0), ("bb", 3026)):
            res["rebin_full_" + tag] = np.asarray(tls.convert_spectrum(list(lam_cm), list(full), list(centre), list(inter),
                                                                       extrapolate_with_BB_T=temp), np.float64)
            res["rebin_centres_" + tag] = np.asarray(tls.convert_spectrum(list(lam_cm), list(full), list(centres_only), None,
                                                                          extrapolate_with_BB_T=temp), np.float64)
            res["rebin_muscles_" + tag] = np.asarray(tls.convert_spectrum(
                list(res["read_muscles_like_lambda"]), list(res["read_muscles_like_flux"]), list(centre), list(inter),
                extrapolate_with_BB_T=temp), np.float64)
        el, ef, ei = edge_case()
        res["edge_lambda"], res["edge_flux"], res["edge_inter"] = el, ef, ei
        for tag, temp in (("none", 0), ("bb", 4000.0)):
            res["edge_" + tag] = np.asarray(tls.convert_spectrum(list(el), list(ef), list((ei[1:] + ei[:-1]) / 2), list(ei),
                                                                 extrapolate_with_BB_T=temp), np.float64)
        # the Planck integral: wide and narrow bins, cold and hot, both ends of the grid
        pl = [(t, inter[k], inter[k + 1]) for t in (2300, 3026.5, 12000.0) for k in (0, 1, 150, len(inter) - 3, len(inter) - 2)]
        pl += [(5772, 1e-4, 1.000001e-4), (5772, 199.99e-4, 200e-4)]
        res["planck_args"] = np.asarray(pl, np.float64)
        res["planck"] = np.asarray([np.pi * tls.calc_analyt_planck_in_interval(int(t) if float(t).is_integer() else t, lo, hi)
                                    for t, lo, hi in pl], np.float64)
        # main_loop in its automatic mode; the plot and the question are answered by stand-ins
        sys.modules["matplotlib.pyplot"].subplots = lambda *a, **k: (_Anything(), _Anything())
        sys.modules["matplotlib.pyplot"].show = lambda *a, **k: None
        builtins.input = lambda *a: "yes"
        seen = []
        planck = tls.calc_analyt_planck_in_interval

        def recording(temp, lo, hi):
            seen.append(float(temp))
            return planck(temp, lo, hi)
        tls.calc_analyt_planck_in_interval = recording
        gj = {"data_format": "phoenix", "name": "full", "temp": 3026, "log_g": 4.944, "m": 0.39}
        for star, grid, convert_to in ((gj, "grid_r50.h5", "r50_kdistr"), (sun, "grid_r50.h5", "r50_kdistr"),
                                       (mus, "grid_r50.h5", "r50_kdistr"), (bts, "grid_r50.h5", "r50_kdistr"),
                                       (gj, "grid_centres.h5", "centres")):
            del seen[:]
            fc.main_loop(star, convert_to=convert_to, opac_file_for_lambdagrid=os.path.join(OUT, grid),
                         output_file="star.h5", plot_and_tweak="automatic", save_ascii="yes" if star is sun else "no",
                         save_in_hdf5="yes")
            res["loop_%s_%s_bb_temp" % (star["name"], convert_to)] = np.float64(seen[-1])
        tls.calc_analyt_planck_in_interval = planck
        with h5py.File("output/star.h5", "r") as f:
            def visit(name, obj):
                if isinstance(obj, h5py.Dataset):
                    res["file/" + name] = np.asarray(obj[()], np.float64)
            f.visititems(visit)
        for tail in ("_orig.dat", "_r50_kdistr.dat"):
            shutil.copy("output/sun_like" + tail, os.path.join(OUT, "sun_like" + tail))
    finally:
        os.chdir(here)
        shutil.rmtree(work, ignore_errors=True)
    np.savez_compressed(os.path.join(OUT, "reference.npz"), **res)
    total = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(OUT) for f in fs)
    print("%d results, %d bytes of fixtures under %s" % (len(res), total, OUT))
    for k in sorted(res):
        if k.endswith("bb_temp"):
            print(k, repr(float(res[k])))


if __name__ == "__main__":
    main()
