"""star.py on the CPU: the numpy backend against what the reference's own functions made of the committed inputs
(tests/golden/star/, make_star_golden.py) and against the long-double restatement (tests/star_reference.py), under the
project's rule -- every entry within max(1e-13, 8 eps_ref) relative of the restatement, eps_ref being the reference's own
deviation from it at that entry, and 0 where the reference is 0.  The minimal FITS reader, the refusals, the file that
Read.read_star takes, the command line, and the sweep's new axes.  (The device: tests/test_gpu_star.py.)"""
import json
import os

import numpy as np
import pytest

import star_cases as sc
import star_reference as sr
import table_files as tf
from helios_amd import fits_lite, star

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _numpy_blend(name):
    t, g, m = sc.blend_cases()[name]
    terms, div = star.blend_plan(int(t) if float(t).is_integer() else t, g, m)
    d = star.PhoenixDirectory(sc.PHOENIX)
    return star.numpy_blend({n: d.flux(n) for n, _ in terms}, terms, div)


@pytest.mark.parametrize("name", sorted(sc.blend_cases()))
def test_blend_is_the_references_to_the_bit_and_within_the_rule_of_the_restatement(name):
    """fp64 in the reference's order of operations: the same bits as its result under numpy 1.26, where an fp32 scalar times
    a Python number is fp64"""
    ref = sc.golden()["blend_" + name]
    mine = _numpy_blend(name)
    assert np.array_equal(mine, ref), np.abs(mine / ref - 1).max()
    sc.hold(mine, sc.restated_blend(name), ref, "blend " + name)


def test_the_eight_branches_and_both_ends_of_the_metallicity_axis_are_among_the_cases():
    counts = sorted(len(star.blend_plan(*[int(p[0])] + list(p[1:]))[0]) for p in sc.blend_cases().values())
    assert counts.count(8) >= 3 and counts.count(4) >= 3 and counts.count(2) >= 2 and counts.count(1) >= 1
    assert {p[2] for p in sc.blend_cases().values()} >= {-2.0, 1.0}
    # the 7000 K change of spacing: 100 K nodes below, 200 K nodes from there
    assert star.corner_nodes(6950, 4.5, 0.0)[:2] == (6900, 7000) and star.corner_nodes(7100, 4.5, 0.0)[:2] == (7000, 7200)
    assert star.corner_nodes(7000, 4.5, 0.0)[:2] == (7000, 7000)
    # [M/H] between -0.5 and 0: the reference spells the upper node -0.0
    assert star.blend_plan(7000, 4.2, -0.3)[0][0][0] == "07000_4.50_-0.0.fits"


REBIN = {"full": ("r50", None), "centres": ("centres", None), "muscles": ("r50", "muscles_like")}


@pytest.mark.parametrize("tag,temp", [("none", 0), ("bb", 3026)])
@pytest.mark.parametrize("case", sorted(REBIN))
def test_rebinning_against_the_reference_and_the_restatement(case, tag, temp):
    """Every entry within max(1e-13, 8 eps_ref) of the restatement, eps_ref the reference's own deviation at that entry.
    In the extrapolated bins beyond a few micron the reference's series cancels (eps_ref up to 1.2e-11 here); the backend
    evaluates the same terms without the cancellation (star.planck_term) and stays below 4e-14"""
    g = sc.golden()
    grid, reader = REBIN[case]
    lam, flux = (sc.phoenix_lambda(), g["blend_full"]) if reader is None else (g["read_%s_lambda" % reader],
                                                                               g["read_%s_flux" % reader])
    inter = sc.grids()[grid][1]
    ref = g["rebin_%s_%s" % (case, tag)]
    pbot, state = star.interface_plan(lam, inter)
    extrapol = star.numpy_planck_bins(temp, inter[:-1], inter[1:])
    mine = star.numpy_rebin(lam, flux, inter, pbot, state, extrapol)
    restated = sr.reference_rebin(lam, flux, inter, sr.reference_planck(temp, inter[:-1], inter[1:]))
    assert np.array_equal(mine == 0, ref == 0)
    sc.hold(mine, restated, ref, "re-binning %s %s" % (case, tag))


@pytest.mark.parametrize("tag,temp", [("none", 0), ("bb", 4000.0)])
def test_every_case_of_the_rebinning_at_its_edge(tag, temp):
    """interfaces on the first (the index -1 wraps), an interior and the last tabulated wavelength, bins without a point and
    with one, straddling each end, wholly outside, and a tabulated 0 that makes an interface value 0"""
    g = sc.golden()
    lam, flux, inter, ref = g["edge_lambda"], g["edge_flux"], g["edge_inter"], g["edge_" + tag]
    pbot, state = star.interface_plan(lam, inter)
    assert pbot[2] == -1 and state[2] == 1 and list(state[:2]) == [0, 0] and list(state[-2:]) == [0, 0] and state[-3] == 1
    extrapol = star.numpy_planck_bins(temp, inter[:-1], inter[1:])
    mine = star.numpy_rebin(lam, flux, inter, pbot, state, extrapol)
    F = star.numpy_interface_values(lam, flux, inter, pbot, state)
    assert F[7] == 0 and state[7] == 1                      # the tabulated 0 at 3 micron
    assert mine[6] == extrapol[6] and mine[7] == extrapol[7]
    restated = sr.reference_rebin(lam, flux, inter, sr.reference_planck(temp, inter[:-1], inter[1:]))
    assert np.array_equal(mine == 0, ref == 0)
    sc.hold(mine, restated, ref, "edge case " + tag)


def test_planck_values_against_the_reference_and_the_restatement():
    g = sc.golden()
    for (t, lo, hi), ref in zip(g["planck_args"], g["planck"]):
        mine = star.numpy_planck_bins(int(t) if float(t).is_integer() else t, np.array([lo]), np.array([hi]))
        sc.hold(mine, sr.reference_planck(t, np.array([lo]), np.array([hi])), np.array([ref]), "Planck %g K %g cm" % (t, lo))


LOOPS = {"full_r50_kdistr": ("phoenix", "full", "r50", "r50_kdistr"), "full_centres": ("phoenix", "full", "centres", "centres"),
         "sun_like_r50_kdistr": ("ascii", "sun_like", "r50", "r50_kdistr"),
         "muscles_like_r50_kdistr": ("muscles", "muscles_like", "r50", "r50_kdistr"),
         "btsettl_like_r50_kdistr": ("btsettl", "btsettl_like", "r50", "r50_kdistr")}
STARS = {
    "full": {"data_format": "phoenix", "name": "full", "temp": 3026, "log_g": 4.944, "m": 0.39},
    "sun_like": {"data_format": "ascii", "source_file": os.path.join(sc.GOLD, "sun_like.txt"), "name": "sun_like",
                 "w_conversion_factor": 1e-7, "flux_conversion_factor": 1e10, "temp": 5772},
    "muscles_like": {"data_format": "muscles", "name": "muscles_like", "source_file": os.path.join(sc.GOLD, "muscles_like.fits"),
                     "w_conversion_factor": 1e-8, "flux_conversion_factor": 1e8, "distance_from_Earth": 4.67517,
                     "R_star": 0.366999654557, "temp": 3293.7},
    "btsettl_like": {"data_format": "btsettl", "name": "btsettl_like", "source_file": os.path.join(sc.GOLD, "btsettl_like.fits"),
                     "w_conversion_factor": 1e-4, "flux_conversion_factor": 1e4, "temp": 2600},
}


def parity_figures():
    """per golden run of the reference's main loop: the reference's fitted temperature, the restatement's from the same bin
    flux, their relative deviation, and the numpy backend's"""
    g, out = sc.golden(), {}
    for key, (fmt, name, grid, convert_to) in sorted(LOOPS.items()):
        inter = sc.grids()[grid][1]
        r = star.convert_stars([dict(STARS[name])], inter, "automatic", "numpy", sc.PHOENIX)[0]
        first = star.convert_stars([dict(STARS[name])], inter, "fixed", "numpy", sc.PHOENIX)[0]["flux"]
        idx = r["fit_index"]
        restated = sr.reference_secant(inter, idx, first[idx], STARS[name]["temp"])
        ref = float(g["loop_%s_bb_temp" % key])
        out[key] = {"fit_index": idx, "reference": ref, "restatement": restated, "numpy_backend": float(r["BB_temp"]),
                    "reference_deviation": abs(ref / restated - 1), "numpy_backend_deviation": abs(r["BB_temp"] / restated - 1)}
    return out


def test_the_fitted_temperature_and_the_file_of_the_main_loop():
    """the reference's main loop in automatic mode converts with T_eff, fits, and converts ONCE MORE with the fitted temperature:
    the data sets it wrote are what the numpy backend returns; the fitted temperature is held to the restatement's, fed with
    the same bin flux, within eight times the reference's own largest deviation on these runs (profiles/star_parity.json
    holds the figures)"""
    g, fig = sc.golden(), parity_figures()
    margin = 8 * max(v["reference_deviation"] for v in fig.values())
    print(json.dumps(fig, indent=1), "margin %.3e" % margin)
    for key, (fmt, name, grid, convert_to) in sorted(LOOPS.items()):
        assert fig[key]["numpy_backend_deviation"] <= max(margin, 8 * np.finfo(np.float64).eps), key
        inter = sc.grids()[grid][1]
        r = star.convert_stars([dict(STARS[name])], inter, "automatic", "numpy", sc.PHOENIX)[0]
        ref = g["file/%s/%s/%s" % (convert_to, fmt, name)]
        lo, hi = inter[:-1], inter[1:]
        pbot, state = star.interface_plan(r["orig_lambda"], inter)
        restated = sr.reference_rebin(r["orig_lambda"], r["orig_flux"], inter, sr.reference_planck(fig[key]["restatement"], lo, hi))
        # extrapolated bins carry the fitted temperature's own deviation, times the black body's sensitivity to it,
        # d ln B / d ln T, which the restatement gives
        ext = (r["flux"] == star.numpy_planck_bins(r["BB_temp"], lo, hi)) & (ref != 0)
        sc.hold(r["flux"][~ext], restated[~ext], ref[~ext], "main loop %s" % key)
        moved = sr.reference_planck(fig[key]["restatement"] * (1 + 1e-6), lo, hi)[ext]
        sens = np.abs(np.log((moved / restated[ext]).astype(np.float64))) / 1e-6
        dev = sr.rel_dev(r["flux"][ext], restated[ext])
        allowed = 1e-13 + sens * max(margin, 8 * np.finfo(np.float64).eps) + 8 * sr.rel_dev(ref[ext], restated[ext])
        assert np.all(dev <= allowed), (key, float(np.max(dev / allowed)))
    saved = json.load(open(os.path.join(ROOT, "profiles", "star_parity.json")))
    assert sorted(saved["runs"]) == sorted(fig)


def test_original_phoenix_data_sets_and_the_ascii_files(tmp_path):
    g = sc.golden()
    out = star.main(["-data_format", "phoenix", "-name", "full", "-temp", "3026", "-log_g", "4.944", "-m", "0.39",
                     "-phoenix_directory", sc.PHOENIX, "-opac_file_for_lambdagrid", sc.GRID_R50, "-backend", "numpy",
                     "-output_file", str(tmp_path / "star.npz")])
    d = dict(np.load(out))
    assert np.array_equal(d["original/phoenix/full"], g["file/original/phoenix/full"])
    assert np.array_equal(d["original/phoenix/lambda"], g["file/original/phoenix/lambda"])
    assert np.array_equal(d["r50_kdistr/lambda"], g["file/r50_kdistr/lambda"])
    # a second star into the same file: the file is extended, an existing data set replaced
    star.main(["-data_format", "ascii", "-name", "sun_like", "-source_file", STARS["sun_like"]["source_file"], "-temp", "5772",
               "-w_conversion_factor", "1e-7", "-flux_conversion_factor", "1e10", "-opac_file_for_lambdagrid", sc.GRID_R50,
               "-backend", "numpy", "-save_ascii", "yes", "-output_file", out])
    d2 = dict(np.load(out))
    assert set(d) < set(d2) and "r50_kdistr/ascii/sun_like" in d2
    for tail in ("_orig.dat", "_r50_kdistr.dat"):
        mine, ref = open(str(tmp_path / ("sun_like" + tail))).read().split("\n"), open(os.path.join(sc.GOLD, "sun_like" + tail)).read().split("\n")
        assert mine[0] == ref[0] and len(mine) == len(ref)
        a, b = np.array([l.split() for l in mine[1:]], float), np.array([l.split() for l in ref[1:]], float)
        np.testing.assert_allclose(a, b, rtol=2e-7)      # seven digits are printed


def test_fits_lite_reads_the_astropy_written_files_bit_for_bit():
    g = sc.golden()
    lam = fits_lite.getdata(os.path.join(sc.PHOENIX, star.PHOENIX_WAVE_FILE), 0, force_lite=True)
    assert lam.dtype == np.float64 and np.array_equal(lam * 1e-8, g["file/original/phoenix/lambda"])
    c = fits_lite.getdata(os.path.join(sc.PHOENIX, "03000_5.00_0.5.fits"), 0, force_lite=True)
    assert c.dtype == np.float32 and np.array_equal(c, g["blend_all_nodes"])          # the branch that returns the corner
    t = fits_lite.getdata(os.path.join(sc.GOLD, "muscles_like.fits"), 1, force_lite=True)
    assert sorted(t) == ["ERROR", "EXPTIME", "FLUX", "WAVELENGTH"] and t["ERROR"].dtype == np.float32 and t["EXPTIME"].dtype == np.int32
    assert np.array_equal(t["EXPTIME"], np.arange(600)) and t["FLUX"][300] == 0
    for name in ("muscles_like", "btsettl_like", "sun_like"):
        reader = {"muscles_like": star.read_muscles_file, "btsettl_like": star.read_btsettl_file, "sun_like": star.read_ascii_file}[name]
        l, f = reader(STARS[name])
        assert np.array_equal(l, g["read_%s_lambda" % name]) and np.array_equal(f, g["read_%s_flux" % name]), name
    with pytest.raises(IOError, match="no HDU 3"):
        fits_lite.getdata(os.path.join(sc.GOLD, "muscles_like.fits"), 3, force_lite=True)


def test_the_written_file_is_read_back_by_read_star(tmp_path):
    from helios_amd import quantities, read
    for ending in (".h5", ".npz"):
        out = star.main(["-data_format", "btsettl", "-name", "bt", "-source_file", STARS["btsettl_like"]["source_file"],
                         "-temp", "2600", "-w_conversion_factor", "1e-4", "-flux_conversion_factor", "1e4", "-backend", "numpy",
                         "-opac_file_for_lambdagrid", sc.GRID_R50, "-output_file", str(tmp_path / ("star" + ending))])
        assert out.endswith(ending)
        r, q = read.Read(), quantities.Store()
        r.stellar_model, r.stellar_path, r.stellar_data_set = "file", out, "/r50_kdistr/btsettl/bt"
        q.nbin = len(sc.grids()["r50"][0])
        r.read_star(q)
        assert int(q.real_star) == 1 and np.all(np.asarray(q.starflux) > 0)
        one = star.convert_stars([dict(STARS["btsettl_like"], name="bt")], sc.grids()["r50"][1], backend="numpy")[0]["flux"]
        assert np.array_equal(q.starflux, one)


def test_every_refusal_raises_with_its_reason(tmp_path):
    inter = sc.grids()["r50"][1]
    gj = dict(STARS["full"])
    with pytest.raises(IOError, match=r"not in .*03500_4\.50_0\.0\.fits.*Nothing is fetched"):
        star.convert_stars([dict(gj, temp=3550)], inter, backend="numpy", phoenix_directory=sc.PHOENIX)
    with pytest.raises(IOError, match="WAVE_PHOENIX"):
        star.convert_stars([gj], inter, backend="numpy", phoenix_directory=str(tmp_path))
    with pytest.raises(IOError, match="-phoenix_directory"):
        star.convert_stars([gj], inter, backend="numpy")
    for m in (-2.5, 1.01):
        with pytest.raises(ValueError, match=r"outside the PHOENIX grid"):
            star.convert_stars([dict(gj, m=m)], inter, backend="numpy", phoenix_directory=sc.PHOENIX)
    short = tmp_path / "pho"
    os.makedirs(str(short))
    for f in os.listdir(sc.PHOENIX):
        data = open(os.path.join(sc.PHOENIX, f), "rb").read()
        open(str(short / f), "wb").write(data)
    bt = open(os.path.join(sc.GOLD, "btsettl_like.fits"), "rb").read()
    open(str(short / "03000_5.00_0.5.fits"), "wb").write(bt)           # a file of another shape
    with pytest.raises(IOError, match="holds 1000 points, the wavelength file 1500"):
        star.convert_stars([dict(gj, temp=3000, log_g=5.0, m=0.5)], inter, backend="numpy", phoenix_directory=str(short))
    down = tmp_path / "down.txt"
    down.write_text("h\n" * 8 + "300 1\n200 2\n400 3\n")
    with pytest.raises(IOError, match="do not ascend"):
        star.convert_stars([dict(STARS["sun_like"], source_file=str(down))], inter, backend="numpy")
    with pytest.raises(IOError, match="interactive mode"):
        star.convert_stars([gj], inter, "yes", "numpy", sc.PHOENIX)
    with pytest.raises(IOError, match="unknown data format 'kurucz'"):
        star.convert_stars([dict(gj, data_format="kurucz")], inter, backend="numpy")
    with pytest.raises(ValueError, match="cannot be negative"):
        star.convert_stars([dict(gj, BB_temp=-5.0)], inter, "fixed", "numpy", sc.PHOENIX)
    with pytest.raises(IOError, match="Unable to read wavelength data set"):
        np.savez(str(tmp_path / "nogrid.npz"), kpoints=np.zeros(3))
        star.read_lambda_grid(str(tmp_path / "nogrid.npz"))
    # the tool holds no address and no code that fetches
    text = open(star.__file__).read() + open(fits_lite.__file__).read() + open(os.path.join(ROOT, "star.py")).read()
    for word in ("ftp:", "http", "urllib", "wget", "socket", "requests"):
        assert word not in text, word


def test_a_star_list_goes_onto_one_grid_in_one_call(tmp_path):
    lst = tmp_path / "stars.dat"
    lst.write_text("# three stars that share corners, and one of another format\n"
                   "name=a data_format=phoenix temp=3026 log_g=4.944 m=0.39\n"
                   "name=b data_format=phoenix temp=3050 log_g=4.7 m=0.2\n"
                   "name=c data_format=phoenix temp=3000 log_g=5.0 m=0.5\n"
                   "name=s data_format=ascii source_file=%s temp=5772 w_conversion_factor=1e-7 flux_conversion_factor=1e10\n"
                   % STARS["sun_like"]["source_file"])
    out = star.main(["-star_list", str(lst), "-phoenix_directory", sc.PHOENIX, "-opac_file_for_lambdagrid", sc.GRID_R50,
                     "-backend", "numpy", "-output_file", str(tmp_path / "stars.npz"), "-convert_to", "r50"])
    d = dict(np.load(out))
    assert {"r50/phoenix/a", "r50/phoenix/b", "r50/phoenix/c", "r50/ascii/s", "r50/lambda", "original/phoenix/b"} <= set(d)
    # the same star as the golden run: covered bins to rounding; extrapolated ones carry the fitted temperature's deviation
    # (at most profiles/star_parity.json's margin, 2e-11) times d ln B / d ln T = hc / (lambda k T) < 200 on this grid
    np.testing.assert_allclose(d["r50/phoenix/a"], sc.golden()["file/r50_kdistr/phoenix/full"], rtol=1e-13 + 200 * 2e-11)
    with pytest.raises(IOError, match="is not one of"):
        lst.write_text("name=a colour=red\n")
        star.read_star_list(str(lst))


def test_the_sweep_axes_expand_and_a_blackbody_file_mix_lands_in_two_batches(tmp_path):
    from helios_amd import sweep as sw
    assert {"dataset_in_stellar_spectrum_file", "path_to_stellar_spectrum_file"} <= set(sw.PER_COLUMN_OPTIONS)
    cols = sw.expand_sweep("dataset_in_stellar_spectrum_file=/g/phoenix/a,/g/phoenix/b;temperature_star=3000,3100")
    assert len(cols) == 4 and cols[1] == {"dataset_in_stellar_spectrum_file": "/g/phoenix/a", "temperature_star": "3100"}
    table = tf.write_table(str(tmp_path / "opac.npz"), 24, *tf.CHEMISTRIES[0])
    lst = tmp_path / "stars.dat"
    lst.write_text("name=a data_format=phoenix temp=3026 log_g=4.944 m=0.39\nname=b data_format=phoenix temp=3050 log_g=4.7 m=0.2\n")
    stars = star.main(["-star_list", str(lst), "-phoenix_directory", sc.PHOENIX, "-opac_file_for_lambdagrid", table,
                       "-backend", "numpy", "-output_file", str(tmp_path / "stars.npz"), "-convert_to", "g"])
    base = ["-parameter_file", "/nonexistent", "-opacity_mixing", "premixed", "-number_of_layers", "14", "-name", "s",
            "-path_to_opacity_file", table, "-path_to_stellar_spectrum_file", stars]
    opened = []
    from helios_amd import read as read_mod
    orig = read_mod.Read._open_table
    shared = {}
    try:
        read_mod.Read._open_table = staticmethod(lambda p: (opened.append(str(p)), orig(p))[1])
        qa, qb = [sw._prepare_column(base + ["-stellar_spectral_model", "file"], {"dataset_in_stellar_spectrum_file": d}, shared)[0]
                  for d in ("/g/phoenix/a", "/g/phoenix/b")]
        qbb = sw._prepare_column(base + ["-stellar_spectral_model", "blackbody"], {}, shared)[0]
    finally:
        read_mod.Read._open_table = staticmethod(orig)
    assert opened.count(stars) == 1                                  # one stellar file, opened once per process
    assert int(qa.real_star) == 1 and int(qbb.real_star) == 0 and not np.array_equal(qa.starflux, qb.starflux)
    assert sw._batch_signature(qa) == sw._batch_signature(qb) != sw._batch_signature(qbb)


def test_the_star_entries_are_declared_exported_and_bound():
    from helios_amd import _lib
    names = {"hx_star_create", "hx_star_destroy", "hx_star_add_corner", "hx_star_set_grid", "hx_star_set_star", "hx_star_put_flux",
             "hx_star_run", "hx_star_get"}
    assert names <= set(_lib.prototypes())
    lib = _lib.lib()
    for n in names:
        assert getattr(lib, n).argtypes is not None
