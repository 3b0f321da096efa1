"""helios_amd/mie.py on the CPU: the numpy backend against the goldens and the long-double restatement under the rule of
tests/mie_cases.py, the limits of the contract, the file format as clouds.py reads it, the tool and its refusals."""
import os
import types

import numpy as np
import pytest

import mie_cases as mc
import mie_reference
from helios_amd import mie
from helios_amd.clouds import Cloud, R_VALUES


def test_the_restated_constants_are_the_modules():
    assert (mie.X_SMALL, mie.SERIES_TERMS, mie.LENTZ_TOL_EPS, mie.TINY) == (
        mie_reference.X_SMALL, mie_reference.SERIES_TERMS, mie_reference.LENTZ_TOL_EPS, mie_reference.TINY)
    assert "X_SMALL = 0.5" in mie.__doc__
    x = np.array([1e-6, 0.3, 0.5, 7.0, 20944.0])
    assert mie.n_terms(x).tolist() == [mie_reference.n_terms(float(v)) for v in x]


def test_numpy_backend_on_every_golden():
    g = mc.goldens()
    values = mie.numpy_series(g["x"], g["m_re"], g["m_im"])
    mc.check_backend(values, g["m_re"], g["m_im"], g["x"], golden=(g["q_ext"], g["q_sca"], g["g"]), label="numpy backend")


@pytest.mark.parametrize("m", [complex(1.5, 0.1), complex(1.33, 0.0)])
@pytest.mark.parametrize("x", [1e-4, 1e-3])
def test_rayleigh_limit(m, x):
    pol = (m * m - 1) / (m * m + 2)
    t = mie.mie_table([1.0], [m.real], [m.imag], radii_um=[x / (2 * np.pi)], backend="numpy")
    geo = np.pi * (x / (2 * np.pi) * 1e-4) ** 2
    assert t["size"][0, 0] == pytest.approx(x, rel=1e-15)
    q_sca, q_abs = t["scat"][0, 0] / geo, t["absorb"][0, 0] / geo
    assert abs(q_sca / (8.0 / 3.0 * x ** 4 * abs(pol) ** 2) - 1) <= 10 * x * x
    if m.imag > 0:
        assert abs(q_abs / (4 * x * pol.imag) - 1) <= 10 * x * x
    else:
        assert q_abs == 0.0


def test_a_lossless_material_absorbs_exactly_nothing(tmp_path):
    lam = np.array([0.5, 1.0, 7.0, 30.0])
    radii = np.array([0.01, 0.3, 2.0, 40.0])
    t = mie.mie_table(lam, [1.5, 1.4, 1.33, 0.9], np.zeros(4), radii_um=radii, backend="numpy")
    assert np.all(t["absorb"] == 0.0) and t["absorb"].shape == (4, 4)
    assert np.array_equal(t["ext"], t["scat"]) and np.all(t["scat"] > 0)
    paths = mie.write_mie_directory(str(tmp_path), lam, radii, t)
    for p in paths:
        tab = np.loadtxt(p, skiprows=1)
        assert np.all(tab[:, 5] == 1.0) and np.all(tab[:, 4] == 0.0) and np.array_equal(tab[:, 2], tab[:, 3])
    # a tiny k: Q_ext - Q_sca may round below 0 and is then 0, never negative
    t = mie.mie_table(lam, [1.5, 1.4, 1.33, 0.9], np.full(4, 1e-17), radii_um=radii, backend="numpy")
    assert np.all(t["absorb"] >= 0.0)


def test_results_come_back_in_input_order():
    lam = np.array([0.4, 3.0, 11.0])
    n, k = np.array([1.5, 1.6, 2.0]), np.array([0.0, 0.01, 0.7])
    radii = np.array([30.0, 0.02, 400.0, 1.0, 0.5])
    t = mie.mie_table(lam, n, k, radii_um=radii, backend="numpy")
    order = np.argsort(radii)
    s = mie.mie_table(lam, n, k, radii_um=radii[order], backend="numpy")
    for key in ("size", "ext", "scat", "absorb", "g"):
        assert np.array_equal(t[key][order], s[key]), key
    for j, r in enumerate(radii):                     # and every row is its own radius's: against the pairs one by one
        one = mie.mie_table(lam, n, k, radii_um=[r], backend="numpy")
        assert np.array_equal(one["ext"][0], t["ext"][j]) and np.array_equal(one["g"][0], t["g"][j])
    assert np.array_equal(t["size"], 2.0 * np.pi * radii[:, None] / lam[None, :])


# ---- the directory as clouds.py reads it ------------------------------------------------------------------------------------
LAM_DIR = 2.0 * (250.0 / 2.0) ** (np.arange(12) / 11.0)


@pytest.fixture(scope="module")
def directories(tmp_path_factory):
    """two directories from the tool itself: a lossless material and the smooth synthetic one; with what main() printed"""
    import contextlib
    import io
    out = {}
    n, k = mc.smooth_material(LAM_DIR)
    for name, kk in (("lossless", np.zeros(len(LAM_DIR))), ("lossy", k)):
        wd = tmp_path_factory.mktemp(name)
        nk = os.path.join(str(wd), "nk.dat")
        mc.write_nk_file(nk, LAM_DIR, n, kk, header=("made for a test", "two header lines"))
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            d = mie.main(["-refractive_index_file", nk, "-header_lines", "2", "-output_directory", os.path.join(str(wd), "mie"),
                          "-backend", "numpy"])
        out[name] = dict(path=d, n=n, k=kk, printed=buf.getvalue())
    return out


def test_the_directory_is_what_clouds_reads(directories):
    d = directories["lossy"]
    assert d["path"].endswith("/")
    names = sorted(os.listdir(d["path"]))
    assert names == sorted("r{:.6f}.dat".format(r) for r in R_VALUES) and len(names) == 51
    table = mie.mie_table(LAM_DIR, d["n"], d["k"], backend="numpy")
    for j in (0, 17, 50):
        path = d["path"] + "r{:.6f}.dat".format(R_VALUES[j])
        with open(path) as f:
            lines = f.read().splitlines()
        assert lines[0].startswith("#") and len(lines) == 1 + len(LAM_DIR) and len(lines[1].split()) == 7
        lam, scat, absorb, g = Cloud.read_mie_file(path)
        assert np.array_equal(lam, LAM_DIR * 1e-4)
        assert np.array_equal(scat, table["scat"][j]) and np.array_equal(absorb, table["absorb"][j])
        assert np.array_equal(g, table["g"][j])
        full = np.loadtxt(path, skiprows=1)
        assert np.array_equal(full[:, 1], table["size"][j]) and np.array_equal(full[:, 2], table["ext"][j])
        assert np.array_equal(full[:, 5], table["scat"][j] / table["ext"][j])
    whole = Cloud.mie_table(d["path"])
    assert np.array_equal(whole["lamda_mie"], LAM_DIR * 1e-4)
    assert np.array_equal(whole["scat"], table["scat"]) and np.array_equal(whole["absorb"], table["absorb"])
    assert "covers 2 ... 250 micron" in d["printed"] and "WARNING" in d["printed"] and "no cloud opacity" in d["printed"]


@pytest.mark.parametrize("name", ["lossless", "lossy"])
def test_cloud_pre_processing_from_the_directory(directories, name):
    q = types.SimpleNamespace()
    nbin, nlayer = 9, 6
    q.nbin, q.nlayer, q.ninterface = np.int32(nbin), np.int32(nlayer), np.int32(nlayer + 1)
    q.opac_interwave = 3.0e-4 * (100.0 / 3.0) ** (np.arange(nbin + 1) / nbin)        # 3 - 100 micron: inside the table
    q.opac_wave = 0.5 * (q.opac_interwave[1:] + q.opac_interwave[:-1])
    lev = [1e8 * (1e0 / 1e8) ** (i / (2 * nlayer - 1)) for i in range(2 * nlayer)]
    q.p_lay, q.p_int = lev[1::2], lev[0::2] + [1e0 * (1e0 / 1e8) ** (1 / (2 * nlayer - 1))]
    q.clouds, q.iso = np.int32(1), np.int32(0)
    c = Cloud()
    c.nr_cloud_decks, c.mie_path, c.cloud_r_mode, c.cloud_r_std_dev = 1, [directories[name]["path"]], [1.0], [1.8]
    c.cloud_mixing_ratio_setting, c.p_cloud_bot, c.f_cloud_bot, c.cloud_to_gas_scale_height = "manual", [1e6], [1e-13], [0.5]
    c.cloud_pre_processing(q)
    for stem in ("abs_cross_all_clouds", "scat_cross_all_clouds", "g_0_all_clouds"):
        for lev_name in ("_lay", "_int"):
            assert np.all(np.isfinite(getattr(q, stem + lev_name))), stem + lev_name
    assert q.scat_cross_all_clouds_lay.max() > 0 and q.scat_cross_all_clouds_int.max() > 0
    if name == "lossless":
        assert np.all(q.abs_cross_all_clouds_lay == 0.0)
    else:
        assert q.abs_cross_all_clouds_lay.max() > 0


# ---- -wavelength_grid -----------------------------------------------------------------------------------------------------
def test_wavelength_grid():
    lam_file = np.array([0.25, 0.5, 1.0, 4.0, 16.0, 300.0])
    n_file, k_file = np.array([1.7, 1.65, 1.6, 1.5, 1.9, 2.2]), np.array([0.0, 1e-4, 1e-3, 0.02, 0.7, 0.1])
    lam, n, k = mie.wavelength_grid("7 0.25 16", lam_file, n_file, k_file)
    assert len(lam) == 7 and lam[0] == 0.25 and lam[-1] == 16.0
    np.testing.assert_allclose(np.diff(np.log(lam)), np.log(64.0) / 6, rtol=1e-13)
    np.testing.assert_allclose(lam, 0.25 * 2.0 ** np.arange(7), rtol=1e-14)
    assert (n[0], k[0]) == (1.7, 0.0) and (n[-1], k[-1]) == (1.9, 0.7)       # nodes on file wavelengths: the file's values
    # linear in log10 lambda: 2 micron lies half way between 1 and 4
    assert n[3] == pytest.approx(0.5 * (1.6 + 1.5), rel=1e-13) and k[3] == pytest.approx(0.5 * (1e-3 + 0.02), rel=1e-13)
    for spec, what in (("5 0.2 16", "0.2"), ("5 0.5 301", "301")):
        with pytest.raises(IOError, match="outside the file") as e:
            mie.wavelength_grid(spec, lam_file, n_file, k_file)
        assert what in str(e.value) and "nothing is extrapolated" in str(e.value)
    for spec in ("1 1 2", "5 2 1", "5 1", "a b c"):
        with pytest.raises(IOError, match="nw lo hi"):
            mie.wavelength_grid(spec, lam_file, n_file, k_file)


def test_the_tool_with_a_wavelength_grid(tmp_path, capsys):
    lam_file = np.array([0.25, 1.0, 16.0, 300.0])
    nk = os.path.join(str(tmp_path), "nk.dat")
    mc.write_nk_file(nk, lam_file, [1.7, 1.6, 1.9, 2.2], [0.0, 1e-3, 0.7, 0.1])
    d = mie.main(["-refractive_index_file", nk, "-output_directory", os.path.join(str(tmp_path), "out"), "-wavelength_grid", "3 1 100",
                  "-backend", "numpy"])
    lam, _, _, _ = Cloud.read_mie_file(d + "r{:.6f}.dat".format(R_VALUES[20]))
    np.testing.assert_allclose(lam, np.array([1.0, 10.0, 100.0]) * 1e-4, rtol=1e-14)
    assert "covers 1 ... 100 micron" in capsys.readouterr().out
    with pytest.raises(IOError, match="outside the file"):
        mie.main(["-refractive_index_file", nk, "-output_directory", os.path.join(str(tmp_path), "out2"), "-wavelength_grid",
                  "3 0.1 100", "-backend", "numpy"])
    assert not os.path.exists(os.path.join(str(tmp_path), "out2"))


# ---- refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows, message", [
    (["1.0 1.5 0.1", "2.0 0 0.1"], "n > 0 and k >= 0"),
    (["1.0 1.5 0.1", "2.0 -1.5 0.1"], "n > 0 and k >= 0"),
    (["1.0 1.5 0.1", "2.0 1.5 -1e-9"], "n > 0 and k >= 0"),
    (["1.0 1.5 0.1", "1.0 1.5 0.2"], "strictly ascending"),
    (["2.0 1.5 0.1", "1.0 1.5 0.2"], "strictly ascending"),
    (["1.0 1.5 0.1", "2.0 nan 0.2"], "not finite"),
    (["1.0 1.5 0.1", "inf 1.5 0.2"], "not finite"),
    (["1.0 1.5 0.1", "2.0 1.5"], "does not hold wavelength, n and k"),
    (["1.0 1.5 0.1", "2.0 1.5 x"], "does not hold wavelength, n and k"),
])
def test_refused_lines_are_named(tmp_path, rows, message):
    nk = os.path.join(str(tmp_path), "nk.dat")
    with open(nk, "w") as f:
        f.write("# a comment\n" + "\n".join(rows) + "\n")
    with pytest.raises(IOError, match=message) as e:
        mie.read_refractive_index_file(nk)
    assert "line 3 of" in str(e.value) and repr(rows[1]) in str(e.value)


def test_fewer_than_two_rows_and_skipped_lines(tmp_path):
    nk = os.path.join(str(tmp_path), "nk.dat")
    with open(nk, "w") as f:
        f.write("title\n# comment\n1.0 1.5 0.1\n")
    with pytest.raises(IOError, match="fewer than two rows"):
        mie.read_refractive_index_file(nk, header_lines=1)
    with open(nk, "w") as f:
        f.write("9 9 9 is a header line\n# comment\n1.0 1.5 0.1\n\n# another\n2.5 1.25 0\n")
    lam, n, k = mie.read_refractive_index_file(nk, header_lines=1)
    assert lam.tolist() == [1.0, 2.5] and n.tolist() == [1.5, 1.25] and k.tolist() == [0.1, 0.0]


def test_refused_arguments_of_the_library():
    with pytest.raises(ValueError, match="backend is device or numpy"):
        mie.mie_table([1.0], [1.5], [0.0], backend="eager")
    with pytest.raises(ValueError, match="m_re = 0.0 is not a finite number > 0"):
        mie.mie_table([1.0], [0.0], [0.0], backend="numpy")
    with pytest.raises(ValueError, match="m_im = -0.5 is not a finite number >= 0"):
        mie.mie_table([1.0], [1.5], [-0.5], backend="numpy")
    with pytest.raises(ValueError, match="every radius is a finite number > 0"):
        mie.mie_table([1.0], [1.5], [0.0], radii_um=[0.0], backend="numpy")
    with pytest.raises(ValueError, match="every wavelength is a finite number > 0"):
        mie.mie_table([np.inf], [1.5], [0.0], backend="numpy")
    # a pair whose D_n do not fit the buffer is refused by the host with its radius, wavelength and bytes, before a device is
    # asked for: this passes on a machine without one
    with pytest.raises(ValueError, match="r = 1000 micron, lambda = 0.5 micron") as e:
        mie.mie_table([0.5, 20.0], [1.5, 1.5], [0.0, 0.0], radii_um=[1.0, 1000.0], scratch_bytes=100000)
    need = (mie_reference.n_terms(2 * np.pi * 1000.0 / 0.5) + 1) * 16
    assert "needs %d bytes" % need in str(e.value) and "holds 100000" in str(e.value) and "nothing was launched" in str(e.value)
