"""Cloud decks built on the device (helios_amd/csrc/clouds.hip): the deck spectra at the edges of the re-binning contract
against the long-double restatement, the six planes bit for bit against the host's statements on the device's spectra, the
plumbing of a cloud sweep, the sharing of Mie tables and the refusals."""
import json
import os

import numpy as np
import pytest

import cases
import cloud_reference as cr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLANE_NAMES = ("abs_cross_all_clouds_lay", "abs_cross_all_clouds_int", "scat_cross_all_clouds_lay", "scat_cross_all_clouds_int",
               "g_0_all_clouds_lay", "g_0_all_clouds_int")


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


@pytest.fixture(scope="module")
def mie(tmp_path_factory):
    """name -> (directory, table): two tables on the 37-point grid, one beyond the chunk k_cloud_deck_spectra stages"""
    out = {}
    for name, nw, seed in (("a", cr.NW_EDGE, 5), ("b", cr.NW_EDGE, 6), ("long", cr.NW_BEYOND_CHUNK, 7)):
        lam_um, scat, absorb, g = cr.synthetic_mie(nw, seed)
        path = cr.write_mie_directory(str(tmp_path_factory.mktemp("mie") / name), lam_um, scat, absorb, g)
        out[name] = (path, cr.table_of(lam_um, scat, absorb))
    return out


def _batch(ctx, inter, nlayer=3, iso=0, ncol=1, clouds=1):
    """a batch on the bins `inter` whose cloud planes hold the synthetic clouds of tests/cases.py"""
    from helios_amd.rt import batch_from_case
    nbin = len(inter) - 1
    c = cases.make_case(nbin=max(nbin, 3), nlayer=nlayer, clouds=clouds, iso=iso)
    if nbin < c.nbin:          # the synthetic tables need three bins: keep the first `nbin` of every array
        ntp, made = c.ntemp * c.npress, c.nbin
        c.opac_k = np.ascontiguousarray(c.opac_k.reshape(ntp, made, c.ny)[:, :nbin]).reshape(-1)
        c.opac_scat_cross = np.ascontiguousarray(c.opac_scat_cross.reshape(ntp, made)[:, :nbin]).reshape(-1)
        c.surf_albedo, c.starflux = c.surf_albedo[:nbin].copy(), c.starflux[:nbin].copy()
        for n in PLANE_NAMES:
            c[n] = np.ascontiguousarray(c[n].reshape(-1, made)[:, :nbin]).reshape(-1)
        c.nbin = nbin
    c.opac_interwave = np.asarray(inter, np.float64)
    c.opac_wave = 0.5 * (c.opac_interwave[1:] + c.opac_interwave[:-1])
    c.opac_deltawave = c.opac_interwave[1:] - c.opac_interwave[:-1]
    return batch_from_case(ctx, c, ncol=ncol), c


def _record_parity(case, ratio):
    path = os.path.join(ROOT, "profiles", "cloud_decks_parity.json")
    try:
        held = json.load(open(path)) if os.path.exists(path) else {}
        held.setdefault("largest deviation / tolerance per case", {})[case] = float("%.3e" % ratio)
        with open(path, "w") as f:
            json.dump(held, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError:
        pass        # a read-only tree: the assertion above has been made


# (nbin, tables of the decks): two decks on one table at every grid, two decks on two tables, the long table in one bin (every
# pass of one workgroup) and in many
SPECTRA_CASES = [(1, "aa"), (63, "aa"), (65, "aa"), (257, "aa"), (65, "ab"), (257, "ba"), (1, "long"), (63, "long")]


@pytest.mark.parametrize("nbin,decks", SPECTRA_CASES, ids=["%s-nbin%d" % (d, n) for n, d in SPECTRA_CASES])
def test_deck_spectra_at_the_edges_against_the_restatement(ctx, mie, nbin, decks):
    """every deck's three spectra within max(1e-13, 8 eps_host) of the restatement, zeros exact"""
    cr.require_extended_precision()
    names = [decks] if decks == "long" else list(decks)
    if decks == "long":
        assert cr.NW_BEYOND_CHUNK > 2 * 1024 + 1        # three passes of k_cloud_deck_spectra's staging
    lam = mie[names[0]][1]["lamda_mie"]
    inter = cr.bin_grid(lam, nbin)
    if decks == "long" and nbin == 1:
        assert cr.grid_features(lam, inter)["most_points"] > 2 * 1024 + 1
    r_mode, sigma = [0.8, 6.0][:len(names)], [1.7, 2.3][:len(names)]
    weights = np.array([cr.radius_weight(r, s) for r, s in zip(r_mode, sigma)])
    rt, c = _batch(ctx, inter)
    try:
        index = {}
        for n in names:
            if n not in index:
                index[n] = rt.add_mie_table(mie[n][1]["lamda_mie"], mie[n][1]["scat"], mie[n][1]["absorb"])
        assert rt.mie_table_count() == len(index)
        nd = len(names)
        rt.set_column_cloud_decks(0, [index[n] for n in names], weights, np.full((nd, c.nlayer), 1e-12),
                                  np.full((nd, c.nlayer + 1), 1e-12))
        got = rt.get("cloud_deck_spectra", 0).reshape(nd, 3, nbin)
    finally:
        rt.close()
    quant = cr.Quant(inter)
    host_cloud = cr.host_cloud([mie[n][0] for n in names], r_mode, sigma)
    worst = 0.0
    for d, n in enumerate(names):
        ref = cr.reference_spectra(mie[n][1], weights[d], inter)
        host = cr.host_spectra(host_cloud, d, quant)
        assert np.any(ref > 0)
        worst = max(worst, cr.hold(got[d], ref, host, "device, deck %d on table %s, nbin = %d" % (d, n, nbin)))
    _record_parity("%s-nbin%d" % (decks, nbin), worst)


@pytest.mark.parametrize("nbin", [65, 257])
@pytest.mark.parametrize("ndecks", [1, 3])
@pytest.mark.parametrize("iso", [0, 1])
@pytest.mark.parametrize("nlayer", [1, 7, 100])
def test_planes_are_the_hosts_statements_on_the_devices_spectra_bit_for_bit(ctx, mie, nlayer, iso, ndecks, nbin):
    """column 1 of two: its six planes after the deck call equal add_individual_cloud_decks_to_total + normalize_g_0 on the
    spectra read back; with iso = 1 the interface planes, and in every case column 0's planes, stay as they were"""
    names = ["a", "b", "a"][:ndecks]
    lam = mie["a"][1]["lamda_mie"]
    inter = cr.bin_grid(lam, nbin)
    rng = np.random.default_rng(100 * nlayer + 10 * ndecks + iso)
    f_lay = 10.0 ** rng.uniform(-14, -9, (ndecks, nlayer))
    f_int = 10.0 ** rng.uniform(-14, -9, (ndecks, nlayer + 1))
    if nlayer > 1:
        f_lay[0, 0] = 0.0      # below a deck's base
    weights = np.array([cr.radius_weight(r, 2.0) for r in (0.5, 3.0, 20.0)[:ndecks]])
    rt, c = _batch(ctx, inter, nlayer=nlayer, iso=iso, ncol=2)
    try:
        before = [{n: rt.get(n, col) for n in PLANE_NAMES} for col in range(2)]
        index = {n: rt.add_mie_table(mie[n][1]["lamda_mie"], mie[n][1]["scat"], mie[n][1]["absorb"]) for n in sorted(set(names))}
        rt.set_column_cloud_decks(1, [index[n] for n in names], weights, f_lay, None if iso else f_int)
        spec = rt.get("cloud_deck_spectra", 1).reshape(ndecks, 3, nbin)
        after = [{n: rt.get(n, col) for n in PLANE_NAMES} for col in range(2)]
    finally:
        rt.close()
    assert all(np.any(before[0][n] != 0) for n in PLANE_NAMES if iso == 0 or n.endswith("_lay"))
    # the host's own statements, on the device's spectra
    from helios_amd.clouds import Cloud
    quant, cloud = cr.Quant(inter, nlayer=nlayer, iso=iso), Cloud()
    quant.f_all_clouds_lay, quant.f_all_clouds_int = np.zeros(nlayer), np.zeros(nlayer + 1)
    for n in PLANE_NAMES:
        setattr(quant, n, np.zeros((nlayer if n.endswith("_lay") else nlayer + 1) * nbin))
    for d in range(ndecks):
        cloud.abs_cross_one_cloud, cloud.scat_cross_one_cloud, cloud.g_0_one_cloud = spec[d]
        cloud.f_one_cloud_lay, cloud.f_one_cloud_int = f_lay[d], f_int[d]
        cloud.add_individual_cloud_decks_to_total(quant)
    Cloud.normalize_g_0(quant)
    for n in PLANE_NAMES:
        np.testing.assert_array_equal(after[0][n], before[0][n], err_msg="column 0 " + n)
        if iso == 1 and n.endswith("_int"):
            np.testing.assert_array_equal(after[1][n], before[1][n], err_msg=n)
        else:
            np.testing.assert_array_equal(after[1][n], getattr(quant, n), err_msg=n)
    # bins outside the table scatter nothing: g_0 there is exactly 0, elsewhere it is a mean of the third spectrum
    dark = np.all(spec[:, 1, :] == 0, axis=0)
    assert dark.any() and not dark.all()
    g_lay, s_lay = after[1]["g_0_all_clouds_lay"].reshape(nlayer, nbin), after[1]["scat_cross_all_clouds_lay"].reshape(nlayer, nbin)
    assert np.all(g_lay[:, dark] == 0) and np.all(s_lay[:, dark] == 0)
    assert np.all(s_lay[-1, ~dark] > 0) and np.all(g_lay[-1, ~dark] > 0)


SWEEP_BASE = ["-parameter_file", "/nonexistent", "-opacity_mixing", "synthetic", "-synthetic", "64 6 5 11", "-number_of_layers", "20",
              "-maximum_number_of_iterations", "20000", "-radiative_equilibrium_criterion", "1e-4", "-convective_adjustment", "no",
              "-number_of_cloud_decks", "1", "-aerosol_radius_geometric_std_dev", "2", "-cloud_bottom_mixing_ratio", "1e-9",
              "-cloud_to_gas_scale_height_ratio", "0.5", "-name", "cl"]
SWEEP_SPEC = "aerosol_radius_mode=1,4;cloud_bottom_pressure=1e5,1e3"


def _same_files(dir_a, dir_b):
    files = sorted(os.listdir(dir_a))
    assert files and files == sorted(os.listdir(dir_b))
    assert any(f.endswith("_tp.dat") for f in files) and any("cloud" in f for f in files)
    for f in files:
        with open(os.path.join(dir_a, f), "rb") as fa, open(os.path.join(dir_b, f), "rb") as fb:
            assert fa.read() == fb.read(), f


def test_device_built_planes_give_the_run_of_the_same_planes_uploaded(tmp_path, mie, monkeypatch):
    """a 4-column sweep over radius mode x base pressure on the device path, then the same sweep with every column's planes
    handed over through hx_rt_set_column_clouds -- the planes read back from the first: the same files, byte for byte"""
    import sweep
    from helios_amd import rt as rt_mod
    monkeypatch.delenv("HELIOS_CLOUD_DECKS", raising=False)
    wd, base = str(tmp_path), SWEEP_BASE + ["-path_to_mie_files", mie["a"][0]]
    planes, deck_calls = {}, []
    decks, close = rt_mod.RTBatch.set_column_cloud_decks, rt_mod.RTBatch.close

    def recording_decks(batch, col, *args):
        deck_calls.append(col)
        decks(batch, col, *args)
        planes[col] = [batch.get(n, col) for n in ("abs_cross_all_clouds_lay", "abs_cross_all_clouds_int",
                                                   "scat_cross_all_clouds_lay", "scat_cross_all_clouds_int",
                                                   "g_0_all_clouds_lay", "g_0_all_clouds_int")]
    monkeypatch.setattr(rt_mod.RTBatch, "set_column_cloud_decks", recording_decks)
    cols, spectra = sweep.main(["-sweep", SWEEP_SPEC] + base + ["-output_directory", wd + "/device/"])
    assert sorted(deck_calls) == [0, 1, 2, 3] and all(np.any(planes[k][0] > 0) for k in range(4))
    monkeypatch.setattr(rt_mod.RTBatch, "set_column_cloud_decks",
                        lambda batch, col, *args: batch.set_column_clouds(col, *planes[col]))
    cols2, spectra2 = sweep.main(["-sweep", SWEEP_SPEC] + base + ["-output_directory", wd + "/uploaded/"])
    np.testing.assert_array_equal(spectra, spectra2)
    for k in range(4):
        assert int(cols[k].iter_value) == int(cols2[k].iter_value) > 0
        np.testing.assert_array_equal(cols[k].T_lay, cols2[k].T_lay)
        _same_files(os.path.join(wd, "device", "cl_%d" % k), os.path.join(wd, "uploaded", "cl_%d" % k))
    for a, b in ((0, 1), (0, 2), (1, 3)):          # the clouds do tell the columns apart
        assert np.abs(np.asarray(cols[a].T_lay) / np.asarray(cols[b].T_lay) - 1.0).max() > 1e-6, (a, b)


def test_host_built_cloud_sweep_equals_the_single_runs(tmp_path, mie, monkeypatch):
    """HELIOS_CLOUD_DECKS=host: the same sweep with every column's planes from cloud_pre_processing is held to four helios.py
    runs as the table sweeps are (tests/test_gpu_table_sweep.py): equal iteration counts, T_lay and spectrum at rtol = 1e-12"""
    import helios
    import sweep
    from helios_amd import rt as rt_mod
    monkeypatch.setenv("HELIOS_CLOUD_DECKS", "host")
    monkeypatch.setattr(rt_mod.RTBatch, "set_column_cloud_decks",
                        lambda *a: pytest.fail("the host path made a deck call"))
    wd, base = str(tmp_path), SWEEP_BASE + ["-path_to_mie_files", mie["a"][0]]
    cols, spectra = sweep.main(["-sweep", SWEEP_SPEC] + base + ["-output_directory", wd + "/batch/"])
    k = 0
    for r_mode in ("1", "4"):
        for p_bot in ("1e5", "1e3"):
            single = helios.run_helios(base + ["-aerosol_radius_mode", r_mode, "-cloud_bottom_pressure", p_bot,
                                               "-output_directory", wd + "/single/", "-name", "cl_%d" % k])
            assert single.rt is not None
            print("column %d: %d iterations, single run %d; max |T_lay / single - 1| = %.3e"
                  % (k, int(cols[k].iter_value), int(single.iter_value),
                     np.abs(np.asarray(cols[k].T_lay) / np.asarray(single.T_lay) - 1.0).max()))
            assert int(cols[k].iter_value) == int(single.iter_value), k
            np.testing.assert_allclose(cols[k].T_lay, single.T_lay, rtol=1e-12, err_msg="column %d" % k)
            np.testing.assert_allclose(spectra[k], single.F_up_band[-64:], rtol=1e-12, err_msg="column %d" % k)
            k += 1


def test_eight_columns_naming_two_mie_directories_leave_two_resident_tables(ctx, mie):
    from helios_amd import computation
    from helios_amd.sweep import _prepare_column, expand_sweep
    base = SWEEP_BASE + ["-cloud_bottom_pressure", "1e4"]
    overrides = expand_sweep("path_to_mie_files=%s,%s;aerosol_radius_mode=1,2,3,4" % (mie["a"][0], mie["b"][0]))
    shared = {"cloud_decks": "device"}
    quants = [_prepare_column(base, dict(ov, name="c%d" % k), shared)[0] for k, ov in enumerate(overrides)]
    assert len(quants) == 8 and len(shared["mie"]) == 2
    computer = computation.Compute()
    for q in quants:
        q._ctx = computer.ctx
    rt = computer.make_rt_batch(quants)
    try:
        assert rt.mie_table_count() == 2
        spec = [rt.get("cloud_deck_spectra", c) for c in range(8)]
    finally:
        rt.close()
    assert not np.array_equal(spec[0], spec[4]) and not np.array_equal(spec[0], spec[1])      # other table, other radius mode


def test_refusals_name_the_value_and_leave_the_batch_usable(ctx, mie):
    from helios_amd._lib import HeliosHipError
    table = mie["a"][1]
    lam, nr = table["lamda_mie"], table["scat"].shape[0]
    inter = cases.make_case(nbin=24).opac_interwave
    rt, c = _batch(ctx, inter, nlayer=9, ncol=2)
    L = c.nlayer
    w, fl, fi = np.full((1, nr), 1e-3), np.full((1, L), 1e-12), np.full((1, L + 1), 1e-12)
    try:
        bad = lam.copy()
        bad[3] = bad[2]
        with pytest.raises(HeliosHipError, match=r"status 1: .*not ascending: lamda_mie\[3\]"):
            rt.add_mie_table(bad, table["scat"], table["absorb"])
        assert rt.mie_table_count() == 0
        with pytest.raises(HeliosHipError, match=r"status 1: .*Mie table index 0 of deck 0 out of range.*holds 0 Mie"):
            rt.set_column_cloud_decks(0, [0], w, fl, fi)
        assert rt.add_mie_table(lam, table["scat"], table["absorb"]) == 0
        with pytest.raises(HeliosHipError, match=r"status 1: .*Mie table index 5 of deck 0 out of range.*holds 1 Mie"):
            rt.set_column_cloud_decks(0, [5], w, fl, fi)
        with pytest.raises(HeliosHipError, match=r"status 1: .*Mie table index -1 of deck 0"):
            rt.set_column_cloud_decks(0, [-1], w, fl, fi)
        with pytest.raises(HeliosHipError, match=r"status 1: .*%d radius weights for deck 0.*table 0 has %d radii" % (nr - 1, nr)):
            rt.set_column_cloud_decks(0, [0], w[:, :-1], fl, fi)
        with pytest.raises(HeliosHipError, match=r"status 1: .*column index 2 out of range"):
            rt.set_column_cloud_decks(2, [0], w, fl, fi)
        with pytest.raises(HeliosHipError, match=r"status 1: .*f_int is NULL"):
            rt.set_column_cloud_decks(0, [0], w, fl, None)
        before = rt.get("abs_cross_all_clouds_lay", 0)
        rt.set_column_cloud_decks(1, [0], w, fl, fi)
        np.testing.assert_array_equal(rt.get("abs_cross_all_clouds_lay", 0), before)       # the refusals wrote nothing
        assert np.any(rt.get("abs_cross_all_clouds_lay", 1) != before)
        rt.build_planck_table(1)
        rt.run(0, 12)
        assert np.isfinite(rt.get("T_lay", 0)).all() and np.isfinite(rt.get("T_lay", 1)).all()
    finally:
        rt.close()
    one, c = _batch(ctx, inter, nlayer=1)          # a one-layer batch holds planes; it is told that it cannot iterate
    try:
        one.build_planck_table(1)
        with pytest.raises(HeliosHipError, match=r"status 3: .*has 1 layer; refresh and iterations need at least 2"):
            one.run(0, 1)
        with pytest.raises(HeliosHipError, match=r"status 3: .*has 1 layer"):
            one.refresh()
    finally:
        one.close()
    clear, c = _batch(ctx, inter, nlayer=9, clouds=0)
    try:
        with pytest.raises(HeliosHipError, match=r"status 4: .*clouds = 0"):
            clear.add_mie_table(lam, table["scat"], table["absorb"])
        with pytest.raises(HeliosHipError, match=r"status 4: .*clouds = 0"):
            clear.set_column_cloud_decks(0, [0], w, fl, fi)
        clear.build_planck_table(1)
        clear.run(0, 3)
        assert np.isfinite(clear.get("T_lay", 0)).all()
    finally:
        clear.close()
