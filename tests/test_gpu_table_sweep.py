"""A sweep over premixed opacity tables on the device: one batch holds several table sets and every column reads its own
(hx_rt_add_premixed_tables, hx_rt_set_column_table).  A single helios.py run is what the parity tests pin, so a table sweep
is held to the single runs with the same table -- equal iteration counts, T_lay and emission spectrum at rtol = 1e-12, the
criterion of test_sweep_over_fastchem_directories_equals_individual_runs -- and its first refresh to the CPU oracle's
look-up in the column's own table (1e-12, as the full-size reference tests hold the same arrays)."""
import os

import numpy as np
import pytest

import cases
import table_files as tf

pytestmark = pytest.mark.gpu

NBIN = 24
BASE = ["-parameter_file", "/nonexistent", "-opacity_mixing", "premixed", "-number_of_layers", "14",
        "-maximum_number_of_iterations", "20000", "-radiative_equilibrium_criterion", "1e-4", "-name", "tab"]
T_INTERN = ("100", "700")
VARIANTS = {
    "fused_lookup": ["-convective_adjustment", "no"],                      # no beam: the look-up inside k_rt_coef
    "direct_beam": ["-convective_adjustment", "no", "-direct_irradiation_beam", "yes"],   # k_tp_spectral on the stored indices, k_rt_dtau_halves
    "isothermal": ["-convective_adjustment", "no", "-isothermal_layers", "yes"],
    "matrix": ["-convective_adjustment", "no", "-flux_calculation_method", "matrix", "-surface_albedo", "0.1"],
    "single": ["-convective_adjustment", "no", "-precision", "single"],    # fp32 planes in the sweep and in the single runs
    "convection": ["-convective_adjustment", "yes", "-kappa_value", "0.285714"],
}


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


class _Watch(object):
    """counts the device batches a sweep builds and keeps their graph captures and table counts (read when a batch closes)"""

    def __init__(self, monkeypatch):
        from helios_amd import computation, rt
        self.batches, self.graph_builds, self.table_counts = 0, [], []
        make, close = computation.Compute.make_rt_batch, rt.RTBatch.close
        watch = self

        def counting_make(comp, quants):
            watch.batches += 1
            return make(comp, quants)

        def recording_close(batch):
            if batch.handle and batch.dims.nspecies == 0:
                watch.graph_builds.append([int(v) for v in batch.get("graph_builds")])
                watch.table_counts.append(batch.premixed_table_count())
            close(batch)
        monkeypatch.setattr(computation.Compute, "make_rt_batch", counting_make)
        monkeypatch.setattr(rt.RTBatch, "close", recording_close)


def _table_sweep(tables, extra, out):
    import sweep
    return sweep.main(["-sweep", "path_to_opacity_file=%s;internal_temperature=%s" % (",".join(tables), ",".join(T_INTERN))]
                      + BASE + extra + ["-output_directory", out])


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_table_sweep_equals_the_single_runs_with_the_same_table(tmp_path, monkeypatch, variant):
    """three tables x two internal temperatures, six columns in ONE device batch: every column ends where the single run
    with its table ends, and columns of different tables end elsewhere (no column reads another's table)"""
    import helios
    wd = str(tmp_path)
    tables = tf.write_chemistries(os.path.join(wd, "tables"), NBIN, count=3)
    extra = VARIANTS[variant]
    watch = _Watch(monkeypatch)
    cols, spectra = _table_sweep(tables, extra, wd + "/batch/")
    assert len(cols) == 6 and spectra.shape == (6, NBIN)
    assert watch.batches == 1 and watch.table_counts == [3]
    if variant == "single":
        assert all(str(q.prec) == "single" for q in cols)
    k = 0
    for t, path in enumerate(tables):
        for T in T_INTERN:
            single = helios.run_helios(BASE + extra + ["-path_to_opacity_file", path, "-internal_temperature", T,
                                                       "-output_directory", wd + "/single/", "-name", "tab_%d" % k])
            assert single.rt is not None
            print("column %d (table %d, T_intern %s): %d iterations, single run %d; max |T_lay / single - 1| = %.3e"
                  % (k, t, T, int(cols[k].iter_value), int(single.iter_value),
                     np.abs(np.asarray(cols[k].T_lay) / np.asarray(single.T_lay) - 1.0).max()))
            assert int(cols[k].iter_value) == int(single.iter_value), k
            np.testing.assert_allclose(cols[k].T_lay, single.T_lay, rtol=1e-12, err_msg="column %d" % k)
            np.testing.assert_allclose(spectra[k], single.F_up_band[-NBIN:], rtol=1e-12, err_msg="column %d" % k)
            if variant != "convection":
                # (where the convection loop runs for ANY column of a batch, hx_rt_conv_adjust re-evaluates the mean molecular
                # mass of every column, the frozen ones at their final temperatures; their single runs keep the last refresh's
                # -- 6e-5 apart in this diagnostic, whatever the number of tables)
                np.testing.assert_allclose(cols[k].meanmolmass_lay, single.meanmolmass_lay, rtol=1e-12, err_msg="column %d" % k)
            if variant == "fused_lookup" and k == 3:
                _same_files(os.path.join(wd, "batch", "tab_3"), os.path.join(wd, "single", "tab_3"), "tab_3")
            k += 1
    for a, b in ((0, 2), (0, 4), (2, 4), (1, 3), (1, 5), (3, 5)):       # same internal temperature, different tables
        assert np.abs(np.asarray(cols[a].T_lay) / np.asarray(cols[b].T_lay) - 1.0).max() > 1e-4, (a, b)


def _same_files(batch_dir, single_dir, name):
    """every output file of the sweep's column is the single run's file byte for byte, apart from lines that carry the run's
    name"""
    files = sorted(os.listdir(single_dir))
    assert files and files == sorted(os.listdir(batch_dir))
    assert any(f.endswith("_tp.dat") for f in files) and any("opac" in f or "extinction" in f for f in files)
    for f in files:
        with open(os.path.join(batch_dir, f), "rb") as fa, open(os.path.join(single_dir, f), "rb") as fb:
            a = [ln for ln in fa.read().split(b"\n") if name.encode() not in ln]
            b = [ln for ln in fb.read().split(b"\n") if name.encode() not in ln]
        assert a == b, f


def test_a_table_sweep_captures_its_graphs_as_often_as_the_same_sweep_with_one_table(tmp_path, monkeypatch):
    """the column-to-table map is device data: assigning table sets changes no kernel argument, so the graphs of the loop
    are captured as often as in the same sweep (six columns, the same internal temperatures) over ONE table"""
    wd = str(tmp_path)
    tables = tf.write_chemistries(os.path.join(wd, "tables"), NBIN, count=3)
    watch = _Watch(monkeypatch)
    _table_sweep(tables, VARIANTS["fused_lookup"], wd + "/three/")
    _table_sweep([tables[0]] * 3, VARIANTS["fused_lookup"], wd + "/one/")
    assert watch.batches == 2 and watch.table_counts == [3, 1]
    print("graph captures (nine-iteration graph, decade graph): three tables %s, one table %s" % tuple(watch.graph_builds))
    assert watch.graph_builds[0] == watch.graph_builds[1]
    assert max(watch.graph_builds[0]) >= 1           # the loops did run on captured graphs


def _three_table_batch(ctx, ncol=6):
    """a batch of `ncol` columns over three table sets (column c reads set c % 3) with a temperature profile per column"""
    from helios_amd.rt import batch_from_case
    c0 = cases.make_case(nbin=NBIN, nlayer=14)
    sets = []
    for seed, scale, mu, ray in tf.CHEMISTRIES[:3]:
        d = tf.table_arrays(c0.nbin, seed, scale, mu, ray, ny=c0.ny, ntemp=c0.ntemp, npress=c0.npress)
        np.testing.assert_array_equal(d["temperatures"], c0.ktemp)
        np.testing.assert_array_equal(d["pressures"], c0.kpress)
        from helios_amd import phys_const as pc
        sets.append((d["kpoints"], d["weighted Rayleigh cross-sections"], d["meanmolmass"] * pc.AMU))
    c0.opac_k, c0.opac_scat_cross, c0.opac_meanmass = sets[0]
    rt = batch_from_case(ctx, c0, ncol=ncol)
    T = [np.linspace(700.0 + 90.0 * c, 1900.0 - 60.0 * c, c0.nlayer + 1) for c in range(ncol)]
    return rt, c0, sets, T


@pytest.mark.parametrize("fused_lookup", [True, False])
def test_first_refresh_looks_every_column_up_in_its_own_table(ctx, port, monkeypatch, fused_lookup):
    """opacities, Rayleigh cross-sections and mean molecular mass of every column of a three-table batch after the first
    refresh against the CPU oracle's opac_interpol / meanmolmass_interpol in THAT column's table: with the look-up fused
    into k_rt_coef (the arrays are rebuilt on demand for hx_rt_get) and with HELIOS_RT_FUSED_LOOKUP=0 (k_tp_spectral on the stored indices)"""
    if fused_lookup:
        monkeypatch.delenv("HELIOS_RT_FUSED_LOOKUP", raising=False)
    else:
        monkeypatch.setenv("HELIOS_RT_FUSED_LOOKUP", "0")
    rt, c0, sets, T = _three_table_batch(ctx)
    X, Y, L, I = c0.nbin, c0.ny, c0.nlayer, c0.nlayer + 1
    try:
        assert rt.premixed_table_count() == 1
        assert [rt.add_premixed_tables(*s) for s in sets[1:]] == [1, 2]
        assert rt.premixed_table_count() == 3 and [rt.column_table(c) for c in range(6)] == [0] * 6
        for c in range(6):
            rt.set_column_table(c, c % 3)
            rt.set_temperatures(c, T[c])
        assert [rt.column_table(c) for c in range(6)] == [0, 1, 2, 0, 1, 2]
        rt.build_planck_table(1)
        rt.step(0, step_temperature=False)
        got = [{n: rt.get(n, c) for n in ("opac_wg_lay", "opac_wg_int", "scat_cross_lay", "scat_cross_int",
                                          "meanmolmass_lay", "meanmolmass_int", "T_int")} for c in range(6)]
    finally:
        rt.close()
    for c in range(6):
        k, ray, mm = sets[c % 3]
        want = {n: np.zeros(s) for n, s in (("opac_wg_lay", Y * X * I), ("opac_wg_int", Y * X * I), ("scat_cross_lay", X * I),
                                            ("scat_cross_int", X * I), ("meanmolmass_lay", I), ("meanmolmass_int", I))}
        port.opac_interpol(T[c], c0.ktemp, c0.p_lay, c0.kpress, k, want["opac_wg_lay"], ray, want["scat_cross_lay"],
                           c0.npress, c0.ntemp, Y, X, L)
        port.opac_interpol(got[c]["T_int"], c0.ktemp, c0.p_int, c0.kpress, k, want["opac_wg_int"], ray,
                           want["scat_cross_int"], c0.npress, c0.ntemp, Y, X, I)
        port.meanmolmass_interpol(T[c], c0.ktemp, want["meanmolmass_lay"], mm, c0.p_lay, c0.kpress, c0.npress, c0.ntemp, L)
        port.meanmolmass_interpol(got[c]["T_int"], c0.ktemp, want["meanmolmass_int"], mm, c0.p_int, c0.kpress, c0.npress,
                                  c0.ntemp, I)
        for n, nlev, per in (("opac_wg_lay", L, Y * X), ("opac_wg_int", I, Y * X), ("scat_cross_lay", L, X),
                             ("scat_cross_int", I, X), ("meanmolmass_lay", L, 1), ("meanmolmass_int", I, 1)):
            g, w = got[c][n][:nlev * per], want[n][:nlev * per]
            print("column %d (table %d) %s: max relative difference %.3e" % (c, c % 3, n, np.abs(g / w - 1.0).max()))
            np.testing.assert_allclose(g, w, rtol=1e-12, err_msg="column %d %s" % (c, n))
    # and the tables do tell the columns apart: the same array in a column of another table is far away
    for n in ("opac_wg_lay", "scat_cross_lay", "meanmolmass_lay"):
        assert np.abs(got[0][n][:L] / got[1][n][:L] - 1.0).max() > 1e-2, n


@pytest.mark.parametrize("nlayer", [50, 100])
def test_eight_columns_over_four_tables_at_moderate_size(ctx, nlayer):
    """1 000 bins x 50 layers x 20 Gauss points (several workgroups per column in every kernel; 7 rows on 16 lanes) and the
    same with 100 layers (the headline's 13-row tiling), four tables, eight columns with their own internal flux and gravity:
    after 30 iterations every column is where a one-column batch with the same table is after the same 30 iterations"""
    from helios_amd import phys_const as pc
    from helios_amd.rt import batch_from_case
    c0 = cases.make_case(nbin=1000, nlayer=nlayer)
    sets = []
    for seed, scale, mu, ray in tf.CHEMISTRIES:
        d = tf.table_arrays(c0.nbin, seed, scale, mu, ray, ny=c0.ny, ntemp=c0.ntemp, npress=c0.npress)
        sets.append((d["kpoints"], d["weighted Rayleigh cross-sections"], d["meanmolmass"] * pc.AMU))
    columns = [dict(F_intern=pc.SIGMA_SB * (100.0 + 80.0 * c) ** 4, g=1000.0 + 150.0 * c) for c in range(8)]
    table_of = [c % 4 for c in range(8)]
    c0.opac_k, c0.opac_scat_cross, c0.opac_meanmass = sets[0]
    rt = batch_from_case(ctx, c0, ncol=8, columns=columns)
    try:
        tiling = rt.flux_tiling()
        print("tiling at %d layers: %s" % (nlayer, tiling))
        assert -(-c0.nbin // tiling["nxb"]) > 1, tiling            # several workgroups per column
        if nlayer == 100:
            assert tiling["ROWS"] == 13 and tiling["k"] == 16, tiling
        for s in sets[1:]:
            rt.add_premixed_tables(*s)
        for c in range(8):
            rt.set_column_table(c, table_of[c])
        rt.build_planck_table(1)
        rt.run(0, 30)
        got = [{n: rt.get(n, c) for n in ("T_lay", "F_up_band")} for c in range(8)]
    finally:
        rt.close()
    for c in range(8):
        c1 = c0.copy()
        c1.opac_k, c1.opac_scat_cross, c1.opac_meanmass = sets[table_of[c]]
        one = batch_from_case(ctx, c1, ncol=1, columns=[columns[c]])
        try:
            one.build_planck_table(1)
            one.run(0, 30)
            want = {n: one.get(n, 0) for n in ("T_lay", "F_up_band")}
        finally:
            one.close()
        for n in want:
            print("column %d (table %d) %s: max difference / max value %.3e"
                  % (c, table_of[c], n, np.abs(got[c][n] - want[n]).max() / np.abs(want[n]).max()))
            np.testing.assert_allclose(got[c][n], want[n], rtol=1e-12, err_msg="column %d %s" % (c, n))
        assert np.abs(want["T_lay"] - c0.T_lay).max() > 1e-3      # the iterations moved the profile
    assert np.abs(got[0]["T_lay"] / got[1]["T_lay"] - 1.0).max() > 1e-4


def test_table_errors_carry_the_librarys_message_and_leave_the_batch_usable(ctx):
    """an index out of range, a set added after the first refresh and table calls on an on-the-fly batch raise with the
    library's text (index and count); nothing is launched for them and the batch goes on"""
    from helios_amd._lib import HeliosHipError
    from helios_amd.rt import batch_from_case
    rt, c0, sets, T = _three_table_batch(ctx, ncol=2)
    try:
        assert rt.add_premixed_tables(*sets[1]) == 1
        with pytest.raises(HeliosHipError, match=r"table index 2 out of range.*holds 2 premixed"):
            rt.set_column_table(0, 2)
        with pytest.raises(HeliosHipError, match=r"table index -1 out of range.*holds 2 premixed"):
            rt.set_column_table(1, -1)
        with pytest.raises(HeliosHipError, match="column index out of range"):
            rt.set_column_table(2, 0)
        rt.set_column_table(1, 1)
        rt.build_planck_table(1)
        rt.run(0, 3)
        with pytest.raises(HeliosHipError, match=r"table set 2 comes after the first refresh.*keeps its 2 set"):
            rt.add_premixed_tables(*sets[2])
        assert rt.premixed_table_count() == 2 and rt.column_table(1) == 1
        rt.set_column_table(1, 0)            # assigning stays possible: in effect from the next refresh
        rt.run(3, 8)
        assert np.isfinite(rt.get("T_lay", 1)).all()
    finally:
        rt.close()
    c = cases.make_case(nbin=NBIN, nlayer=14)
    otf = batch_from_case(ctx, c, ncol=1, nspecies=1)
    try:
        with pytest.raises(HeliosHipError, match=r"on-the-fly mixing \(1 species\).*0 premixed table sets"):
            otf.add_premixed_tables(*sets[0])
        with pytest.raises(HeliosHipError, match=r"on-the-fly mixing \(1 species\).*table index 0.*0 premixed table sets"):
            otf.set_column_table(0, 0)
        assert otf.premixed_table_count() == 0
    finally:
        otf.close()


def test_a_set_assigned_after_a_refresh_is_in_effect_from_the_next_refresh(ctx):
    """three columns on one profile, sets 0, 1, 0: after the first refresh column 0 is given set 1 -- what hx_rt_get rebuilds
    for it (the fused look-up keeps no opacity arrays) is still set 0's, bit for bit column 2's; after the next refresh it is
    column 1's"""
    rt, c0, sets, T = _three_table_batch(ctx, ncol=3)
    names = ("opac_wg_lay", "opac_wg_int", "scat_cross_lay", "meanmolmass_lay")
    try:
        assert rt.add_premixed_tables(*sets[1]) == 1
        rt.set_column_table(1, 1)
        rt.build_planck_table(1)
        rt.step(0, step_temperature=False)
        rt.set_column_table(0, 1)
        assert rt.column_table(0) == 1
        before = [{n: rt.get(n, c) for n in names} for c in range(3)]
        rt.step(10, step_temperature=False)           # itervalue 10: a refresh
        after = [{n: rt.get(n, c) for n in names} for c in range(3)]
    finally:
        rt.close()
    for n in names:
        np.testing.assert_array_equal(before[0][n], before[2][n], err_msg=n)
        assert not np.array_equal(before[0][n], before[1][n]), n
        np.testing.assert_array_equal(after[0][n], after[1][n], err_msg=n)
        np.testing.assert_array_equal(after[2][n], before[2][n], err_msg=n)
