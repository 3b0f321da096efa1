"""Premixed k-tables built on the device from the on-the-fly species set (helios_amd/premix.py, csrc/premix.hip): the nodes
against the CPU oracle's species chain, a column placed on the nodes, the tool end to end where both paths are the same
function, the cell-error map, and the sweep form."""
import os
import shutil

import numpy as np
import pytest

import cases
from test_premix import SPECIES_NO_FILE, _host_golden_module

pytestmark = pytest.mark.gpu

AMU = 1.6605390666e-24


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def _species_case(nbin=40, nspecies=4, ntemp=6, npress=5, seed=3, with_h2o=True, tables=(1,)):
    """cases.add_species' set -- constant mixing ratios, one CIA pair, H2O scattering -- with (T, P) tables of the mixing
    ratio (as FastChem species have them) for the species in `tables` and for H2O"""
    c = cases.add_species(cases.make_case(nbin=nbin, nlayer=2, ntemp=ntemp, npress=npress), nspecies=nspecies, seed=seed,
                          with_h2o=with_h2o)
    rng = np.random.default_rng(seed + 100)
    for k, sp in enumerate(c.species):
        sp["vmr_tab"] = None
        if k in tables or sp["is_h2o"]:
            sp["vmr_tab"] = sp["vmr"] * 10.0 ** rng.uniform(-1.0, 1.0, ntemp * npress)
    return c


def _premixer(ctx, c, refine=(1, 1), correlated_k=False):
    from helios_amd.premix import Premixer
    pm = Premixer(ctx, c.nbin, c.ny, c.ntemp, c.npress, len(c.species), refine, correlated_k)
    pm.set_grid(c.opac_wave, c.gauss_y, c.gauss_weight, c.ktemp, c.kpress)
    for k, sp in enumerate(c.species):
        pm.set_species(k, sp["pretab"], sp["scat"], sp["vmr_tab"], sp["vmr"], sp["weight"], sp["absorbing"], sp["scattering"],
                       is_h2o=sp["is_h2o"], is_cia=sp["is_cia"], in_mu=0 if sp["is_cia"] else 1)
    return pm


def _oracle_nodes(port, c, T, P, vmr):
    """the oracle's species chain at the points (T[i], P[i]) with the mixing ratios vmr[s][i]: opac_species_interpol +
    add_to_mixed_opac, mean mass and scattering as tests/cases.py::refresh_onthefly drives them"""
    X, Y, N = c.nbin, c.ny, len(T)
    inmu = np.array([0.0 if sp["is_cia"] else 1.0 for sp in c.species])
    w = np.array([sp["weight"] for sp in c.species])
    amu = (vmr * (w * inmu)[:, None]).sum(0) / (vmr * inmu[:, None]).sum(0)
    mmm = amu * AMU
    mix, spec = np.zeros(Y * X * N), np.zeros(Y * X * N)
    scat, sc = np.zeros(X * N), np.zeros(X * N)
    for k, sp in enumerate(c.species):
        v = np.ascontiguousarray(vmr[k])
        if sp["absorbing"]:
            port.opac_species_interpol(T, c.ktemp, P, c.kpress, sp["pretab"], spec, c.npress, c.ntemp, Y, X, N)
            port.add_to_mixed_opac(v, spec, mix, mmm, c.gauss_weight, c.gauss_y, sp["weight"] * AMU, k,
                                   0 if sp["is_cia"] else 1, Y, X, N)
        if sp["scattering"]:
            if sp["is_h2o"]:
                port.calc_h2o_scat(T, P, c.opac_wave, sc, v, sp["weight"] * AMU, X, N)
            else:
                sc[:] = np.tile(sp["scat"], N)
            port.add_to_mixed_scat(v, sc, scat, X, N)
    return mix, scat, amu


def _node_vmr(c, nT, nP):
    """mixing ratios at the species tables' own nodes: the table's entries, or the constant"""
    return np.array([sp["vmr_tab"] if sp["vmr_tab"] is not None else np.full(nT * nP, sp["vmr"]) for sp in c.species])


@pytest.mark.parametrize("nspecies,slab_rows", [(5, 0), (5, 2), (49, 0)])
def test_nodes_against_the_oracle(ctx, port, nspecies, slab_rows):
    """every kpoints entry of a 6 x 5 table, 40 bins x 20 Gauss points, against the oracle's species chain at the node's
    (T, P) at the tolerance tests/test_gpu_onthefly.py holds opac_wg_* to (rtol 1e-9); Rayleigh table and mean molecular mass
    at 1e-12.  49 absorbers need two mixing launches; slab_rows = 2 builds the table in three slabs."""
    c = _species_case(nbin=40 if nspecies < 10 else 12, nspecies=nspecies, tables=(1, 3))
    if nspecies > 10:
        rng = np.random.default_rng(5)
        for sp in c.species[1:nspecies]:
            sp["vmr"] = float(10.0 ** rng.uniform(-3.0, -2.0))
            if sp["vmr_tab"] is not None:
                sp["vmr_tab"] = sp["vmr"] * 10.0 ** rng.uniform(-0.3, 0.3, c.ntemp * c.npress)
    pm = _premixer(ctx, c)
    try:
        pm.set_slab_rows(slab_rows)
        pm.run(True)
        T, P = pm.get("temperatures"), pm.get("pressures")
        np.testing.assert_array_equal(T, c.ktemp)
        np.testing.assert_array_equal(P, c.kpress)
        TT, PP = np.repeat(T, len(P)), np.tile(P, len(T))                  # node i = p + nP * t
        mix, scat, amu = _oracle_nodes(port, c, TT, PP, _node_vmr(c, len(T), len(P)))
        k = pm.get("kpoints")
        print("kpoints: largest relative difference %.3e" % np.abs(k / mix - 1.0).max())
        np.testing.assert_allclose(k, mix, rtol=1e-9, atol=1e-300)
        np.testing.assert_allclose(pm.get("scat_cross"), scat, rtol=1e-12, atol=0)
        np.testing.assert_allclose(pm.get("meanmolmass"), amu, rtol=1e-12, atol=0)
        # the mix went through random overlap
        for sp in c.species:
            sp["is_cia"] = sp["is_cia"] or sp["absorbing"]
        ck, _s, _a = _oracle_nodes(port, c, TT, PP, _node_vmr(c, len(T), len(P)))
        assert np.abs(ck - k).max() > 1e-3 * np.abs(k).max()
    finally:
        pm.close()


def _column_on_nodes(c, T_node):
    """a 2-layer column whose five levels are the table's pressure nodes, isothermal at a temperature node"""
    c = c.copy()
    P = np.asarray(c.kpress, np.float64)
    assert len(P) == 5 and c.nlayer == 2
    c.p_int, c.p_lay = P[[4, 2, 0]].copy(), P[[3, 1]].copy()
    c.T_lay = np.full(3, float(T_node))
    return c


def _first_refresh(ctx, c, nspecies):
    from helios_amd.rt import batch_from_case
    rt = batch_from_case(ctx, c, ncol=1, nspecies=nspecies)
    try:
        if nspecies:
            for k, sp in enumerate(c.species):
                rt.set_species(k, sp["pretab"], sp["scat"], sp["weight"], is_h2o=2 if sp["is_h2o"] else 0,
                               is_cia=1 if sp["is_cia"] else 0, in_mu=0 if sp["is_cia"] else 1)
            vl, vi = cases.species_vmr_arrays(c)
            rt.set_column_vmr(-1, vl, vi)
            for k, sp in enumerate(c.species):
                if sp["vmr_tab"] is not None:
                    rt.set_species_vmr_table(k, sp["vmr_tab"])
        rt.build_planck_table(1 if c.T_star > 10 else 0)
        rt.run(0, 1)
        return {k: rt.get(k) for k in ("opac_wg_lay", "opac_wg_int", "scat_cross_lay", "scat_cross_int", "meanmolmass_lay",
                                       "meanmolmass_int", "T_int")}
    finally:
        rt.close()


def test_a_column_on_the_nodes(ctx):
    """An on-the-fly batch whose 2L + 1 pressure levels are the table's pressure nodes, isothermal at a temperature node:
    its first refresh gives the built table's rows.  rtol 1e-9: a level's fractional index misses its node by a few ulp of
    log10 (<= 1e-14 of a cell), the tables vary by at most 1e3 between neighbouring nodes -- two decades of margin.  A
    premixed batch on the built table gives the same; at the two END nodes of the pressure axis the premixed look-up does not
    return the node's row but the blend at its clamp, 0.001 of a cell inside the table (kernels.cu:545-559), so those two
    levels are held -- at the same 1e-9 -- to that blend of the table's rows."""
    c0 = _species_case(nbin=40, nspecies=5, tables=(1, 3))
    pm = _premixer(ctx, c0)
    try:
        pm.run(False)
        kp = pm.get("kpoints").reshape(c0.ntemp, c0.npress, -1)
        sc = pm.get("scat_cross").reshape(c0.ntemp, c0.npress, -1)
        mm = pm.get("meanmolmass").reshape(c0.ntemp, c0.npress)
    finally:
        pm.close()
    it = 2
    c = _column_on_nodes(c0, c0.ktemp[it])
    f = _first_refresh(ctx, c, len(c.species))
    np.testing.assert_allclose(f["T_int"], c.ktemp[it], rtol=1e-15)
    nc = c.nbin * c.ny
    lay_nodes, int_nodes = [3, 1], [4, 2, 0]
    for name, nodes in (("lay", lay_nodes), ("int", int_nodes)):
        for i, p in enumerate(nodes):
            np.testing.assert_allclose(f["opac_wg_" + name][nc * i:nc * (i + 1)], kp[it, p], rtol=1e-9, atol=0,
                                       err_msg="on the fly, %s %d" % (name, i))
            np.testing.assert_allclose(f["scat_cross_" + name][c.nbin * i:c.nbin * (i + 1)], sc[it, p], rtol=1e-9, atol=0)
            np.testing.assert_allclose(f["meanmolmass_" + name][i], mm[it, p] * AMU, rtol=1e-12)
    cp = c.copy()
    cp.species = None
    cp.opac_k_factors = None
    cp.opac_k, cp.opac_scat_cross, cp.opac_meanmass = kp.reshape(-1), sc.reshape(-1), mm.reshape(-1) * AMU
    g = _first_refresh(ctx, cp, 0)
    nP = c.npress

    def looked_up(table, p):
        if p == 0:
            return table[it, 0] * (1 - 0.001) + table[it, 1] * (0.001 - 0)
        if p == nP - 1:
            pf = nP - 1.001
            return table[it, nP - 2] * ((nP - 1) - pf) + table[it, nP - 1] * (pf - (nP - 2))
        return table[it, p]
    for name, nodes in (("lay", lay_nodes), ("int", int_nodes)):
        for i, p in enumerate(nodes):
            np.testing.assert_allclose(g["opac_wg_" + name][nc * i:nc * (i + 1)], looked_up(kp, p), rtol=1e-9, atol=0,
                                       err_msg="premixed, %s %d" % (name, i))
            if 0 < p < nP - 1:
                np.testing.assert_allclose(g["opac_wg_" + name][nc * i:nc * (i + 1)],
                                           f["opac_wg_" + name][nc * i:nc * (i + 1)], rtol=1e-9, atol=0)


def _write_inputs(wd, species_text, seed=9, nbin=14):
    _host_golden_module().write_species_inputs(wd, seed=seed, nbin=nbin, ny=20, sorted_k=True)
    with open(os.path.join(wd, "species.dat"), "w") as f:
        f.write(species_text)


def _otf_argv(wd, extra=()):
    return ["-parameter_file", "/nonexistent", "-path_to_species_file", os.path.join(wd, "species.dat"),
            "-directory_with_fastchem_files", os.path.join(wd, "chem") + "/",
            "-directory_with_opacity_files", os.path.join(wd, "opac") + "/"] + list(extra)


RUN = ["-number_of_layers", "18", "-maximum_number_of_iterations", "20000", "-radiative_equilibrium_criterion", "1e-4",
       "-convective_adjustment", "no", "-toa_pressure", "1e3", "-boa_pressure", "1e7"]


def test_end_to_end_where_the_two_paths_are_the_same_function(tmp_path):
    """constant mixing ratios, `correlated-k`, no H2O scattering, a profile strictly inside the table: the mix is
    sum const * kappa_s(T, P), bilinear, so the premixed look-up is exact.  premix.py, then helios.py on its table against
    helios.py on the fly: equal iteration counts, T within 1e-7, F_up_band within 1e-6 + 1e-12 of its maximum (the
    tolerances of test_run_helios_on_the_fly_from_files); the cell-error map of this table is <= 1e-12 everywhere"""
    import helios
    import premix as premix_tool
    wd = str(tmp_path)
    _write_inputs(wd, "species      absorbing       scattering         mixing_ratio\n\n"
                      "H2O  yes no 1e-3\nH2   no  yes  0.85\nCO2  yes no  3e-4\nCH4 yes no 1e-4\nHe  no yes 0.15\n"
                      "CIA_H2He yes no 0.85&0.15\n")
    ck = ["-k_coefficients_mixing_method", "correlated-k"]
    table = os.path.join(wd, "mix.npz")
    written = premix_tool.main(_otf_argv(wd, ck) + ["-premix_output", table])
    assert written == [table]
    err = np.load(table)["premix cell error max"]
    print("cell error max: %.3e" % err.max())
    assert err.shape == (4,) and err.max() <= 1e-12
    out = ["-output_directory", wd + "/"]
    a = helios.run_helios(["-parameter_file", "/nonexistent", "-opacity_mixing", "premixed", "-path_to_opacity_file", table,
                           "-name", "pre"] + RUN + out)
    b = helios.run_helios(_otf_argv(wd, ck) + ["-opacity_mixing", "on-the-fly", "-name", "otf"] + RUN + out)
    print("iterations %d / %d, T %.3e, F_up_band %.3e" % (a.iter_value, b.iter_value, np.abs(a.T_lay / b.T_lay - 1).max(),
                                                         np.abs(a.F_up_band - b.F_up_band).max() / b.F_up_band.max()))
    assert 200.0 < min(a.T_lay.min(), b.T_lay.min()) and max(a.T_lay.max(), b.T_lay.max()) < 1800.0     # inside the table
    assert int(a.iter_value) == int(b.iter_value) and int(a.iter_value) > 3
    np.testing.assert_allclose(a.T_lay, b.T_lay, rtol=1e-7)
    np.testing.assert_allclose(a.F_up_band, b.F_up_band, rtol=1e-6, atol=1e-12 * b.F_up_band.max())


def test_the_cell_error_map_is_what_it_claims(ctx):
    """random overlap: the centres of the (1, 1) table's cells are nodes of the (2, 2) table, so the coarse map follows from
    the two kpoints arrays -- the look-up's blend of the four coarse corners (kernels.cu:561-567 at one half, one half)
    against the fine table's node; 1e-12, and bit-identical between two runs"""
    c = _species_case(nbin=40, nspecies=5, tables=(1, 3))
    got = {}
    for refine in ((1, 1), (2, 2)):
        pm = _premixer(ctx, c, refine)
        try:
            pm.run(True)
            got[refine] = (pm.get("kpoints").reshape(pm.nT, pm.nP, -1), pm.get("cell_error_max"), pm.get("cell_error_mean"))
            pm.run(True)
            np.testing.assert_array_equal(pm.get("cell_error_max"), got[refine][1])
            np.testing.assert_array_equal(pm.get("cell_error_mean"), got[refine][2])
            np.testing.assert_array_equal(pm.get("kpoints").reshape(pm.nT, pm.nP, -1), got[refine][0])
        finally:
            pm.close()
    k1, emax, emean = got[(1, 1)]
    k2 = got[(2, 2)][0]
    np.testing.assert_array_equal(k2[::2, ::2], k1)
    dd, ud, du, uu = k1[:-1, :-1], k1[:-1, 1:], k1[1:, :-1], k1[1:, 1:]
    tab = dd * 0.5 * 0.5 + ud * 0.5 * 0.5 + du * 0.5 * 0.5 + uu * 0.5 * 0.5
    otf = k2[1::2, 1::2]
    rel = np.abs(tab - otf) / otf
    print("cell error: max %.3e, mean %.3e" % (emax.max(), emean.mean()))
    assert emax.max() > 1e-3                         # a random-overlap mix of log-random tables is not bilinear
    np.testing.assert_allclose(emax, rel.max(axis=-1).reshape(-1), rtol=1e-12, atol=0)
    np.testing.assert_allclose(emean, rel.mean(axis=-1).reshape(-1), rtol=1e-12, atol=0)


def test_the_sweep_form(tmp_path, capsys):
    """two FastChem directories through `premix.py -sweep`, then `sweep.py -sweep "path_to_opacity_file=..."` over the two
    files: every column ends where its own single premixed run ends (the assertions of tests/test_gpu_table_sweep.py), and
    the two tables differ"""
    import helios
    import premix as premix_tool
    import sweep
    wd = str(tmp_path)
    _write_inputs(wd, SPECIES_NO_FILE)
    alt = os.path.join(wd, "alt")
    _host_golden_module().write_species_inputs(alt, seed=21, nbin=14, ny=20, sorted_k=True)
    shutil.copytree(os.path.join(alt, "chem"), os.path.join(wd, "chem1"))
    dirs = [os.path.join(wd, "chem") + "/", os.path.join(wd, "chem1") + "/"]
    written = premix_tool.main(_otf_argv(wd) + ["-premix_output", os.path.join(wd, "grid.npz"),
                                                "-sweep", "directory_with_fastchem_files=" + ",".join(dirs)])
    assert written == [os.path.join(wd, "grid_0.npz"), os.path.join(wd, "grid_1.npz")]
    line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("-sweep ")][-1]
    assert line == "-sweep \"path_to_opacity_file=%s\"" % ",".join(written)
    k0, k1 = np.load(written[0])["kpoints"], np.load(written[1])["kpoints"]
    assert k0.shape == k1.shape and np.abs(k0 / k1 - 1.0).max() > 1e-3
    base = ["-parameter_file", "/nonexistent", "-opacity_mixing", "premixed", "-name", "tab"] + RUN
    cols, spectra = sweep.main(["-sweep", "path_to_opacity_file=" + ",".join(written)] + base +
                               ["-output_directory", wd + "/batch/"])
    assert len(cols) == 2
    for k, path in enumerate(written):
        single = helios.run_helios(base + ["-path_to_opacity_file", path, "-output_directory", wd + "/single/",
                                           "-name", "s%d" % k])
        assert int(cols[k].iter_value) == int(single.iter_value), k
        np.testing.assert_allclose(cols[k].T_lay, single.T_lay, rtol=1e-12, err_msg="column %d" % k)
        np.testing.assert_allclose(spectra[k], single.F_up_band[-14:], rtol=1e-12)
    assert np.abs(cols[0].T_lay / cols[1].T_lay - 1.0).max() > 1e-4
