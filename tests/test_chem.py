"""chem.py (helios_amd/chem.py), numpy backend, under the rule of the table tools: every entry within max(1e-13, 8 eps) relative of
the long-double restatement (tests/chem_reference.py), eps the deviation of the same statements in plain fp64 at that entry;
against what the reference's script computed for the 200 cases of its figure (tests/golden/chem/reference.npz, made by
tests/golden/make_chem_golden.py) within max(1e-13, 8 eps_ref), eps_ref the reference's own deviation from the restatement at
that entry.  Then the root the contract chooses, the element balances, the file through both readers, the sweep, the refusals and
the chain into ktable.py's mixing stage.  No GPU.

Measured when the golden was made (profiles/chem_parity.json): eps_ref is 2.2e-15 for CH4 and 5.2e-15 for C2H2 (the
companion-matrix roots), and 2.6e-10 for H2O and CO and 5.1e-10 for CO2, at C/O > 1, where the reference forms water as a
difference of large numbers."""
import os

import numpy as np
import pytest

import chem_reference as cr
from helios_amd import chem, ktable_mix
from helios_amd.read import Read

GAS = float(cr.golden()["gas_constant"])
HE = 0.085
TEMPS = [500.0, np.nextafter(500.0, 1e9), 800.0, np.nextafter(800.0, 0.0), 1234.5, 2950.0, 3000.0]
PRESS = [1e-9, 1e-6, 1e-3, 1.0, 10.0, 1e3]
C_TO_O = [1e-6, 0.01, 0.55, 0.999, 1.0 - 1e-12, 1.0, 1.0 + 1e-12, 1.001, 2.0, 10.0]
N_O = 5e-4


def rule(got, want, eps, what):
    """got within max(1e-13, 8 eps) of want, entry by entry; returns the largest deviation"""
    worst = 0.0
    for idx in np.ndindex(want.shape):
        dev = cr.deviation(got[idx], want[idx])
        assert dev <= max(1e-13, 8 * eps[idx]), (what, idx, dev, eps[idx])
        worst = max(worst, dev)
    return worst


@pytest.fixture(scope="module")
def table():
    return chem.GibbsTable(*cr.golden_table())


@pytest.fixture(scope="module")
def restated():
    """{key: long double [chem][T][P]} and the plain-fp64 deviation of the same entries"""
    w = chem.weights()
    shape = (len(C_TO_O), len(TEMPS), len(PRESS))
    want = {k: np.zeros(shape, np.longdouble) for k in cr.ALL}
    eps = {k: np.zeros(shape) for k in cr.ALL}
    for ic, co in enumerate(C_TO_O):
        for it, t in enumerate(TEMPS):
            for jp, p in enumerate(PRESS):
                args = (cr.golden_table(), t, p, N_O, co * N_O, HE, GAS, w)
                ld, pf = cr.node(*args), cr.plain_fp64(*args)
                for k in cr.ALL:
                    want[k][ic, it, jp] = ld[k]
                    eps[k][ic, it, jp] = cr.deviation(pf[k], ld[k])
    return want, eps


def test_numpy_backend_against_the_restatement(table, restated):
    want, eps = restated
    o = np.full(len(C_TO_O), N_O)
    got = chem.numpy_nodes(table, TEMPS, PRESS, o, np.array(C_TO_O) * N_O, HE, GAS)
    for k in cr.ALL:
        print("%s: largest deviation %.3e, largest eps %.3e" % (k, rule(got[k], want[k], eps[k], k), eps[k].max()))
    lib = chem.cho_chemistry(table, TEMPS, PRESS, o, np.array(C_TO_O) * N_O, HE, "numpy", GAS)
    assert sorted(lib) == sorted(chem.KEYS)
    for k in chem.KEYS:
        assert lib[k].dtype == np.float64 and lib[k].tobytes() == got[k].tobytes()


def test_the_default_gas_constant_is_phys_consts(table):
    from helios_amd import phys_const as pc
    a = chem.cho_chemistry(table, [800.0], [1.0], [N_O], [0.55 * N_O], HE, "numpy")
    b = chem.cho_chemistry(table, [800.0], [1.0], [N_O], [0.55 * N_O], HE, "numpy", pc.K_B * pc.N_A * 1e-7)
    c = chem.cho_chemistry(table, [800.0], [1.0], [N_O], [0.55 * N_O], HE, "numpy", GAS)
    assert a["CH4"].tobytes() == b["CH4"].tobytes() and a["CH4"].tobytes() != c["CH4"].tobytes()


def golden_parity(table):
    """per species of the reference: (largest eps_ref, largest deviation of the numpy backend from the restatement); every one of
    the 200 cases is held to max(1e-13, 8 eps_ref)"""
    g = cr.golden()
    w = chem.weights()
    n_o, n_c, press = float(g["case_n_o"]), g["case_n_c"], float(g["case_pressure_bar"])
    temps = g["case_temperatures"]
    got = chem.numpy_nodes(table, temps, [press], np.full(len(n_c), n_o), n_c, HE, GAS)
    out = {}
    for ref_key, key in (("n_CH4", "CH4"), ("n_H2O", "H2O"), ("n_CO", "CO"), ("n_CO2", "CO2"), ("n_C2H2", "C2H2")):
        worst_ref = worst_got = 0.0
        for it, t in enumerate(temps):
            for ic in range(len(n_c)):
                ld = cr.node(cr.golden_table(), t, press, n_o, n_c[ic], HE, GAS, w)
                want = ld[key] / ld["H2"]                              # n_X: the mixing ratio over H2's
                mine = np.longdouble(got[key][ic, it, 0]) / np.longdouble(got["H2"][ic, it, 0])
                ref = g[ref_key][it, ic]
                eps_ref = cr.deviation(ref, want)
                bound = max(1e-13, 8 * eps_ref)
                assert cr.deviation(mine, want) <= bound, (key, t, ic, cr.deviation(mine, want), eps_ref)
                assert float(abs(mine - np.longdouble(ref)) / abs(want)) <= bound, (key, t, ic, eps_ref)
                worst_ref, worst_got = max(worst_ref, eps_ref), max(worst_got, cr.deviation(mine, want))
        out[key] = (worst_ref, worst_got)
    return out


def test_the_200_figure_cases_of_the_reference(table):
    g = cr.golden()
    assert g["n_CH4"].shape == (2, 100) and float(g["largest_imaginary_part"]) == 0.0
    for key, (eps_ref, dev) in golden_parity(table).items():
        print("%s: eps_ref %.3e, numpy backend %.3e" % (key, eps_ref, dev))
        assert dev <= 1e-13


def test_the_contracts_root_is_the_only_one_in_its_bracket_and_polyroots_4_is_not_always_it(table):
    """a thinned version of the grid the contract was decided on: one sign change in [x_min, 2 n_C] and f(x_min) <= 0 at every
    case; the reference's pick -- the root of largest real part -- is complex or another root at cold, dense nodes, and is the
    contract's root in the cases of its own figure"""
    tab = cr.golden_table()
    cases = [(t, p, n_o, co) for t in (500.0, 650.0, 800.0, 1500.0, 3000.0) for p in (1e-9, 1e-4, 1.0, 10.0, 1e3)
             for n_o in (5e-5, 5e-4, 5e-2) for co in (0.01, 0.55, 0.999, 1.0, 1.001, 2.0, 10.0)]
    figure = [(t, 1.0, 5e-4, co) for t in (800.0, 3000.0) for co in (0.1, 0.55, 1.0, 3.0, 10.0)]
    other = {False: 0, True: 0}
    limit = 0
    for case in cases + figure:
        t, p, n_o, co = case
        changes, below, all_methane, a = cr.sign_changes(tab, t, p, n_o, co * n_o, GAS)
        x = chem.numpy_nodes(table, [t], [p], [n_o], [co * n_o], HE, GAS)["n_CH4"][0, 0, 0]
        if all_methane:               # f(2 n_C) <= 0 by rounding: the root is the bracket's end, and no sign is left to change
            assert changes == 0 and below and x == 2.0 * (co * n_o), (case, changes, x)
            limit += 1
            continue
        assert changes == 1 and below, (case, changes, below)
        if not np.all(np.isfinite(a)):
            continue
        pick = np.polynomial.polynomial.polyroots(a)[4]
        differs = bool(abs(pick.imag) > 0 or abs(pick.real - x) > 1e-9 * x)
        other[case in figure] += differs
    print("polyroots(...)[4] is not the contract's root in %d of %d grid cases, %d of %d figure cases"
          % (other[False], len(cases), other[True], len(figure)))
    print("all methane by rounding in %d cases" % limit)
    assert other[False] > 0 and other[True] == 0 and limit < len(cases) // 10


def abundances_per_h2(table):
    o = np.full(len(C_TO_O), N_O)
    c = np.array(C_TO_O) * N_O
    r = chem.numpy_nodes(table, TEMPS, PRESS, o, c, HE, GAS)
    return {k: r[k] / r["H2"] for k in chem.SPECIES}, o[:, None, None], c[:, None, None], r


def test_the_element_balances_close(table, restated):
    """2 n_O = H2O + CO + 2 CO2 and 2 n_C = CH4 + CO + CO2 + 2 C2H2 within 1e-13, as far as the contract's polynomial allows.

    By algebra on the contract's coefficients (no run needed): the quintic is the oxygen balance with n_H2O = 2 K3 x^2 + x +
    2 (n_O - n_C) put in, and that water is the oxygen balance minus a carbon balance that counts CO2 TWICE,
    2 n_C = CH4 + CO + 2 CO2 + 2 C2H2.  At the contract's root therefore, exactly,
        CH4 + CO + CO2 + 2 C2H2 = 2 n_C - n_CO2,
    and the carbon balance as stated holds within 1e-13 where and only where n_CO2 / (2 n_C) does not reach that: no root of
    this polynomial does better.  Held here on every node and abundance of this file: oxygen within 1e-13; the identity above
    within 1e-13 (so the stated balance's whole defect is the one term the published polynomial leaves out); and the stated
    carbon balance itself within 1e-13 on the nodes where the long-double RESTATEMENT, not the backend, puts n_CO2 / (2 n_C)
    below 1e-14 -- a tenth of the bound, the rest is the sums' rounding.  Elsewhere the defect is what the identity says:
    0.108 at 500 K, 1e-9 bar, C/O = 1e-6, the largest on this grid, and 1.2e-4 at most in the 200 cases of the reference's
    figure."""
    want, _eps = restated
    n, o, c, _r = abundances_per_h2(table)
    carbon = n["CH4"] + n["CO"] + n["CO2"] + 2 * n["C2H2"]
    oxygen = n["H2O"] + n["CO"] + 2 * n["CO2"]
    assert np.max(np.abs(oxygen / (2 * o) - 1)) <= 1e-13
    assert np.max(np.abs((carbon + n["CO2"]) / (2 * c) - 1)) <= 1e-13
    left_out = (want["CO2"] / want["H2"] / np.longdouble(2) / c).astype(np.float64)
    small = left_out < 1e-14
    print("oxygen %.3e, carbon with the term %.3e, as stated %.3e on %d of %d nodes, %.3e at most elsewhere"
          % (np.max(np.abs(oxygen / (2 * o) - 1)), np.max(np.abs((carbon + n["CO2"]) / (2 * c) - 1)),
             np.max(np.abs(carbon / (2 * c) - 1)[small]), small.sum(), small.size, np.max(np.abs(carbon / (2 * c) - 1)[~small])))
    # hot, thin and carbon-rich is where CO2 is nothing (n_CO2 / n_CO = n_H2O / K2): such a node is among those held as stated
    assert small[C_TO_O.index(10.0), TEMPS.index(3000.0), PRESS.index(1e-9)]
    assert np.max(np.abs(carbon / (2 * c) - 1)[small]) <= 1e-13
    assert np.max(np.abs(carbon / (2 * c) - 1 + left_out)) <= 1e-13


def test_the_mixing_ratios_sum_to_one(table):
    _n, _o, _c, r = abundances_per_h2(table)
    assert np.max(np.abs(sum(r[k] for k in chem.SPECIES) - 1)) <= 8 * 2.0 ** -52


def write_gibbs(tmp_path):
    return chem.write_gibbs_file(os.path.join(str(tmp_path), "gibbs.dat"), *cr.golden_table())


def test_the_file_through_both_readers(table, tmp_path):
    temps, press = [500.0, 1234.5, 3000.0], [1e-9, 3e-3, 1.0, 1e3]
    r = chem.cho_chemistry(table, temps, press, [N_O, 5e-3], [0.55 * N_O, 6e-3], HE, "numpy", GAS)
    d = os.path.join(str(tmp_path), "fc")
    path = chem.write_fastchem_directory(d, temps, press, r, 1)
    assert path == os.path.join(d, "chem.dat")
    assert open(path).readline().split() == ["#P(bar)", "T(k)", "m(u)", "H2", "He", "H2O1", "C1O1", "C1H4", "C1O2", "C2H2"]
    names = ["mu", "H2", "He", "H2O1", "C1O1", "C1H4", "C1O2", "C2H2"]
    keys = ["mu"] + list(chem.SPECIES)
    reader = Read()
    reader.fastchem_path = d + "/"
    reader.load_fastchem_data()
    assert list(reader.fastchem_data.dtype.names) == ["Pbar", "Tk"] + names
    assert reader.fastchem_temp == temps and reader.fastchem_press == [p * 1e6 for p in press]
    mix = ktable_mix.Chemistry(d)
    assert np.array_equal(mix.temp, temps) and np.array_equal(mix.press, [p * 1e6 for p in press])
    for name, key in zip(names, keys):
        want = r[key][1].reshape(-1)                               # entry p + np * t
        assert np.asarray(reader._fastchem_column(name), np.float64).tobytes() == want.tobytes(), name
        assert mix.column(name).tobytes() == want.tobytes(), name
    assert mix.column("Pbar").tobytes() == np.tile(press, len(temps)).tobytes()
    assert mix.column("Tk").tobytes() == np.repeat(temps, len(press)).tobytes()


def test_sweep_numbering_and_the_printed_list(tmp_path, capsys):
    out = os.path.join(str(tmp_path), "grid")
    dirs = chem.main(["-gibbs_file", write_gibbs(tmp_path), "-temperature_grid", "500 3000 1250", "-pressure_grid", "-6 3 4",
                      "-output_directory", out, "-backend", "numpy", "-sweep", "c_to_o=0.3,0.55,1.1;metallicity=1,10"])
    assert dirs == ["%s_%d/" % (out, k) for k in range(6)]
    printed = capsys.readouterr().out.strip().splitlines()[-1]
    assert printed == "-sweep \"directory_with_fastchem_files=%s\"" % ",".join(dirs)
    # the first key slowest: directory 3 is C/O 0.55 at ten times the metallicity
    table = chem.read_gibbs_file(os.path.join(str(tmp_path), "gibbs.dat"))
    temps, press = 500.0 + 1250.0 * np.arange(3), 10.0 ** np.linspace(-6.0, 3.0, 4)
    for k, (co, z) in enumerate([(0.3, 1), (0.3, 10), (0.55, 1), (0.55, 10), (1.1, 1), (1.1, 10)]):
        n_o = z * chem.O_TO_H_SOLAR
        want = chem.cho_chemistry(table, temps, press, [n_o], [co * n_o], 0.085, "numpy")
        got = ktable_mix.Chemistry(dirs[k])
        assert got.column("C1H4").tobytes() == want["CH4"].reshape(-1).tobytes(), k
        assert got.column("mu").tobytes() == want["mu"].reshape(-1).tobytes(), k
    # what premix.py's -sweep takes
    from helios_amd import premix
    opt, _rest = premix.parse_args(["-sweep", printed[len("-sweep \""):-1]])
    assert opt.fastchem_dirs == dirs
    # and a single call writes the directory itself
    one = chem.main(["-gibbs_file", os.path.join(str(tmp_path), "gibbs.dat"), "-temperature_grid", "500 3000 1250",
                     "-pressure_grid", "-6 3 4", "-output_directory", out, "-backend", "numpy"])
    assert one == [out + "/"] and os.path.exists(out + "/chem.dat")


def test_grid_like_takes_the_nodes_of_a_container(tmp_path):
    import ktable_mix_reference as kr
    temps, press = np.array([600.0, 900.0, 2000.0]), np.array([1e1, 1e6, 1e8])
    nc = 4 * kr.N_GAUSS
    np.savez(os.path.join(str(tmp_path), "X_opac_ip_kdistr.npz"),
             **dict(kr.grid_arrays(), temperatures=temps, pressures=press, kpoints=np.ones(9 * nc)))
    out = os.path.join(str(tmp_path), "like")
    argv = ["-gibbs_file", write_gibbs(tmp_path), "-grid_like", os.path.join(str(tmp_path), "X_opac_ip_kdistr.npz"),
            "-output_directory", out, "-backend", "numpy"]
    chem.main(argv)
    got = ktable_mix.Chemistry(out)
    assert np.array_equal(got.temp, temps) and got.column("Pbar").tobytes() == np.tile(press * 1e-6, 3).tobytes()
    np.savez(os.path.join(str(tmp_path), "Y_opac_ip_kdistr.npz"),
             **dict(kr.grid_arrays(), temperatures=np.array([450.0, 900.0]), pressures=press, kpoints=np.ones(6 * nc)))
    with pytest.raises(ValueError, match="450"):
        chem.main(argv[:3] + [os.path.join(str(tmp_path), "Y_opac_ip_kdistr.npz")] + argv[4:])


def test_refusals_name_the_value_or_the_line(table, tmp_path):
    def gibbs(text):
        path = os.path.join(str(tmp_path), "bad.dat")
        with open(path, "w") as f:
            f.write(text)
        return path
    with pytest.raises(IOError, match="holds 1 rows"):
        chem.read_gibbs_file(gibbs("# T dG\n500 1 2 3\n"))
    with pytest.raises(IOError, match="line 3 .*finite"):
        chem.read_gibbs_file(gibbs("# T dG\n500 1 2 3\n600 1 nan 3\n"))
    with pytest.raises(IOError, match="line 2 .*finite"):
        chem.read_gibbs_file(gibbs("500 1 2 3\n600 1 2\n"))
    with pytest.raises(IOError, match="line 3 .*600.*does not lie above 600"):
        chem.read_gibbs_file(gibbs("500 1 2 3\n600 1 2 3\n600 1 2 3\n"))
    with pytest.raises(IOError, match="row 1.*does not lie above"):
        chem.GibbsTable([500.0, 400.0], [1, 2], [1, 2], [1, 2])
    with pytest.raises(IOError, match="holds 1 rows"):
        chem.GibbsTable([500.0], [1], [1], [1])
    with pytest.raises(IOError, match="row 0.*inf"):
        chem.GibbsTable([500.0, 600.0], [np.inf, 2], [1, 2], [1, 2])

    def run(temps=(800.0,), press=(1.0,), o=(N_O,), c=(N_O,), he=HE, tab=table):
        return chem.cho_chemistry(tab, temps, press, o, c, he, "numpy", GAS)
    with pytest.raises(ValueError, match="499.9.*outside"):
        run(temps=[800.0, 499.9])
    with pytest.raises(ValueError, match="3000.0000000000005.*outside"):
        run(temps=[np.nextafter(3000.0, 1e9)])
    with pytest.raises(ValueError, match="nan.*outside"):
        run(temps=[np.nan])
    for p in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="pressure %s" % ("-1.0" if p == -1.0 else repr(float(p)))):
            run(press=[1.0, p])
    for bad in (np.nan, np.inf, 0.0, -5e-4):
        with pytest.raises(ValueError, match="n_O = %s" % repr(float(bad))):
            run(o=[bad])
        with pytest.raises(ValueError, match="n_C = %s" % repr(float(bad))):
            run(c=[bad])
    for bad in (-0.1, np.nan):
        with pytest.raises(ValueError, match="He/H = %s" % repr(float(bad))):
            run(he=bad)
    with pytest.raises(ValueError, match="backend"):
        chem.cho_chemistry(table, [800.0], [1.0], [N_O], [N_O], HE, "eager", GAS)
    with pytest.raises(IOError, match="unknown key 'n_to_o'"):
        chem.parse_sweep("c_to_o=1,2;n_to_o=3")
    with pytest.raises(IOError, match="no list of numbers"):
        chem.parse_sweep("c_to_o=a,b")
    # more rows than the kernel stages: refused by both backends before anything runs
    many = chem.GibbsTable(500.0 + np.arange(chem.MAX_ROWS + 1), *[np.zeros(chem.MAX_ROWS + 1)] * 3)
    for backend in ("numpy", "device"):
        with pytest.raises(ValueError, match="%d Gibbs rows" % (chem.MAX_ROWS + 1)):
            chem.cho_chemistry(many, [800.0], [1.0], [N_O], [N_O], HE, backend, GAS)
    with pytest.raises(ValueError, match="nodes"):
        chem.cho_chemistry(table, np.linspace(500.0, 3000.0, 4097), np.logspace(-9, 3, 4097), [N_O], [N_O], HE, "device", GAS)


def test_a_directory_from_chem_py_goes_through_the_mixing_stage(tmp_path):
    """chem.py -> ktable.py -mixed_table_production yes -backend numpy with every species' mixing ratio from `FastChem`: the mixed
    table is the weighted sum of the containers with the weights x w / mu of the chemistry, and its mean molecular mass the
    chemistry's"""
    import ktable_mix_reference as kr
    from helios_amd import ktable
    root = str(tmp_path)
    temps, press_bar = 500.0 + 500.0 * np.arange(6), 10.0 ** np.linspace(-6.0, 3.0, 4)
    dirs = chem.main(["-gibbs_file", write_gibbs(tmp_path), "-temperature_grid", "500 3000 500", "-pressure_grid", "-6 3 4",
                      "-output_directory", os.path.join(root, "chem"), "-backend", "numpy", "-c_to_o", "1.1"])
    absorbers = ["H2O", "CO", "CH4", "CO2", "C2H2"]
    species = [("H2", "no", "yes", "FastChem"), ("He", "no", "yes", "FastChem")] + [(n, "yes", "no", "FastChem") for n in absorbers]
    grid = kr.grid_arrays()
    nc = len(grid["center wavelengths"]) * kr.N_GAUSS
    press = 10.0 ** np.linspace(0.0, 9.0, 4)
    rng = np.random.default_rng(3)
    tables = {n: 10.0 ** rng.uniform(-6, 2, len(temps) * len(press) * nc) for n in absorbers}
    cont = {n + "_opac_ip_kdistr": dict(grid, temperatures=temps, pressures=press, kpoints=tables[n]) for n in absorbers}
    kr.write_inputs(root, species, {}, cont, lambda stem, data: np.savez(stem + ".npz", **data))
    written = ktable.main(["-mixed_table_production", "yes", "-backend", "numpy", "-container", "npz",
                           "-path_to_final_species_file", os.path.join(root, "final_species.dat"),
                           "-path_to_fastchem_output", dirs[0], "-directory_with_individual_files", os.path.join(root, "opac"),
                           "-mixed_table_output_directory", os.path.join(root, "mixed"),
                           "-temperature_grid", "500 3000 500", "-pressure_grid", "0 9 4"])
    got = np.load(written[-1])
    r = chem.cho_chemistry(chem.read_gibbs_file(os.path.join(root, "gibbs.dat")), temps, press_bar,
                           [chem.O_TO_H_SOLAR], [1.1 * chem.O_TO_H_SOLAR], 0.085, "numpy")
    mu = r["mu"][0].reshape(-1)
    # (the chemistry's nodes are the table's but for a rounding of 1e6 * 10^x against 10^(x + 6), where the stage interpolates)
    assert np.max(np.abs(got["meanmolmass"] / mu - 1)) < 1e-9
    w = dict(zip(chem.SPECIES, chem.weights()))
    want = sum((r[n][0].reshape(-1) * w[n] / mu)[:, None] * tables[n].reshape(len(mu), nc) for n in absorbers)
    assert np.max(np.abs(got["kpoints"].reshape(len(mu), nc) / want - 1)) < 1e-9
    assert [str(n) for n in got["included molecules"]] == absorbers
