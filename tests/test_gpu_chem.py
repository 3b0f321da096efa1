"""k_chem_nodes (csrc/chem.hip, helios_amd/chem.py) on the device against the long-double restatement of the contract
(tests/chem_reference.py) under the rule of the table tools: every entry within max(1e-13, 8 eps), eps the numpy backend's
deviation at that entry.  Node counts from the workgroup of 256 and the wavefront of 64; 1 and 3 chemistries per launch; Gibbs
tables of 2 rows, 26 rows and the kernel's limit; temperatures on a row and one ulp beside it, on the first and the last row;
C/O = 1 and 1 +- 1e-12, 1e-6 and 10; all carbon in methane at 500 K and 1e3 bar; 3000 K at 1e-9 bar, where the root lies tens of
orders of magnitude below its bracket (tests/chem_cases.py).  Then bits that repeat, refusals that launch nothing, and the chain
into the mixing stage of ktable.py."""
import numpy as np
import pytest

import chem_cases as cc
import chem_reference as cr
from helios_amd import chem
from helios_amd._lib import HeliosHipError

pytestmark = pytest.mark.gpu

WG, WAVE = chem.THREADS, 64
SIZES = [1, WAVE - 1, WAVE, WAVE + 1, WG - 1, WG, WG + 1, 3 * WG + 71]


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def device_run(ctx, rows, n, chems, handle=None):
    """vmr [chem][8][n] for the chemistries `chems` (indices into cc.C_TO_O)"""
    table = cc.gibbs_table(rows)
    h = handle or chem.ChemDevice(ctx, rows, n, len(chems))
    try:
        if handle is None:
            h.set_table(table, cc.gas_constant())
            h.set_nodes(*cc.nodes(table, n))
        co = np.array([cc.C_TO_O[c] for c in chems])
        h.run(np.full(len(chems), cc.N_O), co * cc.N_O, cc.HE)
        return h.get("vmr")
    finally:
        if handle is None:
            h.close()


def held(vmr, rows, chems, what):
    want, eps = cc.restated(rows)
    n_points = want.shape[2]
    worst = 0.0
    for row, c in enumerate(chems):
        for k in range(len(cr.KEYS)):
            for i in range(vmr.shape[2]):
                p = i % n_points
                dev = cr.deviation(vmr[row, k, i], want[c, k, p])
                assert dev <= max(1e-13, 8 * eps[c, k, p]), (what, cc.C_TO_O[c], cr.KEYS[k], i, dev, eps[c, k, p])
                worst = max(worst, dev)
    print("%s: largest deviation %.3e (numpy backend: %.3e)" % (what, worst, eps.max()))


@pytest.mark.parametrize("n", SIZES)
def test_every_edge_at_every_size(ctx, n):
    first, second = device_run(ctx, 26, n, [0, 1, 2]), device_run(ctx, 26, n, [3, 4, 5])
    held(first, 26, [0, 1, 2], "%d nodes, C/O 1 and beside" % n)
    held(second, 26, [3, 4, 5], "%d nodes, C/O 1e-6, 10, 0.55" % n)
    # a row of a three-chemistry launch is that chemistry run alone, bit for bit
    for row, c in ((1, 1), (2, 5)):
        alone = device_run(ctx, 26, n, [c])
        held(alone, 26, [c], "%d nodes, one chemistry" % n)
        assert alone[0].tobytes() == (first, second)[c // 3][row].tobytes(), (n, c)


@pytest.mark.parametrize("rows", [2, 26, chem.MAX_ROWS])
def test_gibbs_tables_of_two_rows_to_the_limit(ctx, rows):
    n = WG + 1
    held(device_run(ctx, rows, n, [0, 4, 5]), rows, [0, 4, 5], "%d Gibbs rows" % rows)
    held(device_run(ctx, rows, n, [3]), rows, [3], "%d Gibbs rows, one chemistry" % rows)


def test_the_limits_are_where_the_cases_say(ctx):
    """all carbon in methane at the first point, and a root more than twenty orders below 2 n_C at the second"""
    vmr = device_run(ctx, 26, 2, [5])
    n_ch4 = vmr[0, 4] / vmr[0, 0]
    assert abs(n_ch4[0] / (2 * 0.55 * cc.N_O) - 1) < 1e-12
    assert 0 < n_ch4[1] < 1e-20 * (2 * 0.55 * cc.N_O)


def test_a_launch_repeated_gives_the_same_bits(ctx):
    n = 3 * WG + 71
    table = cc.gibbs_table(26)
    h = chem.ChemDevice(ctx, 26, n, 3)
    try:
        h.set_table(table, cc.gas_constant())
        h.set_nodes(*cc.nodes(table, n))
        a = device_run(ctx, 26, n, [0, 3, 4], h)
        b = device_run(ctx, 26, n, [0, 3, 4], h)
        assert a.tobytes() == b.tobytes()
        assert h.get("timing_ms")[1] == 2
    finally:
        h.close()
    assert device_run(ctx, 26, n, [0, 3, 4]).tobytes() == a.tobytes()


def test_the_library_function_on_the_device(ctx):
    table = chem.GibbsTable(*cc.gibbs_table(26))
    temps, press = [500.0, 800.0, 1234.5, 3000.0], [1e-9, 1e-3, 1.0, 1e3]
    o, c = [cc.N_O, 5e-3], [0.55 * cc.N_O, 6e-3]
    timing = {}
    dev = chem.cho_chemistry(table, temps, press, o, c, cc.HE, "device", cc.gas_constant(), ctx, timing)
    host = chem.cho_chemistry(table, temps, press, o, c, cc.HE, "numpy", cc.gas_constant())
    assert sorted(dev) == sorted(chem.KEYS) and timing["kernel_ms"] > 0
    for k in chem.KEYS:
        assert dev[k].shape == (2, 4, 4) and dev[k].dtype == np.float64
        assert np.max(np.abs(dev[k] / host[k] - 1)) <= 1e-13, k


def test_the_handles_refusals_launch_nothing(ctx):
    table = cc.gibbs_table(26)
    gas = cc.gas_constant()
    with pytest.raises(ValueError, match="%d Gibbs rows" % (chem.MAX_ROWS + 1)):
        chem.ChemDevice(ctx, chem.MAX_ROWS + 1, 4, 1)
    h = chem.ChemDevice(ctx, 26, 4, 2)
    try:
        with pytest.raises(HeliosHipError, match="no Gibbs rows"):
            h.set_nodes([800.0], [1.0])
        with pytest.raises(HeliosHipError, match="27 Gibbs rows, the handle holds 2 ... 26"):
            h.set_table(cc.gibbs_table(27), gas)
        with pytest.raises(HeliosHipError, match="row 1: T = 500 does not lie above 500"):      # past the Python class's own check
            h._call("set_table", 2, *[chem.dp(np.array(a)) for a in ([500.0, 500.0], [1.0, 2.0], [1.0, 2.0], [1.0, 2.0])] + [gas])
        h.set_table(table, gas)
        with pytest.raises(HeliosHipError, match="no nodes"):
            h.run([cc.N_O], [cc.N_O], cc.HE)
        with pytest.raises(HeliosHipError, match="5 nodes, the handle holds 1 ... 4"):
            h.set_nodes([800.0] * 5, [1.0] * 5)
        with pytest.raises(HeliosHipError, match="node 1: T = 499.8999.* lies outside the Gibbs rows 500 ... 3000"):
            h.set_nodes([800.0, 499.9], [1.0, 1.0])
        with pytest.raises(HeliosHipError, match="node 1: P = 0 "):
            h.set_nodes([800.0, 900.0], [1.0, 0.0])
        h.set_nodes([800.0, 900.0], [1.0, 1e-3])
        h.run([cc.N_O], [0.55 * cc.N_O], cc.HE)
        good = h.get("vmr")
        assert h.get("timing_ms")[1] == 1
        refused = [(([cc.N_O] * 3, [cc.N_O] * 3, cc.HE), "3 chemistries, the handle holds 1 ... 2"),
                   (([cc.N_O, np.nan], [cc.N_O, cc.N_O], cc.HE), "chemistry 1: n_O = nan"),
                   (([cc.N_O], [0.0], cc.HE), "chemistry 0: n_C = 0 "),
                   (([cc.N_O], [-1e-4], cc.HE), "chemistry 0: n_C = -0.0001"),
                   (([np.inf], [cc.N_O], cc.HE), "chemistry 0: n_O = inf"),
                   (([cc.N_O], [cc.N_O], -0.1), "He/H = -0.1")]
        for args, message in refused:
            with pytest.raises(HeliosHipError, match=message):
                h.run(*args)
            assert h.get("timing_ms")[1] == 1, message                   # nothing was launched
            with pytest.raises(HeliosHipError, match="no chemistry has been run"):
                h.get("vmr")
        with pytest.raises(HeliosHipError, match="unknown name"):
            h.get("n_CH4")
        h.run([cc.N_O], [0.55 * cc.N_O], cc.HE)
        assert h.get("vmr").tobytes() == good.tobytes() and h.get("timing_ms")[1] == 2
    finally:
        h.close()


def test_the_chain_into_the_mixing_stage(tmp_path):
    """chem.py on the device and with the numpy backend, both through ktable.py -mixed_table_production yes on the device: the
    mixed tables and their mean molecular masses differ by no more than the chemistry's tolerance implies (cc.chain_bound)"""
    diff = cc.chain_difference(str(tmp_path))
    k_bound, mu_bound = cc.chain_bound()
    print("kpoints %.3e (bound %.3e), meanmolmass %.3e (bound %.3e)" % (diff["kpoints"], k_bound, diff["meanmolmass"], mu_bound))
    assert diff["kpoints"] <= k_bound and diff["meanmolmass"] <= mu_bound
