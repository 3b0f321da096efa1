"""What tests/test_gpu_chem.py and tools/chem_parity.py share: Gibbs tables of 2 rows, the golden's 26 and the kernel's limit, the
(T, P) points and abundances at the contract's edges, their long-double restatement (computed once per table), and the chain
chem.py -> ktable.py -mixed_table_production yes."""
import os

import numpy as np

import chem_reference as cr
import ktable_mix_reference as kr
from helios_amd import chem

HE = 0.085
N_O = 5e-4
# C/O = 1 and a rounding beside it, the ends of the range, and a solar-like value
C_TO_O = (1.0, 1.0 - 1e-12, 1.0 + 1e-12, 1e-6, 10.0, 0.55)
ABSORBERS = ("H2O", "CO", "CH4", "CO2", "C2H2")


def gas_constant():
    return float(cr.golden()["gas_constant"])


def gibbs_table(rows):
    """2: the golden's first and last row; 26: the golden; else `rows` temperatures between them, dG linear in the golden's"""
    t, g1, g2, g3 = cr.golden_table()
    if rows == len(t):
        return t, g1, g2, g3
    if rows == 2:
        return tuple(np.array([a[0], a[-1]]) for a in (t, g1, g2, g3))
    tt = np.linspace(t[0], t[-1], rows)
    return (tt,) + tuple(np.interp(tt, t, g) for g in (g1, g2, g3))


def points(table):
    """(T, P [bar]): T on a row and one ulp to either side, the first and the last row and one ulp inside them, a T between
    rows; the all-methane limit at the first row and 1e3 bar; the last row at 1e-9 bar, where the root lies tens of orders of
    magnitude below 2 n_C"""
    t = np.asarray(table[0])
    mid = t[(len(t) - 1) // 2] if len(t) > 2 else 0.5 * (t[0] + t[-1])
    between = 0.25 * t[0] + 0.75 * t[-1] + 0.123
    return [(t[0], 1e3), (t[-1], 1e-9), (mid, 1.0), (np.nextafter(mid, 0.0), 1.0), (np.nextafter(mid, 1e9), 1.0),
            (t[0], 1.0), (np.nextafter(t[0], 1e9), 1e-3), (t[-1], 1e3), (np.nextafter(t[-1], 0.0), 1.0), (between, 1e-3),
            (t[-1], 1e-6), (t[0], 1e-9)]


def nodes(table, n):
    """n nodes that walk through the points"""
    p = points(table)
    return (np.array([p[i % len(p)][0] for i in range(n)]), np.array([p[i % len(p)][1] for i in range(n)]))


_RESTATED = {}


def restated(rows):
    """(want [chem][8][point] in long double, eps [chem][8][point]: the numpy backend's deviation) for the table of `rows` rows"""
    if rows not in _RESTATED:
        table = gibbs_table(rows)
        pts, w, gas = points(table), chem.weights(), gas_constant()
        want = np.zeros((len(C_TO_O), len(cr.KEYS), len(pts)), np.longdouble)
        eps = np.zeros(want.shape)
        for ic, co in enumerate(C_TO_O):
            for ip, (t, p) in enumerate(pts):
                ld = cr.node(table, t, p, N_O, co * N_O, HE, gas, w)
                mine = chem.numpy_nodes(table, [t], [p], [N_O], [co * N_O], HE, gas)
                for ik, k in enumerate(cr.KEYS):
                    want[ic, ik, ip] = ld[k]
                    eps[ic, ik, ip] = cr.deviation(mine[k][0, 0, 0], ld[k])
        _RESTATED[rows] = (want, eps)
    return _RESTATED[rows]


# ---- the chain ------------------------------------------------------------------------------------------------------------------
CHAIN_T = "500 3000 500"
CHAIN_P_BAR, CHAIN_P_CGS = "-6 3 4", "0 9 4"


def chain_inputs(root, seed=3):
    """a Gibbs file, a species file with every mixing ratio from FastChem and containers of the five absorbers on the chain's
    6 x 4 nodes, 4 bins x 3 Gauss points; returns (Gibbs file, the absorbers' tables)"""
    os.makedirs(root, exist_ok=True)
    gibbs = chem.write_gibbs_file(os.path.join(root, "gibbs.dat"), *cr.golden_table())
    species = [("H2", "no", "yes", "FastChem"), ("He", "no", "yes", "FastChem")] + [(n, "yes", "no", "FastChem") for n in ABSORBERS]
    grid = kr.grid_arrays()
    nc = len(grid["center wavelengths"]) * kr.N_GAUSS
    temps, press = 500.0 + 500.0 * np.arange(6), 10.0 ** np.linspace(0.0, 9.0, 4)
    rng = np.random.default_rng(seed)
    tables = {n: 10.0 ** rng.uniform(-6, 2, len(temps) * len(press) * nc) for n in ABSORBERS}
    cont = {n + "_opac_ip_kdistr": dict(grid, temperatures=temps, pressures=press, kpoints=tables[n]) for n in ABSORBERS}
    kr.write_inputs(root, species, {}, cont, lambda stem, data: np.savez(stem + ".npz", **data))
    return gibbs, tables


def chain_chemistry(root, gibbs, backend, name, c_to_o="1.1"):
    return chem.main(["-gibbs_file", gibbs, "-temperature_grid", CHAIN_T, "-pressure_grid", CHAIN_P_BAR, "-c_to_o", c_to_o,
                      "-output_directory", os.path.join(root, name), "-backend", backend])[0]


def chain_mix(root, chem_dir, backend, out):
    from helios_amd import ktable
    written = ktable.main(["-mixed_table_production", "yes", "-backend", backend, "-container", "npz",
                           "-path_to_final_species_file", os.path.join(root, "final_species.dat"),
                           "-path_to_fastchem_output", chem_dir, "-directory_with_individual_files", os.path.join(root, "opac"),
                           "-mixed_table_output_directory", os.path.join(root, out),
                           "-temperature_grid", CHAIN_T, "-pressure_grid", CHAIN_P_CGS])
    return np.load(written[-1])


def chain_bound(tolerance=1e-13):
    """the bound on the relative difference of two mixed tables whose chemistries agree within `tolerance` per entry, and of
    their mean molecular masses.  The mixing stage interpolates every column in (T, log P) with weights >= 0 that are the same
    in both runs, so a column of positive numbers keeps its relative deviation, `tolerance`.  An absorber's weight is
    x w / mu: tolerance (x) + tolerance (mu) to first order.  kpoints is a sum of positive terms weight * table, whose relative
    deviation is at most the largest of its terms' -- bounded here, as a sum is, by the weights' deviations summed over the
    absorbers.  On top, each run rounds: two interpolations of four products and three sums, a product and a quotient per
    weight, a product and a sum per absorber -- under 16 roundings per absorber in each run, and 16 for mu."""
    rounding = 2.0 ** -52
    k = len(ABSORBERS) * (2 * tolerance) + 2 * 16 * len(ABSORBERS) * rounding
    return k, tolerance + 2 * 16 * rounding


def chain_difference(root):
    """the largest relative difference of kpoints and of meanmolmass between the mixed tables (device mixing stage) of a
    chemistry from the device and one from the numpy backend"""
    gibbs, _tables = chain_inputs(root)
    dev = chain_mix(root, chain_chemistry(root, gibbs, "device", "chem_device"), "hip", "mixed_device")
    host = chain_mix(root, chain_chemistry(root, gibbs, "numpy", "chem_numpy"), "hip", "mixed_numpy")
    out = {}
    for k in ("kpoints", "meanmolmass"):
        a, b = np.asarray(dev[k], np.float64).reshape(-1), np.asarray(host[k], np.float64).reshape(-1)
        assert a.shape == b.shape and np.all(b > 0), k
        out[k] = float(np.max(np.abs(a - b) / b))
    return out
