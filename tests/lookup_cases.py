"""TEST INFRASTRUCTURE: crafted tables and columns that put the levels of the (T, log10 P) table look-up on its edges.  No GPU
here: tests/test_lookup_cases.py proves on the restatement (tests/lookup_reference.py) and the CPU oracle that every case takes
the branches it is named for, tests/test_gpu_lookup_edges.py runs the same cases through the three copies of the look-up.

The grid.  Nodes that fp64 holds exactly: ktemp = 100 + 250 i (i = 0 ... 6: dt = 250 exactly, so t is exact wherever T - 100 is
a multiple of 250 / 2^n), kpress = 10^(2 j) (j = 0 ... 5).

The tables.  k-table, Rayleigh table and mean-mass table all vary from node to node: a trend over (T, P) times a seeded factor
in [0.95, 1.05] per node and entry.  The k-table's trend is the synthetic one (helios_amd/synthetic.py) with the pressure slope
flattened from 0.3 to 0.25 per decade: neighbours along P (two decades apart) then differ by at most 10^0.5 * 1.05 / 0.95 = 3.5,
under the factor 4 that the log10 cap of tests/test_lookup_cases.py is worked out for; along T by 10^-0.05 = 0.89.  The Rayleigh
and the mean-mass table are constant in the synthetic set; here they rise by 1.5 per pressure node and fall by 0.85 per
temperature node.  With these steps any two corners of a cell differ by more than 1 % at every entry, whatever the factors
(corner_separation measures it): a wrong corner or a wrong weight moves a value by far more than the tolerance.

The levels.  T_CLASSES and P_CLASSES name the edges.  A level ON a pressure node may come out on either side of it on the
device (log10), so on that axis only values are held; T on a node is exact.

The ladder batch.  One strictly descending pressure ladder p_int[i] > p_lay[i] > p_int[i + 1] through every P class; the two
nextafter neighbours of a node cannot both be layer centres next to a centre on the node (no fp64 lies between), so the
centres up(1e4), down(1e4) have the node 1e4 as the interface between them, and the centre ON a node is 1e6, its interfaces
up(1e6) and down(1e6).  T_PATTERN -- the T classes and the pair (node - 64, node + 64), whose interface is the node exactly --
is laid over the layers, rotated by one per column, in as many columns as the pattern is long: every (T class, P class) pair
is a layer centre somewhere, and every kernel's per-column indexing is in the test.

The walks.  Aimed at the corner cache of the coefficient kernel's fused look-up, where a thread walks ceil(nlev / k) consecutive
levels and reloads the four corners only when (tdown, tup, pdown, pup) change.  WALKS lists (layers, isothermal, knobs, the
k of flux_tiling() the length is chosen for); every length carries the PATTERNS, one column each, over a slow pressure descent.
"""
import numpy as np

import cases
from helios_amd import phys_const as pc
from helios_amd import synthetic as syn

NBIN, NY, NY_SPECIES = 5, 4, 20
KTEMP = 100.0 + 250.0 * np.arange(7)
KPRESS = np.array([1.0, 1e2, 1e4, 1e6, 1e8, 1e10])
NODE_T, NODE_I = 850.0, 3              # the interior temperature node of the classes, and its index
NODE_P = 1e4
SEED = 20260


def _up(v):
    return float(np.nextafter(v, np.inf))


def _down(v):
    return float(np.nextafter(v, -np.inf))


# half a margin = 0.0005 cell = 0.125 K
T_CLASSES = dict(below=50.0, first_node=100.0, inside_first=100.125, mid_cell=475.0, node_below=_down(NODE_T), node=NODE_T,
                 node_above=_up(NODE_T), inside_last=1599.875, last_node=1600.0, above=1700.0)
P_CLASSES = dict(below=0.1, first_node=1.0, off_node=3e3, node_below=_down(NODE_P), node=NODE_P, node_above=_up(NODE_P),
                 last_node=1e10, above=1e11)
T_PATTERN = list(T_CLASSES.values()) + [NODE_T - 64.0, NODE_T + 64.0]
LADDER_P_LAY = [1e11, 1e10, 3e8, 1e6, _up(1e4), _down(1e4), 3e3, 1.0, 0.1, 0.01]
LADDER_P_INT = [2e11, 3e10, 1e9, _up(1e6), _down(1e6), 1e4, 5e3, 1e2, 0.5, 0.05, 0.001]
LADDER_P_CLASS = ["above", "last_node", "off_node", "node", "node_above", "node_below", "off_node", "first_node", "below", "below"]

# name: (layers, isothermal, knobs of the batch, lanes per spectral point k the tiling has then)
WALKS = {"L17_k8": (17, 0, {"HELIOS_RT_K": 8}, 8), "L33": (33, 0, {}, 16), "L200": (200, 0, {}, 32), "L400": (400, 0, {}, 64),
         "iso20": (20, 1, {}, 8), "L2": (2, 0, {}, 8)}
PATTERNS = ("one_cell", "zigzag", "node_above", "node_below", "on_node")

_kept = {}


def _trend_tables(rng, ny, gauss_y):
    nt, npr = len(KTEMP), len(KPRESS)
    kxy, _ = syn.ktable_factors(rng, NBIN, ny, KTEMP, KPRESS, gauss_y)                    # [x][y] flat
    ftp = 10.0 ** (0.25 * (np.log10(KPRESS)[None, :] - 6.0) - 0.2 * (KTEMP[:, None] / 1000.0))  # [t][p]
    k = ftp[:, :, None] * kxy[None, None, :] * rng.uniform(0.95, 1.05, (nt, npr, NBIN * ny))
    return k


def _frame(nlayer, iso, ny=NY, seed=SEED):
    """cases.make_case's frame on the grid of this module with the three varying tables"""
    c = cases.make_case(nbin=NBIN, nlayer=nlayer, ny=ny, ntemp=len(KTEMP), npress=len(KPRESS), iso=iso, seed=seed)
    rng = np.random.default_rng(seed)
    nt, npr = len(KTEMP), len(KPRESS)
    c.ktemp, c.kpress = KTEMP.copy(), KPRESS.copy()
    c.opac_k = _trend_tables(rng, ny, c.gauss_y).reshape(-1)
    step = (1.5 ** np.arange(npr))[None, :] * (0.85 ** np.arange(nt))[:, None]          # [t][p]
    ray = 1e-24 * (1e-4 / c.opac_wave) ** 4                                              # (the boosted Rayleigh of make_case)
    c.opac_scat_cross = (step[:, :, None] * ray[None, None, :] * rng.uniform(0.95, 1.05, (nt, npr, NBIN))).reshape(-1)
    c.opac_meanmass = (step * 2.3 * pc.AMU * rng.uniform(0.95, 1.05, (nt, npr))).reshape(-1)
    return c


def _set_pressures(c, p_lay, p_int):
    c.p_lay, c.p_int = np.array(p_lay, np.float64), np.array(p_int, np.float64)
    assert np.all(c.p_int[:-1] > c.p_lay) and np.all(c.p_lay > c.p_int[1:])
    c.delta_colmass = (c.p_int[:-1] - c.p_int[1:]) / c.g
    c.delta_col_upper = (c.p_lay - c.p_int[1:]) / c.g
    c.delta_col_lower = (c.p_int[:-1] - c.p_lay) / c.g


def corner_separation(table, tail):
    """the smallest relative difference between any two of the four corners of any (T, P) cell, over every entry"""
    a = np.asarray(table, np.float64).reshape((len(KTEMP), len(KPRESS)) + tail)
    cs = [a[:-1, :-1], a[:-1, 1:], a[1:, :-1], a[1:, 1:]]
    worst = np.inf
    for i in range(4):
        for j in range(i + 1, 4):
            worst = min(worst, float(np.min(np.abs(cs[i] - cs[j]) / np.maximum(np.abs(cs[i]), np.abs(cs[j])))))
    return worst


def pressure_neighbour_ratio(table, tail):
    a = np.asarray(table, np.float64).reshape((len(KTEMP), len(KPRESS)) + tail)
    r = a[:, 1:] / a[:, :-1]
    return float(np.max(np.maximum(r, 1.0 / r)))


def free_levels():
    """the full cross product of the T and P classes as free levels: (T, P, T class, P class)"""
    names = [(tn, pn) for tn in T_CLASSES for pn in P_CLASSES]
    return (np.array([T_CLASSES[t] for t, _ in names]), np.array([P_CLASSES[p] for _, p in names]),
            [t for t, _ in names], [p for _, p in names])


def ladder(ny=NY):
    """the ladder batch: a case with c.T_cols [columns][nlayer + 1], the layer temperatures of every column"""
    key = ("ladder", ny)
    if key not in _kept:
        L, n = len(LADDER_P_LAY), len(T_PATTERN)
        c = _frame(L, 0, ny)
        _set_pressures(c, LADDER_P_LAY, LADDER_P_INT)
        c.T_cols = np.array([[T_PATTERN[(i + col) % n] for i in range(L + 1)] for col in range(n)])
        c.T_lay = c.T_cols[0].copy()
        c.name, c.env, c.k_expected = "ladder", {}, 8
        _kept[key] = c
    return _kept[key].copy()


def walk_temperatures(pattern, n):
    """n layer temperatures (and one for the surface) of a pattern"""
    i = np.arange(n + 1)
    if pattern == "one_cell":            # cell (1, 2): 350 ... 600
        return 360.0 + 230.0 * i / (n + 1.0)
    if pattern == "zigzag":              # a new cell at every level (cells 1 ... 5: the end interfaces stay above 0 K)
        return 100.0 + 250.0 * (np.array([1, 2, 3, 4, 5, 4, 3, 2])[i % 8] + 0.3 + 0.4 * i / (n + 1.0))
    if pattern == "node_above":          # ON the node, then in the cell above it: tup alone changes
        return np.where(i % 2 == 0, NODE_T, NODE_T + 60.0 + 100.0 * i / (n + 1.0))
    if pattern == "node_below":          # ON the node, then in the cell below it: tdown alone changes
        return np.where(i % 2 == 0, NODE_T, NODE_T - 60.0 - 100.0 * i / (n + 1.0))
    if pattern == "on_node":             # on a node throughout, three levels each
        return KTEMP[1 + (i // 3) % 5].copy()
    raise KeyError(pattern)


def walk(name):
    """the walk batch of one length: one column per pattern of PATTERNS over a slow descent inside the table"""
    if name not in _kept:
        L, iso, env, k = WALKS[name]
        c = _frame(L, iso)
        nodes = 10.0 ** (9.9 - 9.6 * np.arange(2 * L + 1) / (2.0 * L))        # 10^9.9 ... 10^0.3
        _set_pressures(c, nodes[1::2], nodes[0::2])
        c.T_cols = np.array([walk_temperatures(p, L) for p in PATTERNS])
        c.T_lay = c.T_cols[0].copy()
        c.name, c.env, c.k_expected = name, dict(env), k
        _kept[name] = c
    return _kept[name].copy()


def run_lengths(c):
    """(levels per run of the layer pass, of the interface pass) of the fused look-up at the tiling the case is chosen for"""
    k = c.k_expected
    return -(-c.nlayer // k), -(-(c.nlayer + 1) // k)


def species_ladder():
    """the ladder batch with 20 Gauss points and a species set for on-the-fly mixing: one absorber, one CIA-flagged absorber
    (both mixed correlated-k: random overlap does not enter) and H2 as the scatterer; mixing ratios that change from level to
    level.  The layer centre with P == kpress[0] has a numerator of p that is exactly 0 whatever log10 returns: with T on the
    node (column ON_NODE_FIRST_P[0], layer ON_NODE_FIRST_P[1]) the look-up without the margin takes the one-term branch"""
    if "species" not in _kept:
        c = ladder(NY_SPECIES)
        rng = np.random.default_rng(SEED + 1)
        L, I = c.nlayer, c.nlayer + 1
        sp = []
        for name, weight, cia in (("ABS", 18.0153, False), ("CIA_H2H2", 4.032, True)):
            sp.append(dict(name=name, absorbing=True, scattering=False, is_h2o=False, is_cia=cia, weight=weight,
                           pretab=_trend_tables(rng, NY_SPECIES, c.gauss_y).reshape(-1), scat=None))
        sp.append(dict(name="H2", absorbing=False, scattering=True, is_h2o=False, is_cia=False, weight=2.016, pretab=None,
                       scat=1e-24 * (1e-4 / c.opac_wave) ** 4))
        c.species = sp
        base = np.array([0.1, 0.05, 0.85])
        c.vmr_lay = base[:, None] * (1.0 + 0.01 * np.arange(L))[None, :]
        c.vmr_int = base[:, None] * (1.0 + 0.01 * np.arange(I) - 0.005)[None, :]
        c.name = "species_ladder"
        _kept["species"] = c
    return _kept["species"].copy()


COLUMN_LAYERS = (2, 65)                 # the column batch: the shortest column, and one level past a 64-thread block
ENTR_TEMP, ENTR_PRESS = np.linspace(100.0, 4000.0, 8), np.logspace(0, 11, 7)


def column_batch(L):
    """three columns whose per-column inputs all differ: temperatures (one walk pattern each), the premixed table set
    (c.second_set = (k, Rayleigh, mean mass) from another seed, read by column 1 alone: c.col_set) and the time step (column 1
    has physical_tstep == 0: c.columns); a kappa / c_p table on a grid of its own (c.entr_*)"""
    key = ("columns", L)
    if key not in _kept:
        c = _frame(L, 0)
        nodes = 10.0 ** (9.9 - 9.6 * np.arange(2 * L + 1) / (2.0 * L))
        _set_pressures(c, nodes[1::2], nodes[0::2])
        c.T_cols = np.array([walk_temperatures(p, L) for p in ("zigzag", "node_above", "on_node")])
        c.T_lay = c.T_cols[0].copy()
        other = _frame(L, 0, seed=SEED + 7)
        c.second_set = (other.opac_k, other.opac_scat_cross, other.opac_meanmass)
        c.col_set = (0, 1, 0)
        c.columns = [dict(physical_tstep=2e-3), dict(physical_tstep=0.0), dict(physical_tstep=1e-3)]
        tt, pp = np.meshgrid(ENTR_TEMP, ENTR_PRESS, indexing="ij")
        c.entr_temp, c.entr_press = ENTR_TEMP.copy(), ENTR_PRESS.copy()
        c.entr_kappa = (0.2 + 0.1 * tt / 4000.0 + 0.005 * np.log10(pp)).reshape(-1)
        c.entr_c_p = (3.5 * pc.R_UNIV * (1.0 + 0.5 * tt / 4000.0 + 0.005 * np.log10(pp))).reshape(-1)
        c.name, c.env = "columns_L%d" % L, {}
        _kept[key] = c
    return _kept[key].copy()


_first_p = LADDER_P_LAY.index(1.0)
ON_NODE_FIRST_P = ((T_PATTERN.index(NODE_T) - _first_p) % len(T_PATTERN), _first_p)       # (column, layer)
