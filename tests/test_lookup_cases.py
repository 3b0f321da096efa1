"""Proofs on the CPU that the crafted tables and columns of tests/lookup_cases.py are what they are named for, that the fp64
restatement of tests/lookup_reference.py is the CPU oracle's look-up, and that the one thing the restatement cannot know about
the device -- the last units of its log10 -- stays under a quarter of the tolerance floor."""
import numpy as np
import pytest

import lines_cases
import lookup_cases as lc
import lookup_reference as lk
from helios_amd import phys_const as pc


def _all_levels(c):
    """(T, P) of every layer centre and interface of every column of a batch case; interfaces get interface_T"""
    T, P = [], []
    for Tc in c.T_cols:
        T.append(Tc[:c.nlayer])
        P.append(c.p_lay)
        if not c.iso:
            T.append(lk.interface_T(Tc, c.nlayer))
            P.append(c.p_int)
    return np.concatenate(T), np.concatenate(P)


def test_constants_and_grid():
    assert lk.AMU == pc.AMU
    assert np.array_equal(lc.KTEMP, [100.0, 350.0, 600.0, 850.0, 1100.0, 1350.0, 1600.0])
    assert (lc.KTEMP[-1] - lc.KTEMP[0]) / (len(lc.KTEMP) - 1.0) == 250.0
    assert np.array_equal(lk.log10_libm(lc.KPRESS), [0.0, 2.0, 4.0, 6.0, 8.0, 10.0])
    assert lc.KTEMP[lc.NODE_I] == lc.NODE_T


@pytest.mark.parametrize("ny", [lc.NY, lc.NY_SPECIES])
def test_tables_vary_from_node_to_node(ny):
    """any two corners of a cell differ by >= 1 % at every entry; pressure neighbours by at most a factor 4"""
    c = lc.species_ladder() if ny == lc.NY_SPECIES else lc.ladder()
    tabs = [("k", c.opac_k, (c.nbin * ny,)), ("rayleigh", c.opac_scat_cross, (c.nbin,)), ("meanmass", c.opac_meanmass, ())]
    if ny == lc.NY_SPECIES:
        tabs += [(sp["name"], sp["pretab"], (c.nbin * ny,)) for sp in c.species if sp["absorbing"]]
    for name, tab, tail in tabs:
        sep, ratio = lc.corner_separation(tab, tail), lc.pressure_neighbour_ratio(tab, tail)
        print("%s: corners differ by >= %.3f, pressure neighbours by <= %.3f" % (name, sep, ratio))
        assert sep >= 0.01 and ratio <= 4.0, (name, sep, ratio)


@pytest.mark.parametrize("margin", [True, False])
def test_branch_census_of_the_free_levels(margin):
    """the cross product of the classes takes all four blend branches and both clamps on each axis; T on a node is exact"""
    T, P, tn, pn = lc.free_levels()
    assert len(T) == len(lc.T_CLASSES) * len(lc.P_CLASSES)
    k = lk.locate(T, P, lc.KTEMP, lc.KPRESS, margin)
    assert set(lk.branch(k).tolist()) == {0, 1, 2, 3}
    nt, npr = len(lc.KTEMP), len(lc.KPRESS)
    lo, hi_t, hi_p = (0.001, nt - 1.001, npr - 1.001) if margin else (0.0, nt - 1.0, npr - 1.0)
    assert np.any(k["t"] == lo) and np.any(k["t"] == hi_t) and np.any(k["p"] == lo) and np.any(k["p"] == hi_p)
    tn, pn = np.array(tn), np.array(pn)
    for cls, want in (("below", lo), ("first_node", lo), ("inside_first", lo if margin else 0.0005), ("mid_cell", 1.5),
                      ("node", float(lc.NODE_I)), ("inside_last", hi_t if margin else 5.9995), ("last_node", hi_t),
                      ("above", hi_t)):
        assert np.all(k["t"][tn == cls] == want), (cls, k["t"][tn == cls], want)
    on = tn == "node"
    assert np.all(k["tdown"][on] == lc.NODE_I) and np.all(k["tup"][on] == lc.NODE_I)
    assert np.all(k["tdown"][tn == "node_below"] == lc.NODE_I - 1) and np.all(k["tup"][tn == "node_below"] == lc.NODE_I)
    assert np.all(k["tdown"][tn == "node_above"] == lc.NODE_I) and np.all(k["tup"][tn == "node_above"] == lc.NODE_I + 1)
    # the neighbours of a node carry a weight of an ulp: (tup - t) and (t - tdown) are both in the blend
    assert np.all(k["tup"][tn == "node_below"] - k["t"][tn == "node_below"] < 1e-15)
    for cls, want in (("below", lo), ("first_node", lo), ("last_node", hi_p), ("above", hi_p)):
        assert np.all(k["p"][pn == cls] == want), (cls, want)
    assert np.all(k["p"][pn == "node"] == 2.0)        # (libm's log10; the device's may differ: test_log10_cap)


def test_the_ladder_batch():
    c = lc.ladder()
    L, n = c.nlayer, len(lc.T_PATTERN)
    assert c.T_cols.shape == (n, L + 1) and L == len(lc.LADDER_P_CLASS)
    assert np.all(c.p_int[:-1] > c.p_lay) and np.all(c.p_lay > c.p_int[1:])
    assert set(lc.LADDER_P_CLASS) == set(lc.P_CLASSES), "every P class is a layer centre"
    for name, cls in zip(lc.LADDER_P_CLASS, c.p_lay):
        if name in ("first_node", "last_node", "above", "node_above", "node_below"):
            assert cls == {"node_above": lc._up(lc.NODE_P), "node_below": lc._down(lc.NODE_P)}.get(name, lc.P_CLASSES.get(name))
    assert lc.NODE_P in c.p_int and 1e6 in c.p_lay and lc._up(1e6) in c.p_int and lc._down(1e6) in c.p_int
    # every (T class, P class) pair is a layer centre somewhere
    seen = {(float(c.T_cols[col, i]), lc.LADDER_P_CLASS[i]) for col in range(n) for i in range(L)}
    for tname, tv in lc.T_CLASSES.items():
        for pname in lc.P_CLASSES:
            assert (tv, pname) in seen, (tname, pname)
    # an interface ON the node by exact halves, at the interface that is ON a pressure node too; the end interfaces beyond the table
    Ti = np.array([lk.interface_T(Tc, L) for Tc in c.T_cols])
    on = Ti == lc.NODE_T
    assert on[:, 1:L].any(axis=0).all(), "every interior interface is ON the temperature node in some column"
    assert np.any(on[:, list(c.p_int).index(lc.NODE_P)])
    assert np.any(Ti[:, 0] < lc.KTEMP[0]) and np.any(Ti[:, 0] > lc.KTEMP[-1])
    assert np.any(Ti[:, L] < lc.KTEMP[0]) and np.any(Ti[:, L] > lc.KTEMP[-1])
    T, P = _all_levels(c)
    k = lk.locate(T, P, c.ktemp, c.kpress, True)
    assert set(lk.branch(k).tolist()) == {0, 1, 2, 3}
    assert c.k_expected == 8 and lc.run_lengths(c) == (2, 2)
    # the species variant: the same levels without the margin, and the designed one-term level
    s = lc.species_ladder()
    col, lay = lc.ON_NODE_FIRST_P
    assert s.T_cols[col, lay] == lc.NODE_T and s.p_lay[lay] == lc.KPRESS[0]
    k = lk.locate(*_all_levels(s), s.ktemp, s.kpress, False)
    assert set(lk.branch(k).tolist()) == {0, 1, 2, 3}


@pytest.mark.parametrize("name", list(lc.WALKS))
def test_walks_produce_their_key_sequences(name):
    c = lc.walk(name)
    L, k = c.nlayer, c.k_expected
    per_lay, per_int = lc.run_lengths(c)
    assert L % k != 0
    if name != "L2":
        assert per_lay >= 2 and per_int >= 2
    if name == "L33":
        assert per_lay * (k - 1) >= L, "the last run of the layer pass is empty"
    assert np.all(c.p_lay < c.kpress[-1]) and np.all(c.p_int > c.kpress[0]), "the descent stays inside the table"
    same_run = (np.arange(L - 1) // per_lay) == (np.arange(1, L) // per_lay)
    for col, pattern in enumerate(lc.PATTERNS):
        q = lk.locate(c.T_cols[col, :L], c.p_lay, c.ktemp, c.kpress, True)
        td, tu, pd, pu = q["tdown"], q["tup"], q["pdown"], q["pup"]
        same_p = (pd[1:] == pd[:-1]) & (pu[1:] == pu[:-1])
        if pattern == "one_cell":
            assert np.all(td == 1) and np.all(tu == 2)
        elif pattern == "zigzag":
            assert np.all(td[1:] != td[:-1]) and np.all(tu[1:] != tu[:-1]) and np.all(tu == td + 1)
        elif pattern == "node_above":
            assert np.all(td == lc.NODE_I) and np.array_equal(tu, lc.NODE_I + (np.arange(L) % 2))
        elif pattern == "node_below":
            assert np.all(tu == lc.NODE_I) and np.array_equal(td, lc.NODE_I - (np.arange(L) % 2))
        elif pattern == "on_node":
            assert np.all(td == tu) and (L < 4 or len(set(td.tolist())) > 1)
        if pattern in ("node_above", "node_below") and name != "L2":
            # successive levels of ONE run whose keys differ in tup (tdown) alone: what a cache keyed on less would miss
            assert np.any(same_run & same_p), (name, pattern)
    if not c.iso:
        # the interfaces of the node patterns lie inside one cell; of "on_node" they are on a node or between two
        Ti = lk.interface_T(c.T_cols[list(lc.PATTERNS).index("node_above")], L)
        q = lk.locate(Ti, c.p_int, c.ktemp, c.kpress, True)
        assert np.all(q["tdown"][1:L] == lc.NODE_I) and np.all(q["tup"][1:L] == lc.NODE_I + 1)


def _ulp_apart(a, b):
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    return float(np.max(np.abs(a - b) / np.spacing(np.maximum(np.abs(a), np.abs(b)))))


def test_fp64_twin_is_the_cpu_oracle(port):
    """plain_fp64 against port.opac_interpol / port.meanmolmass_interpol on every level of the ladder batch and on the free
    levels: the same libm and the same statement order, so equal bits; if not, at most 4 ulp"""
    c = lc.ladder()
    T, P = _all_levels(c)
    Tf, Pf = lc.free_levels()[:2]
    T, P = np.concatenate([T, Tf]), np.concatenate([P, Pf])
    n, X, Y = len(T), c.nbin, c.ny
    opac, scat, mmm = np.zeros(n * X * Y), np.zeros(n * X), np.zeros(n)
    port.opac_interpol(T, c.ktemp, P, c.kpress, c.opac_k, opac, c.opac_scat_cross, scat, c.npress, c.ntemp, Y, X, n)
    port.meanmolmass_interpol(T, c.ktemp, mmm, c.opac_meanmass, P, c.kpress, c.npress, c.ntemp, n)
    twin = lk.plain_fp64(c, T, P)
    for name, got in (("opac", opac), ("scat", scat), ("mmm", mmm)):
        want = twin[name].reshape(-1)
        if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
            d = _ulp_apart(got, want)
            print("%s: the twin and the oracle differ by up to %.2f ulp" % (name, d))
            assert d <= 4.0, (name, d)


def test_fp64_twin_is_the_cpu_oracle_species(port):
    c = lc.species_ladder()
    T, P = _all_levels(c)
    n, X, Y = len(T), c.nbin, c.ny
    k = lk.locate(T, P, c.ktemp, c.kpress, False)
    for sp in c.species:
        if sp["absorbing"]:
            got = np.zeros(n * X * Y)
            port.opac_species_interpol(T, c.ktemp, P, c.kpress, sp["pretab"], got, c.npress, c.ntemp, Y, X, n)
            tab = np.asarray(sp["pretab"]).reshape(c.ntemp, c.npress, X * Y)
            want = lk.blend(*lk.corners(tab, k), k, np.float64, True).reshape(-1)
            if not np.array_equal(got.view(np.uint64), want.view(np.uint64)):
                d = _ulp_apart(got, want)
                print("%s: %.2f ulp" % (sp["name"], d))
                assert d <= 4.0


def test_log10_cap():
    """A condition, not a measurement: moving log10(P) by +-4 ulp (more than the 3 ulp OpenCL allows an fp64 log10) at every
    designed level moves the long-double look-up by less than a quarter of the tolerance floor, relative.  The table design
    (pressure neighbours within a factor 4) is what keeps it so: a level that changes sides of a pressure node, or of a clamp,
    trades a weight of a few 1e-15 between two corners."""
    cap = lines_cases.FLOOR / 4.0
    worst = 0.0
    batches = [lc.ladder(), lc.species_ladder()] + [lc.walk(w) for w in lc.WALKS]
    levels = [_all_levels(c) + (c,) for c in batches]
    Tf, Pf = lc.free_levels()[:2]
    levels.append((Tf, Pf, lc.ladder()))
    for T, P, c in levels:
        lp = lk.log10_libm(P)
        base = lk.long_double(c, T, P, log10p=lp)
        sbase = lk.species_mix(lk.LD, c, T, P, np.full((3, len(T)), 0.3), log10p=lp) if c.get("species") else None
        for sign in (-4.0, 4.0):
            moved_lp = lp + sign * np.spacing(np.abs(lp))
            moved = lk.long_double(c, T, P, log10p=moved_lp)
            pairs = [(base[key], moved[key]) for key in base]
            if sbase is not None:
                smoved = lk.species_mix(lk.LD, c, T, P, np.full((3, len(T)), 0.3), log10p=moved_lp)
                pairs += [(a, b) for a, b in zip(sbase["raw"], smoved["raw"])]
            for a, b in pairs:
                worst = max(worst, float(np.max(np.abs(a - b) / np.abs(a))))
    print("the look-up moves by at most %.3e relative under +-4 ulp of log10 P (cap %.3e)" % (worst, cap))
    assert worst < cap


def test_species_one_term_level():
    """T on the node and P == kpress[0]: the numerator of p is exactly 0 whatever log10 returns, so without the margin the level
    reads ONE table entry, and the mix is fac_0 * entry_0 + fac_1 * entry_1"""
    c = lc.species_ladder()
    col, lay = lc.ON_NODE_FIRST_P
    T, P = c.T_cols[col, lay:lay + 1], c.p_lay[lay:lay + 1]
    assert P[0] == c.kpress[0]            # log10(P) - log10(kpress[0]) subtracts a value from itself
    m = lk.species_mix(np.float64, c, T, P, c.vmr_lay[:, lay:lay + 1])
    assert lk.branch(m["k"]).tolist() == [0] and m["k"]["p"][0] == 0.0 and m["k"]["tdown"][0] == lc.NODE_I
    entries = [np.asarray(sp["pretab"]).reshape(c.ntemp, c.npress, -1)[lc.NODE_I, 0] for sp in c.species if sp["absorbing"]]
    want = 0.0 + m["fac"][0][0] * entries[0] + m["fac"][1][0] * entries[1]
    assert np.array_equal(m["opac"][0], want)
