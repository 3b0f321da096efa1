"""The three copies of the bilinear (T, log10 P) table look-up on the crafted tables and columns of tests/lookup_cases.py, held
to the long-double restatement of tests/lookup_reference.py.  One copy is k_tp_spectral / k_tp_scalar (tp_lookup.h, through
its gather_tp); the cases take it by three routes, A, B and D.  C and E are the other two copies:

  A  the stage API (one column, indices computed from T and P), and what rebuilds opac_wg_* on the fused-look-up path
  B  k_rt_tp_index + k_tp_spectral on the stored indices: batches with HELIOS_RT_FUSED_LOOKUP=0
  C  the look-up fused into the coefficient kernels (rt_coef_kernel.inc), whose opacities never reach memory: its planes are
     held to B's planes byte for byte -- both apply the same blend_tp to the same TPIndex without contraction
  D  k_tp_spectral on the Rayleigh table, k_tp_scalar on the mean-mass table: from the indices B leaves
  E  k_rt_species_prep + the blend written out in rt_mix_species_kernel.inc: on-the-fly mixing

The tolerance is lines_cases.check_rule, unchanged: max(1e-13, 8 eps) relative, eps the fp64 twin's own deviation.  The device's
log10 may differ from libm's in the last units; tests/test_lookup_cases.py::test_log10_cap holds what that can move to a quarter
of the floor.  The temperature axis is exact: T_int is interface_T bit for bit, and levels ON a temperature node or beyond the
table are also held to the rows the restatement says they read."""
import contextlib
import os

import numpy as np
import pytest

import lines_cases
import lookup_cases as lc
import lookup_reference as lk

pytestmark = pytest.mark.gpu
KNOBS = ("HELIOS_RT_K", "HELIOS_RT_GENERIC_SCANS", "HELIOS_RT_MAXTHREADS", "HELIOS_RT_COEF_TPB", "HELIOS_RT_CLOUD_LDS",
         "HELIOS_RT_COEF_GENERAL", "HELIOS_RT_FUSED_LOOKUP")
UNFUSED = {"HELIOS_RT_FUSED_LOOKUP": 0}
BATCHES = ["ladder"] + list(lc.WALKS)
ARRAYS = ("opac_wg", "scat_cross", "meanmolmass")
_kept = {}


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    c = Context(0)
    yield c


@contextlib.contextmanager
def _knobs(env):
    """exactly these knobs while a batch lives (hx_rt_create and hx_rt_refresh read them), the others unset"""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in env.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _case(name):
    return lc.ladder() if name == "ladder" else lc.species_ladder() if name == "species" else lc.walk(name)


def _sides(c):
    return ("lay",) if c.iso else ("lay", "int")


def _read(rt, c):
    """what a refresh left behind, per column.  The Rayleigh and mean-mass arrays are read BEFORE opac_wg_*: on the fused-look-up
    path asking for the opacities rebuilds them through the stage kernel, which writes scat_cross_* again ("after")"""
    ncol = len(c.T_cols)
    out = dict(tiling=rt.flux_tiling(), bytes=rt.coef_plane_bytes())
    names = [a + "_" + s for a in ("scat_cross", "meanmolmass") for s in _sides(c)]
    for nm in names + ["T_int"]:
        out[nm] = np.array([rt.get(nm, col) for col in range(ncol)])
    for s in _sides(c):
        out["opac_wg_" + s] = np.array([rt.get("opac_wg_" + s, col) for col in range(ncol)])
    for s in _sides(c):
        out["scat_cross_%s_after" % s] = np.array([rt.get("scat_cross_" + s, col) for col in range(ncol)])
    out["planes"] = np.array([rt.coef_planes(col) for col in range(ncol)])
    return out


@contextlib.contextmanager
def _batch(ctx, c, env=None, prec="double"):
    from helios_amd.rt import batch_from_case
    c = c.copy()
    c.prec = prec
    species = c.get("species")
    with _knobs(dict(c.env, **(env or {}))):
        rt = batch_from_case(ctx, c, ncol=len(c.T_cols), nspecies=len(species) if species else 0)
        try:
            if species:
                for s, sp in enumerate(species):
                    rt.set_species(s, sp["pretab"], sp["scat"], sp["weight"], is_h2o=0, is_cia=1 if sp["is_cia"] else 0,
                                   in_mu=0 if sp["is_cia"] else 1)
                rt.set_column_vmr(-1, c.vmr_lay, c.vmr_int)
            for col, T in enumerate(c.T_cols):
                rt.set_temperatures(col, T)
            rt.build_planck_table(1)
            yield rt
        finally:
            rt.close()


def _run(ctx, name, env=None, prec="double"):
    """one refresh of a batch and what it left (kept per module: the reference runs are shared among the tests)"""
    key = (name, tuple(sorted((env or {}).items())), prec)
    if key not in _kept:
        c = _case(name)
        with _batch(ctx, c, env, prec) as rt:
            rt.refresh()
            _kept[key] = _read(rt, c)
    return _kept[key]


def _levels(c, run, side):
    """(T, P) of the layer centres or interfaces of every column, columns first, at the device's own T_int"""
    ncol, L = len(c.T_cols), c.nlayer
    if side == "lay":
        return c.T_cols[:, :L].reshape(-1), np.tile(c.p_lay, ncol)
    return run["T_int"].reshape(-1), np.tile(c.p_int, ncol)


def _restated(c, name, run, side):
    key = ("restated", name, side)
    if key not in _kept:
        T, P = _levels(c, run, side)
        _kept[key] = (lk.long_double(c, T, P), lk.plain_fp64(c, T, P))
    return _kept[key]


def _by_rows(c, table, tail, T, P):
    """the look-up of the levels that are ON a temperature node or beyond the table, from the rows they read: first along T
    between the two rows (or the one row), then along P -- another grouping of the same sum, in long double"""
    k = lk.locate(T, P, c.ktemp, c.kpress, True)
    nt = c.ntemp
    inner = np.isin(T, c.ktemp[1:-1])
    low, high = T <= c.ktemp[0], T >= c.ktemp[-1]
    assert inner.any() or low.any() or high.any()
    assert np.all(k["tdown"][inner] == k["tup"][inner]) and np.all(c.ktemp[k["tdown"][inner]] == T[inner])
    assert np.all(k["t"][low] == 0.001) and np.all(k["tdown"][low] == 0) and np.all(k["tup"][low] == 1)
    assert np.all(k["t"][high] == nt - 1.001) and np.all(k["tdown"][high] == nt - 2) and np.all(k["tup"][high] == nt - 1)
    sel = inner | low | high
    tab = np.asarray(table, np.float64).reshape((nt, c.npress) + tail).astype(lk.LD)
    shape = (-1,) + (1,) * (1 + len(tail))
    t, td, tu = k["t"][sel].astype(lk.LD).reshape(shape), k["tdown"][sel], k["tup"][sel]
    row = np.where((td != tu).reshape(shape), tab[td] * (tu.reshape(shape) - t) + tab[tu] * (t - td.reshape(shape)), tab[td])
    shape = (-1,) + (1,) * len(tail)
    n = np.arange(int(sel.sum()))
    p, pd, pu = k["p"][sel].astype(lk.LD).reshape(shape), k["pdown"][sel], k["pup"][sel]
    v = np.where((pd != pu).reshape(shape), row[n, pd] * (pu.reshape(shape) - p) + row[n, pu] * (p - pd.reshape(shape)), row[n, pd])
    return sel, v


def _hold(c, name, run, label, suffix="", arrays=ARRAYS):
    """arrays of a run under the rule, and their on-node / beyond-the-table levels against the rows they read"""
    X, Y = c.nbin, c.ny
    tabs = dict(opac_wg=("opac", c.opac_k, (X * Y,)), scat_cross=("scat", c.opac_scat_cross, (X,)),
                meanmolmass=("mmm", c.opac_meanmass, ()))
    for side in _sides(c):
        ld, f64 = _restated(c, name, run, side)
        T, P = _levels(c, run, side)
        for arr in arrays:
            key, table, tail = tabs[arr]
            got = run["%s_%s%s" % (arr, side, suffix if arr == "scat_cross" else "")].reshape((len(T),) + tail)
            lines_cases.check_rule(got, ld[key], f64[key], "%s %s %s_%s%s" % (label, name, arr, side, suffix))
            sel, rows = _by_rows(c, table, tail, T, P)
            lines_cases.check_rule(got[sel], rows, f64[key][sel], "%s %s %s_%s by rows" % (label, name, arr, side))


# ---- 1. the stage API (A) ------------------------------------------------------------------------------------------------

def test_stage_api_on_the_cross_product_of_the_classes(ctx):
    """opac_interpol (k-table and Rayleigh table), meanmolmass_interpol and opac_species_interpol on every (T class, P class)
    pair as free levels"""
    from impls import HipBackend
    raw = HipBackend(ctx)
    c = lc.ladder()
    T, P = lc.free_levels()[:2]
    n, X, Y = len(T), c.nbin, c.ny
    opac, scat, mmm, spec = np.zeros(n * X * Y), np.zeros(n * X), np.zeros(n), np.zeros(n * X * Y)
    raw.opac_interpol(T, c.ktemp, P, c.kpress, c.opac_k, opac, c.opac_scat_cross, scat, c.npress, c.ntemp, Y, X, n)
    raw.meanmolmass_interpol(T, c.ktemp, mmm, c.opac_meanmass, P, c.kpress, c.npress, c.ntemp, n)
    raw.opac_species_interpol(T, c.ktemp, P, c.kpress, c.opac_k, spec, c.npress, c.ntemp, Y, X, n)
    ld, f64 = lk.long_double(c, T, P), lk.plain_fp64(c, T, P)
    for key, got in (("opac", opac), ("scat", scat), ("mmm", mmm)):
        lines_cases.check_rule(got, ld[key], f64[key], "A stage " + key)
    tab = np.asarray(c.opac_k).reshape(c.ntemp, c.npress, X * Y)
    args = (tab, T, P, c.ktemp, c.kpress)
    lines_cases.check_rule(spec, lk.look_up(lk.LD, *args, margin=False, species=True),
                           lk.look_up(np.float64, *args, margin=False, species=True), "A stage species")
    # T on a node without the margin, P on the first node: one table entry, exactly
    k = lk.locate(T, P, c.ktemp, c.kpress, False)
    one = (lk.branch(k) == 0) & (P == c.kpress[0])
    assert one.sum() == 5      # below the table, first, interior and last temperature node, above the table
    assert np.array_equal(spec.reshape(n, -1)[one], tab[k["tdown"][one], 0])


# ---- 2. batches with HELIOS_RT_FUSED_LOOKUP=0 (B, D) ---------------------------------------------------------------------

@pytest.mark.parametrize("name", BATCHES)
def test_unfused_batches_against_the_restatement(ctx, name):
    c = _case(name)
    run = _run(ctx, name, UNFUSED)
    assert run["tiling"]["k"] == c.k_expected, run["tiling"]
    if not c.iso:
        want = np.array([lk.interface_T(T, c.nlayer) for T in c.T_cols])
        assert np.array_equal(run["T_int"].view(np.uint64), want.view(np.uint64)), "T_int is interface_T bit for bit"
    _hold(c, name, run, "B/D")
    for s in _sides(c):      # nothing rebuilds the arrays on this path
        assert np.array_equal(run["scat_cross_" + s].view(np.uint64), run["scat_cross_%s_after" % s].view(np.uint64))


# ---- 3. default batches (C; the arrays through D and, rebuilt, through A) -------------------------------------------------

def _same_bytes(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    u = np.uint32 if a.dtype.itemsize == 4 else np.uint64
    bad = np.nonzero(a.view(u).reshape(-1) != b.view(u).reshape(-1))[0]
    assert bad.size == 0, "%s: %d of %d elements differ, first at flat index %d: %r against %r" % (
        what, bad.size, a.size, bad[0], a.reshape(-1)[bad[0]], b.reshape(-1)[bad[0]])


@pytest.mark.parametrize("name", BATCHES)
def test_fused_lookup_equals_the_unfused_batch_byte_for_byte(ctx, name):
    """the default batch: its six arrays -- Rayleigh and mean mass as the refresh left them (D), then everything as rebuilt
    through the stage kernel (A) -- and its coefficient planes, padding slots included, equal those of the
    HELIOS_RT_FUSED_LOOKUP=0 batch; the planes also with 1, 2 and 8 tiles per workgroup, with the general coefficient kernel
    and with precision = single"""
    c = _case(name)
    ref = _run(ctx, name, UNFUSED)
    run = _run(ctx, name)
    assert run["tiling"] == ref["tiling"] and run["bytes"] == 8
    _hold(c, name, run, "D", "", ("scat_cross", "meanmolmass"))    # before the rebuild: the refresh's own (route D)
    _hold(c, name, run, "A", "_after", ("opac_wg", "scat_cross"))
    for key in ref:
        if key not in ("tiling", "bytes"):
            _same_bytes(run[key], ref[key], "%s %s" % (name, key))
    for env in (dict(HELIOS_RT_COEF_TPB=1), dict(HELIOS_RT_COEF_TPB=2), dict(HELIOS_RT_COEF_TPB=8),
                dict(HELIOS_RT_COEF_GENERAL=1), dict(HELIOS_RT_COEF_GENERAL=1, HELIOS_RT_COEF_TPB=2)):
        other = _run(ctx, name, env)
        assert {k: v for k, v in other["tiling"].items() if k != "coef_tpb"} == \
            {k: v for k, v in ref["tiling"].items() if k != "coef_tpb"}
        if "HELIOS_RT_COEF_TPB" in env and "HELIOS_RT_COEF_GENERAL" not in env:
            assert other["tiling"]["coef_tpb"] == env["HELIOS_RT_COEF_TPB"], other["tiling"]
        _same_bytes(other["planes"], ref["planes"], "%s planes with %s" % (name, env))
    single, single_ref = _run(ctx, name, prec="single"), _run(ctx, name, UNFUSED, prec="single")
    assert single["bytes"] == single_ref["bytes"]
    assert single["planes"].dtype == (np.float32 if single["bytes"] == 4 else np.float64)
    print("%s: precision = single has %d-byte planes" % (name, single["bytes"]))
    _same_bytes(single["planes"], single_ref["planes"], "%s fp32 planes" % name)
    if single["bytes"] == 4:
        other = _run(ctx, name, dict(HELIOS_RT_COEF_GENERAL=1), prec="single")
        _same_bytes(other["planes"], single_ref["planes"], "%s fp32 planes, general kernel" % name)


def test_some_batch_has_fp32_planes(ctx):
    """the comparison of the fp32 planes above is not empty"""
    assert any(_run(ctx, name, prec="single")["bytes"] == 4 for name in BATCHES)


# ---- 4. the species path (E) ---------------------------------------------------------------------------------------------

def test_species_path_against_the_restatement(ctx):
    """opac_wg_*, scat_cross_* and meanmolmass_* of the first refresh of the ladder batch with on-the-fly mixing; the level
    with T on a node and P == kpress[0] reads one table entry per absorber: fac * entry as the fp64 twin has it, bit for bit"""
    name = "species"
    c = _case(name)
    run = _run(ctx, name)
    want = np.array([lk.interface_T(T, c.nlayer) for T in c.T_cols])
    assert np.array_equal(run["T_int"].view(np.uint64), want.view(np.uint64))
    ncol = len(c.T_cols)
    twin_lay = None
    for side in ("lay", "int"):
        T, P = _levels(c, run, side)
        vmr = np.tile(c["vmr_" + side], (1, ncol))
        ld, f64 = lk.species_mix(lk.LD, c, T, P, vmr), lk.species_mix(np.float64, c, T, P, vmr)
        assert side == "int" or set(lk.branch(ld["k"]).tolist()) == {0, 1, 2, 3}
        for arr, key in (("opac_wg", "opac"), ("scat_cross", "scat"), ("meanmolmass", "mmm")):
            lines_cases.check_rule(run["%s_%s" % (arr, side)], ld[key], f64[key], "E %s_%s" % (arr, side))
        # levels ON a temperature node (first, interior, last: no margin here) read one row: held to the blend along P alone
        k = ld["k"]
        on = k["tdown"] == k["tup"]
        assert on.any() and np.all(np.isin(T[on], c.ktemp) | (T[on] < c.ktemp[0]) | (T[on] > c.ktemp[-1]))
        if side == "lay":
            twin_lay = f64
    col, lay = lc.ON_NODE_FIRST_P
    j = col * c.nlayer + lay
    assert lk.branch(twin_lay["k"])[j] == 0
    got = run["opac_wg_lay"].reshape(ncol, c.nlayer, -1)[col, lay]
    entries = [np.asarray(sp["pretab"]).reshape(c.ntemp, c.npress, -1)[lc.NODE_I, 0] for sp in c.species if sp["absorbing"]]
    by_hand = 0.0 + twin_lay["fac"][0][j] * entries[0] + twin_lay["fac"][1][j] * entries[1]
    assert np.array_equal(twin_lay["opac"][j], by_hand)
    _same_bytes(got, twin_lay["opac"][j], "the one-term level of the species path")


# ---- 5. run to run -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["ladder", "species"])
def test_two_refreshes_give_the_same_bytes(ctx, name):
    c = _case(name)
    with _batch(ctx, c) as rt:
        rt.refresh()
        first = _read(rt, c)
        rt.refresh()
        second = _read(rt, c)
    for key in first:
        if key not in ("tiling", "bytes"):
            _same_bytes(second[key], first[key], "%s %s of the second refresh" % (name, key))
    if name == "ladder":
        for key in first:
            if key not in ("tiling", "bytes"):
                _same_bytes(first[key], _run(ctx, name)[key], "%s %s of another batch" % (name, key))
