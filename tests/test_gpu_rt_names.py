"""The named arrays of a batch through its three entry points -- hx_rt_get, hx_rt_set_state, hx_rt_device_ptr: which names
each call serves, their sizes, their column strides and what col = -1 means, on three two-column batches of the smallest
size an iteration accepts (two layers).  The two columns of a batch are given different inputs, so that a wrong stride
shows."""
import ctypes

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu

KINDS = ("premixed", "onthefly", "matrix")

# hx_rt_set_state: the names written per column (element count from the batch, dtype), and whether hx_rt_get reads them back
SET_NAMES = {"T_lay": ("L1", np.float64, True), "c_p_lay": ("L", np.float64, True),
             "delta_t_prefactor": ("L1", np.float64, True), "T_store": ("L1", np.float64, True),
             "kappa_lay": ("L", np.float64, True), "kappa_int": ("L1", np.float64, True),
             "conv_layer": ("L1", np.int32, True), "conv_unstable": ("L1", np.int32, True),
             "done": (1, np.int32, True), "add_heat_dens": ("L", np.float64, False), "dampara": (1, np.float64, False)}

# hx_rt_device_ptr: name -> the hx_rt_get name it equals (None: an input of the batch, compared with what was handed over)
PTR_NAMES = {"T_lay": "T_lay", "T_int": "T_int", "p_lay": None, "p_int": None, "opac_wg_lay": "opac_wg_lay",
             "opac_wg_int": "opac_wg_int", "F_dir_wg": "F_dir_wg", "Fc_dir_wg": "Fc_dir_wg",
             "scat_cross_lay": "scat_cross_lay", "scat_cross_int": "scat_cross_int",
             "meanmolmass_lay": "meanmolmass_lay", "meanmolmass_int": "meanmolmass_int", "planck_grid": "planck_grid",
             "F_up_band_n": "F_up_band", "F_down_band_n": "F_down_band", "F_net": "F_net", "F_up_tot": "F_up_tot",
             "F_down_tot": "F_down_tot", "gauss_weight": None, "gauss_y": None, "opac_deltawave": None,
             "opac_interwave": None, "abs_cross_all_clouds_lay": "abs_cross_all_clouds_lay", "delta_col_upper": None,
             "delta_col_lower": None}

# read back per column: these differ between the two columns of every batch (their temperatures, pressures, albedos differ)
DIFFER = ["T_lay", "T_int", "F_up_band", "F_down_band", "F_up_tot", "F_down_tot", "F_net", "F_net_diff",
          "planckband_lay", "planckband_int", "opac_wg_lay", "opac_wg_int", "delta_z_lay", "z_lay", "F_up_wg", "Fc_up_wg"]
DIFFER_CLOUDS = ["abs_cross_all_clouds_lay", "abs_cross_all_clouds_int", "scat_cross_all_clouds_lay",
                 "scat_cross_all_clouds_int", "g_0_all_clouds_lay", "g_0_all_clouds_int"]
DIFFER_BEAM = ["F_dir_wg", "Fc_dir_wg", "F_dir_band"]
DIFFER_SPECIES = ["vmr_lay", "vmr_int", "meanmolmass_lay", "meanmolmass_int"]
VMR_FACTOR = np.array([[0.5], [0.75]])    # column 1's mixing ratios over column 0's, per species
# one value per batch: the same through either column
SHARED = ["planck_grid", "premixed_table_count", "mie_table_count", "flux_launch_policy", "graph_replays", "graph_builds"]


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def _strings(consts):
    for v in consts:
        if isinstance(v, str):
            yield v
        elif isinstance(v, tuple):
            for s in _strings(v):
                yield s


def shape_keys(rt):
    """every key of RTBatch._shape: the string constants of its code that it answers to"""
    keys = []
    for s in _strings(type(rt)._shape.__code__.co_consts):
        try:
            rt._shape(s)
        except KeyError:
            continue
        if s not in keys:
            keys.append(s)
    assert len(keys) >= 58 and "T_lay" in keys and "cloud_deck_spectra" in keys and "vmr_int" in keys, keys
    assert "boa_source_factor" in keys
    return keys


def column_inputs(c, col):
    """what column `col` of a batch is given: column 0 the case's own profile, column 1 a warmer one at lower pressures under
    another albedo"""
    if col == 0:
        return c.p_lay, c.p_int, c.T_lay, c.surf_albedo
    return c.p_lay * 0.75, c.p_int * 0.75, c.T_lay * 1.0625 + 3.0, c.surf_albedo + 0.125


class Batch(object):
    """one of the three batches after one step(0)"""

    def __init__(self, ctx, kind):
        from helios_amd.rt import batch_from_case
        self.kind = kind
        if kind == "premixed":
            c = cases.make_case(nbin=3, ny=2, nlayer=2, clouds=1, dir_beam=1, albedo=0.25)
        elif kind == "i2s":       # (not one of KINDS: test_boa_source_factor_per_column's, where E != 1 can occur)
            c = cases.make_case(nbin=3, ny=2, nlayer=2, clouds=1, scat_corr=1, g_0=0.2, dir_beam=1, albedo=0.25)
        elif kind == "onthefly":
            # (two species: one absorber and the scatterer add_species appends)
            c = cases.add_species(cases.make_case(nbin=3, ny=20, nlayer=2, albedo=0.25), nspecies=1, with_h2o=False)
        else:
            c = cases.make_case(nbin=3, ny=2, nlayer=2, albedo=0.25)
            c["flux_calc_method"] = "matrix"
        self.c = c
        species = c.get("species")
        self.rt = rt = batch_from_case(ctx, c, ncol=2, nspecies=len(species) if species else 0)
        try:
            p_lay, p_int, T_lay, albedo = column_inputs(c, 1)
            rt.set_column_profile(1, p_lay, p_int, T_lay, albedo, c.starflux)
            if c.clouds:
                rt.set_column_clouds(1, c.abs_cross_all_clouds_lay * 0.5, c.abs_cross_all_clouds_int * 0.5,
                                     c.scat_cross_all_clouds_lay * 0.25, c.scat_cross_all_clouds_int * 0.25,
                                     c.g_0_all_clouds_lay * 0.5, c.g_0_all_clouds_int * 0.5)
            if species:
                for k, sp in enumerate(species):
                    rt.set_species(k, sp["pretab"], sp["scat"], sp["weight"], is_h2o=0, is_cia=0, in_mu=1)
                vl, vi = cases.species_vmr_arrays(c)
                rt.set_column_vmr(0, vl, vi)
                rt.set_column_vmr(1, vl * VMR_FACTOR, vi * VMR_FACTOR)
            rt.build_planck_table(1)
            rt.step(0)
        except Exception:
            rt.close()
            raise
        self.n = dict(L=rt.nlayer, L1=rt.nlayer + 1)

    def count(self, n):
        return self.n.get(n, n)

    def readable(self):
        """the keys of _shape this batch serves through hx_rt_get as it stands (no decks, no species unless on the fly, no
        clouds unless premixed, down-fluxes only from the direct solve)"""
        keys = [k for k in shape_keys(self.rt) if k != "cloud_deck_spectra"]
        if not self.c.clouds:
            keys = [k for k in keys if not k.startswith("g_0_all_clouds")]
        if not self.c.get("species"):
            keys = [k for k in keys if not k.startswith("vmr_")]
        if self.kind != "matrix":
            keys = [k for k in keys if k not in ("F_down_wg", "Fc_down_wg")]
        return keys

    # the three calls as the library sees them: status and, where it fails, the context's message
    def raw_get(self, col, name, nbytes):
        rt = self.rt
        out = np.zeros(max(1, nbytes), np.uint8)
        rc = rt._l.hx_rt_get(rt.handle, int(col), name.encode(), out.ctypes.data_as(ctypes.c_void_p), nbytes)
        return rc, self.message(rc)

    def raw_set(self, col, name, a):
        rt = self.rt
        a = np.ascontiguousarray(a)
        rc = rt._l.hx_rt_set_state(rt.handle, int(col), name.encode(), a.ctypes.data_as(ctypes.c_void_p), a.nbytes)
        return rc, self.message(rc)

    def raw_ptr(self, col, name):
        rt = self.rt
        p = ctypes.c_void_p()
        rc = rt._l.hx_rt_device_ptr(rt.handle, int(col), name.encode(), ctypes.byref(p))
        return rc, self.message(rc), p

    def message(self, rc):
        return (self.rt._l.hx_last_error(self.rt.ctx.handle) or b"").decode() if rc else ""

    def d2h(self, p, n, dtype=np.float64):
        out = np.zeros(n, dtype)
        self.rt.ctx.check(self.rt._l.hx_d2h(self.rt.ctx.handle, out.ctypes.data_as(ctypes.c_void_p), p, out.nbytes), "hx_d2h")
        return out


@pytest.fixture(params=KINDS)
def batch(ctx, request):
    b = Batch(ctx, request.param)
    yield b
    b.rt.close()


def test_every_name_reads_back_at_its_size_in_both_columns(batch):
    rt, c = batch.rt, batch.c
    got = {}
    for k in batch.readable():
        n, dt = rt._shape(k)
        got[k] = [rt.get(k, col) for col in (0, 1)]
        for a in got[k]:
            assert a.size == n and a.dtype == dt, k
    differ = DIFFER + (DIFFER_CLOUDS + ["g_0_tot_lay", "g_0_tot_int"] if c.clouds else []) \
        + (DIFFER_BEAM if c.dir_beam else []) + (DIFFER_SPECIES if c.get("species") else [])
    for k in differ:
        assert not np.array_equal(got[k][0], got[k][1]), "%s: the same in both columns" % k
    for k in SHARED:
        assert np.array_equal(got[k][0], got[k][1]), k
    # the inputs themselves, through their getters
    for col in (0, 1):
        if c.clouds:
            f = (1.0, 0.5)[col]
            XL, XI = c.nbin * c.nlayer, c.nbin * c.ninterface
            assert np.array_equal(got["abs_cross_all_clouds_lay"][col], c.abs_cross_all_clouds_lay[:XL] * f)
            assert np.array_equal(got["g_0_all_clouds_int"][col], c.g_0_all_clouds_int[:XI] * f)
        if c.get("species"):
            vl, vi = cases.species_vmr_arrays(c)
            f = (1.0, VMR_FACTOR)[col]
            S, I, L = len(c.species), c.ninterface, c.nlayer
            assert np.array_equal(got["vmr_int"][col].reshape(S, I), vi * f)
            assert np.array_equal(got["vmr_lay"][col].reshape(S, I)[:, :L], vl * f)
    if not c.dir_beam:   # no beam: zeros of the reference's size
        assert not got["F_dir_wg"][1].any() and not got["Fc_dir_wg"][0].any()
    # without the I2S correction E = 1 and the surface-emission factor (1 - w0) / (1 - w0) is exactly 1, in either method
    for col in (0, 1):
        assert got["boa_source_factor"][col].size == c.nbin * c.ny and np.all(got["boa_source_factor"][col] == 1.0)
    assert [int(rt.get(k, -1)[0]) for k in ("premixed_table_count", "mie_table_count")] == [0 if c.get("species") else 1, 0]
    assert rt.coef_plane_bytes() == 8 and rt.totals_chunks() >= 1 and rt.flux_tiling()["ROWS"] >= 1
    assert rt.coef_planes(1).shape == rt.coef_planes(0).shape and not np.array_equal(rt.coef_planes(0), rt.coef_planes(1))


def test_boa_source_factor_per_column(ctx):
    """boa_source_factor with the I2S correction on: ny * nbin values per column, get-only; column 1 of the batch is
    column 0 of a batch of one that is given column 1's inputs, bit for bit (the column stride), and the two columns
    differ at every spectral point where either scatters enough for E != 1 (elsewhere both are exactly 1)"""
    from helios_amd.rt import batch_from_case
    b = Batch(ctx, "i2s")
    try:
        rt, c = b.rt, b.c
        n = c.nbin * c.ny
        assert rt._shape("boa_source_factor") == (n, np.float64)
        boa = [rt.get("boa_source_factor", col) for col in (0, 1)]
        for col in (0, 1):
            assert b.raw_get(col, "boa_source_factor", n * 8)[0] == 0
            assert b.raw_get(col, "boa_source_factor", (n - 1) * 8)[0] == 1 and b.raw_get(col, "boa_source_factor", (n + 1) * 8)[0] == 1
        assert b.raw_get(-1, "boa_source_factor", n * 8)[0] == 1 and b.raw_get(2, "boa_source_factor", n * 8)[0] == 1
        assert b.raw_set(0, "boa_source_factor", np.ones(n))[0] == 1 and b.raw_ptr(0, "boa_source_factor")[0] == 1
        for a in boa:
            assert np.all(np.isfinite(a)) and np.all(a > 0.0) and np.all(a <= 1.0)
        corrected = (boa[0] != 1.0) | (boa[1] != 1.0)
        assert corrected.any(), "no spectral point with E != 1: the case does not test the stride"
        assert np.all(boa[0][corrected] != boa[1][corrected])
        one = batch_from_case(ctx, c, ncol=1)
        try:
            p_lay, p_int, T_lay, albedo = column_inputs(c, 1)
            one.set_column_profile(0, p_lay, p_int, T_lay, albedo, c.starflux)
            one.set_column_clouds(0, c.abs_cross_all_clouds_lay * 0.5, c.abs_cross_all_clouds_int * 0.5,
                                  c.scat_cross_all_clouds_lay * 0.25, c.scat_cross_all_clouds_int * 0.25,
                                  c.g_0_all_clouds_lay * 0.5, c.g_0_all_clouds_int * 0.5)
            one.build_planck_table(1)
            one.step(0)
            np.testing.assert_array_equal(one.get("boa_source_factor", 0).view(np.uint64), boa[1].view(np.uint64))
        finally:
            one.close()
    finally:
        b.rt.close()


def test_wrong_sizes_unknown_names_and_columns_are_refused(batch):
    rt = batch.rt
    for k in batch.readable():
        n, dt = rt._shape(k)
        item = np.dtype(dt).itemsize
        for col in (0, 1):
            assert batch.raw_get(col, k, n * item)[0] == 0, k
            assert batch.raw_get(col, k, (n - 1) * item)[0] == 1, "%s: a buffer one element short" % k      # HX_E_ARG
            assert batch.raw_get(col, k, (n + 1) * item)[0] == 1, "%s: a buffer one element long" % k
    for k in ("coef_plane_bytes", "totals_chunks"):
        assert batch.raw_get(-1, k, 4)[0] == 0 and batch.raw_get(-1, k, 8)[0] == 1 and batch.raw_get(-1, k, 0)[0] == 1
    assert batch.raw_get(-1, "flux_tiling", 14 * 4)[0] == 0 and batch.raw_get(-1, "flux_tiling", 13 * 4)[0] == 1
    nplanes = rt.coef_planes(0).nbytes
    assert batch.raw_get(1, "coef_planes", nplanes)[0] == 0
    assert batch.raw_get(1, "coef_planes", nplanes - 8)[0] == 1 and batch.raw_get(1, "coef_planes", nplanes + 8)[0] == 1
    for name, (n, dt, _) in SET_NAMES.items():
        n = batch.count(n)
        assert batch.raw_set(1, name, np.zeros(n - 1, dt))[0] == 1, "%s: one element short" % name
        assert batch.raw_set(1, name, np.zeros(n + 1, dt))[0] == 1, "%s: one element long" % name
    ngrid = rt._shape("planck_grid")[0]
    for name, n in (("keep_down", 1), ("restart", 1)):
        assert batch.raw_set(-1, name, np.zeros(n + 1, np.int32))[0] == 1, name
    assert batch.raw_set(-1, "planck_grid", np.zeros(ngrid - 1))[0] == 1 and batch.raw_set(-1, "planck_grid", np.zeros(ngrid + 1))[0] == 1
    # a name none of the calls knows
    rc, msg = batch.raw_get(0, "no_such_array", 8)
    assert rc == 1 and "unknown array name 'no_such_array'" in msg
    rc, msg = batch.raw_set(0, "no_such_array", np.zeros(1))
    assert rc == 1 and "unknown name 'no_such_array'" in msg
    rc, msg, _ = batch.raw_ptr(0, "no_such_array")
    assert rc == 1 and "unknown name 'no_such_array'" in msg
    # names of one call are not names of another
    assert batch.raw_get(0, "p_lay", rt.nlayer * 8)[0] == 1 and batch.raw_get(0, "dampara", 8)[0] == 1
    assert batch.raw_set(0, "F_net", np.zeros(rt.ninterface))[0] == 1 and batch.raw_set(0, "p_lay", np.zeros(rt.nlayer))[0] == 1
    assert batch.raw_ptr(0, "F_up_band")[0] == 1 and batch.raw_ptr(0, "c_p_lay")[0] == 1 and batch.raw_ptr(0, "done")[0] == 1
    # col = ncol
    rc, msg = batch.raw_get(rt.ncol, "T_lay", (rt.nlayer + 1) * 8)
    assert rc == 1 and "column index out of range" in msg
    rc, msg = batch.raw_set(rt.ncol, "T_lay", np.zeros(rt.nlayer + 1))
    assert rc == 1 and "column index out of range" in msg
    assert batch.raw_ptr(rt.ncol, "T_lay")[0] == 1 and batch.raw_ptr(-1, "T_lay")[0] == 1
    # col = -1: the batch's own values only
    assert batch.raw_get(-1, "T_lay", (rt.nlayer + 1) * 8)[0] == 1 and batch.raw_get(-1, "graph_replays", 24)[0] == 1
    assert batch.raw_get(-1, "premixed_table", 4)[0] == 1 and batch.raw_get(rt.ncol, "mie_table_count", 4)[0] == 0


def test_set_state_round_trips_per_column(batch):
    rt = batch.rt
    for name, (n, dt, has_getter) in SET_NAMES.items():
        if name == "done":
            continue
        n = batch.count(n)
        before = [rt.get(name, col) for col in (0, 1)] if has_getter else None
        one = (np.arange(n) * 1.25 + 7.0).astype(dt)
        rt.set_state(1, name, one)
        if has_getter:
            assert np.array_equal(rt.get(name, 1), one), name
            assert np.array_equal(rt.get(name, 0), before[0]), "%s: a write to column 1 reached column 0" % name
        both = (np.arange(n) * 2.5 + 11.0).astype(dt)
        rt.set_state(-1, name, both)
        if has_getter:
            assert np.array_equal(rt.get(name, 0), both) and np.array_equal(rt.get(name, 1), both), name
    grid = rt.get("planck_grid", 0)
    rt.set_state(-1, "planck_grid", grid * 0.5)
    assert np.array_equal(rt.get("planck_grid", 1), grid * 0.5)
    # `done` freezes a column, `restart` clears the flags of all of them
    rt.set_state(1, "done", np.array([1], np.int32))
    assert [int(rt.get("done", col)[0]) for col in (0, 1)] == [0, 1]
    rt.set_state(-1, "done", np.array([3], np.int32))
    assert [int(rt.get("done", col)[0]) for col in (0, 1)] == [3, 3]
    rt.set_state(-1, "restart", np.array([1], np.int32))
    assert [int(rt.get("done", col)[0]) for col in (0, 1)] == [0, 0]
    assert not rt.get("T_store", 1).any() and not rt.get("delta_t_prefactor", 0).any()


def test_device_pointers_name_the_memory_the_getters_read(batch):
    rt, c = batch.rt, batch.c
    X, I = rt.nbin, rt.ninterface
    for col in (0, 1):
        p_lay, p_int, _, _ = column_inputs(c, col)
        inputs = {"p_lay": p_lay, "p_int": p_int, "gauss_weight": c.gauss_weight, "gauss_y": c.gauss_y,
                  "opac_deltawave": c.opac_deltawave, "opac_interwave": c.opac_interwave,
                  "delta_col_upper": (p_lay - p_int[1:]) / c.g, "delta_col_lower": (p_int[:-1] - p_lay) / c.g}
        for name, getter in PTR_NAMES.items():
            rc, msg, p = batch.raw_ptr(col, name)
            if name in ("F_dir_wg", "Fc_dir_wg") and not c.dir_beam:
                assert rc == 1 and "unknown name" in msg, name
                continue
            assert rc == 0 and p.value, name
            if getter is None:
                want = np.asarray(inputs[name], np.float64)
            else:
                want = rt.get(getter, col)
            have = batch.d2h(p, want.size)
            if name.endswith("_band_n"):      # [bin][interface] on the device, [interface][bin] from the getter
                have = have.reshape(X, I).T.ravel()
            assert np.array_equal(have, want), "%s of column %d" % (name, col)


def test_names_whose_data_the_batch_does_not_hold_are_refused(batch):
    rt, c = batch.rt, batch.c
    X, I, L = rt.nbin, rt.ninterface, rt.nlayer
    rc, msg = batch.raw_get(0, "cloud_deck_spectra", 3 * X * 8)
    assert rc == 4 and "no cloud decks have been set" in msg                                   # HX_E_STATE
    if not c.clouds:
        rc, msg = batch.raw_get(1, "g_0_all_clouds_lay", X * L * 8)
        assert rc == 4 and "clouds = 0" in msg
        assert batch.raw_get(1, "g_0_all_clouds_int", X * I * 8)[0] == 4
    if not c.get("species"):
        rc, msg = batch.raw_get(0, "vmr_lay", I * 8)
        assert rc == 1 and "unknown array name" in msg
    wg = rt._shape("F_down_wg")[0] * 8
    if batch.kind != "matrix":
        for k in ("F_down_wg", "Fc_down_wg"):
            rc, msg = batch.raw_get(0, k, wg)
            assert rc == 4 and "keep_down" in msg, k
        rt.keep_down_fluxes(True)
        rt.step(1)
    down = [rt.get("F_down_wg", col) for col in (0, 1)]
    assert down[0].any() and not np.array_equal(down[0], down[1])
    assert rt.get("Fc_down_wg", 1).size == wg // 8
    assert batch.raw_get(1, "F_down_wg", wg - 8)[0] == 1 and batch.raw_get(1, "Fc_down_wg", wg + 8)[0] == 1
