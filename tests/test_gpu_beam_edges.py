"""The direct stellar beam at its edges, held to the long-double restatement of tests/beam_reference.py by the bound derived
there, entry by entry (tests/test_beam_reference.py anchors that bound to the oracle and the reference without a GPU):

1. hx_fdir_iso and hx_fdir_noniso -- k_fdir_plane<false/true>, k_fdir_sphere<false/true> in csrc/stage_trans.hip -- on the
   crafted optical depths of tests/beam_cases.py: 1, 2 and 33 layers, 1 and 255 ... 260 spectral points, zenith 0, 60 and
   89.9 degrees, rocky and gas heights; `empty` and `dir0` bit for bit; the top slab of Fc_dir_wg and the cells behind every
   output keep their sentinel; plane and sphere agree bit for bit where all heights are equal (at mu_star = -1, -1/2, -1/4,
   whose squares and the root back are exact -- for any other mu_star the sphere's own roundings of mu_ii differ from
   mu_star, within kappa u).
2. The device loop, one refresh per column of beam_cases.LOOP_TABLE: k_rt_dtau_halves, hx_internal_fdir_noniso_batch and
   k_rt_fdir_band (32 x 32 tiles around 31 ... 33 bins and 32, 33 interfaces; the unrolled path at 20 Gauss points and the
   generic one at 4) on what the device saw; a batch of three columns that differ in everything the beam reads, whose middle
   column is then finished and keeps its bits through another refresh.
3. hx_integrate_beamflux (k_integrate_beamflux, a 1024-wide tree) on both sides of 1024 and 2048 bins, band values over 300
   decades: (nbin + 16) 2^-52 sum |term| of the long-double sum.

Every test prints its largest err / bound; with the environment variable BEAM_EDGES_JSON set the figures go into the file
it names.  No bound is adjusted to them.

One MI355X run, largest err / bound (the CPU oracle on the same crafted cases in brackets; tests/test_beam_reference.py):
hx_fdir_iso plane 0.394 (0.394), sphere 0.343 (0.343); hx_fdir_noniso F_dir_wg plane 0.632 (0.632), sphere 0.474 (0.474);
Fc_dir_wg plane 0.484, sphere 0.399 (0.484 over both).  Device loop: F_dir_wg plane 0.478, sphere 0.356, Fc_dir_wg 0.358,
F_dir_band 0.222 at 20 Gauss points and 0.380 at 4; the batch 0.309, 0.320 and 0.357 for the three arrays.  F_dir_tot: 0.017
at one bin, at most 0.0007 from 1023 bins on.

The device's exp does not return 0 where the value is subnormal: the `subnormal` cases (one layer among them, where the
factor itself is subnormal) hold with the absolute term at one subnormal spacing, 2^-1074, per multiplication.  The Gauss
sum's bound, (ny + 2) 2^-53 sum |term|, has no such term: see beam_cases.batch_case for what that means for the batch."""
import ctypes
import json
import os

import numpy as np
import pytest

import beam_cases as bc
import beam_reference as br
from test_beam_reference import hold, FORM_NAME

pytestmark = pytest.mark.gpu
LD = np.longdouble
BEAM_KEYS = ("F_dir_wg", "Fc_dir_wg", "F_dir_band")


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


@pytest.fixture(scope="module")
def hip(ctx):
    from impls import hip_impl
    return hip_impl(ctx)


def record(what, value):
    print("%s: largest err / bound %.3f" % (what, value))
    path = os.environ.get("BEAM_EDGES_JSON")
    if path:
        have = json.load(open(path)) if os.path.exists(path) else {}
        have[what] = max(float(value), have.get(what, 0.0))
        json.dump(have, open(path, "w"), indent=1, sort_keys=True)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. the per-stage entries ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", bc.FORMS, ids=[FORM_NAME[f].replace(" ", "_") for f in bc.FORMS])
def test_stage_entries_on_crafted_optical_depths(hip, form):
    worst_F = worst_Fc = 0.0
    named = [c for c in bc.all_crafted() if (c.sphere, c.iso) == form]
    assert len(named) == 25
    for c in named:
        b = bc.restated(c)
        F, Fc = bc.run_stage(hip, c)
        n, nc = c.nc * (c.L + 1), c.nc
        assert (F[n:] == bc.SENTINEL).all(), "cells behind F_dir_wg, " + c.name
        if Fc is not None:
            assert (Fc[n - nc:] == bc.SENTINEL).all(), "the top slab of Fc_dir_wg and the cells behind it, " + c.name
        assert np.isfinite(F[:n]).all() and (Fc is None or np.isfinite(Fc[:n - nc]).all()), c.name
        rF, rFc = hold(b, F, Fc, c.name)
        worst_F, worst_Fc = max(worst_F, rF), max(worst_Fc, rFc)
        written = [F[:n].reshape(c.L + 1, nc)] + ([Fc[:n - nc].reshape(c.L, nc)] if Fc is not None else [])
        if c.profile == "empty":
            F0 = bc.restate(c, np.float64).F0
            assert F0.all()
            for a in written:
                np.testing.assert_array_equal(bits(a), bits(np.broadcast_to(F0, a.shape)), err_msg=c.name)
        if c.profile == "dir0":
            for a in written:
                assert not a.any(), c.name
        if c.profile == "opaque_layer":
            assert not F[:nc * (c.opaque + 1)].any() and F[nc * (c.opaque + 1):n].all(), c.name
    record("hx_fdir %s F_dir_wg" % FORM_NAME[form], worst_F)
    if not form[1]:
        record("hx_fdir %s Fc_dir_wg" % FORM_NAME[form], worst_Fc)


@pytest.mark.parametrize("iso", (1, 0))
@pytest.mark.parametrize("mu_star", (-1.0, -0.5, -0.25))
def test_plane_and_sphere_agree_where_all_heights_are_equal(hip, mu_star, iso):
    out, worst = [], 0.0
    for sphere in (0, 1):
        c = bc.crafted("span", 33, (51, 5), 60.0, 0, "rocky", iso)       # the same draws for both: the geometry is set below
        scale = abs(mu_star / c.mu_star)                                  # the slant totals stay 1e-6 ... 600
        c.tau_u, c.tau_l = c.tau_u * scale, None if iso else c.tau_l * scale
        c.sphere, c.mu_star, c.z = sphere, mu_star, np.full(c.L, 3.0e8)
        out.append(bc.run_stage(hip, c))
        worst = max((worst,) + hold(bc.restate(c), out[-1][0], out[-1][1], "equal heights, sphere = %d" % sphere))
    record("equal heights, plane and sphere", worst)
    np.testing.assert_array_equal(bits(out[0][0]), bits(out[1][0]))
    assert np.abs(out[0][0][:c.nc * (c.L + 1)]).min() > 1e-290
    if not iso:
        np.testing.assert_array_equal(bits(out[0][1]), bits(out[1][1]))


# ---- 2. the device loop ------------------------------------------------------------------------------------------------------
def d2h(ctx, rt, name, col, n):
    """an array the batch serves by address only, through the library's own copy"""
    out = np.zeros(n)
    ctx.check(ctx._l.hx_d2h(ctx.handle, out.ctypes.data_as(ctypes.c_void_p), rt.device_ptr(name, col), out.nbytes), "hx_d2h")
    return out


def what_the_device_saw(ctx, rt, c, col, g):
    """half_layer_tau's inputs, the stellar row, the heights and the Gauss weights of column `col`, read back"""
    L, I = c.nlayer, c.nlayer + 1
    inp = dict(nbin=c.nbin, ny=c.ny, nlayer=L, iso=c.iso, scat=c.scat, g=g, p_int=d2h(ctx, rt, "p_int", col, I),
               delta_col_upper=d2h(ctx, rt, "delta_col_upper", col, L), delta_col_lower=d2h(ctx, rt, "delta_col_lower", col, L))
    for k in ("opac_wg_lay", "opac_wg_int", "scat_cross_lay", "scat_cross_int", "meanmolmass_lay", "meanmolmass_int"):
        inp[k] = rt.get(k, col)
    return inp, rt.get("planckband_lay", col)[L::L + 2], rt.get("z_lay", col), d2h(ctx, rt, "gauss_weight", 0, c.ny)


def hold_column(ctx, rt, c, col, column, label):
    """F_dir_wg, Fc_dir_wg and F_dir_band of one column against the restatement of what the device saw"""
    L, I, X, Y = c.nlayer, c.nlayer + 1, c.nbin, c.ny
    inp, B, z, gw = what_the_device_saw(ctx, rt, c, col, float(column.get("g", c.g)))
    assert (B > 0).all() and (inp["opac_wg_lay"] > 0).all() and (inp["scat_cross_lay"] > 0).all(), label
    b = bc.restate_column(inp, B, z, c, column)
    F, Fc = rt.get("F_dir_wg", col), rt.get("Fc_dir_wg", col)
    assert np.isfinite(F).all() and F[Y * X * L:].all(), label
    rF, rFc = hold(b, F, Fc, label)
    want, mag = br.band_of(F, gw, X, Y, I)
    err = np.abs(rt.get("F_dir_band", col).reshape(I, X).astype(LD) - want)
    assert (mag[L] > 0).all(), label
    rb = float((err / np.maximum(mag, LD(2.0) ** -1074)).max() / ((Y + 2) * 2.0 ** -53))
    assert (err <= (Y + 2) * 2.0 ** -53 * mag).all(), "%s F_dir_band: %.3f of its bound" % (label, rb)
    return b, rF, rFc, rb


@pytest.mark.parametrize("row", bc.LOOP_TABLE, ids=[bc.loop_name(r) for r in bc.LOOP_TABLE])
def test_one_refresh_of_the_device_loop(ctx, row):
    from helios_amd.rt import batch_from_case
    c = bc.loop_case(row)
    rt = batch_from_case(ctx, c)
    try:
        rt.build_planck_table(1)
        rt.run(0, 1)
        b, rF, rFc, rb = hold_column(ctx, rt, c, 0, {}, c.name)
        assert b.slant[0].min() < 1e-3 and b.slant[0].max() > 745.0, (c.name, b.slant[0].min(), b.slant[0].max())
        if c.iso:
            assert not rt.get("Fc_dir_wg").any()
    finally:
        rt.close()
    record("device loop %s F_dir_wg" % ("sphere" if c.geom_zenith_corr else "plane"), rF)
    if not c.iso:
        record("device loop Fc_dir_wg", rFc)
    record("device loop F_dir_band ny = %d" % c.ny, rb)


def test_three_column_batch_and_a_finished_column(ctx):
    from helios_amd.rt import batch_from_case
    c = bc.batch_case()
    L = c.nlayer
    rt = batch_from_case(ctx, c, ncol=3, columns=bc.BATCH_COLUMNS)
    worst = [0.0, 0.0, 0.0]
    try:
        rt.build_planck_table(1)
        rt.run(0, 1)
        first = []
        for k, col in enumerate(bc.BATCH_COLUMNS):
            res = hold_column(ctx, rt, c, k, col, "column %d of the batch" % k)
            assert 1.0 < res[0].slant.max() < bc.BATCH_SLANT_LIMIT, k              # beam_cases.batch_case: normal numbers only
            worst = [max(a, b) for a, b in zip(worst, res[1:])]
            first.append({n: rt.get(n, k) for n in BEAM_KEYS})
            assert int(rt.get("done", k)[0]) == 0
        assert len({first[k]["F_dir_wg"][-1] for k in range(3)}) == 3           # three different beams at the top
        rt.set_state(1, "done", np.ones(1, np.int32))
        for k, dT in enumerate((70.0, -45.0, 110.0)):
            rt.set_temperatures(k, c.T_lay + dT)
        rt.run(10, 1)                                                           # iteration 10 refreshes
        for n in BEAM_KEYS:
            np.testing.assert_array_equal(bits(rt.get(n, 1)), bits(first[1][n]), err_msg="the finished column's " + n)
        for k in (0, 2):
            res = hold_column(ctx, rt, c, k, bc.BATCH_COLUMNS[k], "column %d of the batch at its new state" % k)
            assert 1.0 < res[0].slant.max() < bc.BATCH_SLANT_LIMIT, k
            worst = [max(a, b) for a, b in zip(worst, res[1:])]
            for n in BEAM_KEYS:
                assert (rt.get(n, k)[:c.ny * c.nbin * L] != first[k][n][:c.ny * c.nbin * L]).any(), (k, n)
    finally:
        rt.close()
    for name, v in zip(BEAM_KEYS, worst):
        record("batch of three columns " + name, v)


# ---- 3. hx_integrate_beamflux ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbin", (1, 1023, 1024, 1025, 2049))
def test_integrate_beamflux_against_the_long_double_sum(hip, nbin):
    ni = 3
    rng = np.random.default_rng(7100 + nbin)
    band = -(10.0 ** rng.uniform(-300.0, 0.0, nbin * ni))
    band[rng.integers(0, nbin, 1)] = -1.0                       # (interface 0 holds the top decade whatever the draws)
    dl = rng.uniform(1e-6, 1e-4, nbin)
    tot = np.full(ni + bc.GUARD, bc.SENTINEL)
    hip.integrate_beamflux(tot, band, dl, nbin, ni)
    assert (tot[ni:] == bc.SENTINEL).all()
    term = band.reshape(ni, nbin).astype(LD) * dl.astype(LD)[None, :]
    want, mag = term.sum(axis=1), np.abs(term).sum(axis=1)
    assert np.log10(np.abs(band).max() / np.abs(band).min()) > (0 if nbin == 1 else 290)
    err = np.abs(tot[:ni].astype(LD) - want)
    bound = (nbin + 16) * 2.0 ** -52 * mag
    record("hx_integrate_beamflux F_dir_tot nbin = %d" % nbin, float((err / bound).max()))
    assert (err <= bound).all()
