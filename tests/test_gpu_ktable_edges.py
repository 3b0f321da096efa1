"""k_ktable_bins and k_ktable_regrid (csrc/ktable.hip) at the sizes where they change their path, against the long-double
reference of tests/ktable_reference.py: bins around the scan's run lengths and the hand-over from the LDS sort to the
scratch, slabs of ties, floored values and fp32's extremes, 1 to 1100 abscissae, ragged batches, a builder that changes its
grid, re-gridding from degenerate source grids and beyond one pass of its launch, and every refusal of hx_ktable_*.  The
builder is driven directly; no files.

Bound per (grid, slab, Gauss set): max(1e-13, 8 eps64) in log10 k, eps64 being the deviation of the plain fp64 evaluation
(ktable.numpy_bin with its plain sequential sum, not the compensated one the backend ships) from the reference at the same inputs -- the noise of a correct fp64 implementation
there, worked out on the CPU without the kernel; the factor 8 covers the tree scan's other order of summation.  With the
environment variable KTABLE_EDGES_JSON set, the figures go into the file it names (profiles/ktable_edges.json).

No slab holds inf: the contract does not define what becomes of it."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest

import ktable_reference as kr
from helios_amd import ktable
from helios_amd._lib import HeliosHipError
from helios_amd._tool import dp, ip

pytestmark = pytest.mark.gpu

LD = np.longdouble
PLAIN_FP64 = functools.partial(ktable.numpy_bin, plain_sum=True)


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def record(figures):
    path = os.environ.get("KTABLE_EDGES_JSON")
    if path:
        have = json.load(open(path)) if os.path.exists(path) else {}
        have.update(figures)
        json.dump(have, open(path, "w"), indent=1, sort_keys=True)


def device_table(ctx, c, yg, lds_points=ktable.LDS_POINTS, per_launch=5, firsts=None):
    """kpoints[slab][bin][abscissa] of the case's five slabs, `per_launch` at a time in the order `firsts`"""
    n_tp = len(c.slabs)
    b = ktable.KTableBuilder(ctx, len(c.lam), len(c.start), len(yg), n_tp, per_launch, lds_points)
    try:
        b.set_grid(c.lam, c.start, c.end, c.inter, yg)
        for first in (range(0, n_tp, per_launch) if firsts is None else firsts):
            b.run(c.slabs[first:first + per_launch], first)
        return b.get("kpoints").reshape(n_tp, len(c.start), len(yg))
    finally:
        b.close()


@pytest.mark.parametrize("gauss", ["ng1", "ng20", "ng1100"])
@pytest.mark.parametrize("grid", kr.REFERENCE_CASES)
def test_sort_scan_and_search_against_the_reference(ctx, grid, gauss):
    """every entry of every bin: 0 ... 5 and 63 ... 65 points, 1023 ... 4097 (runs of 1, 2, 3 and 5 points in the scan),
    16383 ... 32769 (the LDS sort's last size, the scratch with one merge level), 70001 (three levels, odd); the second
    grid's last bin holds nu = 0.  Five slabs; the fifth is a bit copy of the first and must give the same bits."""
    c = kr.edge_case(grid)
    yg = c.gauss[gauss]
    ref = c.reference(yg)
    eps64 = c.eps64(PLAIN_FP64, yg, ref)
    got = device_table(ctx, c, yg)
    assert np.all(np.isfinite(got)) and np.all(got > 0)
    dev = np.abs(np.log10(got.astype(LD)) - ref)
    worst = dev.reshape(len(c.slabs), -1).max(axis=1).astype(np.float64)
    bound = np.maximum(1e-13, 8 * eps64)
    figures = {}
    for t in range(len(c.slabs)):
        x = int(np.argmax(dev[t].max(axis=1)))
        print("device %s %s slab %d: deviation %.3e (bin of %d points), eps64 %.3e, bound %.3e"
              % (grid, gauss, t, worst[t], c.end[x] - c.start[x], eps64[t], bound[t]))
        figures["%s %s slab %d" % (grid, gauss, t)] = {"eps64": float(eps64[t]), "bound": float(bound[t]),
                                                       "deviation": float(worst[t])}
    record(figures)
    assert np.all(worst <= bound)
    np.testing.assert_array_equal(got[4], got[0])


@pytest.mark.parametrize("grid", ["sort-0.3", "sort-on-point"])
def test_the_two_sort_paths_bit_for_bit(ctx, grid):
    """bins of 3 ... 2049 points sorted in LDS and through the scratch from blocks of 2, 4, 16 and 64 keys: with blocks of
    2 every merge level of the scratch path runs at every size"""
    c = kr.edge_case(grid)
    yg = c.gauss["ng20"]
    want = device_table(ctx, c, yg)
    for lds_points in (2, 4, 16, 64):
        np.testing.assert_array_equal(device_table(ctx, c, yg, lds_points=lds_points), want, err_msg="lds_points %d" % lds_points)
    # and the table itself is the contract's
    ref = c.reference(yg)
    bound = np.maximum(1e-13, 8 * c.eps64(PLAIN_FP64, yg, ref))
    worst = np.abs(np.log10(want.astype(LD)) - ref).reshape(len(c.slabs), -1).max(axis=1).astype(np.float64)
    print("device %s: deviation %s, bound %s" % (grid, worst, bound))
    assert np.all(worst <= bound)


@pytest.mark.parametrize("lds_points", [ktable.LDS_POINTS, 16])
def test_ragged_batches_bit_for_bit(ctx, lds_points):
    """five slabs, 1, 2 (2, 2, 1) and 4 (4, 1) per launch, and the launches in descending order of their first slab; with
    blocks of 16 keys every slab after a launch's first sorts in its own stretch of the scratch"""
    c = kr.edge_case("sort-0.3")
    yg = c.gauss["ng20"]
    want = device_table(ctx, c, yg, lds_points=lds_points, per_launch=5)
    for per_launch in (1, 2, 4):
        got = device_table(ctx, c, yg, lds_points=lds_points, per_launch=per_launch)
        np.testing.assert_array_equal(got, want, err_msg="%d per launch" % per_launch)
    for per_launch, firsts in ((2, [4, 2, 0]), (4, [4, 0]), (1, [4, 3, 2, 1, 0])):
        got = device_table(ctx, c, yg, lds_points=lds_points, per_launch=per_launch, firsts=firsts)
        np.testing.assert_array_equal(got, want, err_msg="%d per launch, descending" % per_launch)


def test_one_builder_two_grids(ctx):
    """a grid whose bins all fit the LDS sort, then one with a bin above it: the scratch is allocated at the second
    set_grid, and the second table is a fresh builder's"""
    sizes_a, sizes_b = [3, 64, 33, 17], [3, 65, 33, 170]
    grid_a, grid_b = kr.synthetic_grid(sizes_a, 40, 0.01, 0.3, first=3), kr.synthetic_grid(sizes_b, 40, 0.01, 0.3, first=3)
    slabs = kr.edge_slabs(len(grid_a[0]), 21)[:3]
    yg = kr.gauss_sets([])["ng20"]

    def both(first_grid):
        b = ktable.KTableBuilder(ctx, len(grid_a[0]), 4, len(yg), 3, 3, lds_points=64)
        try:
            out = []
            for lam, start, end, inter in ([grid_a, grid_b] if first_grid else [grid_b]):
                b.set_grid(lam, start, end, inter, yg)
                b.run(slabs, 0)
                out.append(b.get("kpoints"))
            return out
        finally:
            b.close()

    a_then_b, b_alone = both(True), both(False)
    np.testing.assert_array_equal(a_then_b[1], b_alone[0])
    assert not np.array_equal(a_then_b[0], a_then_b[1])


# ---- re-gridding -----------------------------------------------------------------------------------------------------------------
def device_regrid(ctx, temps, press, k, nx, ny, targets):
    """kpoints_ip per (temp_new, press_new) of `targets`, one after the other on the same builder"""
    b = ktable.KTableBuilder(ctx, 8, nx, ny, len(temps) * len(press))
    try:
        ctx.check(b._l.hx_ktable_put(b.handle, dp(np.ascontiguousarray(k, np.float64))), "hx_ktable_put")
        out = []
        for temp_new, press_new in targets:
            b.regrid(temps, press, temp_new, press_new)
            out.append(b.get("kpoints_ip"))
        np.testing.assert_array_equal(b.get("kpoints"), k)
        return out
    finally:
        b.close()


@pytest.mark.parametrize("temps,press", kr.REGRID_SOURCES, ids=["1x1", "1x3", "3x1", "3x4"])
def test_regridding_from_small_source_grids(ctx, temps, press):
    """targets below, on, between and above the source's nodes in both axes, sources with a single temperature or pressure;
    a second target on the same builder replaces the first result"""
    nx, ny = 7, 5
    k = kr.regrid_source(temps, press, nx * ny)
    second = ([250.0, 450.0], [1e2, 2e6, 1e7])
    got, got2 = device_regrid(ctx, temps, press, k, nx, ny, [(kr.REGRID_T, kr.REGRID_P), second])
    host = ktable.numpy_regrid(press, temps, k, kr.REGRID_T, kr.REGRID_P, nx, ny)
    ref = np.log10(kr.reference_regrid(temps, press, k, kr.REGRID_T, kr.REGRID_P, nx * ny).reshape(-1))
    eps64 = float(np.abs(np.log10(host.astype(LD)) - ref).max())
    dev = float(np.abs(np.log10(got.astype(LD)) - ref).max())
    bound = max(1e-13, 8 * eps64)
    print("regrid %dx%d: deviation %.3e, eps64 %.3e, bound %.3e" % (len(temps), len(press), dev, eps64, bound))
    record({"regrid %dx%d" % (len(temps), len(press)): {"eps64": eps64, "bound": bound, "deviation": dev}})
    assert got.shape == host.shape and np.all(np.isfinite(got)) and dev <= bound
    np.testing.assert_array_equal(got, host)
    assert got2.shape == (2 * 3 * nx * ny,)
    np.testing.assert_array_equal(got2, ktable.numpy_regrid(press, temps, k, second[0], second[1], nx, ny))


def test_regridding_beyond_one_pass_of_the_launch(ctx):
    """2 x 2 source nodes of 322 x 20 entries onto the default 120 x 28 grid: 21.6 M elements, more than the 65536 x 256
    the launch covers in one pass.  Bit for bit numpy_regrid's, and at the bound against the reference."""
    nx, ny = 322, 20
    nc = nx * ny
    temps, press = [1000.0, 3000.0], [1e3, 1e6]
    k = kr.regrid_source(temps, press, nc, seed=5)
    temp_new, press_new = ktable.default_target_grid()
    assert len(temp_new) * len(press_new) * nc > 65536 * 256
    got, = device_regrid(ctx, temps, press, k, nx, ny, [(temp_new, press_new)])
    host = ktable.numpy_regrid(press, temps, k, temp_new, press_new, nx, ny)
    np.testing.assert_array_equal(got, host)
    got, host = got.reshape(len(temp_new), -1), host.reshape(len(temp_new), -1)
    eps64 = dev = 0.0
    for rows in np.array_split(np.arange(len(temp_new)), 12):
        ref = kr.reference_regrid(temps, press, k, temp_new, press_new, nc, rows=rows).reshape(len(rows), -1)
        eps64 = max(eps64, float(np.abs(np.log10(host[rows].astype(LD) / ref)).max()))
        dev = max(dev, float(np.abs(np.log10(got[rows].astype(LD) / ref)).max()))
    bound = max(1e-13, 8 * eps64)
    print("regrid 2x2 -> 120x28: deviation %.3e, eps64 %.3e, bound %.3e" % (dev, eps64, bound))
    record({"regrid 2x2 to 120x28": {"eps64": eps64, "bound": bound, "deviation": dev}})
    assert dev <= bound


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    """host-side checks all: none launches a kernel or hands one an index out of range; the builder works afterwards"""
    c = kr.edge_case("sort-0.3")
    yg = c.gauss["ng20"]
    n, nbin, ng = len(c.lam), len(c.start), len(yg)
    for lds_points in (0, 3, 24, 32768):
        with pytest.raises(HeliosHipError, match="power of two"):
            ktable.KTableBuilder(ctx, n, nbin, ng, 5, 2, lds_points)
    b = ktable.KTableBuilder(ctx, n, nbin, ng, 5, 2)
    try:
        with pytest.raises(HeliosHipError, match="set the grid first"):
            b.run(c.slabs[:1], 0)
        # grids
        end = c.end.copy()
        end[-1] = n + 1
        with pytest.raises(HeliosHipError, match="outside the spectral axis"):
            b.set_grid(c.lam, c.start, end, c.inter, yg)
        start = c.start.copy()
        start[0] = -1
        with pytest.raises(HeliosHipError, match="outside the spectral axis"):
            b.set_grid(c.lam, start, c.end, c.inter, yg)
        inter = c.inter.copy()
        inter[3] = inter[2]
        with pytest.raises(HeliosHipError, match="interfaces are not ascending"):
            b.set_grid(c.lam, c.start, c.end, inter, yg)
        start = c.start.copy()
        start[5] -= 1                                     # one point shared with the bin below
        with pytest.raises(HeliosHipError, match="overlap"):
            b.set_grid(c.lam, start, c.end, c.inter, yg)
        with pytest.raises(HeliosHipError, match="overlap"):
            b.set_grid(c.lam, c.start[::-1], c.end[::-1], c.inter, yg)
        with pytest.raises(HeliosHipError, match="set the grid first"):      # a refused grid is no grid
            b.run(c.slabs[:1], 0)
        b.set_grid(c.lam, c.start, c.end, c.inter, yg)
        # launches
        with pytest.raises(HeliosHipError, match="max_tp_per_launch"):
            b.run(c.slabs[:3], 0)
        for first in (4, 5, -1):
            with pytest.raises(HeliosHipError, match="reach beyond"):
                b.run(c.slabs[:2], first)
        # results
        buf = np.zeros(5 * nbin * ng + 1, np.float64)
        get = lambda name, nbytes: ctx.check(b._l.hx_ktable_get(b.handle, name, buf.ctypes.data_as(ctypes.c_void_p), nbytes), "get")
        with pytest.raises(HeliosHipError, match="bytes expected"):
            get(b"kpoints", buf.nbytes)
        with pytest.raises(HeliosHipError, match="bytes expected"):
            get(b"timing_ms", 24)
        with pytest.raises(HeliosHipError, match="unknown name"):
            get(b"kpoints_old", buf.nbytes)
        with pytest.raises(HeliosHipError, match="re-grid first"):
            get(b"kpoints_ip", 8)
        # re-gridding: 5 source nodes are 1 x 5 or 5 x 1
        one, five = np.array([300.0]), np.array([1.0, 2.0, 3.0, 4.0, 5.0])
        zero, i4, i5 = np.zeros(1, np.int32), np.array([4], np.int32), np.array([5], np.int32)
        new = np.array([4.5])

        def regrid(nt_old, np_old, t_left, t_red, p_left, p_red):
            t_old, p_old = (one, five) if nt_old == 1 else (five, one)
            ctx.check(b._l.hx_ktable_regrid(b.handle, nt_old, np_old, 1, 1, ip(t_left), ip(t_red),
                                            ip(p_left), ip(p_red), dp(t_old), dp(p_old),
                                            dp(new), dp(new)), "hx_ktable_regrid")

        clamped = np.ones(1, np.int32)
        with pytest.raises(HeliosHipError, match="not the table's number"):
            regrid(2, 2, zero, clamped, zero, clamped)
        with pytest.raises(HeliosHipError, match="not the table's number"):
            regrid(5, 5, zero, clamped, zero, clamped)
        with pytest.raises(HeliosHipError, match="pressure plan out of range"):
            regrid(1, 5, zero, clamped, i4, zero)             # the last node, not clamped: reads node 5 of 5
        with pytest.raises(HeliosHipError, match="pressure plan out of range"):
            regrid(1, 5, zero, clamped, i5, clamped)
        with pytest.raises(HeliosHipError, match="temperature plan out of range"):
            regrid(5, 1, i4, zero, zero, clamped)
        with pytest.raises(HeliosHipError, match="temperature plan out of range"):
            regrid(1, 5, zero, zero, zero, clamped)           # a single temperature cannot be interpolated
        with pytest.raises(HeliosHipError, match="temperature plan out of range"):
            regrid(5, 1, np.array([-1], np.int32), clamped, zero, clamped)
        with pytest.raises(HeliosHipError, match="re-grid first"):
            get(b"kpoints_ip", 8)
        # and the builder still does its work
        for first in (0, 2, 4):
            b.run(c.slabs[first:first + 2], first)
        got = b.get("kpoints").reshape(5, nbin, ng)
    finally:
        b.close()
    np.testing.assert_array_equal(got, device_table(ctx, c, yg))
