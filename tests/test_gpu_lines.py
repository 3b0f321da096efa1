"""k_lines_prepare_nodes, k_lines_sum_nodes_fp64 and the sum's K (csrc/lines.hip) through hx_lines and lines.py on the device,
under the rule of tests/lines_cases.py: K at the goldens; point counts around the tile and line counts around the LDS block, derived from the
constants the module exports; the placements at which the sum decides; and a species from its line list to a k-table."""
import os

import numpy as np
import pytest

import lines_cases as lc
import lines_reference as lr
from helios_amd import lines
from helios_amd._lib import HeliosHipError

pytestmark = pytest.mark.gpu

TILE, BLOCK = lines.TILE_POINTS, lines.LDS_BLOCK
ATM = lines.ATM


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def run_node(ctx, line, temp, press, grid, cutoff, x_self=0.0, molar_mass=lc.M_H2O, twice=True):
    """(kappa64, kappa32, line_params, timing) of one node through a handle of its own, one node per launch with fp64 rows;
    the node is run twice and the bits compared"""
    q = lc.q_table()
    h = lines.LineOpacity(ctx, len(line["nu0"]), grid[2], 1, 1, with_fp64=True)
    try:
        h.set_lines(line)
        h.set_nodes([temp], [press], [lines.partition_value(q, temp)], lines.partition_value(q, 296.0), molar_mass, x_self, cutoff, *grid)
        h.run_nodes(0, 1)
        out = h.get("kappa64")[0], h.get("slabs32")[0], h.get("line_params")[0], h.get("timing_ms")
        if twice:
            h.run_nodes(0, 1)
            assert np.array_equal(h.get("kappa64")[0].view(np.uint64), out[0].view(np.uint64))
            assert np.array_equal(h.get("line_params")[0].view(np.uint64), out[2].view(np.uint64))
        return out
    finally:
        h.close()


def check_node(ctx, line, temp, press, grid, cutoff, label, x_self=0.0):
    """runs the node and holds kappa64 and line_params to the rule, kappa32 to kappa64's rounding; returns kappa64, line_params"""
    k64, k32, prm, timing = run_node(ctx, line, temp, press, grid, cutoff, x_self)
    assert k64.shape == (grid[2],) and k32.dtype == np.float32 and prm.shape == (4, len(line["nu0"]))
    assert timing[0] > 0 and timing[1] > 0
    ld, f64 = lc.restated(line, temp, press, x_self, cutoff, *grid)
    lc.check_rule(k64, ld, f64, label + ", kappa64")
    pld, pf64 = lc.restated_params(line, temp, press, x_self)
    lc.check_rule(prm, pld, pf64, label + ", line_params")
    with np.errstate(over="ignore"):
        assert np.array_equal(k32.view(np.uint32), k64.astype(np.float32).view(np.uint32))
    return k64, prm


# ---- K ------------------------------------------------------------------------------------------------------------------
def test_the_kernels_k_at_every_golden_pair_against_the_restatement(ctx):
    g = lc.goldens()
    k = lines.device_voigt(ctx, g["x"], g["y"])
    lc.check_rule(k, lr.voigt_k(g["x"], g["y"], np.longdouble), lr.voigt_k(g["x"], g["y"], np.float64), "hx_lines_voigt")


@pytest.mark.parametrize("reg", [0, 1, 2, 3])
def test_the_kernels_k_against_mpmath(ctx, reg):
    """1e-6 relative of the goldens in every region, both sides of |z| = 6 and of the boundaries 6.5, 15 and 100 included; the
    regions measure what the restatement measures (tests/test_lines_reference.py::test_k_against_mpmath)"""
    g = lc.goldens()
    m = lr.region(g["x"], g["y"]) == reg
    k = lines.device_voigt(ctx, g["x"][m], g["y"][m])
    dev = np.abs(k.astype(np.longdouble) / g["k"][m] - 1)
    j = int(np.argmax(dev))
    print("region %d on the device: worst deviation from mpmath %.3e at x = %.17g, y = %g" % (reg, float(dev[j]), g["x"][m][j],
                                                                                              g["y"][m][j]))
    assert dev.max() <= lc.GOLDEN_BOUND


# ---- sizes at which the sum changes path ------------------------------------------------------------------------------
DNU, CUTOFF = 0.25, 2.0                       # a tile is TILE / 4 cm^-1 wide, a line reaches 17 points


def spread_lines(n, n_points, seed):
    """n lines within the first tile's stretch of the grid (or within the whole grid if that is shorter)"""
    width = min(n_points, TILE) * DNU
    return lc.synthetic_lines(n, 1000.0 + 0.02 * width, 1000.0 + 0.98 * width, seed=seed)


@pytest.mark.parametrize("n_points", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_point_counts_around_the_tile(ctx, n_points):
    line = lc.join(spread_lines(BLOCK + 1, n_points, seed=n_points), lc.synthetic_lines(40, 1000.0, 1000.0 + n_points * DNU, seed=5))
    k64, _ = check_node(ctx, line, 700.0, 1e5, (1000.0, DNU, n_points), CUTOFF, "%d points" % n_points)
    assert np.count_nonzero(k64) >= min(n_points, 400)


@pytest.mark.parametrize("n_lines", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1])
def test_line_counts_around_the_lds_block(ctx, n_lines):
    """n_lines in reach of the first tile, and a hundred lines beyond the last point + cut-off, which no tile takes"""
    n_points = TILE + 1
    beyond = lc.synthetic_lines(100, 1000.0 + n_points * DNU + CUTOFF + 1.0, 1000.0 + n_points * DNU + 500.0, seed=8)
    line = lc.join(spread_lines(n_lines, n_points, seed=20 + n_lines), beyond) if n_lines else beyond
    k64, _ = check_node(ctx, line, 700.0, 1e5, (1000.0, DNU, n_points), CUTOFF, "%d lines in reach" % n_lines)
    if n_lines == 0:
        assert not k64.any()
    else:
        assert 16 <= np.count_nonzero(k64) <= 17 * n_lines


# ---- placements ---------------------------------------------------------------------------------------------------------
def test_a_line_centred_on_a_point_and_the_cutoff_to_the_ulp(ctx):
    """nu_0 = 100 on point 400 of a grid of step 1/4: the points at 75 and 125 lie exactly C = 25 away and are in; with nu_0 one
    ulp below 100 the point at 125 is out and the one at 75 stays in"""
    grid = (0.0, 0.25, 801)
    k64, prm = check_node(ctx, lc.one_line(100.0), 300.0, 1e5, grid, 25.0, "centred")
    assert prm[0, 0] == 100.0 and int(np.argmax(k64)) == 400
    assert np.nonzero(k64)[0].tolist() == list(range(300, 501))
    below = float(np.nextafter(100.0, 0.0))
    k64, prm = check_node(ctx, lc.one_line(below), 300.0, 1e5, grid, 25.0, "one ulp below")
    assert prm[0, 0] == below and 125.0 - below > 25.0
    assert np.nonzero(k64)[0].tolist() == list(range(300, 500))


def test_a_line_outside_the_grid_whose_wing_enters_it(ctx):
    grid = (100.0, 0.25, TILE + 40)
    k64, _ = check_node(ctx, lc.one_line(90.0), 300.0, 1e6, grid, 25.0, "wing from outside")
    assert np.nonzero(k64)[0].tolist() == list(range(0, 61)) and np.all(np.diff(k64[:61]) < 0)
    after = 100.0 + (TILE + 39) * 0.25 + 10.0
    k64, _ = check_node(ctx, lc.one_line(after), 300.0, 1e6, grid, 25.0, "wing from beyond the last point")
    assert np.count_nonzero(k64) == 61 and k64[-1] > 0 and not k64[:TILE - 21].any()


def test_shifted_centres_cross_and_the_order_of_summation_stays(ctx):
    """at 1e3 atm the shifts of +-0.01 cm^-1 / atm take 100.000 to 110 and 100.001 to 90.001: the restatement adds in the order of the
    list, and so does the kernel"""
    pair = lc.join(lc.one_line(100.0, delta_air=0.01, s_ref=1e-20), lc.one_line(100.001, delta_air=-0.01, s_ref=3e-21))
    line = lc.join(pair, lc.synthetic_lines(30, 60.0, 140.0, seed=6))
    k64, prm = check_node(ctx, line, 500.0, 1e3 * ATM, (50.0, 0.25, 401), 25.0, "crossing centres")
    j = int(np.nonzero(line["nu0"] == 100.0)[0][0])
    assert line["nu0"][j + 1] == 100.001 and prm[0, j] == 110.0 and abs(prm[0, j + 1] - 90.001) < 1e-12
    assert np.all(k64 > 0)


def test_y_at_the_clamp(ctx):
    line = lc.synthetic_lines(12, 1000.0, 1003.0, seed=4)
    k64, prm = check_node(ctx, line, 300.0, 1e-4, (999.0, 0.002, TILE + 500), 1.0, "y at the clamp")
    assert np.all(prm[3] == lines.Y_MIN)
    reg = lines.region(prm[2, 0] * (999.0 + np.arange(TILE + 500) * 0.002 - prm[0, 0]), prm[3, 0])
    assert set(reg.tolist()) == {0, 1, 2, 3}


def test_a_node_where_every_pair_lies_beyond_100(ctx):
    """1e3 atm: every line's y lies beyond FAR_Z, the kernel's own condition for the loop that knows the region"""
    line = lc.synthetic_lines(BLOCK + 30, 1000.0, 1256.0, seed=12)
    grid = (1000.0, 0.25, TILE + 1)
    k64, prm = check_node(ctx, line, 300.0, 1e3 * ATM, grid, 25.0, "all pairs beyond |z| = 100")
    assert prm[3].min() > lines.FAR_Z
    assert np.all(k64 > 0)


def test_both_loops_in_one_tile_and_a_wavefront_across_all_four_regions(ctx):
    """low pressure at 0.01 cm^-1: a step is 4 to 6 units of x, so the 64 consecutive points of one wavefront around a line's
    centre pass through all four regions; the tile takes the general loop for the block of the lines inside it and the loop
    that knows the region for a block of lines that all lie far outside it"""
    near = lc.synthetic_lines(BLOCK, 1002.0, 1008.0, seed=13)
    far = lc.synthetic_lines(BLOCK, 985.0, 995.0, seed=14)
    line = lc.join(far, near)
    grid = (1000.0, 0.01, TILE)
    k64, prm = check_node(ctx, line, 300.0, 1e3, grid, 25.0, "all regions")
    nu = grid[0] + np.arange(TILE) * grid[1]
    j = BLOCK + 5
    centre = int(np.argmin(np.abs(nu - prm[0, j])))
    wave = slice(centre - centre % lines.WAVEFRONT, centre - centre % lines.WAVEFRONT + lines.WAVEFRONT)
    assert set(lines.region(prm[2, j] * (nu[wave] - prm[0, j]), prm[3, j]).tolist()) == {0, 1, 2, 3}
    dist = np.maximum(np.maximum(prm[0, :BLOCK] - nu[-1], nu[0] - prm[0, :BLOCK]), 0.0)
    assert np.all(prm[2, :BLOCK] * dist > lines.FAR_Z) and np.all(line["nu0"][:BLOCK] < 1000.0)
    assert not np.all(prm[2, BLOCK:] * np.maximum(np.maximum(prm[0, BLOCK:] - nu[-1], nu[0] - prm[0, BLOCK:]), 0.0) > lines.FAR_Z)


# ---- the handle -----------------------------------------------------------------------------------------------------------
def test_refusals_name_the_count_and_leave_the_handle_usable(ctx):
    line = lc.synthetic_lines(20, 1000.0, 1050.0, seed=2)
    q = lc.q_table()
    node = ([700.0], [1e5], [lines.partition_value(q, 700.0)], lines.partition_value(q, 296.0), lc.M_H2O, 0.0, CUTOFF)
    h = lines.LineOpacity(ctx, 19, 300, 1, 1, with_fp64=True)
    try:
        with pytest.raises(HeliosHipError, match=r"20 lines, the handle holds 1 \.\.\. 19") as e:
            h.set_lines(line)
        assert "status 1:" in str(e.value)
        with pytest.raises(HeliosHipError, match="no line list"):
            h.set_nodes(*(node + (1000.0, DNU, 200)))
        fewer = dict((k, line[k][:19]) for k in lr.FIELDS)
        h.set_lines(fewer)
        with pytest.raises(HeliosHipError, match="no nodes have been run"):
            h.get("kappa64")
        with pytest.raises(HeliosHipError, match=r"301 spectral points, the handle holds 1 \.\.\. 300"):
            h.set_nodes(*(node + (1000.0, DNU, 301)))
        with pytest.raises(HeliosHipError, match=r"T = -700 is not a finite number > 0"):
            h.set_nodes(*(([-700.0],) + node[1:] + (1000.0, DNU, 200)))
        with pytest.raises(HeliosHipError, match=r"x_self = 1\.5 lies outside \[0, 1\]"):
            h.set_nodes(*(node[:5] + (1.5, CUTOFF, 1000.0, DNU, 200)))
        unsorted = dict((k, fewer[k][::-1].copy()) for k in lr.FIELDS)
        with pytest.raises(HeliosHipError, match=r"line 1: nu0 = .* lies below line 0's .*: the list is sorted"):
            h.set_lines(unsorted)
        h.set_lines(fewer)
        h.set_nodes(*(node + (1000.0, DNU, 200)))
        h.run_nodes(0, 1)
        got = h.get("kappa64")[0]
    finally:
        h.close()
    ld, f64 = lc.restated(fewer, 700.0, 1e5, 0.0, CUTOFF, 1000.0, DNU, 200)
    lc.check_rule(got, ld, f64, "after the refusals")


def test_line_opacity_on_the_device_equals_the_numpy_backend_under_the_rule(ctx):
    line = lc.synthetic_lines(60, 995.0, 1030.0, seed=15)
    grid = (1000.0, 0.05, 500)
    temps, press = [300.0, 1200.0], [1e2, 1e7]
    timing = {}
    dev = lines.line_opacity(line, lc.q_table(), temps, press, grid, lc.M_H2O, 0.1, 5.0, backend="device", ctx=ctx, timing=timing)
    host = lines.line_opacity(line, lc.q_table(), temps, press, grid, lc.M_H2O, 0.1, 5.0, backend="numpy", timing={})
    assert dev.shape == host.shape == (2, 2, 500) and timing["sum_ms"] > 0 and timing["pairs"] > 0
    for it, t in enumerate(temps):
        for ip, p in enumerate(press):
            ld, f64 = lc.restated(line, t, p, 0.1, 5.0, *grid)
            lc.check_rule(dev[it, ip], ld, f64, "line_opacity on the device at %g K, %g" % (t, p))
            lc.check_rule(host[it, ip], ld, f64, "numpy at %g K, %g" % (t, p))


# ---- from a line list to a k-table ----------------------------------------------------------------------------------------
def test_from_a_line_list_to_a_k_table(tmp_path):
    """lines.py on 300 synthetic lines, 2 temperatures x 2 pressure codes, 0 - 2000 cm^-1 at 0.05 cm^-1, then ktable.py on that
    directory with a coarse grid inside the range, both on the device: every entry is finite and log10 k ascends along y"""
    import ktable as ktable_tool
    import lines as lines_tool
    wd = str(tmp_path)
    line = lc.synthetic_lines(300, 150.0, 1950.0, seed=21)
    lc.write_par_file(os.path.join(wd, "h2o.par"), line)
    lc.write_q_file(os.path.join(wd, "q.txt"))
    out = os.path.join(wd, "opac", "H2O")
    written = lines_tool.main(["-name", "H2O", "-line_list", os.path.join(wd, "h2o.par"), "-partition_function",
                               os.path.join(wd, "q.txt"), "-temperatures", "300 900", "-pressure_codes", "n300 p000", "-numin", "0",
                               "-numax", "2000", "-dnu", "0.05", "-output_directory", out])
    assert len(written) == 4 and all(os.path.getsize(w) == 4 * 40000 for w in written)
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nH2O %s\n" % out)
    tables = ktable_tool.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-wavelength_grid", "20 6 40",
                               "-number_of_gaussian_points", "8", "-directory_with_individual_files", os.path.join(wd, "tables"),
                               "-container", "npz", "-interpolate", "no"])
    assert [os.path.basename(t) for t in tables] == ["H2O_opac_kdistr.npz"]
    t = np.load(tables[0])
    nx, ny = len(t["center wavelengths"]), len(t["ypoints"])
    assert ny == 8 and nx >= 30 and t["temperatures"].tolist() == [300.0, 900.0] and len(t["pressures"]) == 2
    k = t["kpoints"].reshape(4, nx, ny)
    assert np.all(np.isfinite(k)) and np.all(k > 0)
    assert np.all(np.diff(np.log10(k), axis=2) >= 0)
    assert k.max() > 1e3 * k.min()
