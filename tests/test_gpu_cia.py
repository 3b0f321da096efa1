"""k_cia_nodes (csrc/cia.hip) through hx_cia and cia.py on the device.  The contract has no libm call and nothing is contracted, so
every comparison with the numpy backend is bit for bit, in the fp64 rows and in the fp32 slabs: on the table whose points stand
on and one ulp beside the grid's (tests/cia_cases.py), at the sizes at which the kernel changes path -- derived from the constants
the module exports -- and from a file to the k-table and into a run of helios.py."""
import os

import numpy as np
import pytest

import cia_cases as cc
from helios_amd import cia, ktable
from helios_amd._lib import HeliosHipError

pytestmark = pytest.mark.gpu

TILE, WINDOW = cia.TILE_POINTS, cia.WINDOW
PER = 3                                       # nodes per launch of the handles here
FP32_MIN_NORMAL = 1.1754943508222875e-38


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def numpy_rows(bands, nodes, grid):
    """kappa64 [node][n_points] of the numpy backend"""
    return np.stack([cia.numpy_node(bands, t, p, grid[0], grid[1], grid[2], cc.M_H2) for t, p in nodes])


def device_rows(ctx, bands, nodes, grid, per_launch=PER, points_max=None):
    """(kappa64, slabs32) [node][n_points] of the nodes in batches of per_launch, through a handle of its own"""
    h = cia.CiaOpacity(ctx, bands, points_max or grid[2], per_launch, len(nodes), True)
    try:
        h.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], cc.M_H2, *grid)
        k64, k32 = [], []
        for first in range(0, len(nodes), per_launch):
            h.run_nodes(first, min(per_launch, len(nodes) - first))
            k64.append(h.get("kappa64"))
            k32.append(h.get("slabs32"))
        timing = h.get("timing_ms")
        assert timing[0] > 0 and timing[1] == -(-len(nodes) // per_launch)
        return np.concatenate(k64), np.concatenate(k32)
    finally:
        h.close()


def same_bits(got, want, label):
    assert got.dtype == want.dtype and got.shape == want.shape, label
    view = np.uint64 if got.dtype == np.float64 else np.uint32
    bad = np.nonzero(got.view(view) != want.view(view))
    assert len(bad[0]) == 0, (label, len(bad[0]), [tuple(int(v) for v in b) + (float(got[b]), float(want[b])) for b in zip(*bad)][:5])


def check(ctx, bands, nodes, grid, label, **how):
    want = numpy_rows(bands, nodes, grid)
    k64, k32 = device_rows(ctx, bands, nodes, grid, **how)
    same_bits(k64, want, label + ", kappa64")
    with np.errstate(under="ignore"):
        same_bits(k32, want.astype(np.float32), label + ", slabs32")
    return k64, k32


def window(block, tile_lo, tile_hi):
    """entries of the block that k_cia_nodes stages for a tile tile_lo ... tile_hi"""
    n = len(block.nu)
    lo, hi = (min(max(int(np.searchsorted(block.nu, v, side="right")) - 1, 0), n - 2) for v in (tile_lo, tile_hi))
    return hi + 1 - lo + 1


# ---- the table of the edges -------------------------------------------------------------------------------------------------
def test_the_table_of_the_edges(ctx):
    """Every point of the edge table at every temperature of EDGE_TEMPS and, for two of them, at a pressure that takes kappa into
    fp32's subnormals: 15 nodes in launches of 4, 4, 4 and 3.  Tile 0 straddles band a's start, tile 1 lies inside it, tile 2
    meets both bands and the gap, tile 3 (37 points) lies outside every band; the 200 K and 300 K blocks have grids of their own
    and the 400 K block has 2 points"""
    bands = cia.bands_of(cc.edge_blocks())
    grid = cc.EDGE_GRID
    assert grid[2] % TILE == 37 and [len(b.blocks) for b in bands] == [3, 1]
    nu = cc.grid_nu(grid)
    for t in range(2):                        # tiles 0 and 1 stage their windows of the 200 K and 300 K blocks
        assert all(window(b, nu[t * TILE], nu[(t + 1) * TILE - 1]) <= WINDOW for b in bands[0].blocks)
    assert bands[0].numax > nu[2 * TILE] and bands[1].numin < nu[3 * TILE - 1] < nu[3 * TILE] and bands[1].numax < nu[3 * TILE]
    nodes = [(t, 1e6) for t in cc.EDGE_TEMPS] + [(250.0, 1e-20), (300.0, 1e-23)]
    k64, k32 = check(ctx, bands, nodes, grid, "edges", per_launch=4)
    assert not k64[:, :cc.A_LO + 1].any() and not k64[:, cc.A_HI + 1:cc.B_LO].any() and not k64[:, cc.B_HI:].any()
    assert np.all(np.count_nonzero(k64, axis=1) > 2000)
    tiny = k32[-2:]
    assert np.count_nonzero((tiny > 0) & (tiny < FP32_MIN_NORMAL)) > 100 and tiny.max() > FP32_MIN_NORMAL
    assert np.count_nonzero((tiny == 0) & (k64[-2:] > 0)) > 0          # and values that fp32 no longer holds


@pytest.mark.parametrize("n_nodes", [1, PER, PER + 1])
def test_node_counts_around_a_launch(ctx, n_nodes):
    """rows with the stride n_points in buffers of longer rows; the last launch of PER + 1 nodes fills one row"""
    bands = cia.bands_of(cc.edge_blocks())
    nodes = [(180.0 + 70.0 * k, 10.0 ** (3 + k)) for k in range(n_nodes)]
    k64, _ = check(ctx, bands, nodes, cc.EDGE_GRID, "%d nodes" % n_nodes, points_max=cc.EDGE_GRID[2] + 5)
    assert len({row.tobytes() for row in k64}) == n_nodes


@pytest.mark.parametrize("n_points", [1, TILE - 1, TILE, TILE + 1])
def test_grid_lengths_around_the_tile(ctx, n_points):
    bands = cia.bands_of(cc.edge_blocks())
    k64, _ = check(ctx, bands, [(250.0, 1e5), (450.0, 1e6)], (30.0, 0.173, n_points), "%d points" % n_points, points_max=n_points + 3)
    assert np.count_nonzero(k64) >= 2 * n_points - 4


@pytest.mark.parametrize("extra", [0, 1])
def test_a_window_of_the_lds_capacity_and_one_more(ctx, extra):
    """a block at every whole wavenumber from 100 on and a tile from 100.5 over WINDOW - 2 + extra of its intervals: the window
    holds WINDOW + extra entries.  The second tile is short and stages in both cases"""
    rng = np.random.default_rng(5)
    blocks = [cc.block(90.0, 900.0, 300.0, 100.0 + np.arange(WINDOW + 60), rng),
              cc.block(90.0, 900.0, 500.0, [95.0, 700.0], rng)]
    bands = cia.bands_of(blocks)
    grid = (100.5, (WINDOW - 2 + extra) / (TILE - 1.0), TILE + 37)
    nu = cc.grid_nu(grid)
    assert window(bands[0].blocks[0], nu[0], nu[TILE - 1]) == WINDOW + extra and window(bands[0].blocks[1], nu[0], nu[TILE - 1]) == 2
    assert window(bands[0].blocks[0], nu[TILE], nu[-1]) < WINDOW
    k64, _ = check(ctx, bands, [(300.0, 1e6), (410.0, 1e6), (600.0, 1e4)], grid, "window of %d" % (WINDOW + extra))
    assert np.all(np.count_nonzero(k64, axis=1) > TILE)


def test_refusals_name_the_value_and_leave_the_handle_usable(ctx):
    bands = cia.bands_of(cc.edge_blocks())
    grid = (30.0, 0.173, 500)
    nodes = [(250.0, 1e5), (450.0, 1e6), (300.0, 1e3)]
    want = numpy_rows(bands, nodes, grid)
    h = cia.CiaOpacity(ctx, bands, 500, 2, 3, True)
    try:
        with pytest.raises(HeliosHipError, match="no nodes"):
            h.run_nodes(0, 1)
        with pytest.raises(HeliosHipError, match=r"4 nodes, the handle holds 1 \.\.\. 3"):
            h.set_nodes([300.0] * 4, [1e5] * 4, cc.M_H2, *grid)
        with pytest.raises(HeliosHipError, match=r"501 spectral points, the handle holds 1 \.\.\. 500"):
            h.set_nodes([300.0], [1e5], cc.M_H2, 30.0, 0.173, 501)
        with pytest.raises(HeliosHipError, match=r"node 1: T = -5 is not a finite number > 0"):
            h.set_nodes([300.0, -5.0], [1e5, 1e5], cc.M_H2, *grid)
        with pytest.raises(HeliosHipError, match=r"M = 0 is not a finite number > 0"):
            h.set_nodes([300.0], [1e5], 0.0, *grid)
        h.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], cc.M_H2, *grid)
        with pytest.raises(HeliosHipError, match="no nodes have been run"):
            h.get("slabs32")
        with pytest.raises(HeliosHipError, match=r"3 nodes in one call, the handle holds 1 \.\.\. 2 per launch"):
            h.run_nodes(0, 3)
        with pytest.raises(HeliosHipError, match=r"nodes 2 \.\.\. 3, hx_cia_set_nodes gave 0 \.\.\. 2"):
            h.run_nodes(2, 2)
        h.run_nodes(1, 2)
        same_bits(h.get("kappa64"), want[1:3], "after the refusals")
        off, nu, k, temp, first, numin, numax = cia.pack(bands)
        bad = nu.copy()
        bad[off[1] + 4] = bad[off[1] + 3]
        with pytest.raises(HeliosHipError, match=r"block 1, point 4: nu = .* does not lie above"):
            h.set_blocks(off, bad, k, temp, first, numin, numax)
        with pytest.raises(HeliosHipError, match=r"band 1 starts at .*, band 0 ends at .*: bands neither overlap nor touch"):
            h.set_blocks(off, nu, k, temp, first, numin, np.array([numin[1], numax[1]]))
        h.run_nodes(0, 2)                                 # a refused table leaves the one before it, and its nodes
        same_bits(h.get("kappa64"), want[0:2], "after the refused tables")
        h.set_blocks(off, nu, k, temp, first, numin, numax)
        with pytest.raises(HeliosHipError, match="no nodes"):
            h.run_nodes(0, 1)
        h.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], cc.M_H2, *grid)
        h.run_nodes(0, 1)
        same_bits(h.get("kappa64"), want[0:1], "after the table was set again")
    finally:
        h.close()
    lean = cia.CiaOpacity(ctx, bands, 500, 2, 3)
    try:
        lean.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], cc.M_H2, *grid)
        lean.run_nodes(0, 2)
        with np.errstate(under="ignore"):
            same_bits(lean.get("slabs32"), want[0:2].astype(np.float32), "without fp64 rows")
        with pytest.raises(HeliosHipError, match="the handle keeps no fp64 rows"):
            lean.get("kappa64")
        assert lean.slab_pointer().value
    finally:
        lean.close()


def test_cia_opacity_on_the_device_equals_the_numpy_backend(ctx):
    temps, press = [150.0, 250.0, 1200.0], [1e2, 1e7]
    grid = (15.0, 0.21, TILE + 300)
    timing = {}
    dev = cia.cia_opacity(cc.edge_blocks(), temps, press, grid, cc.M_H2, backend="device", ctx=ctx, nodes_per_launch=4, timing=timing)
    host = cia.cia_opacity(cc.edge_blocks(), temps, press, grid, cc.M_H2, backend="numpy")
    assert dev.shape == (3, 2, TILE + 300) and timing["nodes_ms"] > 0 and np.count_nonzero(dev) > 6 * TILE
    same_bits(dev, host, "cia_opacity")


def test_a_handle_made_for_fewer_nodes_takes_them_in_turns(ctx):
    """three nodes through a handle made for two, two per launch: turns of 2 + 1 and a short last launch, on one full tile and
    one point of the edge table's band a.  Bit for bit what the same call gives with a handle of its own, which takes the three
    in one turn; the handle given stays open"""
    temps, press, grid = [250.0, 350.0, 450.0], [1e5], (30.0, 0.173, TILE + 1)
    own, turns = {}, {}
    want = cia.cia_opacity(cc.edge_blocks(), temps, press, grid, cc.M_H2, backend="device", ctx=ctx, timing=own)
    h = cia.CiaOpacity(ctx, cia.bands_of(cc.edge_blocks()), TILE + 1, 2, 2, True)
    try:
        got = cia.cia_opacity(cc.edge_blocks(), temps, press, grid, cc.M_H2, backend="device", ctx=ctx, handle=h, timing=turns)
        assert h.handle and h.n_nodes == 1 and h.rows_run == 1               # left open, after the turn of one node
    finally:
        h.close()
    assert got.shape == (3, 1, TILE + 1) and np.all(np.count_nonzero(got, axis=2) > TILE - 10)
    assert len({row.tobytes() for row in got[:, 0]}) == 3
    same_bits(got, want, "in turns")
    assert own["nodes_ms"] > 0 and turns["nodes_ms"] > 0


# ---- from the file to the k-table and into a run ------------------------------------------------------------------------------
def test_the_fused_containers_equal_the_two_step_routes_on_the_device(tmp_path):
    """`cia.py` then `ktable.py` against `cia.py -ktable yes`, all on the device, four nodes in launches of 3 and 1"""
    import cia as cia_tool
    import ktable as ktable_tool
    wd = str(tmp_path)
    path = cc.write_cia_file(os.path.join(wd, "h2h2.cia"), cc.tool_blocks())
    argv = ["-name", "CIA_H2H2", "-cia_file", path, "-temperatures", "900 300", "-pressure_codes", "p000 n300", "-numax", "2000",
            "-dnu", "0.05", "-nodes_per_launch", "3"]
    grid = ["-wavelength_grid", "20 6 40", "-number_of_gaussian_points", "8", "-container", "npz", "-temperature_grid", "200 1000 400",
            "-pressure_grid", "2 6 3"]
    files = cia_tool.main(argv + ["-output_directory", os.path.join(wd, "opac", "CIA_H2H2")])
    assert len(files) == 4 and all(os.path.getsize(f) == 4 * 40000 for f in files)
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nCIA_H2H2 %s\n" % os.path.join(wd, "opac", "CIA_H2H2"))
    want = ktable_tool.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat"), "-directory_with_individual_files",
                             os.path.join(wd, "two_step")] + grid)
    got = cia_tool.main(argv + ["-ktable", "yes", "-directory_with_individual_files", os.path.join(wd, "fused")] + grid)
    assert [os.path.basename(p) for p in got] == ["CIA_H2H2_opac_kdistr.npz", "CIA_H2H2_opac_ip_kdistr.npz"]
    assert [os.path.basename(p) for p in want] == [os.path.basename(p) for p in got]
    for g, w in zip(got, want):
        with np.load(g) as a, np.load(w) as b:
            assert sorted(a.files) == sorted(b.files)
            for k in b.files:
                assert a[k].tobytes() == b[k].tobytes(), (os.path.basename(g), k)
            assert np.all(np.isfinite(a["kpoints"])) and a["kpoints"].max() > 1e3 * a["kpoints"].min()
    host = cia_tool.main(argv + ["-backend", "numpy", "-output_directory", os.path.join(wd, "opac_numpy")])
    for d, h in zip(files, host):
        assert open(d, "rb").read() == open(h, "rb").read(), os.path.basename(d)


def test_the_chain_with_a_cia_table_this_repository_wrote(tmp_path):
    """H2O from synthetic HELIOS-K files through ktable.py, CIA_H2H2 from a synthetic `.cia` file through `cia.py -ktable yes` on
    the same grids, Rayleigh H2 and He with -grid_like; helios.py on the fly with and without the CIA line, and premix.py on
    the directory"""
    import cia as cia_tool
    import helios
    import ktable as ktable_tool
    import ktable_cases as kc
    import premix as premix_tool
    from test_gpu_ktable import _otf_argv
    wd = str(tmp_path)
    kc.write_dir(os.path.join(wd, "hk_h2o"), kc.load("a"))
    with open(os.path.join(wd, "list.dat"), "w") as f:
        f.write("species path\nH2O %s\n" % os.path.join(wd, "hk_h2o"))
    opac = os.path.join(wd, "opac")
    grids = ["-wavelength_grid", "10 30 2000", "-temperature_grid", "200 800 200", "-pressure_grid", "3 7 5",
             "-directory_with_individual_files", opac, "-container", "npz"]
    first = ktable_tool.main(["-path_to_individual_species_file", os.path.join(wd, "list.dat")] + grids)
    path = cc.write_cia_file(os.path.join(wd, "h2h2.cia"), cc.tool_blocks(numax=200.0))
    second = cia_tool.main(["-name", "CIA_H2H2", "-cia_file", path, "-temperatures", "200 500 800", "-pressure_codes", "n300 p100",
                            "-numax", "200", "-dnu", "0.1", "-ktable", "yes"] + grids)
    assert [os.path.basename(p) for p in second] == ["CIA_H2H2_opac_kdistr.npz", "CIA_H2H2_opac_ip_kdistr.npz"]
    with np.load(first[1]) as a, np.load(second[1]) as b:
        for k in ("interface wavelengths", "center wavelengths", "ypoints", "temperatures", "pressures"):
            assert a[k].tobytes() == b[k].tobytes(), k
        assert b["kpoints"].shape == a["kpoints"].shape and b["kpoints"].max() > 1e-3
    ktable_tool.main(["-rayleigh_species", "H2,He", "-grid_like", first[1], "-directory_with_individual_files", opac, "-container",
                      "npz"])
    runs = {}
    for name, line in (("with", "CIA_H2H2 yes no 0.85&0.85\n"), ("without", "")):
        with open(os.path.join(wd, "species.dat"), "w") as f:
            f.write("species      absorbing       scattering         mixing_ratio\n\nH2O  yes no 1e-3\n" + line
                    + "H2   no  yes  0.85\nHe  no yes 0.15\n")
        runs[name] = run = helios.run_helios(
            _otf_argv(wd) + ["-opacity_mixing", "on-the-fly", "-name", "cia_" + name, "-output_directory", wd + "/",
                             "-energy_budget_correction", "no", "-internal_temperature", "100", "-number_of_layers", "15",
                             "-maximum_number_of_iterations", "20000", "-radiative_equilibrium_criterion", "1e-4",
                             "-convective_adjustment", "no", "-toa_pressure", "1e3", "-boa_pressure", "1e7"])
        print("%s: iterations %d, T %.1f ... %.1f" % (name, run.iter_value, run.T_lay.min(), run.T_lay.max()))
        assert int(run.nlayer) == 15 and int(run.ny) == 20
        assert 3 < int(run.iter_value) < 20000 and np.all(np.isfinite(run.T_lay))
        if name == "with":
            table = os.path.join(wd, "mix.npz")
            assert premix_tool.main(_otf_argv(wd) + ["-premix_output", table]) == [table]
            with np.load(table) as t:
                assert t["kpoints"].shape == (4 * 5 * int(run.nbin) * 20,) and np.all(t["kpoints"] > 0)
    assert [sp.name for sp in runs["with"].species_list] == ["H2O", "CIA_H2H2", "H2", "He"]
    assert [sp.name for sp in runs["without"].species_list] == ["H2O", "H2", "He"]
    a, b = (np.asarray(runs[k].opac_band_lay, np.float64) for k in ("with", "without"))
    assert a.shape == b.shape and np.all(np.isfinite(a)) and not np.array_equal(a, b)
