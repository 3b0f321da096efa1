"""Several nodes per launch (k_lines_prepare_nodes, k_lines_sum_nodes) and the k-table built from their slabs on the device
(hx_kt_run_device, lines.line_ktable, `lines.py -ktable yes`).  Every comparison is bit for bit: a row of "slabs32" against the
"slabs32" of that node run alone through a handle for one node, a table against lines.py (files) followed by ktable.build_species."""
import os

import numpy as np
import pytest

import lines_cases as lc
from helios_amd import ktable, lines
from helios_amd._lib import HeliosHipError

pytestmark = pytest.mark.gpu

TILE, BLOCK = lines.TILE_POINTS, lines.LDS_BLOCK
ATM = lines.ATM
DNU, CUTOFF = 0.25, 2.0                       # a tile is TILE / 4 cm^-1 wide, a line reaches 17 points
NU0 = 1000.0
X_SELF = 0.1


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def q_of(temps):
    q = lc.q_table()
    return [lines.partition_value(q, t) for t in temps], lines.partition_value(q, 296.0)


def alone(ctx, line, nodes, cutoff, grid):
    """slabs32 [node][n_points], each node through a one-node handle by itself: a plain handle, and a set_nodes of the one node"""
    h = lines.LineOpacity(ctx, len(line["nu0"]), grid[2], 1, 1)
    try:
        h.set_lines(line)
        rows = []
        for node in nodes:
            set_nodes(h, [node], cutoff, grid)
            h.run_nodes(0, 1)
            rows.append(h.get("slabs32")[0])
        return np.stack(rows)
    finally:
        h.close()


def set_nodes(h, nodes, cutoff, grid):
    q_t, q_ref = q_of([n[0] for n in nodes])
    h.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], q_t, q_ref, lc.M_H2O, X_SELF, cutoff, *grid)


def same_bits(got, want, label):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, label
    bad = np.nonzero(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad[0]) == 0, (label, len(bad[0]), [tuple(int(v) for v in b) for b in zip(*bad)][:5])


def batched(ctx, line, nodes, cutoff, grid, per_launch=None, points_max=None):
    """slabs32 of one run_nodes call over all the nodes"""
    h = lines.LineOpacity(ctx, len(line["nu0"]), points_max or grid[2], per_launch or len(nodes), len(nodes))
    try:
        h.set_lines(line)
        set_nodes(h, nodes, cutoff, grid)
        h.run_nodes(0, len(nodes))
        return h.get("slabs32"), h.get("timing_ms")
    finally:
        h.close()


def spread_lines(n, n_points, seed):
    """n lines within the first tile's stretch of the grid (or within the whole grid if that is shorter)"""
    width = min(n_points, TILE) * DNU
    return lc.synthetic_lines(n, NU0 + 0.02 * width, NU0 + 0.98 * width, seed=seed)


TWO_NODES = [(300.0, 1e3), (900.0, 1e6)]


# ---- rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_points", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_row_ends(ctx, n_points):
    """two rows with the stride n_points in a buffer of longer rows: a wrong row offset, or a last partial tile that writes into
    the next row, changes a row"""
    line = lc.join(spread_lines(BLOCK + 1, n_points, seed=n_points), lc.synthetic_lines(40, NU0, NU0 + n_points * DNU, seed=5))
    grid = (NU0, DNU, n_points)
    got, timing = batched(ctx, line, TWO_NODES, CUTOFF, grid, points_max=n_points + 3)
    want = alone(ctx, line, TWO_NODES, CUTOFF, grid)
    same_bits(got, want, "%d points" % n_points)
    assert np.count_nonzero(got[0]) >= min(n_points, 400) and not np.array_equal(got[0], got[1])
    assert timing[0] > 0 and timing[1] > 0


@pytest.mark.parametrize("n_lines", [0, 1, BLOCK - 1, BLOCK, BLOCK + 1])
def test_line_counts_around_the_lds_block(ctx, n_lines):
    """n_lines in reach of the first tile, and a hundred lines beyond the last point + cut-off, which no tile takes"""
    n_points = TILE + 1
    beyond = lc.synthetic_lines(100, NU0 + n_points * DNU + CUTOFF + 1.0, NU0 + n_points * DNU + 500.0, seed=8)
    line = lc.join(spread_lines(n_lines, n_points, seed=20 + n_lines), beyond) if n_lines else beyond
    grid = (NU0, DNU, n_points)
    got, _ = batched(ctx, line, TWO_NODES, CUTOFF, grid)
    same_bits(got, alone(ctx, line, TWO_NODES, CUTOFF, grid), "%d lines in reach" % n_lines)
    if n_lines == 0:
        assert not got.any()
    else:
        assert all(16 <= np.count_nonzero(row) <= 17 * n_lines for row in got)


def test_batch_sizes_and_refusals(ctx):
    """3 nodes per launch, 7 nodes: (0, 3), (3, 3), (6, 1); a fourth node in a call and node 7 are refused with the counts, and
    the handle runs on"""
    line = lc.synthetic_lines(BLOCK + 40, NU0 - 2.0, NU0 + (TILE + 1) * DNU + 2.0, seed=31)
    grid = (NU0, DNU, TILE + 1)
    nodes = [(300.0 + 150.0 * k, 10.0 ** (2 + k % 4)) for k in range(7)]
    want = alone(ctx, line, nodes, CUTOFF, grid)
    h = lines.LineOpacity(ctx, len(line["nu0"]), grid[2], 3, 7)
    try:
        h.set_lines(line)
        with pytest.raises(HeliosHipError, match="no nodes"):
            h.run_nodes(0, 1)
        with pytest.raises(HeliosHipError, match=r"8 nodes, the handle holds 1 \.\.\. 7"):
            set_nodes(h, nodes + nodes[:1], CUTOFF, grid)
        with pytest.raises(HeliosHipError, match=r"node 2: T = -5 is not a finite number > 0"):
            h.set_nodes([300.0, 450.0, -5.0], [1e2, 1e3, 1e4], [1.0, 1.0, 1.0], 1.0, lc.M_H2O, X_SELF, CUTOFF, *grid)
        set_nodes(h, nodes, CUTOFF, grid)
        with pytest.raises(HeliosHipError, match="no nodes have been run"):
            h.get("slabs32")
        for first, n in ((0, 3), (3, 3), (6, 1)):
            h.run_nodes(first, n)
            same_bits(h.get("slabs32"), want[first:first + n], "nodes %d ... %d" % (first, first + n - 1))
        with pytest.raises(HeliosHipError, match=r"4 nodes in one call, the handle holds 1 \.\.\. 3 per launch"):
            h.run_nodes(0, 4)
        with pytest.raises(HeliosHipError, match=r"nodes 7 \.\.\. 7, hx_lines_set_nodes gave 0 \.\.\. 6"):
            h.run_nodes(7, 1)
        with pytest.raises(HeliosHipError, match=r"nodes 5 \.\.\. 7, hx_lines_set_nodes gave 0 \.\.\. 6"):
            h.run_nodes(5, 3)
        same_bits(h.get("slabs32"), want[6:7], "the slabs after the refusals")
        h.run_nodes(2, 3)
        same_bits(h.get("slabs32"), want[2:5], "a run after the refusals")
        assert np.all(h.get("timing_ms") > 0)
    finally:
        h.close()


def test_unlike_nodes_in_one_launch(ctx):
    """300 K at 1e-4 dyne cm^-2 (every y at the clamp), 300 K at 1e3 atm (every pair beyond |z| = 100: the loop that knows the
    region) and 1200 K at 1e5, each with the tile ranges of its own pressure: a line cutoff + 5 cm^-1 beyond the last point with
    delta_air = -0.01 is in reach at 1e3 atm alone, where it is the only line that reaches the last points"""
    cutoff = 25.0
    grid = (NU0, DNU, TILE + 1)
    last = NU0 + TILE * DNU
    far = lc.one_line(last + cutoff + 5.0, s_ref=1e-19, delta_air=-0.01)
    line = lc.join(lc.synthetic_lines(BLOCK + 30, NU0, last - 60.0, seed=12), far)
    assert np.abs(line["delta_air"]).max() == 0.01 and np.count_nonzero(line["delta_air"]) == len(line["nu0"])
    nodes = [(300.0, 1e-4), (300.0, 1e3 * ATM), (1200.0, 1e5)]
    got, _ = batched(ctx, line, nodes, cutoff, grid)
    same_bits(got, alone(ctx, line, nodes, cutoff, grid), "unlike nodes")
    q_t, q_ref = q_of([n[0] for n in nodes])
    prm = [lines.line_params(line, t, p, q, q_ref, lc.M_H2O, X_SELF) for (t, p), q in zip(nodes, q_t)]
    assert np.all(prm[0][3] == lines.Y_MIN) and prm[1][3].min() > lines.FAR_Z
    assert np.all(got[1][-20:] > 0) and not got[0][-20:].any() and not got[2][-20:].any()
    assert np.all(got[:, :TILE - 300] > 0)


def test_no_dependence_on_what_ran_before(ctx):
    line = lc.synthetic_lines(BLOCK + 40, NU0 - 2.0, NU0 + (2 * TILE) * DNU, seed=33)
    grid_a, grid_b = (NU0, DNU, 2 * TILE - 5), (NU0 + 100.0, 0.05, TILE + 9)
    nodes_a, nodes_b = [(400.0, 1e4), (1500.0, 1e7), (700.0, 1e4)], [(2000.0, 1e2), (350.0, 1e8)]
    h = lines.LineOpacity(ctx, len(line["nu0"]), 2 * TILE, 3, 3)
    try:
        h.set_lines(line)
        set_nodes(h, nodes_a, CUTOFF, grid_a)
        h.run_nodes(0, 3)
        first = h.get("slabs32")
        h.run_nodes(0, 3)
        same_bits(h.get("slabs32"), first, "the same call twice")
        same_bits(first, alone(ctx, line, nodes_a, CUTOFF, grid_a), "grid a")
        set_nodes(h, nodes_b, 5.0, grid_b)
        h.run_nodes(0, 2)
        same_bits(h.get("slabs32"), alone(ctx, line, nodes_b, 5.0, grid_b), "grid b on the same handle")
        set_nodes(h, [(400.0, 1e4)], 5.0, grid_b)                             # one other node between the two runs
        h.run_nodes(0, 1)
        assert h.get("slabs32").shape == (1, grid_b[2]) and h.get("timing_ms")[1] > 0
        set_nodes(h, nodes_b, 5.0, grid_b)
        h.run_nodes(1, 1)
        same_bits(h.get("slabs32"), alone(ctx, line, nodes_b[1:], 5.0, grid_b), "after a run of one other node")
    finally:
        h.close()


def test_the_k_table_refuses_a_null_pointer_and_sorts_device_slabs_as_uploaded_ones(ctx):
    line = lc.synthetic_lines(200, 150.0, 1950.0, seed=3)
    n_points = 8000
    grid = (0.0, DNU, n_points)
    inter = ktable.wavelength_grid("fixed_resolution", "20 6 40".split())
    lam = ktable.spectral_axis(0, 2000, 2000 / n_points)
    start, end = ktable.bin_ranges(lam, inter)
    yg = ktable.grid_datasets(inter, 8)[2]
    h = lines.LineOpacity(ctx, len(line["nu0"]), n_points, 2, 2)
    tables = []
    try:
        h.set_lines(line)
        set_nodes(h, TWO_NODES, 25.0, grid)
        h.run_nodes(0, 2)
        slabs = h.get("slabs32")
        for device in (True, False):
            b = ktable.KTableBuilder(ctx, n_points, len(start), 8, 2, 2)
            try:
                b.set_grid(lam, start, end, inter, yg)
                if device:
                    with pytest.raises(HeliosHipError, match="the device slabs are a null pointer"):
                        b.run_device(None, 2, 0)
                    with pytest.raises(HeliosHipError, match="1 ... max_tp_per_launch slabs per call"):
                        b.run_device(h.slab_pointer(), 3, 0)
                    b.run_device(h.slab_pointer(), 2, 0)
                else:
                    b.run(slabs, 0)
                tables.append(b.get("kpoints"))
                assert b.get("timing_ms")[0] > 0 and b.get("timing_ms")[3] == 2
            finally:
                b.close()
    finally:
        h.close()
    assert tables[0].tobytes() == tables[1].tobytes() and np.all(tables[0] > 0)


# ---- the table ------------------------------------------------------------------------------------------------------------
TABLE_NODES = {"2x2": ("900 300", "p000 n300"), "2x3": ("900 300", "p000 n300 n100")}
TARGET = ktable.target_grid("200 1000 400", "2 6 3")            # 200, 600, 1000 K; 1e2, 1e4, 1e6 dyne cm^-2


@pytest.fixture(scope="module")
def species(tmp_path_factory):
    """the list, the partition function and, per set of nodes, the directory lines.py writes on the device: made once"""
    wd = str(tmp_path_factory.mktemp("gpu_lines_ktable"))
    lc.write_par_file(os.path.join(wd, "h2o.par"), lc.synthetic_lines(300, 150.0, 1950.0, seed=21))
    lc.write_q_file(os.path.join(wd, "q.txt"))
    dirs = {}
    for key, (temps, codes) in TABLE_NODES.items():
        dirs[key] = os.path.join(wd, "opac_" + key, "H2O")
        written = lines.main(tool_argv(wd, temps, codes) + ["-output_directory", dirs[key]])
        assert len(written) == len(temps.split()) * len(codes.split())
    return wd, dirs


def tool_argv(wd, temps="900 300", codes="p000 n300"):
    return ["-name", "H2O", "-line_list", os.path.join(wd, "h2o.par"), "-partition_function", os.path.join(wd, "q.txt"),
            "-temperatures", temps, "-pressure_codes", codes, "-numax", "2000", "-dnu", "0.05"]


@pytest.mark.parametrize("nodes,per_launch,lds_points,grid,n_gauss,target", [
    ("2x2", 4, ktable.LDS_POINTS, "20 6 40", 8, None),
    ("2x3", 1, ktable.LDS_POINTS, "20 6 40", 8, None),
    ("2x3", 4, ktable.LDS_POINTS, "20 6 40", 20, None),          # a full batch and a tail of 2
    ("2x3", 6, ktable.LDS_POINTS, "20 6 40", 8, TARGET),         # one call for all
    ("2x3", 4, 64, "20 6 400", 8, TARGET),                       # bins of 1667 ... 25 points: through the scratch and in LDS
])
def test_the_table_equals_the_file_routes(ctx, species, nodes, per_launch, lds_points, grid, n_gauss, target):
    wd, dirs = species
    temps, codes = TABLE_NODES[nodes]
    inter = ktable.wavelength_grid("fixed_resolution", grid.split())
    want = ktable.build_species(dirs[nodes], inter, n_gauss, backend="hip", ctx=ctx, lds_points=lds_points, target=target)
    line, _ = lines.read_line_list(os.path.join(wd, "h2o.par"))
    timing = {}
    got = lines.line_ktable(line, lines.read_partition_function(os.path.join(wd, "q.txt")), [int(t) for t in temps.split()],
                            codes.split(), 2000, 0.05, inter, n_gauss, lc.M_H2O, 0.0, lines.DEFAULT_CUTOFF, target, "device", ctx,
                            per_launch, lds_points, timing)
    if lds_points == 64:
        start, end = ktable.bin_ranges(ktable.spectral_axis(0, 2000, 2000 / 40000), inter)
        assert (end - start).min() <= 64 < (end - start).max()
    for g, w, name in zip(got, want, ("kpoints", "kpoints_ip")):
        assert (g is None) == (w is None) == (target is None and name == "kpoints_ip")
        if w is not None:
            assert sorted(g) == sorted(w)
            for k in w:
                assert np.asarray(g[k]).tobytes() == np.asarray(w[k]).tobytes(), (name, k)
            assert np.all(np.isfinite(g["kpoints"])) and g["kpoints"].max() > 1e3 * g["kpoints"].min()
    n_nodes = len(temps.split()) * len(codes.split())
    assert timing["prepare_ms"] > 0 and timing["sum_ms"] > 0 and timing["device_ms"][0] > 0 and timing["pairs"] > 0
    assert timing["device_ms"][1] == -(-n_nodes // per_launch) and timing["device_ms"][3] == n_nodes == timing["points"]


def test_the_tool_end_to_end(species, tmp_path):
    """`lines.py -ktable yes` on the device writes the two containers; the product's reader opens the second as a species table"""
    import lines as lines_tool
    from helios_amd.read import Read
    wd, dirs = species
    out = os.path.join(str(tmp_path), "tables")
    written = lines_tool.main(tool_argv(wd) + ["-ktable", "yes", "-wavelength_grid", "20 6 40", "-number_of_gaussian_points", "8",
                                               "-container", "npz", "-temperature_grid", "200 1000 400", "-pressure_grid", "2 6 3",
                                               "-directory_with_individual_files", out, "-nodes_per_launch", "3"])
    assert [os.path.basename(w) for w in written] == ["H2O_opac_kdistr.npz", "H2O_opac_ip_kdistr.npz"]
    inter = ktable.wavelength_grid("fixed_resolution", "20 6 40".split())
    want = ktable.build_species(dirs["2x2"], inter, 8, backend="hip", target=TARGET)
    for path, w in zip(written, want):
        with np.load(path) as g:
            assert sorted(g.files) == sorted(w)
            for k in w:
                assert g[k].tobytes() == np.asarray(w[k]).tobytes(), (path, k)

    class Q(object):
        pass
    q = Q()
    k = np.asarray(Read().read_opac_file(q, written[1], type="species", read_grid_parameters=True), np.float64)
    assert int(q.ntemp) == 3 and int(q.npress) == 3 and int(q.nbin) == len(inter) - 1 and int(q.ny) == 8
    assert k.tobytes() == np.asarray(want[1]["kpoints"], np.float64).tobytes()
