"""cia.py with the numpy backend: the contract against the restatements of tests/cia_reference.py under the rule of
tests/cia_cases.py, the sanity figure, the parser with every refusal, and `-ktable yes` against cia.py (files) followed by
ktable.py, container by container as raw bytes."""
import os

import numpy as np
import pytest

import cia_cases as cc
import cia_reference as cr
from helios_amd import cia, ktable
from helios_amd import phys_const as pc


def test_the_restated_constants_are_the_modules():
    assert (cr.K_B, cr.N_A) == (pc.K_B, pc.N_A)
    assert cia.TILE_POINTS == cia.THREADS * cia.POINTS_PER_THREAD
    # the kernel's sizes, which the GPU tests derive theirs from, are the ones csrc/cia.hip is built with
    import re
    text = open(os.path.join(os.path.dirname(os.path.abspath(cia.__file__)), "csrc", "cia.hip")).read()
    sizes = dict((k, int(v)) for k, v in re.findall(r"constexpr int (CIA_[A-Z]+) = (\d+);", text))
    assert (sizes["CIA_THREADS"], sizes["CIA_PPT"], sizes["CIA_WINDOW"]) == (cia.THREADS, cia.POINTS_PER_THREAD, cia.WINDOW)
    assert (cr.K_B, cr.N_A) == tuple(float(v) for v in re.search(r"CC_KB = ([0-9.e+-]+), CC_NA = ([0-9.e+-]+);", text).groups())


def test_the_sanity_figure():
    """sigma = 1e-45 at 1000 K and 1e6 dyne cm^-2 per gram of H2"""
    flat = [cia.Block(0.0, 10.0, 500.0, [0.0, 10.0], [1e-45, 1e-45])]
    got = cia.cia_opacity(flat, [1000.0], [1e6], (1.0, 1.0, 3), 2.01588, backend="numpy")
    assert got.shape == (1, 1, 3) and np.all(got == 2.163729387072754e-3)
    assert float(cr.kappa(cc.plain(cia.bands_of(flat)), 2.0, 1000.0, 1e6, 2.01588, np.float64)) == 2.163729387072754e-3


# ---- the contract ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("press", [1e6, 1e-20])
def test_the_numpy_backend_on_the_table_of_the_edges(press):
    """every grid point of the edge table at every temperature of EDGE_TEMPS: tabulated points, block ends and band ends on a grid
    point and one ulp beside it, T on a block's temperature and one ulp beside it"""
    bands = cia.bands_of(cc.edge_blocks())
    assert [len(b.blocks) for b in bands] == [3, 1]
    got = cia.cia_opacity(cc.edge_blocks(), cc.EDGE_TEMPS, [press], cc.EDGE_GRID, cc.M_H2, backend="numpy")
    nu = cc.grid_nu(cc.EDGE_GRID)
    for it, t in enumerate(cc.EDGE_TEMPS):
        ld, f64 = cc.restated(bands, cc.EDGE_GRID, t, press)
        cc.check_rule(got[it, 0], ld, f64, "numpy at %.17g K, %g" % (t, press))
    k = got[:, 0]
    # outside the bands, at the grid points one ulp outside them, and in the gap: zeros; on the bands' ends: values
    assert not k[:, :cc.A_LO + 1].any() and not k[:, cc.A_HI + 1:cc.B_LO].any() and not k[:, cc.B_HI:].any()
    assert np.all(k[:, cc.B_LO] > 0) and np.all(k[:, cc.B_HI - 1] > 0)
    # the 200 K block starts on g[120]: below 200 K nothing before it; the 400 K block starts on g[118]
    assert not k[0, :120].any() and k[0, 120] > 0 and k[-1, 117] == 0 and k[-1, 118] > 0
    # the 300 K block starts one ulp above g[130] and ends on g[2280]
    assert k[6, 130] == 0 and k[6, 131] > 0 and k[6, 2280] > 0 and k[6, 2281] == 0
    # on a tabulated point the value is the tabulated one
    b200 = bands[0].blocks[0]
    j = int(np.nonzero(b200.nu == nu[700])[0][0])
    assert k[2, 700] == b200.k[j] * (press / (pc.K_B * 200.0)) * pc.N_A / cc.M_H2
    # band b has one temperature: the same sigma at every T
    sig = k[:, cc.B_LO:cc.B_HI] * (np.asarray(cc.EDGE_TEMPS)[:, None] / 300.0)
    assert np.allclose(sig, sig[6], rtol=1e-14, atol=0)


def test_random_evaluations_on_steep_tables_with_zeros():
    """tables spanning 1e-60 ... 1e-40 with a tenth of the entries zero: the numpy backend under the rule, and plain fp64 itself
    close to the long double everywhere -- the two weights from differences lose no digit.  The contract rounds 16 times on the
    way to kappa (two differences, a quotient and a product per weight in nu and in T, two sums, five factors), every term is
    >= 0 and every difference is one of given numbers, so no rounding is amplified: 16 * 2^-53 = 1.8e-15 bounds plain fp64"""
    rng = np.random.default_rng(3)
    worst = 0.0
    for case in range(4):
        blocks = [cc.block(10.0, 900.0, t, rng.uniform(10.0, 900.0, 120), rng) for t in (150.0, 400.0, 950.0)]
        bands = cia.bands_of(blocks)
        grid = (float(rng.uniform(0.0, 20.0)), float(rng.uniform(0.3, 0.4)), 2500)
        for t in rng.uniform(100.0, 1100.0, 4):
            got = cia.cia_opacity(blocks, [t], [1e5], grid, cc.M_H2, backend="numpy")[0, 0]
            ld, f64 = cc.restated(bands, grid, float(t), 1e5)
            _, eps = cc.check_rule(got, ld, f64, "case %d at %.3f K" % (case, t))
            worst = max(worst, eps)
            assert np.count_nonzero(got) > 2000
    print("plain fp64 against long double over 40000 evaluations: %.3e" % worst)
    assert worst <= 16 * 2.0 ** -53


# ---- the parser ----------------------------------------------------------------------------------------------------------
def test_blocks_bands_and_their_order(tmp_path, capsys):
    blocks = cc.tool_blocks()
    blocks[1].k[[3, 17]] = -1e-50                  # negative values count as 0
    path = cc.write_cia_file(str(tmp_path / "h2h2.cia"), blocks)
    got, negatives = cia.read_cia_file(path)
    assert negatives == 2 and len(got) == 4 and [b.symbol for b in got] == ["H2-H2"] * 4
    for g, b in zip(got, blocks):
        assert (g.numin, g.numax, g.temp) == (b.numin, b.numax, b.temp) and np.array_equal(g.nu, b.nu)
        assert np.array_equal(g.k, np.where(b.k < 0, 0.0, b.k))
    assert got[1].k[3] == 0 and got[1].k[17] == 0
    bands = cia.group_bands(got)
    assert [(b.numin, b.numax) for b in bands] == [(20.0, 1000.0), (1200.0, 1900.0)]
    assert [b.temps().tolist() for b in bands] == [[200.0, 400.0, 1000.0], [300.0]]
    assert [len(b.nu) for b in bands[0].blocks] == [250, 197, 99]
    assert [b.numin for b in cia.select_bands(bands, [1])] == [1200.0]
    assert [b.numin for b in cia.select_bands(bands, [1, 0, 1])] == [20.0, 1200.0]
    assert cia.outside_counts(bands, [100, 300, 900, 1200]) == [2, 3]
    written = cia.main(["-name", "CIA_H2H2", "-cia_file", path, "-temperatures", "100 300", "-pressure_codes", "p000", "-numax", "2000",
                        "-dnu", "0.5", "-backend", "numpy", "-bands", "1", "-output_directory", str(tmp_path / "out")])
    out = capsys.readouterr().out
    assert "4 blocks in 2 bands, 2 negative values taken as 0" in out
    assert "band 0: 20 ... 1000 cm^-1, 3 temperatures 200 ... 1000 K, 99 ... 250 points" in out
    assert "band 1: 1200 ... 1900 cm^-1, 1 temperatures 300 ... 300 K, 141 points" in out
    assert "1 of the 2 node temperatures lie outside 300 ... 300 K of band 1" in out and "of band 0" not in out
    assert [os.path.basename(w) for w in written] == ["Out_CIA_H2H2_00000_02000_00100_p000.bin", "Out_CIA_H2H2_00000_02000_00300_p000.bin"]
    k = np.fromfile(written[1], np.float32)
    assert k.shape == (4000,) and not k[:2400].any() and np.count_nonzero(k[2400:3801]) > 1200 and not k[3801:].any()


def _file(tmp_path, text):
    path = str(tmp_path / "bad.cia")
    with open(path, "w") as f:
        f.write(text)
    return path


def test_refusals_of_the_parser(tmp_path):
    rng = np.random.default_rng(1)
    good = cc.block(20.0, 100.0, 300.0, [20.0, 50.0, 100.0], rng)
    text = cc.block_text(good)
    rows = text.split("\n")
    with pytest.raises(IOError, match=r"line 1 of .* holds 30 characters, a header needs 54"):
        cia.read_cia_file(_file(tmp_path, rows[0][:30] + "\n" + "\n".join(rows[1:])))
    with pytest.raises(IOError, match=r"line 1 of .*: numax = ' +abc' \(columns 30:40\) is not a finite number"):
        cia.read_cia_file(_file(tmp_path, text.replace("   100.000", "       abc", 1)))
    with pytest.raises(IOError, match=r"line 1 of .*: temperature = ' +inf' \(columns 47:54\) is not a finite number"):
        cia.read_cia_file(_file(tmp_path, text.replace("  300.0", "    inf", 1)))
    with pytest.raises(IOError, match=r"line 1 of .* announces 3 data lines, 2 follow"):
        cia.read_cia_file(_file(tmp_path, "\n".join(rows[:3]) + "\n"))
    with pytest.raises(IOError, match=r"line 1 of .* announces 3 data lines, 2 follow: line 4 "):
        cia.read_cia_file(_file(tmp_path, "\n".join(rows[:3]) + "\n" + text))
    with pytest.raises(IOError, match=r"line 1 of .*: a block of 1 points"):
        cia.read_cia_file(_file(tmp_path, cc.header("H2-H2", 20.0, 100.0, 1, 300.0) + "\n20 1e-45\n"))
    with pytest.raises(IOError, match=r"line 4 of .*: nu = 50 does not lie above 50: nu strictly ascends"):
        cia.read_cia_file(_file(tmp_path, text.replace("\n100 ", "\n50 ", 1)))
    with pytest.raises(IOError, match=r"line 3 \('50 nan'\) does not hold the finite numbers nu and k"):
        cia.read_cia_file(_file(tmp_path, "\n".join(rows[:2] + ["50 nan"] + rows[3:])))
    with pytest.raises(IOError, match=r"line 5 of .*: the file holds more than one symbol \('H2-H2' and 'H2-He'\)"):
        cia.read_cia_file(_file(tmp_path, text + cc.block_text(good, symbol="H2-He")))
    with pytest.raises(IOError, match=r"holds no block"):
        cia.read_cia_file(_file(tmp_path, "\n\n"))
    twice = cia.read_cia_file(_file(tmp_path, text + text))[0]
    with pytest.raises(IOError, match=r"the band 20 \.\.\. 100 cm\^-1 holds two blocks at T = 300 K \(headers in lines 1 and 5\)"):
        cia.group_bands(twice)


def test_refusals_of_the_selection_and_of_the_tool(tmp_path, monkeypatch):
    rng = np.random.default_rng(2)
    a = cc.block(20.0, 100.0, 300.0, [20.0, 100.0], rng)
    touching = cc.block(100.0, 200.0, 300.0, [100.0, 200.0], rng)
    inside = cc.block(50.0, 60.0, 300.0, [50.0, 60.0], rng)
    apart = cc.block(100.001, 200.0, 300.0, [101.0, 200.0], rng)
    with pytest.raises(IOError, match=r"band 0 \(20 \.\.\. 100 cm\^-1\) and band 1 \(100 \.\.\. 200 cm\^-1\) overlap or touch: choose .* -bands"):
        cia.bands_of([a, touching])
    with pytest.raises(IOError, match=r"band 0 \(20 \.\.\. 100 cm\^-1\) and band 1 \(50 \.\.\. 60 cm\^-1\) overlap or touch"):
        cia.bands_of([inside, a])
    assert len(cia.bands_of([apart, a])) == 2
    bands = cia.group_bands([a, touching, inside])
    assert [b.numin for b in cia.select_bands(bands, [0])] == [20.0]
    with pytest.raises(IOError, match=r"-bands 3: the file holds the bands 0 \.\.\. 2"):
        cia.select_bands(bands, [0, 3])
    with pytest.raises(ValueError, match="no partner mass"):
        cia.cia_opacity([a], [300.0], [1e6], (0.0, 1.0, 10), None, backend="numpy")
    with pytest.raises(ValueError, match="backend is device or numpy"):
        cia.cia_opacity([a], [300.0], [1e6], (0.0, 1.0, 10), 2.0, backend="cuda")

    path = cc.write_cia_file(str(tmp_path / "pair.cia"), [a, touching, inside])
    monkeypatch.setattr(cia, "numpy_sigma", lambda *a, **k: pytest.fail("a node was computed"))

    def tool(*more, **how):
        argv = ["-name", how.get("name", "CIA_H2H2"), "-cia_file", path, "-temperatures", how.get("temps", "300"), "-pressure_codes",
                how.get("codes", "p000"), "-numax", "300", "-dnu", how.get("dnu", "0.5"), "-backend", "numpy"]
        return cia.main(argv + (["-output_directory", str(tmp_path / "refused")] if how.get("files", True) else []) + list(more))
    with pytest.raises(IOError, match=r"band 0 .* and band 1 .* overlap or touch"):
        tool()
    with pytest.raises(IOError, match=r"-bands 7: the file holds the bands 0 \.\.\. 2"):
        tool("-bands", "0 7")
    with pytest.raises(IOError, match=r"-bands 'x'"):
        tool("-bands", "x")
    with pytest.raises(IOError, match=r"no partner mass: 'CIA_XeXe' is not in species_data.py, give -partner_mass"):
        tool("-bands", "0", name="CIA_XeXe")
    with pytest.raises(IOError, match=r"no partner mass: -partner_mass -1.0 is not > 0"):
        tool("-bands", "0", "-partner_mass", "-1")
    with pytest.raises(IOError, match=r"No such file|no such file"):
        cia.main(["-name", "CIA_H2H2", "-cia_file", str(tmp_path / "missing.cia"), "-temperatures", "300", "-pressure_codes", "p000",
                  "-numax", "300", "-dnu", "0.5", "-output_directory", str(tmp_path / "refused")])
    # what lines.py refuses of temperatures, pressure codes, dnu and chunks
    with pytest.raises(IOError, match="the temperature '300.5' is not an integer in K"):
        tool("-bands", "0", temps="300.5")
    with pytest.raises(IOError, match="pressure code 'p900' is not in the table"):
        tool("-bands", "0", codes="p900")
    with pytest.raises(IOError, match="does not divide the chunk"):
        tool("-bands", "0", dnu="0.7")
    with pytest.raises(IOError, match="-chunk_width 0 is not > 0"):
        tool("-bands", "0", "-chunk_width", "0")
    assert not os.path.exists(str(tmp_path / "refused"))


# ---- two steps against the fused route ---------------------------------------------------------------------------------------
GRID = ["-wavelength_grid", "20 6 40", "-number_of_gaussian_points", "8", "-container", "npz"]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    wd = str(tmp_path_factory.mktemp("cia_ktable"))
    cc.write_cia_file(os.path.join(wd, "h2h2.cia"), cc.tool_blocks())
    return wd


def _argv(wd, *more, **how):
    return ["-name", "CIA_H2H2", "-cia_file", os.path.join(wd, "h2h2.cia"), "-temperatures", how.get("temps", "900 300"),
            "-pressure_codes", "p000 n300", "-numax", "2000", "-dnu", "0.05", "-backend", "numpy"] + list(more)


@pytest.fixture(scope="module")
def two_step(inputs):
    """{interpolate: paths} of cia.py (files) followed by ktable.py, computed once"""
    out = os.path.join(inputs, "opac", "CIA_H2H2")
    written = cia.main(_argv(inputs, "-output_directory", out))
    assert len(written) == 4
    with open(os.path.join(inputs, "list.dat"), "w") as f:
        f.write("species path\nCIA_H2H2 %s\n" % out)
    paths = {}
    for interpolate in ("yes", "no"):
        paths[interpolate] = ktable.main(["-path_to_individual_species_file", os.path.join(inputs, "list.dat"), "-backend", "numpy",
                                          "-directory_with_individual_files", os.path.join(inputs, "two_step_" + interpolate),
                                          "-interpolate", interpolate] + GRID)
    return paths


def same_containers(got, want):
    assert [os.path.basename(p) for p in got] == [os.path.basename(p) for p in want]
    for g, w in zip(got, want):
        with np.load(g) as a, np.load(w) as b:
            assert sorted(a.files) == sorted(b.files)
            for k in b.files:
                assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape, (g, k)
                assert a[k].tobytes() == b[k].tobytes(), (os.path.basename(g), k)


def test_the_containers_are_the_two_step_routes_to_the_byte(inputs, two_step):
    got = cia.main(_argv(inputs, "-ktable", "yes", "-directory_with_individual_files", os.path.join(inputs, "fused_yes")) + GRID)
    assert [os.path.basename(p) for p in got] == ["CIA_H2H2_opac_kdistr.npz", "CIA_H2H2_opac_ip_kdistr.npz"]
    same_containers(got, two_step["yes"])
    with np.load(got[0]) as t:
        assert t["temperatures"].tolist() == [300.0, 900.0] and t["pressures"].tolist() == [1e3, 1e6]
        k = t["kpoints"].reshape(4, -1, 8)
        assert np.all(np.isfinite(k)) and k.max() > 1e3 * k.min()


def test_the_order_of_the_nodes_given_does_not_matter(inputs, two_step):
    out = os.path.join(inputs, "fused_sorted")
    got = cia.main(_argv(inputs, "-ktable", "yes", "-interpolate", "no", "-directory_with_individual_files", out, temps="300 900") + GRID)
    assert os.listdir(out) == ["CIA_H2H2_opac_kdistr.npz"]
    same_containers(got, two_step["no"])


def test_the_library_function_returns_build_species_data_sets(inputs, two_step):
    blocks, _ = cia.read_cia_file(os.path.join(inputs, "h2h2.cia"))
    inter = ktable.wavelength_grid("fixed_resolution", "20 6 40".split())
    timing = {}
    native, table_ip = cia.cia_ktable(blocks, [900, 300, 900], ["p000", "n300"], 2000, 0.05, inter, 8, 2.01588, backend="numpy",
                                      timing=timing)
    assert table_ip is None and timing["points"] == 4 and timing["resolution"] == 2000 / 40000
    with np.load(two_step["no"][0]) as want:
        assert sorted(native) == sorted(want.files)
        for k in want.files:
            assert np.asarray(native[k]).tobytes() == want[k].tobytes(), k


@pytest.mark.parametrize("more,reason", [
    (["-numin", "100"], r"cia: -ktable yes with -numin 100: the k-table's wavelength axis starts at 0 cm\^-1"),
    (["-chunk_width", "500"], r"cia: -ktable yes with -chunk_width 500: the table is built from the one chunk 0 \.\.\. numax"),
    (["-output_format", "text"], r"cia: -ktable yes with -output_format text: no opacity file is written"),
    (["-output_directory", "somewhere"], r"cia: -ktable yes with -output_directory somewhere: a call writes the files or the table"),
])
def test_refusals_with_ktable(inputs, more, reason, monkeypatch):
    monkeypatch.setattr(cia, "numpy_sigma", lambda *a, **k: pytest.fail("a node was computed"))
    with pytest.raises(IOError, match=reason):
        cia.main(_argv(inputs, "-ktable", "yes", "-directory_with_individual_files", os.path.join(inputs, "refused")) + GRID + more)
    assert not os.path.exists(os.path.join(inputs, "refused"))


def test_without_ktable_the_output_directory_is_required(inputs, capsys):
    with pytest.raises(SystemExit):
        cia.main(_argv(inputs))
    assert "the following arguments are required: -output_directory" in capsys.readouterr().err


def test_chunks_and_the_text_format(inputs, tmp_path):
    """-chunk_width 500 and -output_format text: four chunks per node, the columns nu and kappa, a chunk's nu from its own start"""
    written = cia.main(_argv(inputs, "-chunk_width", "500", "-output_format", "text", "-output_directory", str(tmp_path / "chunks"),
                             temps="300"))
    assert len(written) == 8 and os.path.basename(written[2]) == "Out_CIA_H2H2_00500_01000_00300_p000.dat"
    rows = np.loadtxt(written[2])
    assert rows.shape == (10000, 2) and rows[0, 0] == 500.0 and abs(rows[-1, 0] - 999.95) < 1e-9 and np.count_nonzero(rows[:, 1]) > 5000
