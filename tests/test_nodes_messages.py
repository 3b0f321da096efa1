"""The refusals of the frame that lines.py, cia.py and exomol.py share, each with its full text: what the tool says of its options,
of the nodes and the grid, of the mass it cannot find and of a k-table axis that is not the kernel's grid.  Nothing is computed
and no input file is opened except where a case names one.  `said` is the word a message of the grid and of the node lists
carries: cia.py and exomol.py took those refusals from lines.py with its word, and they have kept it."""
import numpy as np
import pytest

from helios_amd import cia, exomol, lines

Q_TABLE = (np.array([50.0, 3000.0]), np.array([10.0, 5000.0]))
TRANS = {"nu0": np.array([100.0])}


def _lines_ktable(temps, codes, numax, dnu, mass, backend="numpy"):
    return lines.line_ktable(None, Q_TABLE, temps, codes, numax, dnu, None, 8, mass, backend=backend)


def _cia_ktable(temps, codes, numax, dnu, mass, backend="numpy"):
    return cia.cia_ktable([], temps, codes, numax, dnu, None, 8, mass, backend=backend)


def _exomol_ktable(temps, codes, numax, dnu, mass, backend="numpy"):
    return exomol.exomol_ktable(None, TRANS, None, Q_TABLE, temps, codes, numax, dnu, None, 8, mass, backend=backend)


# per tool: the inputs stand in for files and lists that no refusal here gets to read
TOOLS = {
    "lines": dict(module=lines, mass="molar", kernel="line kernel's", name="H2O",
                  files=["-line_list", "none.par", "-partition_function", "none.txt"], ktable=_lines_ktable,
                  opacity=lambda temps, press, grid, mass, **how: lines.line_opacity(None, Q_TABLE, temps, press, grid, mass, **how),
                  slabs=lambda: lines.LineSlabs(None, Q_TABLE, [300], [1e6], 100, 0.5, 200, 18.0, 0.0, 25.0)),
    "cia": dict(module=cia, mass="partner", kernel="kernel's", name="CIA_H2H2", files=["-cia_file", "none.cia"], ktable=_cia_ktable,
                opacity=lambda temps, press, grid, mass, **how: cia.cia_opacity([], temps, press, grid, mass, **how),
                slabs=lambda: cia.CiaSlabs([], [300], [1e6], 100, 0.5, 200, 2.0)),
    "exomol": dict(module=exomol, mass="molar", kernel="line kernel's", name="H2O",
                   files=["-states", "none.states", "-trans", "none.trans", "-partition_function", "none.txt"], ktable=_exomol_ktable,
                   opacity=lambda temps, press, grid, mass, **how: exomol.exomol_opacity(None, TRANS, None, Q_TABLE, temps, press, grid,
                                                                                        mass, **how),
                   slabs=lambda: exomol.ExomolSlabs(None, TRANS, None, Q_TABLE, [300], [1e6], 100, 0.5, 200, 18.0, 25.0, 0.0)),
}
SAID = "lines"


def refused(kind, call):
    with pytest.raises(kind) as e:
        call()
    assert type(e.value) is kind
    return str(e.value)


def run_tool(tool, *more, **how):
    t = TOOLS[tool]
    argv = ["-name", how.get("name", t["name"])] + t["files"] + ["-temperatures", how.get("temps", "300"), "-pressure_codes",
                                                                 how.get("codes", "p000"), "-numax", how.get("numax", "100"), "-dnu",
                                                                 how.get("dnu", "0.5"), "-backend", "numpy"]
    return t["module"].main(argv + ([] if how.get("ktable") else ["-output_directory", "never_made"]) + list(more))


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_what_ktable_yes_refuses(tool, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    for more, text in [
        (["-numin", "50"], "-ktable yes with -numin 50: the k-table's wavelength axis starts at 0 cm^-1, and ktable.py refuses a directory "
                           "whose first chunk does not"),
        (["-chunk_width", "50"], "-ktable yes with -chunk_width 50: the table is built from the one chunk 0 ... numax; a chunk's "
                                 "points are lo + i dnu, which are other bits than 0 + i dnu"),
        (["-output_format", "text"], "-ktable yes with -output_format text: no opacity file is written, the fp32 opacities stay on the "
                                     "device"),
        (["-output_directory", "somewhere"], "-ktable yes with -output_directory somewhere: a call writes the files or the table, not "
                                             "both; the table goes to -directory_with_individual_files"),
        (["-number_of_gaussian_points", "0"], "-number_of_gaussian_points is an integer >= 1"),
        (["-nodes_per_launch", "0"], "-nodes_per_launch is an integer >= 1"),
    ]:
        assert refused(IOError, lambda: run_tool(tool, "-ktable", "yes", *more, ktable=True)) == "%s: %s" % (tool, text)
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_what_the_tool_refuses_of_nodes_grid_and_mass(tool, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    mass = TOOLS[tool]["mass"]
    for how, text in [
        (dict(temps="300.5"), SAID + ": the temperature '300.5' is not an integer in K (the file name carries it)"),
        (dict(temps="300 0"), SAID + ": the temperature '0' is not > 0 K"),
        (dict(temps=" "), SAID + ": -temperatures holds no temperature"),
        (dict(codes="p000 p900"), SAID + ": pressure code 'p900' is not in the table (n800 ... p400)"),
        (dict(codes=" "), SAID + ": -pressure_codes holds no code"),
        (dict(dnu="0"), SAID + ": -dnu 0.0 is not > 0"),
        (dict(dnu="nan"), SAID + ": -dnu nan is not > 0"),
        (dict(numax="0"), SAID + ": -numax 0 is not above -numin 0"),
        (dict(dnu="0.7"), SAID + ": dnu = 0.69999999999999996 does not divide the chunk 0 ... 100 cm^-1 into a whole number of points "
                                 "(142.85714285714286)"),
        (dict(name="XYZ"), "%s: no %s mass: 'XYZ' is not in species_data.py, give -%s_mass" % (tool, mass, mass)),
    ]:
        assert refused(IOError, lambda: run_tool(tool, **how)) == text
    assert refused(IOError, lambda: run_tool(tool, "-chunk_width", "0")) == SAID + ": -chunk_width 0 is not > 0"
    assert refused(IOError, lambda: run_tool(tool, "-%s_mass" % mass, "-1")) == "%s: no %s mass: -%s_mass -1.0 is not > 0 g/mol" % (
        tool, mass, mass)
    assert refused(IOError, lambda: run_tool(tool, "-%s_mass" % mass, "nan")) == "%s: no %s mass: -%s_mass nan is not > 0 g/mol" % (
        tool, mass, mass)
    assert list(tmp_path.iterdir()) == []


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_what_the_library_function_refuses(tool):
    opacity, mass = TOOLS[tool]["opacity"], TOOLS[tool]["mass"]
    good = ([300.0], [1e6], (0.0, 1.0, 10), 18.0)
    for args, text in [
        (([300.0, -1.0],) + good[1:], "every temperature is a finite number > 0 (got [300.0, -1.0])"),
        (([],) + good[1:], "every temperature is a finite number > 0 (got [])"),
        ((good[0], [np.inf]) + good[2:], "every pressure is a finite number > 0 dyne cm^-2 (got [inf])"),
        (good[:2] + ((0.0, 0.0, 10), 18.0), "dnu = 0.0 is not > 0"),
        (good[:2] + ((0.0, 1.0, 0), 18.0), "the grid (nu_first, dnu, points) = (0.0, 1.0, 0) needs a finite start and at least one point"),
        (good[:3] + (None,), "no %s mass (got None): give one > 0 g/mol" % mass),
        (good[:3] + (-2.0,), "no %s mass (got -2.0): give one > 0 g/mol" % mass),
    ]:
        assert refused(ValueError, lambda: opacity(*args, backend="numpy")) == "%s: %s" % (tool, text)
    assert refused(ValueError, lambda: opacity(*good, backend="cuda")) == "%s: backend is device or numpy (got 'cuda')" % tool


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_what_the_ktable_function_refuses(tool):
    ktable = TOOLS[tool]["ktable"]
    for args, kind, text in [
        (([300], ["p000", "p900"], 100, 0.5, 18.0), IOError, tool + ": pressure code 'p900' is not in the table (n800 ... p400)"),
        (([300, 300.5], ["p000"], 100, 0.5, 18.0), IOError, tool + ": the temperature 300.5 is not an integer in K"),
        (([300], ["p000"], 100, 0.7, 18.0), IOError, SAID + ": dnu = 0.69999999999999996 does not divide the chunk 0 ... 100 cm^-1 into a "
                                                            "whole number of points (142.85714285714286)"),
        (([300], ["p000"], 100, 0.0, 18.0), IOError, SAID + ": -dnu 0.0 is not > 0"),
        (([-300], ["p000"], 100, 0.5, 18.0), ValueError, tool + ": every temperature is a finite number > 0 (got [-300.0])"),
        (([300], ["p000"], 100, 0.5, None), ValueError, "%s: no %s mass (got None): give one > 0 g/mol" % (tool, TOOLS[tool]["mass"])),
        (([300], ["p000"], 300000000, 1.0, 18.0), IOError, tool + ": 300000000 spectral points, the k-table's kernel takes 1 ... "
                                                           "268435456"),
    ]:
        assert refused(kind, lambda: ktable(*args)) == text
    text = refused(ValueError, lambda: ktable([300], ["p000"], 100, 0.5, 18.0, "cuda"))
    assert text == "%s: backend is device or numpy (got 'cuda')" % tool


@pytest.mark.parametrize("tool", sorted(TOOLS))
def test_an_axis_that_is_not_the_kernels_grid(tool):
    source = TOOLS[tool]["slabs"]()
    assert source.axis() == (0, 100, 0.5) and (source.temps, source.press) == ([300], [1e6])
    for call in (lambda: next(source.host_slabs(None, 199)), lambda: source.feed(None, None, 199)):
        assert refused(IOError, call) == ("%s: the k-table's axis 0 ... 100 cm^-1 at 0.5 cm^-1 has 199 points, the %s grid at -dnu 0.5 has "
                                          "200" % (tool, TOOLS[tool]["kernel"]))
    source.close()


def test_the_partition_function_names_its_caller(tmp_path):
    """lines.py's two functions say `lines:` to a library caller of either tool; exomol.py, the tool, says its own word"""
    outside = "T = 10 K lies outside the partition function's 50 ... 3000 K"
    assert refused(ValueError, lambda: lines.partition_value(Q_TABLE, 10.0)) == "lines: " + outside
    text = refused(ValueError, lambda: TOOLS["exomol"]["opacity"]([10.0], [1e6], (0.0, 1.0, 10), 18.0, backend="numpy"))
    assert text == "lines: " + outside
    path = str(tmp_path / "q.txt")
    with open(path, "w") as f:
        f.write("# T Q\n50 10\n3000 5000\n")
    for tool, temps, text in [("lines", "10", "lines: " + outside), ("exomol", "10", "exomol: " + outside)]:
        files = TOOLS[tool]["files"][:-1] + [path]
        argv = ["-name", "H2O"] + files + ["-temperatures", temps, "-pressure_codes", "p000", "-numax", "100", "-dnu", "0.5", "-backend",
                                           "numpy", "-output_directory", str(tmp_path / "never_made")]
        assert refused(IOError, lambda: TOOLS[tool]["module"].main(argv)) == text
    with open(path, "w") as f:
        f.write("# T Q\n50 10\n")
    for tool in ("lines", "exomol"):
        files = TOOLS[tool]["files"][:-1] + [path]
        argv = ["-name", "H2O"] + files + ["-temperatures", "300", "-pressure_codes", "p000", "-numax", "100", "-dnu", "0.5", "-backend",
                                           "numpy", "-output_directory", str(tmp_path / "never_made")]
        assert refused(IOError, lambda: TOOLS[tool]["module"].main(argv)) == "lines: %s holds fewer than two rows of T and Q(T)" % path
    assert not (tmp_path / "never_made").exists()
