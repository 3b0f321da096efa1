"""Host side of the angular emission spectrum: the option, the quadrature, the output file."""
import os

import numpy as np
import pytest

import emission_reference as er


def _read(argv):
    from helios_amd import quantities, read
    q = quantities.Store(ctx=object())
    read.Read().read_param_file_and_command_line(q, None, ["-parameter_file", "/nonexistent"] + argv)
    return q


def test_option_table_entry_and_values():
    from helios_amd import quantities, read
    names = [o[0] for o in read._OPTIONS]
    assert names.index("emission angles") == names.index("transit depth spectrum") + 1
    assert [o for o in read._OPTIONS if o[0] == "emission angles"] == [("emission angles", "emission_angles", "emission_angles", "0")]
    for argv, want in (([], 0), (["-emission_angles", "0"], 0), (["-emission_angles", "1"], 1), (["-emission_angles", "16"], 16)):
        q = _read(argv)
        assert int(q.emission_angles) == want and q.emission_intensity is None
    assert int(quantities.Store(ctx=object()).emission_angles) == 0            # a Store no reader filled: off


@pytest.mark.parametrize("value", ["-1", "17", "2.5", "8.0", "many", "1e1"])
def test_refused_values_are_named(value):
    with pytest.raises(IOError, match="emission angles.*" + value.replace(".", r"\.")):
        _read(["-emission_angles=" + value])


def test_option_from_the_parameter_file(tmp_path):
    from helios_amd import quantities, read
    p = tmp_path / "param.dat"
    p.write_text("transit depth spectrum = no    [yes, no]   (CL: Y)\nemission angles = 8    [0 ... 16]   (CL: Y)\n")
    q = quantities.Store(ctx=object())
    read.Read().read_param_file_and_command_line(q, None, ["-parameter_file", str(p)])
    assert int(q.emission_angles) == 8 and int(q.transit_depth_spectrum) == 0
    p.write_text("transit depth spectrum = yes    [yes, no]   (CL: Y)\n")          # a file without the line parses as before
    q = quantities.Store(ctx=object())
    read.Read().read_param_file_and_command_line(q, None, ["-parameter_file", str(p)])
    assert int(q.emission_angles) == 0 and int(q.transit_depth_spectrum) == 1
    p.write_text("emission angles = 20\n")
    with pytest.raises(IOError, match="20"):
        read.Read().read_param_file_and_command_line(quantities.Store(ctx=object()), None, ["-parameter_file", str(p)])


def test_quadrature_is_the_restatements():
    from helios_amd.computation import Compute
    for N in (1, 2, 4, 8, 16):
        for got, want in zip(Compute.emission_quadrature(N), er.angles(N)):
            assert got.dtype == np.float64 and np.array_equal(got, want)


class _Reader(object):
    pass


def _store(tmp_path, N):
    from helios_amd import quantities
    q = quantities.Store(ctx=object())
    q.name, q.nbin, q.nlayer = "hand", 3, 2
    q.opac_wave = np.array([1e-4, 2.5e-4, 1e-3])
    q.F_up_band = np.arange(9.0) * 1.1 + 0.123456789012345678            # [x + nbin * i]: TOA is the last three
    q.emission_angles = np.int32(N)
    if N > 0:
        q.emission_mu, q.emission_weight, _ = er.angles(N)
        q.emission_intensity = np.array([[1.0 / 3.0, 2e-310, 7.123456789012345e9], [0.1, 0.2, 0.3]])[:N]
        q.emission_angular_flux = np.array([np.pi / 3.0, 0.0, 1.0e10 / 7.0])
    rd = _Reader()
    rd.output_path = str(tmp_path)
    return q, rd, os.path.join(str(tmp_path), "hand", "hand_emission_angles.dat")


def test_writer_format_digit_by_digit(tmp_path):
    from helios_amd import write
    q, rd, path = _store(tmp_path, 2)
    write.Write.write_emission_angles(q, rd)
    lines = open(path).read().split("\n")
    assert len(lines) == 4 + 3
    assert lines[0].startswith("This file contains the intensity leaving TOA along 2 emission angles [erg s^-1 cm^-3 sr^-1]")
    # the header: mu_m = (1 -+ 1 / sqrt 3) / 2, w_m = 1 / 2, seventeen digits each
    assert lines[1] == "mu: 0.21132486540518713 0.78867513459481287"
    assert lines[2] == "weight: 0.5 0.5"
    assert [float(v) for v in lines[1].split()[1:]] == q.emission_mu.tolist()
    assert lines[3].split() == ["bin", "cent_lambda[um]", "angular_flux", "two_stream_flux", "I(mu_0)", "I(mu_1)"]
    assert [lines[3].index(n) for n in ("cent_lambda", "angular_flux", "two_stream_flux", "I(mu_0)", "I(mu_1)")] == [8, 26, 52, 78, 104]
    assert lines[4] == ("{:<8}{:<18}{:<26}{:<26}{:<26}{:<26}".format("0", "1", "1.0471975511965976", "6.7234567890123458",
                                                                       "0.33333333333333331", "0.10000000000000001"))
    for x, ln in enumerate(lines[4:]):
        cells = ln.split()
        assert len(cells) == 6 and int(cells[0]) == x and float(cells[1]) == float("%.9g" % (q.opac_wave[x] * 1e4))
        # the results survive the file bit for bit
        assert float(cells[2]) == q.emission_angular_flux[x] and float(cells[3]) == q.F_up_band[x + 2 * 3]
        assert [float(c) for c in cells[4:]] == [q.emission_intensity[m][x] for m in range(2)]


def _only_the_emission_writer(monkeypatch):
    """write_all with every other writer silenced: what is left is its decision about this file"""
    from helios_amd import write
    for name in dir(write.Write):
        if (name.startswith("write_") and name not in ("write_all", "write_emission_angles")) or name == "create_output_dir_and_copy_param_file":
            monkeypatch.setattr(write.Write, name, staticmethod(lambda *a, **k: None))
    return write.Write()


def test_write_all_writes_the_file_only_with_the_option_on(tmp_path, monkeypatch):
    w = _only_the_emission_writer(monkeypatch)
    q, rd, path = _store(tmp_path / "off", 0)
    w.write_all(q, rd)
    assert not os.path.exists(path) and not os.path.exists(os.path.dirname(path))
    q, rd, path = _store(tmp_path / "on", 1)
    w.write_all(q, rd)
    assert os.path.exists(path) and os.listdir(os.path.dirname(path)) == ["hand_emission_angles.dat"]


def test_the_kernel_is_declared_next_to_the_transit_depth():
    from helios_amd import _lib
    protos = _lib.prototypes()
    assert "hx_emission_angles" in protos and len(protos["hx_emission_angles"][1]) == 24
    names = list(protos)
    assert names.index("hx_emission_angles") == names.index("hx_transit_depth") + 1
    assert protos["hx_emission_angles"][2][-2:] == ["I_band", "I_wg"]
