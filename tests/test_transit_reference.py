"""The restatement of the transit-depth contract (tests/transit_reference.py) held to facts it does not come from, and the
host side of the feature that needs no GPU: the option, the shell boundaries, the writer."""
import os

import numpy as np
import pytest

import transit_reference as tr

LD = np.longdouble
W3 = np.array([0.5, 1.0, 0.5])          # dyadic "Gauss weights": they sum to 2 exactly in any precision


def _integer_column(S=12, nbin=3, seed=5, R0=70000.0):
    """altitudes and optical depths made of small integers: every boundary, centre and thickness is exact in fp64"""
    rng = np.random.default_rng(seed)
    zb = np.concatenate(([-48.0], -48.0 + np.cumsum(6.0 * rng.integers(1, 5, S))))
    dtau = rng.integers(0, 9, (S, nbin, len(W3))).astype(float) / 8.0
    cloud = rng.integers(0, 3, (S, nbin)).astype(float) / 4.0
    return dtau, cloud, zb, R0


def test_empty_bins_occult_nothing_above_the_floor():
    dtau, cloud, zb, R0 = _integer_column()
    for fn in (tr.transit, tr.plain_fp64):
        r = fn(0 * dtau, 0 * cloud, zb, W3, R0, R_star=7e5)
        assert np.all(r["T_band"] == 1) and np.all(r["A"] == 0)
        assert np.all(r["R_eff"] == R0 + zb[0]) and np.all(r["T_floor"] == 1)
        assert np.abs(r["depth"] / ((R0 + zb[0]) / 7e5) ** 2 - 1).max() < 1e-15


def test_opaque_bins_occult_the_whole_annulus():
    dtau, cloud, zb, R0 = _integer_column()
    for fn in (tr.transit, tr.plain_fp64):
        r = fn(0 * dtau + 1e6, 0 * cloud, zb, W3, R0)
        assert np.all(r["T_band"] == 0)
        # sum over the shells of (zb[j+1] - zb[j]) (2 R0 + zb[j+1] + zb[j]) = (R0 + zb[S])^2 - (R0 + zb[0])^2: integers here
        assert np.all(r["A"] == (R0 + zb[-1]) ** 2 - (R0 + zb[0]) ** 2)
        assert np.all(r["R_eff"] == R0 + zb[-1])


def test_single_shell_is_the_closed_form():
    zb = np.array([-3.0e7, 5.0e7])
    R0, dt = 7.0e9, np.array([[[0.3, 2.0]], ])
    w = np.array([1.25, 0.75])
    r = tr.transit(dt, np.array([[0.1]]), zb, w, R0)
    z0 = (LD(zb[0]) + LD(zb[1])) / 2
    b0 = LD(R0) + z0
    alpha = (dt[0, 0].astype(LD) + LD(0.1)) / (LD(zb[1]) - LD(zb[0]))
    T = np.exp(-2 * alpha * np.sqrt((LD(zb[1]) - z0) * (LD(R0) + LD(zb[1]) + b0)))
    want = (LD(0.5) * LD(1.25)) * T[0] + (LD(0.5) * LD(0.75)) * T[1]
    assert abs(r["T_band"][0, 0] - want) <= 64 * np.finfo(LD).eps * want
    assert abs(r["A"][0] - (1 - want) * (LD(zb[1]) - LD(zb[0])) * (2 * LD(R0) + LD(zb[1]) + LD(zb[0]))) <= 1e-17 * r["A"][0]


def test_splitting_every_shell_in_three_leaves_the_chords_alone():
    """the same extinction on a three times finer grid: tau along the ORIGINAL impact parameters (the centres of the
    middle thirds) is unchanged.  Integer altitudes with thicknesses divisible by 6 make thirds and centres exact."""
    dtau, cloud, zb, R0 = _integer_column()
    S = len(zb) - 1
    zb3 = np.concatenate([zb[s] + (zb[s + 1] - zb[s]) * np.array([0, 1, 2]) / 3.0 for s in range(S)] + [zb[-1:]])
    assert np.all(zb3 == np.round(zb3)) and np.all(zb3[::3] == zb)
    dtau3, cloud3 = np.repeat(dtau, 3, axis=0) / 3.0, np.repeat(cloud, 3, axis=0) / 3.0
    for fn, tol in ((tr.transit, 1e-13), (tr.plain_fp64, 1e-13)):
        coarse = fn(dtau, cloud, zb, W3, R0)["tau"]
        fine = fn(dtau3, cloud3, zb3, W3, R0, chords=[3 * j + 1 for j in range(S)])["tau"]
        ok = coarse > 0
        rel = np.abs(fine[ok] / coarse[ok] - 1).max()
        print("splitting: largest relative change of tau %.2e (%s)" % (rel, fn.__name__))
        assert rel <= tol and np.all(fine[~ok] == 0)


def _e1(x):
    """exponential integral E1 in long double: the series below 1, the continued fraction (Lentz) above"""
    x = LD(x)
    if x <= 1:
        s, term = LD(0), LD(1)
        for k in range(1, 60):
            term = term * (-x) / k
            s = s - term / k
        return -LD(np.euler_gamma) - np.log(x) + s
    tiny = LD(1e-300)
    b = x + 1
    c, d = 1 / tiny, 1 / b
    h = d
    for i in range(1, 200):
        a = -LD(i) * i
        b = b + 2
        d = 1 / (a * d + b)
        c = b + a / c
        h = h * c * d
    return h * np.exp(-x)


def _hydrostatic_difference(nlayer, R0=7e9, H=7e6, a0=1e-6, scale_heights=25):
    """(R_eff - R0) of a grey isothermal hydrostatic column, alpha(z) = a0 exp(-z / H), minus H [gamma + ln tau0 + E1(tau0)],
    in units of H.  Each shell's optical depth is the exact integral of alpha over the shell."""
    zb = np.linspace(0.0, scale_heights * H, nlayer + 1)
    e = np.exp(-zb.astype(LD) / LD(H))
    dtau = (LD(a0) * LD(H) * (e[:-1] - e[1:])).astype(np.float64)
    r = tr.transit(dtau[:, None, None], np.zeros((nlayer, 1)), zb, np.array([2.0]), R0)
    tau0 = LD(a0) * np.sqrt(2 * LD(np.pi) * LD(R0) * LD(H))
    want = LD(H) * (LD(np.euler_gamma) + np.log(tau0) + _e1(tau0))
    return float(((r["R_eff"][0] - LD(R0)) - want) / LD(H))


def test_e1_values():
    # Abramowitz & Stegun table 5.1
    assert abs(float(_e1(0.5)) - 0.5597735948) < 1e-10 and abs(float(_e1(2.0)) - 0.0489005107) < 1e-10


def test_hydrostatic_limit():
    """the analytic transit radius of an exponential atmosphere (truncation error O(H / R0) = 1e-3 H and the 25 scale heights'
    own e^-25): the midpoint rule over one chord per shell converges towards it"""
    d = {n: _hydrostatic_difference(n) for n in (100, 400, 800)}
    print("hydrostatic limit, (R_eff - R0 - analytic) / H:", d)
    assert abs(d[400]) <= 0.01
    assert abs(d[800]) < abs(d[400]) < abs(d[100])


def test_bound_is_the_projects_rule():
    ref = np.array([1.0, 2.0], LD)
    b = tr.bound(ref, np.array([1.0, 2.0 + 1e-12]))
    assert b[0] == LD(1e-13) and abs(float(b[1]) - 8e-12) < 1e-15


# ---- host side of the feature ------------------------------------------------------------------------------------------
def test_option_table_entry():
    from helios_amd import quantities, read
    entry = [o for o in read._OPTIONS if o[0] == "transit depth spectrum"]
    assert entry == [("transit depth spectrum", "transit_depth_spectrum", "transit_depth_spectrum", "no")]
    for argv, want in (([], 0), (["-transit_depth_spectrum", "yes"], 1), (["-transit_depth_spectrum", "no"], 0)):
        q = quantities.Store(ctx=object())
        read.Read().read_param_file_and_command_line(q, None, ["-parameter_file", "/nonexistent"] + argv)
        assert int(q.transit_depth_spectrum) == want
    with pytest.raises(IOError):
        read.Read().read_param_file_and_command_line(quantities.Store(ctx=object()), None,
                                                     ["-parameter_file", "/nonexistent", "-transit_depth_spectrum", "maybe"])
    assert int(quantities.Store(ctx=object()).transit_depth_spectrum) == 0       # a Store no reader filled: off


def test_option_from_the_parameter_file(tmp_path):
    from helios_amd import quantities, read
    p = tmp_path / "param.dat"
    p.write_text("transit depth spectrum = yes    [yes, no]   (CL: Y)\n")
    q = quantities.Store(ctx=object())
    read.Read().read_param_file_and_command_line(q, None, ["-parameter_file", str(p)])
    assert int(q.transit_depth_spectrum) == 1


class _Column(object):
    pass


def _column(iso, z_lay, dz):
    q = _Column()
    q.nlayer, q.iso, q.z_lay, q.delta_z_lay = len(dz), iso, np.array(z_lay, float), np.array(dz, float)
    return q


def test_shell_boundaries_of_a_gas_and_a_rocky_column():
    from helios_amd.computation import Compute
    dz = np.array([2.0, 4.0, 6.0, 2.0])
    z_gas = np.array([-3.0, 0.0, 5.0, 9.0])           # z = 0 at the centre of layer 1
    for iso in (1, 0):
        zb = Compute.transit_shell_boundaries(_column(iso, z_gas, dz))
        want = [-4, -2, 2, 8, 10] if iso else [-4, -3, -2, 0, 2, 5, 8, 9, 10]
        assert zb.dtype == np.float64 and zb.tolist() == want
        assert np.array_equal(zb, tr.shell_boundaries(z_gas, dz, iso))
    zb = Compute.transit_shell_boundaries(_column(0, [1.0, 4.0, 9.0, 13.0], dz))      # rocky: the surface is z = 0
    assert zb[0] == 0 and zb[-1] == 14
    # over-allocated arrays (the Store's layer arrays may be longer than nlayer) are cut
    q = _column(1, list(z_gas) + [0.0], list(dz) + [0.0])
    q.nlayer = 4
    assert Compute.transit_shell_boundaries(q).tolist() == [-4, -2, 2, 8, 10]


@pytest.mark.parametrize("iso", [1, 0])
def test_a_column_that_does_not_ascend_is_refused(iso):
    from helios_amd.computation import Compute
    with pytest.raises(ValueError, match="layer 2"):
        Compute.transit_shell_boundaries(_column(iso, [1.0, 3.0, 5.0, 6.0], [2.0, 2.0, 0.0, 2.0]))
    with pytest.raises(ValueError, match="layer 1"):
        Compute.transit_shell_boundaries(_column(iso, [1.0, 3.0, 5.0, 6.0], [2.0, np.nan, 1.0, 2.0]))


class _Reader(object):
    pass


def _written(tmp_path, on):
    from helios_amd import quantities, write
    q = quantities.Store(ctx=object())
    q.name, q.nbin = "hand", 3
    q.opac_wave = np.array([1e-4, 2.5e-4, 1e-3])
    q.transit_depth_spectrum = np.int32(on)
    q.transit_radius = np.array([7.1e9, 7.123456789012345e9, 7.2e9])
    q.transit_depth = (q.transit_radius / 6.957e10) ** 2
    q.transit_floor_transmission = np.array([0.0, 1.25e-7, 3.5e-310])
    rd = _Reader()
    rd.output_path = str(tmp_path)
    write.Write.write_transit_depth(q, rd)
    return q, os.path.join(str(tmp_path), "hand", "hand_transit_depth.dat")


def test_writer_format(tmp_path):
    q, path = _written(tmp_path, 1)
    lines = open(path).read().split("\n")
    assert len(lines) == 3 + 3 and not lines[-1].endswith(" \n")
    assert lines[0].startswith("This file contains the transit radius [cm] and the transit depth")
    assert lines[1].startswith("Largest transmission of the deepest chord: 1.25e-07 ")
    assert lines[2].split() == ["bin", "cent_lambda[um]", "transit_radius[cm]", "transit_depth", "floor_transmission"]
    assert lines[2].index("cent_lambda") == 8 and lines[2].index("transit_radius") == 26 and lines[2].index("transit_depth") == 52
    for x, ln in enumerate(lines[3:]):
        cells = ln.split()
        assert len(cells) == 5 and int(cells[0]) == x and ln[8] != " " and ln[26] != " " and ln[52] != " " and ln[78] != " "
        assert float(cells[1]) == float("%.9g" % (q.opac_wave[x] * 1e4))
        # the three results survive the file bit for bit
        assert float(cells[2]) == q.transit_radius[x] and float(cells[3]) == q.transit_depth[x]
        assert float(cells[4]) == q.transit_floor_transmission[x]


def test_writer_is_silent_when_the_option_is_off(tmp_path):
    _q, path = _written(tmp_path, 0)
    assert not os.path.exists(path) and not os.path.exists(os.path.dirname(path))
    from helios_amd import write
    import inspect
    assert "Write.write_transit_depth" in inspect.getsource(write.Write.write_all)
