"""star.py on the device (csrc/star.hip): k_star_blend bit for bit against the numpy backend, k_star_rebin_* and
k_star_planck_bins against the long-double restatement (tests/star_reference.py) under the project's rule -- within
max(1e-13, 8 eps) relative per entry, eps being the numpy backend's own deviation from the restatement there -- and the tool
end to end: the file it writes drives helios.py and a two-column sweep over its data sets."""
import os

import numpy as np
import pytest

import star_cases as sc
import star_reference as sr
import table_files as tf
from helios_amd import star

pytestmark = pytest.mark.gpu

CHUNK = 64            # the smallest staging chunk the library takes: the edge cases stay small


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    c = Context(0)
    yield c
    c.close()


def _device_blend(ctx, cases, n_points=None):
    """the stars of `cases` (names of the golden blend cases) in ONE launch, every distinct corner uploaded once"""
    plans = []
    for name in cases:
        t, g, m = sc.blend_cases()[name]
        plans.append(star.blend_plan(int(t) if float(t).is_integer() else t, g, m))
    d = star.PhoenixDirectory(sc.PHOENIX)
    names = sorted(set(n for terms, _ in plans for n, _ in terms))
    n = len(sc.phoenix_lambda()) if n_points is None else n_points
    corners = {k: np.resize(d.flux(k), n) for k in names}
    b = star.StarBuilder(ctx, n, len(names), len(plans), 1)
    try:
        for slot, k in enumerate(names):
            b.add_corner(slot, corners[k])
        for j, (terms, div) in enumerate(plans):
            b.set_star(j, [names.index(k) for k, _ in terms], [w for _, w in terms], div)
        b.run(b.BLEND)
        out = b.get("flux")
    finally:
        b.close()
    return out, [star.numpy_blend(corners, *p) for p in plans], len(names)


def test_blend_every_branch_in_one_launch_is_the_numpy_backend_to_the_bit(ctx):
    """all eight branches, T_eff on and around the 7000 K change of spacing, [M/H] = -2 and 1: twelve stars, one launch"""
    cases = sorted(sc.blend_cases())
    out, ref, _ = _device_blend(ctx, cases)
    for j, name in enumerate(cases):
        assert np.array_equal(out[j], ref[j]), name
        assert np.array_equal(out[j], sc.golden()["blend_" + name]), name       # and the reference's own bits
        sc.hold(out[j], sc.restated_blend(name), ref[j], "device blend " + name)


@pytest.mark.parametrize("stars", [["full"], ["full", "m_node"], ["full", "m_node", "t_node"]])
def test_blend_of_stars_that_share_corners(ctx, stars):
    out, ref, n_corners = _device_blend(ctx, stars)
    assert n_corners == 8                                   # the corners of `full` hold the other two stars' too
    for j in range(len(stars)):
        assert np.array_equal(out[j], ref[j]), stars[j]


@pytest.mark.parametrize("n", [3, 4, 5, 1023, 1024, 1025])
def test_blend_at_the_edges_of_a_threads_and_a_workgroups_share(ctx, n):
    """a thread owns 4 points, a workgroup 1024"""
    out, ref, _ = _device_blend(ctx, ["full", "tg_nodes"], n_points=n)
    assert out.shape == (2, n) and np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])


def _device_rebin(ctx, lam, fluxes, inter, temps, chunk=CHUNK):
    pbot, state = star.interface_plan(lam, inter)
    b = star.StarBuilder(ctx, len(lam), 0, len(fluxes), len(inter) - 1, chunk)
    try:
        b.set_grid(lam, inter, pbot, state)
        for s, f in enumerate(fluxes):
            b.put_flux(s, f)
        b.run(b.PLANCK | b.REBIN, temps)
        return b.get("converted"), b.get("planck")
    finally:
        b.close()


def _hold_rebin(ctx, lam, flux, inter, temp, what):
    assert len(lam) <= 3 * CHUNK + 1 + 4 and len(inter) - 1 <= 64
    out, planck = _device_rebin(ctx, lam, [flux], inter, [temp])
    pbot, state = star.interface_plan(lam, inter)
    lo, hi = inter[:-1], inter[1:]
    mine = star.numpy_rebin(lam, flux, inter, pbot, state, star.numpy_planck_bins(temp, lo, hi))
    restated = sr.reference_rebin(lam, flux, inter, sr.reference_planck(temp, lo, hi))
    ext = mine == star.numpy_planck_bins(temp, lo, hi)
    assert np.array_equal(out[0][ext], planck[0][ext])                  # extrapolated bins ARE the Planck values
    assert np.array_equal(out[0] == planck[0], ext) or temp == 0
    sc.hold(out[0], restated, mine, what)
    return out[0], mine


@pytest.mark.parametrize("counts", [[0, 1, CHUNK - 1, 2, CHUNK + 1, 0], [CHUNK, 1, 0, 17, 16], [3, 2 * CHUNK + 1, 5]])
def test_rebinning_bins_around_the_staging_chunk(ctx, counts):
    """bins without a point, with one, with chunk - 1, chunk, chunk + 1 and 2 chunk + 1 points, and 16 and 17 (the plain
    running sum ends at 16 points)"""
    lam, flux, inter = sc.counted_spectrum(counts, seed=len(counts))
    out, mine = _hold_rebin(ctx, lam, flux, inter, 0, "bins of %s points" % counts)
    assert np.all(out > 0)


@pytest.mark.parametrize("temp", [0, 4000.0])
def test_rebinning_every_case_at_its_edge(ctx, temp):
    """the golden edge case: interfaces on the first, an interior and the last tabulated wavelength, straddling each end,
    wholly outside, a tabulated 0 on an interface"""
    g = sc.golden()
    out, mine = _hold_rebin(ctx, g["edge_lambda"], g["edge_flux"], g["edge_inter"], temp, "edge case at %g K" % temp)
    ref = g["edge_none" if temp == 0 else "edge_bb"]
    assert np.array_equal(out == 0, ref == 0)


def test_rebinning_a_grid_given_by_wavelengths_alone_and_two_stars(ctx):
    lam = sc.phoenix_lambda()[:3 * CHUNK + 1]
    g = sc.golden()
    fluxes = [g["blend_full"][:len(lam)], g["blend_t7100"][:len(lam)]]
    centres = np.linspace(lam[0] * 0.9, lam[-1] * 1.1, 40)
    inter = star.midpoint_interfaces(centres)
    out, planck = _device_rebin(ctx, lam, fluxes, inter, [3026.0, 7100.0])
    pbot, state = star.interface_plan(lam, inter)
    for s, temp in enumerate((3026.0, 7100.0)):
        ext = star.numpy_planck_bins(temp, inter[:-1], inter[1:])
        mine = star.numpy_rebin(lam, fluxes[s], inter, pbot, state, ext)
        restated = sr.reference_rebin(lam, fluxes[s], inter, sr.reference_planck(temp, inter[:-1], inter[1:]))
        sc.hold(out[s], restated, mine, "star %d on mid-point interfaces" % s)


def test_planck_values_at_both_ends_of_the_grid(ctx):
    """the bins at both ends of a 0.3 - 200 micron grid of R = 50, at 2300 K and 12000 K.  At 200 micron the closed forms of a
    term at the bin's two limits agree to ten digits: kernel and numpy backend take such terms from the lower incomplete gamma
    function, and both stay at rounding level there"""
    inter = [0.3e-4]
    while inter[-1] < 200e-4:
        inter.append(inter[-1] * 51.0 / 50.0)
    inter = np.asarray(inter[:65])
    inter[-2:] = [200e-4 * 50.0 / 51.0, 200e-4]             # 64 bins: the first ones of the grid, and its last
    inter[-3] = inter[-2] * 50.0 / 51.0
    lam = np.array([1.0, 2.0]) * 1e-6                       # a table the grid lies beyond: every bin is extrapolated
    out, planck = _device_rebin(ctx, lam, [np.ones(2), np.ones(2)], inter, [2300.0, 12000.0])
    for s, temp in enumerate((2300.0, 12000.0)):
        assert np.array_equal(out[s], planck[s])
        mine = star.numpy_planck_bins(temp, inter[:-1], inter[1:])
        restated = sr.reference_planck(temp, inter[:-1], inter[1:])
        for k in (0, 1, -2, -1):
            print("%g K bin %d: device %.3e, numpy backend %.3e" % (temp, k, sr.rel_dev(planck[s][k:][:1], restated[k:][:1])[0],
                                                                   sr.rel_dev(mine[k:][:1], restated[k:][:1])[0]))
        sc.hold(planck[s][[0, 1, -2, -1]], restated[[0, 1, -2, -1]], mine[[0, 1, -2, -1]], "Planck values at %g K" % temp)


def test_the_library_refuses_indices_outside_the_table(ctx):
    from helios_amd._lib import HeliosHipError
    lam, flux, inter = sc.counted_spectrum([2, 3])
    pbot, state = star.interface_plan(lam, inter)
    b = star.StarBuilder(ctx, len(lam), 0, 1, len(inter) - 1, CHUNK)
    try:
        bad = pbot.copy()
        bad[1] = len(lam) - 1
        with pytest.raises(HeliosHipError, match="outside the table"):
            b.set_grid(lam, inter, bad, state)
        with pytest.raises(HeliosHipError, match="do not ascend"):
            b.set_grid(lam[::-1], inter, pbot, state)
        with pytest.raises(HeliosHipError, match="set the grid first"):
            b.put_flux(0, flux)
            b.run(b.REBIN)
    finally:
        b.close()
    with pytest.raises(HeliosHipError, match="power of two"):
        star.StarBuilder(ctx, 10, 0, 1, 2, 100)


def test_device_tool_end_to_end_into_helios_and_a_sweep(tmp_path):
    """star.py -backend device on the committed PHOENIX-like fixture, two stars in one call onto a 300-bin grid; helios.py runs
    to convergence with each data set, and a two-column sweep over the data sets ends where the two single runs end"""
    import helios
    import sweep
    wd = str(tmp_path)
    table = tf.write_table(os.path.join(wd, "opac.npz"), 300, *tf.CHEMISTRIES[0])
    lst = os.path.join(wd, "stars.dat")
    with open(lst, "w") as f:
        f.write("name=a data_format=phoenix temp=3026 log_g=4.944 m=0.39\nname=b data_format=phoenix temp=7100 log_g=4.2 m=-0.3\n")
    args = ["-star_list", lst, "-phoenix_directory", sc.PHOENIX, "-opac_file_for_lambdagrid", table, "-convert_to", "g"]
    out = star.main(args + ["-backend", "device", "-output_file", os.path.join(wd, "star.npz")])
    chk = star.main(args + ["-backend", "numpy", "-output_file", os.path.join(wd, "check.npz")])
    d, c = dict(np.load(out)), dict(np.load(chk))
    assert sorted(d) == sorted(c)
    for k in ("original/phoenix/a", "original/phoenix/b", "g/lambda"):
        assert np.array_equal(d[k], c[k]), k
    inter = star.read_lambda_grid(table)[1]
    for k in ("g/phoenix/a", "g/phoenix/b"):
        # bins the spectrum covers: two fp64 sums of the same trapezoids.  The extrapolated ones are held to the rule in
        # test_planck_values_at_both_ends_of_the_grid; here they only have to be the black body's, to its series' own noise
        covered = (inter[:-1] >= sc.phoenix_lambda()[0]) & (inter[1:] <= sc.phoenix_lambda()[-1])
        assert covered.sum() > 100
        np.testing.assert_allclose(d[k][covered], c[k][covered], rtol=1e-13, err_msg=k)
        np.testing.assert_allclose(d[k][~covered], c[k][~covered], rtol=1e-5, err_msg=k)
    base = ["-parameter_file", "/nonexistent", "-opacity_mixing", "premixed", "-path_to_opacity_file", table,
            "-number_of_layers", "50", "-maximum_number_of_iterations", "20000", "-radiative_equilibrium_criterion", "1e-4",
            "-convective_adjustment", "no", "-stellar_spectral_model", "file", "-path_to_stellar_spectrum_file", out,
            "-temperature_star", "3026", "-orbital_distance", "0.02"]
    sets = ["/g/phoenix/a", "/g/phoenix/b"]
    cols, spectra = sweep.main(["-sweep", "dataset_in_stellar_spectrum_file=" + ",".join(sets)] + base
                               + ["-name", "sw", "-output_directory", wd + "/batch/"])
    assert len(cols) == 2
    for k, ds in enumerate(sets):
        single = helios.run_helios(base + ["-dataset_in_stellar_spectrum_file", ds, "-name", "one_%d" % k,
                                           "-output_directory", wd + "/single/"])
        assert single.rt is not None and int(single.real_star) == 1
        assert int(single.iter_value) < 20000 and int(cols[k].iter_value) == int(single.iter_value), k
        np.testing.assert_allclose(cols[k].T_lay, single.T_lay, rtol=1e-12, err_msg="column %d" % k)
    assert np.abs(np.asarray(cols[0].T_lay) / np.asarray(cols[1].T_lay) - 1).max() > 1e-4      # two stars, two answers
