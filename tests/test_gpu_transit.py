"""hx_transit_depth on the GPU held to the contract's restatement (tests/transit_reference.py), and the feature end to end.

The rule: A and T_floor relative, T_band absolute, each within max(1e-13, 8 eps), eps being the deviation of the plain fp64
evaluation of the contract from its long-double evaluation at that entry."""
import ctypes
import os

import numpy as np
import pytest

import transit_reference as tr

pytestmark = pytest.mark.gpu

LD = np.longdouble


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def _size(spec):
    from helios_amd import _lib
    return int(eval(spec, {"B": int(_lib.lib().hx_transit_chord_block())}))


def _inputs(S, nbin, ny, clouds, gas, seed):
    """seeded column: extinction falling by 1e7 from the lowest to the highest shell (times a factor 0.5 ... 2 per entry), scaled
    so that the optical depths of the chords span more than 1e3 ... 1e-3; bin 0 empty, bin 1 opaque.  `gas`: z = 0 inside the column (negative zb[0]); else zb[0] = 0."""
    rng = np.random.default_rng(seed)
    R0 = 7.0e9 if gas else 6.4e8
    dz = rng.uniform(0.5, 1.5, S) * (4.0e8 / S)
    zb = np.concatenate(([0.0], np.cumsum(dz)))
    if gas:
        zb = zb - 0.37 * zb[1]                  # z = 0 inside the lowest shell
    assert (gas and zb[0] < 0) or (not gas and zb[0] == 0)
    span = 2.0 * np.sqrt((zb[-1] - zb[0]) * (2.0 * R0 + zb[-1] + zb[0]))       # the longest chord
    fall = 1e-7 ** (np.arange(S) / max(S - 1, 1))
    alpha = (1.0e3 / span) * fall[:, None, None] * rng.uniform(0.5, 2.0, (S, nbin, ny)) * (S if S < 4 else 6.0)
    dtau = alpha * np.diff(zb)[:, None, None]
    cloud = dtau.mean(axis=2) * rng.uniform(0.0, 0.5, (S, nbin)) if clouds else np.zeros((S, nbin))
    dtau[:, 0, :], cloud[:, 0] = 0.0, 0.0
    dtau[:, 1, :] = 1.0e6
    w = np.polynomial.legendre.leggauss(ny)[1]
    return dtau, cloud, zb, w, R0


def _run_kernel(ctx, dtau, cloud, zb, w, R0, iso, chords):
    """hx_transit_depth through the C-ABI.  Non-isothermal layers: shells 2i / 2i + 1 are handed over as the lower / upper
    half of layer i, in the layouts of the run (delta_tau_wg_*[y + ny*x + ny*nbin*i], delta_tau_all_clouds_*[x + nbin*i])."""
    from helios_amd import _lib
    l = _lib.lib()
    S, X, Y = dtau.shape
    null = ctypes.POINTER(ctypes.c_double)()
    if iso:
        dev = [ctx.to_gpu(dtau.ravel()), None, ctx.to_gpu(cloud.ravel()), None]
    else:
        dev = [ctx.to_gpu(dtau[0::2].ravel()), ctx.to_gpu(dtau[1::2].ravel()),
               ctx.to_gpu(cloud[0::2].ravel()), ctx.to_gpu(cloud[1::2].ravel())]
    d_zb, d_w = ctx.to_gpu(zb), ctx.to_gpu(w)
    n_work = int(l.hx_transit_work_doubles(S, X))
    guard = 8
    work = ctx.to_gpu(np.full(n_work + guard, -7.0))
    d_A, d_floor = ctx.to_gpu(np.full(X + guard, -7.0)), ctx.to_gpu(np.full(X + guard, -7.0))
    d_T = ctx.to_gpu(np.full(S * X + guard, -7.0)) if chords else None
    ctx.check(l.hx_transit_depth(ctx.handle, *[d.d if d is not None else null for d in dev], d_zb.d, d_w.d, float(R0), X, Y, S,
                                 work.d, d_A.d, d_floor.d, d_T.d if chords else null), "hx_transit_depth")
    out = {"A": d_A.get(), "T_floor": d_floor.get(), "T_band": d_T.get() if chords else None}
    assert np.all(work.get()[n_work:] == -7.0)                   # nothing is written behind any array
    for k in ("A", "T_floor"):
        assert np.all(out[k][X:] == -7.0), k
        out[k] = out[k][:X]
    if chords:
        assert np.all(out["T_band"][S * X:] == -7.0)
        out["T_band"] = out["T_band"][:S * X].reshape(S, X)
    for d in dev + [d_zb, d_w, work, d_A, d_floor, d_T]:
        if d is not None:
            d.free()
    return out


def _hold(name, got, ref, plain, relative):
    """the rule of the module docstring, figures first"""
    got, ref, plain = np.asarray(got, LD), np.asarray(ref, LD), np.asarray(plain, LD)
    scale = np.abs(ref) if relative else np.ones_like(ref)
    bound = np.maximum(LD(1e-13) * scale, 8 * np.abs(plain - ref))
    err = np.abs(got - ref)
    safe = np.where(scale > 0, scale, 1)
    print("%-8s max %s error %.2e (plain fp64: %.2e), worst error / bound %.2f"
          % (name, "relative" if relative else "absolute", float((err / safe).max()), float((np.abs(plain - ref) / safe).max()),
             float((err / np.where(bound > 0, bound, 1)).max())))
    bad = np.nonzero(~(err <= bound))
    assert not len(bad[0]), (name, [tuple(int(i) for i in b) for b in zip(*bad)][:5], got[bad][:5], ref[bad][:5])


def _check_against_restatement(out, dtau, cloud, zb, w, R0):
    ref = tr.transit(dtau, cloud, zb, w, R0)
    plain = tr.plain_fp64(dtau, cloud, zb, w, R0)
    _hold("A", out["A"], ref["A"], plain["A"], relative=True)
    _hold("T_floor", out["T_floor"], ref["T_floor"], plain["T_floor"], relative=True)
    if out.get("T_band") is not None:
        _hold("T_band", out["T_band"], ref["T_band"], plain["T_band"], relative=False)
    return ref, plain


SHAPES = [(7, 3), (65, 4), (7, 1), (14, 20)]          # nbin x ny: 21 and 260 spectral points (past one workgroup), ny = 1, 20
# clouds, gas-type geometry, T_band asked for: every pair of the three factors in all four combinations
VARIANTS = [(0, 0, 0), (1, 1, 1), (1, 0, 0), (0, 1, 1), (0, 1, 0), (1, 0, 1)]


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("size", ["1", "2", "3", "B-1", "B", "B+1", "2*B+1"])
def test_isothermal_shells(ctx, size, shape, variant):
    """one shell per layer: every shell count around the impact-parameter block B of a thread"""
    S = _size(size)
    clouds, gas, chords = VARIANTS[variant]
    dtau, cloud, zb, w, R0 = _inputs(S, shape[0], shape[1], clouds, gas, seed=1000 * S + 10 * shape[0] + variant)
    out = _run_kernel(ctx, dtau, cloud, zb, w, R0, iso=True, chords=chords)
    ref, plain = _check_against_restatement(out, dtau, cloud, zb, w, R0)
    # the empty bin: the Gauss weights alone, summed in the order of the contract; the opaque bin: nothing
    assert out["A"][0] == plain["A"][0] and out["T_floor"][0] == plain["T_floor"][0] and abs(out["T_floor"][0] - 1) < 1e-15
    assert out["T_floor"][1] == 0 and float(ref["T_floor"][1]) == 0
    if S >= 15:
        tau = np.asarray(ref["tau"][:, 2:], float)
        assert tau.max() > 1e3 and tau.min() < 1e-3        # the chords span what the issue asks for


@pytest.mark.parametrize("variant", range(len(VARIANTS)))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("nlayer", ["1", "B//2", "B//2+1", "B+1"])
def test_half_layer_shells(ctx, nlayer, shape, variant):
    """two shells per layer, handed over as the run holds them: lower and upper halves in arrays of their own"""
    S = 2 * _size(nlayer)
    clouds, gas, chords = VARIANTS[variant]
    dtau, cloud, zb, w, R0 = _inputs(S, shape[0], shape[1], clouds, gas, seed=2000 * S + 10 * shape[0] + variant)
    out = _run_kernel(ctx, dtau, cloud, zb, w, R0, iso=False, chords=chords)
    _check_against_restatement(out, dtau, cloud, zb, w, R0)
    assert out["T_floor"][1] == 0


def test_refused_arguments(ctx):
    from helios_amd import _lib
    l = _lib.lib()
    null = ctypes.POINTER(ctypes.c_double)()
    a = ctx.zeros(64)
    args = lambda up, ny, S: (ctx.handle, a.d, a.d if up else null, a.d, a.d if up else null, a.d, a.d, 1.0, 2, ny, S, a.d, a.d,
                              a.d, null)
    assert l.hx_transit_depth(*args(False, 2, 0)) == 1
    assert l.hx_transit_depth(*args(True, 2, 3)) == 1                 # half-layer shells come in pairs
    assert l.hx_transit_depth(*args(False, 257, 2)) == 3
    assert b"Gauss points" in l.hx_last_error(ctx.handle)
    a.free()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
BASE = ["-parameter_file", "/nonexistent", "-opacity_mixing", "synthetic", "-synthetic", "20 6 5 11", "-number_of_layers", "12",
        "-maximum_number_of_iterations", "20000", "-radiative_equilibrium_criterion", "1e-4", "-convective_adjustment", "no"]


def _read_file(path):
    lines = open(path).read().split("\n")
    assert lines[2].split() == ["bin", "cent_lambda[um]", "transit_radius[cm]", "transit_depth", "floor_transmission"]
    return np.array([[float(v) for v in ln.split()] for ln in lines[3:]]), lines


@pytest.fixture(scope="module")
def single_on(tmp_path_factory):
    import helios
    wd = str(tmp_path_factory.mktemp("transit_on"))
    q = helios.run_helios(BASE + ["-transit_depth_spectrum", "yes", "-name", "tr_0", "-output_directory", wd + "/"])
    return q, os.path.join(wd, "tr_0")


def test_single_run_writes_the_restatement_of_its_own_column(single_on):
    q, out = single_on
    assert q.rt is not None and int(q.iso) == 0
    table, lines = _read_file(os.path.join(out, "tr_0_transit_depth.dat"))
    L, X, Y = int(q.nlayer), int(q.nbin), int(q.ny)
    assert L == 12 and table.shape == (X, 5) and np.array_equal(table[:, 0], np.arange(X))
    half = lambda n: getattr(q, "dev_" + n).get()
    gas = lambda n: half(n)[:L * X * Y].reshape(L, X, Y)
    cl = lambda n: half(n)[:L * X].reshape(L, X)
    dtau = tr.shells_of_layers(gas("delta_tau_wg_lower"), gas("delta_tau_wg_upper"))
    cloud = tr.shells_of_layers(cl("delta_tau_all_clouds_lower"), cl("delta_tau_all_clouds_upper"))
    assert dtau.min() > 0                       # Rayleigh scattering included: no shell is empty
    zb = tr.shell_boundaries(q.dev_z_lay.get(), q.dev_delta_z_lay.get(), iso=False)      # the altitudes the run ended with
    assert np.array_equal(q.z_lay, q.dev_z_lay.get()) and np.array_equal(q.delta_z_lay, q.dev_delta_z_lay.get())
    assert zb[0] < 0 and np.array_equal(zb, q.transit_zb)          # a gas planet: z = 0 at 10 bar, inside the column
    R0, R_star = float(q.R_planet), float(q.R_star)
    ref = tr.transit(dtau, cloud, zb, q.gauss_weight, R0, R_star)
    plain = tr.plain_fp64(dtau, cloud, zb, q.gauss_weight, R0, R_star)
    _hold("R_eff", table[:, 2], ref["R_eff"], plain["R_eff"], relative=True)
    _hold("depth", table[:, 3], ref["depth"], plain["depth"], relative=True)
    _hold("T_floor", table[:, 4], ref["T_floor"], plain["T_floor"], relative=True)
    _hold("A", q.transit_area, ref["A"], plain["A"], relative=True)      # the area itself, which the radius hides behind R0^2
    assert np.array_equal(table[:, 2], q.transit_radius) and np.array_equal(table[:, 3], q.transit_depth)
    assert np.array_equal(table[:, 4], q.transit_floor_transmission)
    assert ("%g" % q.transit_floor_transmission.max()) in lines[1]
    assert np.all(table[:, 2] > R0 + zb[0]) and np.all(table[:, 2] < R0 + zb[-1]) and np.ptp(table[:, 2]) > 0


def test_option_off_changes_no_other_file(single_on, tmp_path):
    import helios
    _q, on = single_on
    q = helios.run_helios(BASE + ["-name", "tr_0", "-output_directory", str(tmp_path) + "/"])
    assert q.transit_depth is None and int(q.transit_depth_spectrum) == 0
    off = os.path.join(str(tmp_path), "tr_0")
    files = sorted(os.listdir(off))
    assert "tr_0_transit_depth.dat" not in files and len(files) > 15
    assert sorted(os.listdir(on)) == sorted(files + ["tr_0_transit_depth.dat"])
    for f in files:
        with open(os.path.join(on, f), "rb") as fa, open(os.path.join(off, f), "rb") as fb:
            assert fa.read() == fb.read(), f


def test_two_column_sweep_writes_what_the_single_runs_write(single_on, tmp_path):
    """Each column of a sweep over radius_planet writes the transit-depth file its single run writes, byte for byte: the
    columns of this batch end where their single runs end (equal iteration counts), and the post-loop path is the same code on
    the same arrays.  Measured on an MI355X: every difference 0.  With the single run held to the restatement
    (test_single_run_writes_the_restatement_of_its_own_column), equality holds the sweep's column to it as well."""
    import helios
    import sweep
    wd = str(tmp_path)
    radii = ["1", "1.3"]
    cols, _spectra = sweep.main(["-sweep", "radius_planet=" + ",".join(radii)] + BASE +
                                ["-transit_depth_spectrum", "yes", "-name", "tr", "-output_directory", wd + "/batch/"])
    assert len(cols) == 2
    for k, r in enumerate(radii):
        if k == 0:
            single, sdir = single_on                  # radius_planet = 1 is the default
        else:
            single = helios.run_helios(BASE + ["-transit_depth_spectrum", "yes", "-radius_planet", r, "-name", "tr_%d" % k,
                                               "-output_directory", wd + "/single/"])
            sdir = os.path.join(wd, "single", "tr_%d" % k)
        paths = (os.path.join(wd, "batch", "tr_%d" % k, "tr_%d_transit_depth.dat" % k),
                 os.path.join(sdir, "tr_%d_transit_depth.dat" % k))
        (a, _), (b, _) = _read_file(paths[0]), _read_file(paths[1])
        assert int(cols[k].iter_value) == int(single.iter_value)
        safe = np.where(b[:, 4] > 0, b[:, 4], 1)
        print("column %d: max relative difference radius %.2e, depth %.2e, floor transmission %.2e"
              % (k, np.abs(a[:, 2] / b[:, 2] - 1).max(), np.abs(a[:, 3] / b[:, 3] - 1).max(), (np.abs(a[:, 4] - b[:, 4]) / safe).max()))
        assert np.array_equal(a, b)
        with open(paths[0], "rb") as fa, open(paths[1], "rb") as fb:
            assert fa.read() == fb.read()
        for n in ("transit_radius", "transit_depth", "transit_floor_transmission", "transit_area", "transit_zb"):
            assert np.array_equal(getattr(cols[k], n), getattr(single, n)), n
        assert np.array_equal(a[:, 2], cols[k].transit_radius) and np.array_equal(a[:, 3], cols[k].transit_depth)
        assert np.array_equal(a[:, 4], cols[k].transit_floor_transmission)
        assert float(cols[k].R_planet) == float(single.R_planet)
    assert float(cols[1].R_planet) > 1.29 * float(cols[0].R_planet)
    assert np.all(cols[1].transit_radius > 1.2 * cols[0].transit_radius)       # two planets, two answers
