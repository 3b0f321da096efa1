"""`precision = single` on the GPU: the device-resident loop with fp32 coefficient planes (hx_rt_flags.coef_fp32) against
the same loop on fp64 planes, against itself (batches, graph replay) and, over whole runs, against the reference's double
kernels in oracle/_ref/.  The planes are rounded once per refresh (6e-8 relative per value); everything else is fp64, so
the first solve stays within 1e-5 of the double one and a whole run converges to a fixed point within 1e-5 of it."""
import os
import sys

import numpy as np
import pytest

import cases
import fused_helpers as fh
from test_gpu_fused import FUSED_CONFIGS

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    c = Context(0)
    yield c


def _single(c0):
    c = c0.copy()
    c.prec = "single"
    return c


FIRST_SOLVE = ["default", "dirbeam", "clouds_g0", "L200_i2s", "default+matrix", "pure_scatterer", "pure_scatterer+matrix"]


def _case(name):
    base, _, method = name.partition("+")
    if base == "pure_scatterer":
        # absorption 1e-14 of what the table holds, scattering as it is, layers up to 1e-6 bar: w0 at the clamp w_0_limit in
        # thin half-layers, where 1 - alpha - beta computed in fp64 comes out slightly negative (csrc/plane_code.h)
        c0 = cases.make_case(nbin=16, nlayer=40, thin_top=True, albedo=0.1 if method else 0.0)
        c0.opac_k = c0.opac_k * 1e-14
    else:
        c0 = cases.make_case(**dict(FUSED_CONFIGS[base], **({"albedo": 0.1} if method else {})))
    if method:
        c0.flux_calc_method = "matrix"
    return c0


@pytest.mark.parametrize("name", FIRST_SOLVE)
def test_first_solve_against_the_double_planes(ctx, name):
    c0 = _case(name)
    keys = ["F_up_wg", "F_down_wg", "Fc_up_wg", "Fc_down_wg", "F_up_band", "F_down_band", "F_up_tot", "F_down_tot"]
    d = fh.run_fused(ctx, c0, 1, keys=keys)
    s = fh.run_fused(ctx, _single(c0), 1, keys=keys)
    if name.endswith("+matrix"):
        # the matrix method keeps fp64 planes (its direct solve of the nearly conservative column amplified the fp32 rounding
        # to 2e-3 of some spectral up-fluxes): the double result, bit for bit
        for k in keys:
            np.testing.assert_array_equal(s[k], d[k], err_msg=k)
        return
    for k in keys[:6]:
        a, b = s[k], d[k]
        assert np.all(np.isfinite(a)), k
        bound = 1e-5 * np.abs(b) + 1e-7 * np.abs(b).max()
        worst = np.max(np.abs(a - b) - bound)
        assert worst <= 0.0, (k, float(np.max(np.abs(a - b) / (np.abs(b) + 1e-300))))
    for k in ("F_up_tot", "F_down_tot"):
        np.testing.assert_allclose(s[k], d[k], rtol=2e-6, atol=1e-12 * np.abs(d[k]).max(), err_msg=k)
    # the planes really are fp32: the result is not the double one
    assert np.any(s["F_up_wg"] != d["F_up_wg"])


def test_plane_width_and_traffic_model(ctx):
    from helios_amd.rt import batch_from_case
    c0 = cases.make_case(**FUSED_CONFIGS["dirbeam"])             # five planes (alpha, beta, u', dd, du)
    rd = batch_from_case(ctx, c0)
    rs = batch_from_case(ctx, _single(c0))
    try:
        assert rd.coef_plane_bytes() == 8 and rs.coef_plane_bytes() == 4
        td, ts = rd.traffic_model(), rs.traffic_model()
    finally:
        rd.close()
        rs.close()
    import ctypes
    from helios_amd import _lib
    k, r = ctypes.c_int(), ctypes.c_int()
    assert _lib.lib().hx_rt_flux_geometry(c0.nlayer, 0, 1, c0.ny, c0.nbin, 1, ctypes.byref(k), ctypes.byref(r)) == 0
    # the planes of the tiles as the geometry lays them out: (bins / bins per workgroup) x (Gauss points / per pass) x ...
    # -- read back from the model itself: double minus single is exactly half the fp64 plane bytes, for steps and refreshes
    plane_bytes_f64 = 2.0 * (td["step_actual"] - ts["step_actual"])
    assert plane_bytes_f64 > 0
    assert td["refresh_actual"] - ts["refresh_actual"] == plane_bytes_f64 / 2.0
    nplane = 5
    tiles = plane_bytes_f64 / (8.0 * nplane)                    # elements of one plane
    assert tiles == int(tiles) and tiles % (64 * r.value) == 0 and tiles >= c0.nbin * c0.ny * 2 * c0.nlayer
    assert td["step_algorithmic"] == ts["step_algorithmic"]

    # a column of 500 layers has no fp32 tiling (k = 64, 16 rows): fp64 planes, and it runs
    c5 = _single(cases.make_case(nbin=3, nlayer=500, dir_beam=1, albedo=0.2))
    rt = batch_from_case(ctx, c5)
    try:
        assert rt.coef_plane_bytes() == 8
        rt.build_planck_table(1)
        rt.run(0, 2)
        assert np.all(np.isfinite(rt.get("F_up_band"))) and np.all(np.isfinite(rt.get("T_lay")))
    finally:
        rt.close()
    # the matrix method keeps fp64 planes
    cm = _single(cases.make_case(**dict(FUSED_CONFIGS["default"], albedo=0.1)))
    cm.flux_calc_method = "matrix"
    rt = batch_from_case(ctx, cm)
    try:
        assert rt.coef_plane_bytes() == 8
        rt.build_planck_table(1)
        rt.run(0, 2)
        assert np.all(np.isfinite(rt.get("F_up_band"))) and np.all(np.isfinite(rt.get("T_lay")))
    finally:
        rt.close()


def test_a_batch_equals_single_columns_bit_for_bit(ctx):
    c0 = _single(cases.make_case(**FUSED_CONFIGS["clouds_g0"]))
    Ts = [c0.T_lay, c0.T_lay * 1.05, c0.T_lay * 0.9 + 30.0]
    keys = ["T_lay", "F_up_band", "F_down_band", "F_up_wg", "F_net"]
    batch = fh.run_fused(ctx, c0, 12, ncol=3, keys=keys, col=[0, 1, 2], T_per_col=Ts)
    for i, T in enumerate(Ts):
        one = fh.run_fused(ctx, c0, 12, ncol=1, keys=keys, T_per_col=[T])
        for k in keys:
            np.testing.assert_array_equal(batch[i][k], one[k], err_msg="%s column %d" % (k, i))


@pytest.mark.parametrize("name", ["L50", "clouds_g0"])
def test_graph_replay_equals_launch_by_launch_bit_for_bit(ctx, name, monkeypatch):
    from helios_amd.rt import batch_from_case
    base, _, method = name.partition("+")
    c0 = _single(cases.make_case(**dict(FUSED_CONFIGS[base], **({"albedo": 0.1} if method else {}))))
    if method:
        c0.flux_calc_method = "matrix"

    def run(graph):
        monkeypatch.setenv("HELIOS_RT_GRAPH", graph)
        rt = batch_from_case(ctx, c0)
        try:
            assert rt.coef_plane_bytes() == 4
            rt.build_planck_table(1)
            rt.run(0, 47)
            out = {k: rt.get(k) for k in ("T_lay", "F_net", "F_up_band", "delta_t_prefactor", "abort")}
            nine, decades, on = rt.get("graph_replays")
            assert (on == 1 and decades + nine >= 2) if graph == "1" else (nine == 0 and decades == 0)
            return out
        finally:
            rt.close()
    a, b = run("1"), run("0")
    for k in b:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("workload,override", [("c1", {}), ("c2", dict(nbin=1000, nlayer=50)),
                                               ("c3small", dict(nbin=500, nlayer=50, nspecies=6))],
                         ids=["config1_300x50", "config2_physics_1000x50", "onthefly_RO_500x50x6"])
def test_whole_run_in_single_against_the_reference_double_kernels(workload, override, monkeypatch):
    """whole runs to radiative equilibrium with fp32 planes against the reference's double kernels on the same GPU
    (tests/loop_to_convergence_on_gpu.py, as tests/test_gpu_trajectories.py uses it): both leave the loop converged,
    within 5 % of each other's iteration count, and the end states agree to 1e-5"""
    import oracle
    if oracle.refgpu is None:
        pytest.skip("oracle/_ref/libhelios_ref_gfx950.so not present")
    import loop_to_convergence_on_gpu as ltc
    build = ltc.bench.build_case

    def build_single(w, seed, *args, **kw):
        c = build(dict(w, **override), seed, *args, **kw)
        c.prec = "single"
        return c
    monkeypatch.setattr(ltc.bench, "build_case", build_single)
    out = ltc.main(["--workload", workload])
    ours, ref = out["libhelios_hip"], out["reference_kernels_on_this_gpu"]
    assert ours["left_the_loop"] == ref["left_the_loop"] == "converged"
    n, m = ours["radiation_loop_iterations"], ref["radiation_loop_iterations"]
    assert abs(n - m) <= 0.05 * m, (n, m)
    end = out["radiation_loop"]["end states (each side where it left the loop)"]
    assert end["T_lay"] < 1e-5, end
    assert end["F_up_tot"] < 1e-5 and end["F_down_tot"] < 1e-5, end
    assert end["emission spectrum (of its maximum)"] < 1e-5, end


def test_run_helios_in_single_runs_to_equilibrium(tmp_path, capsys):
    """helios.py -precision single: the driver's whole run on fp32 planes converges, to within 1e-5 of the double run"""
    import helios
    from helios_amd import host_functions as hs
    runs = {}
    for prec in ("double", "single"):
        argv = ["-parameter_file", "/nonexistent", "-opacity_mixing", "synthetic", "-synthetic", "40 6 5 7",
                "-number_of_layers", "24", "-maximum_number_of_iterations", "20000", "-name", "drv_" + prec,
                "-output_directory", str(tmp_path) + "/", "-radiative_equilibrium_criterion", "1e-3",
                "-convective_adjustment", "no", "-precision", prec]
        runs[prec] = helios.run_helios(argv)
    out = capsys.readouterr().out
    assert "no fp32 coefficient planes" not in out          # 24 layers have an fp32 tiling: nothing to say
    s, d = runs["single"], runs["double"]
    assert s.prec == "single" and int(s.iter_value) > 3
    assert abs(int(s.iter_value) - int(d.iter_value)) <= 0.05 * int(d.iter_value) + 1
    assert abs(hs.global_energy_imbalance(s)) < 1e-3
    np.testing.assert_allclose(s.T_lay, d.T_lay, rtol=1e-5)
    np.testing.assert_allclose(s.F_up_band, d.F_up_band, rtol=1e-4, atol=1e-5 * d.F_up_band.max())
