"""The one host driver of the device-resident loops (helios_amd/loops.py) on the device, where no test had been: kappa and c_p
from a (T, P) table that varies, at the entry to the convection loop -- the batch's own look-up against the per-stage kernels
on the synced Store, bit for bit -- and a convecting sweep with that table against its single runs."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BASE = ["-parameter_file", "/nonexistent", "-opacity_mixing", "synthetic", "-synthetic", "24 6 5 13",
        "-maximum_number_of_iterations", "20000", "-radiative_equilibrium_criterion", "1e-4",
        "-convective_adjustment", "yes", "-kappa_value", "file"]
T_INTERN = ("800", "1500")


def _kappa_table(tmp_path):
    """a kappa / c_p table whose values vary over (T, P): tests/golden/make_host_golden.py's, without `const_kappa`"""
    spec = importlib.util.spec_from_file_location(
        "make_host_golden", os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_host_golden.py"))
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)
    path = os.path.join(str(tmp_path), "delad.dat")
    mk.write_kappa_file(path, False)
    return ["-kappa_file_path", path]


def test_table_kappa_at_the_convection_entry_is_the_per_stage_kernels_bit_for_bit(tmp_path):
    """a single run stopped at the entry of convection_loop: `rt.kappa_cp_refresh()`, which loops.convection uses for every
    batch size, leaves the bits that interpolate_kappa_and_cp (the former entry of a single run) leaves on the synced Store"""
    import helios
    from helios_amd import computation
    captured = {}
    orig = computation.Compute.convection_loop

    def stop(self, quant, write=None, read=None, rt_plot=None):
        captured["computer"], captured["q"] = self, quant
        raise KeyboardInterrupt
    computation.Compute.convection_loop = stop
    try:
        helios.run_helios(BASE + _kappa_table(tmp_path) + ["-number_of_layers", "17", "-internal_temperature", "1500",
                                                           "-name", "entry", "-output_directory", str(tmp_path) + "/"])
    except KeyboardInterrupt:
        pass
    finally:
        computation.Compute.convection_loop = orig
    computer, q = captured["computer"], captured["q"]
    rt = q.rt
    assert rt is not None and computer._kappa_from_table(q) and int(q.iter_value) > 3
    table = np.asarray(q.entr_kappa, np.float64)
    assert table.max() > 1.5 * table.min()                        # the table varies
    computer.interpolate_kappa_and_cp(q)
    rt.kappa_cp_refresh()
    L = int(q.nlayer)
    for name, n in (("kappa_lay", L), ("kappa_int", L + 1), ("c_p_lay", L)):
        stage = np.asarray(getattr(q, "dev_" + name).get(), np.float64)[:n]
        batch = rt.get(name)
        assert batch.shape == (n,) and np.all(np.isfinite(batch)) and np.ptp(batch) > 0, name
        differing = np.nonzero(stage.view(np.uint64) != batch.view(np.uint64))[0]
        assert differing.size == 0, "%s differs at %r: per-stage %r, batch %r" % (name, differing, stage[differing],
                                                                                  batch[differing])


def test_a_convecting_sweep_with_a_kappa_table_equals_its_single_runs(tmp_path):
    """two columns of one batch through both loops: iteration counts, conv_layer and marked_red exact, T_lay and the TOA
    spectrum at rtol = 1e-12 (test_sweep_batch_equals_individual_runs' tolerance)"""
    import helios
    import sweep
    argv = BASE + _kappa_table(tmp_path) + ["-number_of_layers", "14"]
    out = str(tmp_path) + "/"
    cols, spectra = sweep.main(["-sweep", "internal_temperature=" + ",".join(T_INTERN)] + argv +
                               ["-name", "kt", "-output_directory", out + "batch/"])
    assert len(cols) == 2 and spectra.shape == (2, 24)
    assert any(np.asarray(q.conv_layer).sum() > 0 and int(q.iter_value) >= 400 for q in cols)      # one convects at least
    for k, T in enumerate(T_INTERN):
        single = helios.run_helios(argv + ["-name", "s%d" % k, "-internal_temperature", T,
                                           "-output_directory", out + "single/"])
        q = cols[k]
        print("column %d: %d iterations (single %d), %d convective layers" % (k, int(q.iter_value), int(single.iter_value),
                                                                              int(np.asarray(q.conv_layer).sum())))
        assert int(q.iter_value) == int(single.iter_value), k
        np.testing.assert_array_equal(q.conv_layer, single.conv_layer)
        np.testing.assert_array_equal(q.marked_red, single.marked_red)
        np.testing.assert_allclose(q.T_lay, single.T_lay, rtol=1e-12, err_msg="column %d" % k)
        np.testing.assert_allclose(spectra[k], single.F_up_band[-24:], rtol=1e-12)
        np.testing.assert_array_equal(q.kappa_lay, single.kappa_lay)
