"""A sweep over premixed opacity tables (`-sweep "path_to_opacity_file=a.npz,b.npz"`), host side: the option expands, every
table file is read once and shared, batches are keyed on the tables' grid, on-the-fly mixing refuses the option, and the new
C-ABI entries are declared, exported and bound.  (The device side: tests/test_gpu_table_sweep.py.)"""
import ctypes
import os

import numpy as np
import pytest

import table_files as tf

BASE = ["-parameter_file", "/nonexistent", "-opacity_mixing", "premixed", "-number_of_layers", "14",
        "-maximum_number_of_iterations", "20000", "-radiative_equilibrium_criterion", "1e-4",
        "-convective_adjustment", "no", "-name", "tab"]


def test_expand_sweep_takes_the_table_path():
    from helios_amd.sweep import PER_COLUMN_OPTIONS, expand_sweep
    assert "path_to_opacity_file" in PER_COLUMN_OPTIONS
    cols = expand_sweep("path_to_opacity_file=a.npz,b.npz;internal_temperature=100,300")
    assert cols == [{"path_to_opacity_file": "a.npz", "internal_temperature": "100"},
                    {"path_to_opacity_file": "a.npz", "internal_temperature": "300"},
                    {"path_to_opacity_file": "b.npz", "internal_temperature": "100"},
                    {"path_to_opacity_file": "b.npz", "internal_temperature": "300"}]


def test_each_table_file_is_read_once_and_its_arrays_are_shared(tmp_path, monkeypatch):
    """three columns over two files: two reads; the Stores of one file hold the identical array objects, those of the other
    file other arrays -- also through a second batch of the same run_sweep (the cache is the sweep's, not the batch's)"""
    from helios_amd import read as read_mod
    from helios_amd import sweep as sw
    a, b = tf.write_chemistries(str(tmp_path), 24, count=2)
    os.symlink(a, str(tmp_path / "alias.npz"))        # the same file by another name: keyed by the resolved path
    calls = []
    orig = read_mod.Read.read_opac_file

    def counting(self, quant, path, *args, **kw):
        calls.append(os.path.realpath(str(path)))
        return orig(self, quant, path, *args, **kw)
    monkeypatch.setattr(read_mod.Read, "read_opac_file", counting)
    shared = {}
    qs = [sw._prepare_column(BASE, {"path_to_opacity_file": p, "internal_temperature": T}, shared)[0]
          for p, T in ((a, "100"), (b, "100"), (a, "300"))]
    assert sorted(calls) == sorted([os.path.realpath(a), os.path.realpath(b)])
    for n in ("opac_k", "opac_scat_cross", "opac_meanmass", "ktemp", "kpress", "opac_interwave"):
        assert getattr(qs[0], n) is getattr(qs[2], n), n
    for n in ("opac_k", "opac_scat_cross", "opac_meanmass"):
        assert getattr(qs[0], n) is not getattr(qs[1], n), n
        assert not np.array_equal(getattr(qs[0], n), getattr(qs[1], n)), n
    more = [sw._prepare_column(BASE, {"path_to_opacity_file": p}, shared)[0] for p in (b, str(tmp_path / "alias.npz"))]
    assert len(calls) == 2
    assert more[0].opac_k is qs[1].opac_k and more[1].opac_k is qs[0].opac_k
    # what the table says about the column is the column's own
    assert float(qs[0].opac_meanmass[0]) != float(qs[1].opac_meanmass[0])
    assert int(qs[0].nbin) == int(qs[1].nbin) == 24 and int(qs[0].ny) == 20


def test_batches_are_keyed_on_the_tables_grid(tmp_path):
    """same grid, different tables: one batch; a table on other temperature nodes: a batch of its own"""
    from helios_amd import sweep as sw
    a, b = tf.write_chemistries(str(tmp_path), 24, count=2)
    c = tf.write_table(str(tmp_path / "other_T.npz"), 24, *tf.CHEMISTRIES[2], tmax=2500.0)
    shared = {}
    qa, qb, qc = [sw._prepare_column(BASE, {"path_to_opacity_file": p}, shared)[0] for p in (a, b, c)]
    assert qa.opac_k is not qb.opac_k
    assert sw._batch_signature(qa) == sw._batch_signature(qb)
    assert sw._batch_signature(qa) != sw._batch_signature(qc)
    assert len(qa.ktemp) == len(qc.ktemp)           # the same numbers of nodes: the digest tells them apart, not a count


def test_a_table_sweep_with_on_the_fly_mixing_is_refused(tmp_path):
    from helios_amd import sweep as sw
    argv = [("on-the-fly" if v == "premixed" else v) for v in BASE]
    with pytest.raises(ValueError, match="on-the-fly"):
        sw._prepare_column(argv, {"path_to_opacity_file": str(tmp_path / "a.npz")}, {})


def test_the_table_entries_are_declared_exported_and_bound():
    from helios_amd import _lib
    from helios_amd.rt import RTBatch
    protos = _lib.prototypes()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("hx_rt_add_premixed_tables", "hx_rt_set_column_table"):
        assert n in protos and hasattr(raw, n), n
        assert getattr(_lib.lib(), n).argtypes == protos[n][1]
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    assert protos["hx_rt_add_premixed_tables"][1] == [ctypes.c_void_p, dp, dp, dp, ip]
    assert protos["hx_rt_set_column_table"][1] == [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    assert callable(RTBatch.add_premixed_tables) and callable(RTBatch.set_column_table)


def test_the_sweep_quotes_why_a_configuration_is_outside_the_device_loop_without_printing(capsys):
    """`Compute._why_not_fused` is a pure predicate: a sweep quotes its reason when it refuses a configuration and prints
    no notice about per-stage kernels, which it never runs"""
    from helios_amd.computation import Compute

    class Q(object):
        iso, singlewalk, flux_calc_method, nlayer = 0, 0, "iteration", 1025
    comp = Compute.__new__(Compute)
    comp.use_fused = True
    why = comp._why_not_fused(Q())
    assert "1025 layers" in why and capsys.readouterr().out == ""
    Q.nlayer = 1024
    assert comp._why_not_fused(Q()) is None


def test_a_sweep_beyond_the_device_loops_limits_raises_with_the_reason_and_announces_no_fall_back(tmp_path, capsys):
    """1025 layers: `sweep._run_columns` refuses the configuration with the predicate's reason in its IOError and prints no
    notice about per-stage kernels -- a sweep never runs them"""
    from helios_amd import sweep as sw
    from helios_amd.computation import Compute

    class Computer(object):            # what _run_columns asks of a Compute before any device work
        ctx, use_fused = None, True
        _why_not_fused = Compute._why_not_fused
        _fused_supported = Compute._fused_supported
    a, = tf.write_chemistries(str(tmp_path), 24, count=1)
    argv = [("1025" if v == "14" else v) for v in BASE] + ["-path_to_opacity_file", a]
    with pytest.raises(IOError, match=r"1025 layers.*column by column"):
        sw._run_columns(argv, [{}], [0], Computer(), None, {}, [], dict(batch=0.0, loops=0.0, finish=0.0), False)
    out = capsys.readouterr().out
    assert "per-stage kernels" not in out and "slower" not in out
