"""A scripted stand-in for the device-resident batch (`RTBatch`), its context and the Stores around it, for the tests of the
host drivers that pace `hx_rt_run` / `hx_rt_conv_run` (helios_amd/loops.py).  Nothing here touches a device.

The fake batch records every call with its arguments in one list, shared with the fake context, the fake output writer and
the per-stage stand-ins, so that a transcript keeps the order of everything the host did.  Its columns follow a script: the
count at which a column reports `done` in the radiation loop and in the convection loop (None: never), and the profile the
radiation loop left behind.  (tests/test_loops.py; the recorded transcripts: tests/golden/make_loops_golden.py)"""
import contextlib
import io
import re

import numpy as np

L = 4                                   # layers of every scripted column
P_LAY = 1e6 * 0.5 ** np.arange(L)       # the bottom layer first, as everywhere
P_INT = 1.5e6 * 0.5 ** np.arange(L + 1)
STABLE = np.array([900.0, 900.0, 900.0, 900.0, 900.0])        # isothermal, surface as warm as the lowest layer
UNSTABLE = np.array([2000.0, 1000.0, 500.0, 250.0, 2000.0])   # halves per layer: far steeper than any adiabat here
TABLE_KAPPA = dict(kappa_lay=np.array([0.30, 0.29, 0.28, 0.27]), kappa_int=np.array([0.31, 0.30, 0.29, 0.28, 0.27]),
                   c_p_lay=np.array([3.1e8, 3.0e8, 2.9e8, 2.8e8]))


def _plain(v):
    """an argument as the transcript keeps it: arrays as [dtype, values]"""
    if isinstance(v, np.ndarray):
        return [str(v.dtype), v.reshape(-1).tolist()]
    if isinstance(v, (np.integer, int)) and not isinstance(v, bool):
        return int(v)
    if isinstance(v, (np.floating, float)):
        return float(v)
    return v


class FakeRT(object):
    """columns: one dict per column with `rad_done_at`, `conv_done_at` (counts or None), `profile` (T_lay, L + 1 values) and,
    if its surface is to read 20000 K from some count on, `hot_from`"""

    def __init__(self, calls, columns):
        self.calls, self.cols = calls, columns
        self.ncol = len(columns)
        self.count = 0
        self.done = [0] * self.ncol
        self.iters_done = [0] * self.ncol
        self.in_conv = [False] * self.ncol
        self.state = [dict() for _ in columns]
        self.from_table = False

    def _rec(self, *call):
        self.calls.append([_plain(v) for v in call])

    def _advance(self, key, it, n):
        assert it == self.count or it == 0, "a chunk starts where the last one ended"
        self.count = int(it) + int(n)
        for c, col in enumerate(self.cols):
            at = col.get(key)
            if not self.done[c] and at is not None and at <= self.count:
                self.done[c], self.iters_done[c] = 1, int(at)

    def run(self, it, n):
        self._rec("run", it, n)
        assert n >= 1
        self._advance("rad_done_at", it, n)

    def conv_run(self, it, n):
        self._rec("conv_run", it, n)
        assert n >= 1
        self._advance("conv_done_at", it, n)

    def step(self, it, step_temperature=True):
        self._rec("step", it, bool(step_temperature))

    def converged_layers(self):
        self._rec("converged_layers")
        return np.array([(self.count + c) % (L + 2) for c in range(self.ncol)], np.int32)

    def kappa_cp_refresh(self):
        self._rec("kappa_cp_refresh")
        self.from_table = True

    def set_convergence_limit(self, col, limit):
        self._rec("set_convergence_limit", col, limit)

    def set_column_vmr(self, col, vl, vi):
        self._rec("set_column_vmr", col, np.asarray(vl), np.asarray(vi))

    def set_state(self, col, name, array):
        a = np.ascontiguousarray(array)
        self._rec("set_state", col, name, a)
        for c in (range(self.ncol) if col < 0 else [int(col)]):
            if name == "done":
                self.done[c] = int(a[0])
                if not self.done[c]:      # the convection loop starts the column again, counting from zero
                    self.count = 0
            else:
                self.state[c][name] = a.copy()

    def get(self, name, col=0):
        col = int(col)
        self._rec("get", name, col)
        if name == "done":
            return np.array([self.done[col]], np.int32)
        if name == "iters_done":
            return np.array([self.iters_done[col]], np.int32)
        if name == "T_lay":
            T = np.array(self.cols[col]["profile"], np.float64)
            if self.count >= self.cols[col].get("hot_from", np.inf):      # the surface heats beyond the Planck table
                T[L] = 20000.0
            return T
        if name in ("kappa_lay", "kappa_int", "c_p_lay"):
            if self.from_table:
                return TABLE_KAPPA[name] * (1.0 + 0.01 * col)
            return np.asarray(self.state[col].get(name, np.zeros(L + (name == "kappa_int"))), np.float64)
        if name in ("conv_layer", "conv_unstable"):
            return np.asarray(self.state[col].get(name, np.zeros(L + 1, np.int32)), np.int32)
        if name == "marked_red":
            return np.array([(i + col) % 2 for i in range(L + 1)], np.int32)
        return np.arange(L + 1, dtype=np.float64) + col


class FakeContext(object):
    def __init__(self, calls):
        self.calls = calls

    def timer_start(self):        # (what the timer brackets is not part of a transcript: the measured time may differ)
        pass

    def timer_stop_ms(self):
        return 1234.5

    def diag(self):
        self.calls.append(["diag"])
        return dict(negative_down_flux=2, negative_up_flux=0, g_limited=1, ro_rebin_skipped=0, energy_correction=1.0)

    def diag_reset(self):
        self.calls.append(["diag_reset"])


class FakeWrite(object):
    def __init__(self, calls):
        self.calls = calls

    def write_abort_file(self, quant, read):
        self.calls.append(["write_abort_file", int(getattr(quant, "rt_col", 0))])

    def write_tp_for_coupling(self, quant, read):
        self.calls.append(["write_tp_for_coupling", int(getattr(quant, "rt_col", 0))])


class FakeDev(object):
    """a device array of a single run's Store: what is read from it goes on record"""
    d = i = None

    def __init__(self, calls, name, col):
        self.calls, self.name, self.col = calls, name, col

    def set(self, v):
        pass

    def get(self):
        self.calls.append(["dev_get", self.name])
        return TABLE_KAPPA[self.name] * (1.0 + 0.01 * self.col)       # (only the kappa arrays are ever read)


class Species(object):
    source_for_vmr = "file"

    def __init__(self, name, vmr):
        self.name = name
        self.vmr_layer = np.full(L, vmr)
        self.vmr_interface = np.full(L + 1, vmr)


class Quant(object):
    """the attributes of a Store that the drivers read and write"""

    def __init__(self, calls, col, scenario, own_device_arrays):
        s = scenario
        self.name = "col%d" % col
        self.rt_col = col
        self.nlayer, self.ninterface = np.int32(L), np.int32(L + 1)
        self.iso = 0
        self.flux_calc_method = "iteration"
        self.singlewalk = s.get("singlewalk", 0)
        self.opacity_mixing = s.get("opacity_mixing", "premixed")
        self.species_list = [Species("H2O", 1e-3), Species("CO2", 2e-4)] if self.opacity_mixing == "on-the-fly" else []
        self.max_nr_iterations = s.get("max_nr_iterations", 1000)
        self.crit_relaxation_numbers = list(s.get("relax", ()))
        self.physical_tstep = s.get("physical_tstep", 0)
        self.runtime_limit = s.get("runtime_limit", 86400.0)
        self.foreplay = s.get("foreplay", 0)
        self.plancktable_dim, self.plancktable_step = 8000, 2
        self.convection = s.get("convection", 0)
        self.coupling = s.get("coupling", 0)
        self.coupl_tp_write_interval = s.get("coupl_tp_write_interval", 0)
        self.rad_convergence_limit = 1e-8 * (col + 1)
        self.relaxed_criterion_trigger = 0
        self.debug = s.get("debug", 0)
        self.add_heating = 0
        self.fl_prec = np.float64
        self.p_lay, self.p_int = P_LAY.copy(), P_INT.copy()
        self.T_lay = np.zeros(L + 1)
        self.iter_value = None
        self.conv_layer = np.zeros(L + 1, np.int32)
        self.conv_unstable = None
        self.marked_red = np.zeros(L + 1, np.int32)
        if s.get("kappa") == "table":
            self.input_kappa_value, self.entr_kappa = "file", np.ones(12)
        else:
            self.input_kappa_value, self.entr_kappa = 2.0 / 7.0, np.zeros(1)
        self.kappa_lay, self.kappa_int = np.full(L, 2.0 / 7.0), np.full(L + 1, 2.0 / 7.0)
        self.c_p_lay = np.full(L, 3.5e8)
        self.input_dampara = s.get("dampara", "automatic")
        self.rt = None
        self.ktemp, self.kpress, self.ntemp, self.npress = np.array([100.0, 3000.0]), np.array([1.0, 1e9]), 2, 2
        for n in ("T_lay", "T_int", "p_lay", "p_int", "kappa_lay", "kappa_int", "c_p_lay", "F_smooth_sum", "entr_temp", "entr_press",
                  "entr_kappa", "entr_c_p"):
            setattr(self, "dev_" + n, FakeDev(calls, n, col) if own_device_arrays else None)
        self.entr_npress = self.entr_ntemp = 3


def make_computer(calls):
    """a Compute that was never given a library or a device: the loops' own code runs, the per-stage kernels and the copy of
    the batch's state onto the Store go on record instead"""
    from helios_amd.computation import Compute
    comp = Compute.__new__(Compute)
    comp.ctx = FakeContext(calls)
    comp.use_fused = True
    comp._call = lambda name, *args: calls.append(["stage_kernel", name])
    comp.sync_store_from_rt = lambda quant, flux_state=False: calls.append(["sync_store_from_rt", bool(flux_state)])
    return comp


def set_up(scenario, single):
    """(calls, computer, quants, rt, write) of a scenario: {"columns": [{rad_done_at, conv_done_at, profile}, ...], and the
    batch's settings (Quant)}.  `single`: the Store of a single run, with device arrays of its own and an output writer"""
    calls = []
    cols = [dict(c, profile=np.array(c.get("profile", STABLE), np.float64)) for c in scenario["columns"]]
    rt = FakeRT(calls, cols)
    quants = [Quant(calls, c, scenario, single) for c in range(len(cols))]
    for q in quants:
        q.rt = rt
    return calls, make_computer(calls), quants, rt, (FakeWrite(calls) if single else None)


def final_state(quants):
    return [dict(iter_value=int(q.iter_value), convection=int(q.convection), aborted=bool(getattr(q, "aborted", False)),
                 rad_convergence_limit=float(q.rad_convergence_limit),
                 conv_layer=np.asarray(q.conv_layer).tolist(), marked_red=np.asarray(q.marked_red).tolist())
            for q in quants]


def transcript(scenario, single, drive):
    """run `drive(computer, quants, rt, write)` on the scenario; returns {"calls", "stdout", "final"}"""
    calls, computer, quants, rt, write = set_up(scenario, single)
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        try:
            drive(computer, quants, rt, write)
        except SystemExit:
            calls.append(["SystemExit"])
    text = re.sub(r"(iteration \[s\]: )[0-9.]+", r"\1#", out.getvalue())
    return dict(calls=calls, stdout=text, final=final_state(quants))


def _cols(*specs):
    return [dict(rad_done_at=r, conv_done_at=c, profile=(UNSTABLE if u else STABLE).tolist()) for r, c, u in specs]


# ---- the scenarios -------------------------------------------------------------------------------------------------------
# (rad_done_at, conv_done_at, unstable profile) per column.  A sweep's scenarios keep clear of the corners in which the
# sweep's former driver and the single run's differed: no column finishes at a count n with (n - 1) % 100 == 0, at a
# relaxation number or at max_nr_iterations + 1, no surface is hotter than the Planck table, no run is time-stepped.
SINGLE = {
    "rad_done_at_1": dict(columns=_cols((1, None, 0))),
    "rad_done_at_10": dict(columns=_cols((10, None, 0))),
    "rad_done_at_11": dict(columns=_cols((11, None, 0)), debug=1),
    "rad_done_at_101": dict(columns=_cols((101, None, 0)), foreplay=20),
    "rad_done_at_137_relaxed": dict(columns=_cols((137, None, 0)), relax=(7, 100, 999)),
    "rad_never": dict(columns=_cols((None, None, 0)), max_nr_iterations=150),
    "rad_never_relaxed": dict(columns=_cols((None, None, 0)), max_nr_iterations=29, relax=(7, 20)),
    "rad_onthefly_done_at_11": dict(columns=_cols((11, None, 0)), opacity_mixing="on-the-fly"),
    "singlewalk": dict(columns=_cols((None, None, 0)), singlewalk=1),
    "singlewalk_onthefly": dict(columns=_cols((None, None, 0)), singlewalk=1, opacity_mixing="on-the-fly", debug=1),
    "coupled_every_7": dict(columns=_cols((23, None, 0)), coupling=1, coupl_tp_write_interval=7),
    "conv_stable": dict(columns=_cols((11, None, 0)), convection=1),
    "conv_done_at_10": dict(columns=_cols((11, 10, 1)), convection=1),
    "conv_done_at_137_relaxed": dict(columns=_cols((10, 137, 1)), convection=1, relax=(105,), dampara="4"),
    "conv_never": dict(columns=_cols((10, None, 1)), convection=1, max_nr_iterations=25),
    "conv_table_kappa": dict(columns=_cols((137, 11, 1)), convection=1, kappa="table"),
    "conv_table_kappa_stable": dict(columns=_cols((10, None, 0)), convection=1, kappa="table"),
    "conv_onthefly": dict(columns=_cols((11, 11, 1)), convection=1, opacity_mixing="on-the-fly"),
}
SWEEP = {
    "one_done_at_10": dict(columns=_cols((10, None, 0))),
    "one_done_at_11": dict(columns=_cols((11, None, 0)), debug=1),
    "one_done_at_137_relaxed": dict(columns=_cols((137, None, 0)), relax=(7, 100, 999)),
    "one_never": dict(columns=_cols((None, None, 0)), max_nr_iterations=150),
    "one_singlewalk_onthefly": dict(columns=_cols((None, None, 0)), singlewalk=1, opacity_mixing="on-the-fly"),
    "one_conv_done_at_11": dict(columns=_cols((10, 11, 1)), convection=1),
    "one_conv_stable": dict(columns=_cols((10, None, 0)), convection=1),
    "three_done_at_10_11_137": dict(columns=_cols((10, None, 0), (11, None, 0), (137, None, 0))),
    "three_relaxed_one_never": dict(columns=_cols((11, None, 0), (137, None, 0), (None, None, 0)), relax=(7, 100),
                                    max_nr_iterations=150),
    "three_onthefly": dict(columns=_cols((10, None, 0), (137, None, 0), (12, None, 0)), opacity_mixing="on-the-fly"),
    "three_singlewalk": dict(columns=_cols((None, None, 0),) * 3, singlewalk=1),
    "three_conv_none_unstable": dict(columns=_cols((10, None, 0), (11, None, 0), (12, None, 0)), convection=1),
    "three_conv_some_unstable": dict(columns=_cols((10, 137, 1), (11, None, 0), (12, 11, 1)), convection=1, relax=(105,)),
    "three_conv_all_unstable_one_never": dict(columns=_cols((10, 10, 1), (11, None, 1), (12, 11, 1)), convection=1,
                                              max_nr_iterations=25, dampara="4"),
    "three_conv_table_kappa": dict(columns=_cols((10, 12, 1), (11, None, 0), (137, 10, 1)), convection=1, kappa="table"),
    "three_conv_after_abort": dict(columns=_cols((10, 11, 1), (None, 11, 1), (12, 11, 1)), convection=1,
                                   max_nr_iterations=25),
}
