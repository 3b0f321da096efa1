"""The one host driver of the device-resident loops (helios_amd/loops.py), without a device: where a chunk ends, against a
brute-force restatement of the reference's per-iteration conditions; what the driver does on a scripted device
(tests/scripted_device.py), call for call, against what the four hand-written drivers it replaced did
(tests/golden/loops/, recorded by tests/golden/make_loops_golden.py on the commit before); and the corners in which a column of
a sweep now ends where its own single run ends."""
import copy
import json
import os

import pytest

import scripted_device as sd
from helios_amd import loops
from helios_amd.computation import Compute

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "loops")


# ---- 1. next_stop ----------------------------------------------------------------------------------------------------------
def _due(n, radiation, max_nr, relax, tstep, limit, interval):
    """does the reference's loop (source/computation.py) look at or do something behind its n-th completed iteration, the one
    with index n - 1 -- so that a chunk of iterations on the device has to end at count n?"""
    if n % 10 == 0:                                             # :860 / :1046: iteration index n is a refresh
        return True
    if n in relax:                                              # :974 / :1157: iter_value, just incremented, is listed
        return True
    if n == max_nr + 1:                                         # :978 / :1161: the count that exceeds the limit ends the run
        return True
    if interval > 0 and n % interval == interval - 1:           # :968-971 / :1151-1154: the profile of a coupled run
        return True
    if radiation:
        if (n - 1) % 100 == 0:                                  # :946-952: the look at the surface temperature
            return True
        if tstep != 0 and not n * tstep < limit:                # :942: condition3, (iter_value + 1) * tstep < limit
            return True
    return False


class _TimeStepped(object):
    def __init__(self, tstep, limit):
        self.physical_tstep, self.runtime_limit = tstep, limit


RELAX = ((), (7, 10, 11, 100, 101, 999))
MAX_NR = (0, 9, 10, 11, 1000)
RUNTIME = ((0, 0), (1.0, 9.0), (1.0, 10.0), (1.0, 11.0), (1.0, 99.0), (1.0, 100.0), (1.0, 101.0), (0.1, 3.0), (2.5, 0.5))
COUPLING = (0, 1, 2, 7, 10, 13)
# every runtime limit without coupling, every coupling interval without a limit, and some of both
PAIRS = [(r, 0) for r in RUNTIME] + [(RUNTIME[0], n) for n in COUPLING[1:]] + [((1.0, 99.0), 7), ((1.0, 11.0), 13),
                                                                                 ((0.1, 3.0), 2)]


@pytest.mark.parametrize("radiation", [True, False], ids=["radiation", "convection"])
@pytest.mark.parametrize("relax", RELAX, ids=["plain", "relaxed"])
def test_next_stop_is_the_first_count_at_which_the_reference_has_something_to_do(radiation, relax):
    last = 1300
    for max_nr in MAX_NR:
        for (tstep, limit), interval in (PAIRS if radiation else [(RUNTIME[0], n) for n in COUPLING]):
            due = [_due(n, radiation, max_nr, relax, tstep, limit, interval) for n in range(last + 12)]
            first = [0] * (last + 1)                    # first[it]: the smallest due count > it
            nxt = max(n for n in range(last + 12) if due[n])
            for it in range(last + 10, -1, -1):
                if it <= last:
                    first[it] = nxt
                if due[it]:
                    nxt = it
            rli = Compute._runtime_limit_iteration(_TimeStepped(tstep, limit)) if tstep != 0 else None
            for it in range(last + 1):
                got = loops.next_stop(it, max_nr, relax, surface_look=radiation, runtime_limit_iteration=rli,
                                      coupling_interval=interval)
                where = "it %d, max %d, relax %r, tstep %r limit %r, coupling %d" % (it, max_nr, relax, tstep, limit, interval)
                assert got == first[it], where
                assert got > it, where
                assert (got - 1) // 10 == it // 10, where       # no chunk crosses a multiple of 10


# ---- 2. transcripts --------------------------------------------------------------------------------------------------------
def _golden(name):
    with open(os.path.join(GOLDEN, name + ".json")) as f:
        return json.load(f)


def _single(computer, quants, rt, write):
    computer.radiation_loop(quants[0], write, None)
    computer.convection_loop(quants[0], write, None)


def _swept(computer, quants, rt, write):
    loops.radiation(computer, quants, rt)
    loops.convection(computer, quants, rt)


def _as_json(t):
    return json.loads(json.dumps(t))


@pytest.mark.parametrize("name", sorted(sd.SWEEP))
def test_a_batch_is_driven_call_for_call_as_the_sweeps_drivers_drove_it(name):
    assert _as_json(sd.transcript(sd.SWEEP[name], False, _swept)) == _golden("sweep")[name]


def _get(name):
    return ["get", name, 0]


KAPPA_READS = [_get("kappa_lay"), _get("kappa_int"), _get("c_p_lay")]
FREEZE_ALL = ["set_state", -1, "done", ["int32", [1]]]


def _expected_of_a_single_run(name, was):
    """the former single-run driver's transcript, with the differences the one driver makes to a single run, each stated:"""
    was = copy.deepcopy(was)
    calls = was["calls"]
    if sd.SINGLE[name].get("kappa") == "table":
        # kappa and c_p at the entry to convection come from the batch's own look-up, rt.kappa_cp_refresh(), for every batch
        # size -- no longer from the per-stage kernels on the synced Store (bit-identical: tests/test_gpu_loops.py)
        i = calls.index(["stage_kernel", "hx_kappa_interpol"])
        assert calls[i:i + 6] == [["stage_kernel", "hx_kappa_interpol"]] * 2 + [["stage_kernel", "hx_cp_interpol"]] + \
            [["dev_get", n] for n in ("kappa_lay", "kappa_int", "c_p_lay")]
        calls[i - 4:i + 6] = [["kappa_cp_refresh"]] + calls[i - 4:i] + KAPPA_READS
    if _get("F_smooth_sum") in calls:
        # the read-back for the Store's own device array follows the driver's, three reads later
        j = calls.index(_get("F_smooth_sum"))
        assert calls[j + 1:j + 4] == KAPPA_READS
        calls[j:j + 4] = KAPPA_READS + [_get("F_smooth_sum")]
    if ["write_abort_file", 0] in calls:
        # a column that exceeds the iteration limit is frozen on the device and marked `aborted` with its count (and, in the
        # convection loop, read back) before the single run writes its abort file and exits
        k = calls.index(["write_abort_file", 0])
        back = [_get("conv_layer"), _get("conv_unstable"), _get("marked_red")] + KAPPA_READS
        calls[k:k] = [FREEZE_ALL] + (back if ["conv_run", 0, 10] in calls else [])
        was["final"][0].update(aborted=True, iter_value=sd.SINGLE[name]["max_nr_iterations"] + 1)
        if back[0] in calls:
            was["final"][0]["marked_red"] = [0, 1, 0, 1, 0]        # (the scripted device's)
    return was


@pytest.mark.parametrize("name", sorted(sd.SINGLE))
def test_a_single_run_is_driven_and_prints_as_its_own_driver_did(name):
    assert _as_json(sd.transcript(sd.SINGLE[name], True, _single)) == _expected_of_a_single_run(name, _golden("single")[name])


def test_the_single_run_transcripts_that_are_restated_are_the_ones_meant():
    """the restatements above touch the table-kappa, the convecting and the aborting scenarios and leave the others as recorded"""
    changed = sorted(n for n, t in _golden("single").items() if _expected_of_a_single_run(n, t) != t)
    assert changed == ["conv_done_at_10", "conv_done_at_137_relaxed", "conv_never", "conv_onthefly", "conv_table_kappa",
                       "conv_table_kappa_stable", "rad_never", "rad_never_relaxed"]


# ---- 3. the corners: every column of a batch ends where its own single run ends -------------------------------------------

def _ends(scenario):
    """(iter_value, convection, aborted) per column: as a batch, and each column as a batch of one"""
    def ends(s):
        calls, computer, quants, rt, _ = sd.set_up(s, False)
        loops.radiation(computer, quants, rt)
        return [(int(q.iter_value), int(q.convection), bool(getattr(q, "aborted", False))) for q in quants], calls
    together, calls = ends(scenario)
    alone = [ends(dict(scenario, columns=[col]))[0][0] for col in scenario["columns"]]
    return together, alone, calls


def test_the_surface_look_reaches_a_column_that_finished_in_the_same_chunk():
    """(a): columns that report `done` at counts n with (n - 1) % 100 == 0 while their surface is hotter than the Planck table
    switch convection on, as in a single run (reference computation.py:946-952); so does one that is still running there"""
    cols = [dict(rad_done_at=1, hot_from=0), dict(rad_done_at=101, hot_from=50), dict(rad_done_at=137, hot_from=0)]
    together, alone, calls = _ends(dict(columns=cols))
    assert together == alone == [(1, 1, False), (101, 1, False), (1, 1, False)]
    # the running column is frozen from the host, the finished ones need no freezing
    assert [c for c in calls if c[0] == "set_state"] == [["set_state", 2, "done", ["int32", [1]]]]
    cool = [dict(rad_done_at=c["rad_done_at"]) for c in cols]
    together, alone, _ = _ends(dict(columns=cool))
    assert together == alone == [(1, 0, False), (101, 0, False), (137, 0, False)]


@pytest.mark.parametrize("limit,leave_at", [(23.0, 23), (20.0, 20), (21.0, 21), (0.5, 1)])
def test_a_time_stepped_column_of_a_batch_leaves_at_its_runtime_limit(limit, leave_at):
    """(b): physical_tstep = 1 s, the limit inside a decade, on its edge and behind it: the columns still running leave there
    (condition3, computation.py:942), one that finished earlier keeps its count"""
    cols = [dict(rad_done_at=11), dict(rad_done_at=None), dict(rad_done_at=137)]
    s = dict(columns=cols, physical_tstep=1.0, runtime_limit=limit)
    together, alone, calls = _ends(s)
    assert together == alone == [(min(11, leave_at), 0, False), (leave_at, 0, False), (leave_at, 0, False)]
    assert [c[1] + c[2] for c in calls if c[0] == "run"][-1] == leave_at        # nothing runs behind the limit
    frozen = [c[1] for c in calls if c[0] == "set_state" and c[2] == "done"]
    assert frozen == ([0] if leave_at < 11 else []) + [1, 2]


def test_a_column_that_finishes_on_a_relaxation_number_or_behind_the_limit_ends_as_its_single_run_does():
    """two more places where the sweep's former driver skipped a column that had just finished, and the reference (and so the
    single run) does not: the criterion is relaxed behind the iteration whose count is listed (computation.py:974), and the run
    is given up behind the one that exceeds the limit (:978), converged or not"""
    s = dict(columns=[dict(rad_done_at=7), dict(rad_done_at=26), dict(rad_done_at=12)], relax=(7,), max_nr_iterations=25)
    together, alone, _ = _ends(s)
    assert together == alone == [(7, 0, False), (26, 0, True), (12, 0, False)]
    calls, computer, quants, rt, _ = sd.set_up(s, False)
    loops.radiation(computer, quants, rt)
    assert [q.rad_convergence_limit for q in quants] == pytest.approx([1e-7, 2e-7, 3e-7], rel=1e-12)


def test_a_coupled_batch_ends_chunks_at_the_hand_over_and_writes_nothing():
    """(c): coupling = 1 only adds chunk boundaries to a sweep; without a writer no profile is read back"""
    s = dict(columns=[dict(rad_done_at=23), dict(rad_done_at=12)], coupling=1, coupl_tp_write_interval=7)
    calls, computer, quants, rt, _ = sd.set_up(s, False)
    loops.radiation(computer, quants, rt)
    assert [c[1] + c[2] for c in calls if c[0] == "run"] == [1, 6, 10, 13, 20, 27]
    assert [int(q.iter_value) for q in quants] == [23, 12]
    assert [c for c in calls if c[0] == "get" and c[1] == "T_lay"] == [["get", "T_lay", 0], ["get", "T_lay", 1]]   # (count 1)
