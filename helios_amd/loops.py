"""The host driver of the device-resident loops (hx_rt_run, hx_rt_conv_run), for a batch of any size.

The device iterates on its own and freezes a column where the column's criterion is met; the host only paces it, in chunks that
end wherever the reference's loop (source/computation.py:827-1174) looks at something or does something between two iterations:
`next_stop` says where, `radiation` and `convection` do it, per column.  A single run is a batch of one (Compute.radiation_loop,
Compute.convection_loop), a sweep a batch of many (sweep._run_columns): every column ends where its own single run ends.
Counts are numbers of completed iterations; the reference's iteration index is one less.
"""
import numpy as np

from . import host_functions as hsfunc


def next_stop(it, max_nr_iterations, relaxations=(), surface_look=False, runtime_limit_iteration=None,
              coupling_interval=0):
    """the count at which the chunk that starts at count `it` ends: the smallest count > it at which the host has to look"""
    nxt = it + (10 - it % 10)                                  # the refresh every 10th iteration (computation.py:860)
    if int(max_nr_iterations) + 1 > it:
        nxt = min(nxt, int(max_nr_iterations) + 1)             # the count that exceeds the limit (:978)
    for r in relaxations:                                      # a relaxation of the criterion (:974)
        if it < r < nxt:
            nxt = int(r)
    if surface_look:                                           # the look at the surface temperature inside every iteration
        nxt = min(nxt, it + 1 + (100 - it % 100) % 100)        # whose index is a multiple of 100 (:946-952)
    if runtime_limit_iteration is not None:                    # a time-stepped run's condition3, tested every iteration (:942)
        nxt = min(nxt, max(it + 1, int(runtime_limit_iteration)))
    n = int(coupling_interval)
    if n > 0:                                                  # the T-P profile a coupled run hands over (:967-971): the first
        nxt = min(nxt, it + 1 + (n - 1 - (it + 1) % n) % n)    # count > it with count % n == n - 1
    return nxt


def _coupling_interval(q):
    return int(getattr(q, "coupl_tp_write_interval", 0) or 0) if q.coupling == 1 else 0


def _counts(rt, live, it):
    """({column: the device froze it}, {column: its count}) after a chunk that ended at count `it`"""
    done, at = {}, {}
    for c in live:
        done[c] = int(rt.get("done", c)[0])
        at[c] = int(rt.get("iters_done", c)[0]) if done[c] else it       # the device froze the column exactly there
    return done, at


def _between_iterations(computer, quants, rt, live, at, write, read):
    """what the reference does behind every iteration, for the columns `live` at their counts `at`: the profile for a coupled
    run, the relaxation of the criterion, the iteration limit -- whether or not the column has just finished
    (computation.py:967-980, :1150-1163).  Returns the columns that exceed the limit"""
    for c in live:
        computer._coupling_output(quants[c], at[c], write, read)
    for c in live:
        if at[c] in quants[c].crit_relaxation_numbers:
            hsfunc.relax_radiative_convergence_criterion(quants[c])
            rt.set_convergence_limit(c, quants[c].rad_convergence_limit)
    over = [c for c in live if at[c] > quants[c].max_nr_iterations]
    for c in over:
        quants[c].aborted = True
    if over:      # (a chunk ends at the limit, so this is every column still live)
        rt.set_state(-1, "done", np.ones(1, np.int32))
    return over


def radiation(computer, quants, rt, write=None, read=None, progress=False):
    """run every column of `rt` to the end of its radiation loop (reference computation.py:827-990); returns the columns'
    iteration counts, which it also leaves in their `iter_value`.  A column that meets its criterion is frozen by the device; one
    that leaves through the host -- hot surface, runtime limit, iteration limit (`aborted`) -- is frozen from here.
    `progress`: print the single run's progress lines."""
    q0 = quants[0]
    iters = np.zeros(len(quants), np.int64)
    if q0.opacity_mixing == "on-the-fly":
        # once per loop: constant and file-given profiles never change, a FastChem species' profile is re-interpolated on the
        # device at every refresh from its column's (T, P) table (Compute.make_rt_batch)
        for q in quants:
            computer._push_vmr(q)
    live = list(range(len(quants)))
    if q0.singlewalk == 1:
        # post-processing run type (computation.py:983-984): ONE pass over the given T-P profiles -- refresh, 1000*scat+1
        # sweeps inside one launch of the flux kernel, quadrature -- and no temperature step
        rt.step(0, step_temperature=False)
        computer.report_diagnostics(q0)
        live = []
    it = 0
    while live:
        limits = [computer._runtime_limit_iteration(quants[c]) for c in live if quants[c].physical_tstep != 0]
        nxt = next_stop(it, q0.max_nr_iterations, q0.crit_relaxation_numbers, surface_look=True,
                        runtime_limit_iteration=min(limits) if limits else None, coupling_interval=_coupling_interval(q0))
        rt.run(it, nxt - it)
        computer.report_diagnostics(q0)
        if progress:
            converged = rt.converged_layers()
        it_prev, it = it, nxt
        done, at = _counts(rt, live, it)                       # blocks: one small D2H per column and <= 10 iterations
        for c in live:
            if progress and it_prev >= int(quants[c].foreplay) and (it_prev % 100 == 0 or done[c]):
                print("\nWe are running \"" + str(quants[c].name) + "\" at iteration step nr. : " + str(it_prev))
                print("Layers (& surface/BOA) converged: " + str(int(converged[c])) + " out of "
                      + str(int(quants[c].nlayer) + 1) + ".")
        host_exit = []
        for c in live:
            q = quants[c]
            if q.physical_tstep != 0 and not at[c] * q.physical_tstep < q.runtime_limit:       # condition3
                host_exit.append(c)
        for c in live:
            q = quants[c]
            if (at[c] - 1) % 100 == 0:      # computation.py:946-952: a surface hotter than the Planck table ends the loop
                if not rt.get("T_lay", c)[int(q.nlayer)] < q.plancktable_dim * q.plancktable_step - 2:
                    if q.iso == 0:          # (isothermal layers cannot be adjusted: see Compute.convection_loop)
                        q.convection = 1
                    host_exit.append(c)
        for c in sorted(set(host_exit)):
            if not done[c]:
                rt.set_state(c, "done", np.ones(1, np.int32))
        over = _between_iterations(computer, quants, rt, live, at, write, read)
        for c in live:
            iters[c] = at[c]
        live = [c for c in live if not (done[c] or c in host_exit or c in over)]
    for c, q in enumerate(quants):
        q.iter_value = np.int32(iters[c])
    return iters


def convection(computer, quants, rt, write=None, read=None, progress=False):
    """run every column of `rt` that asks for convective adjustment through the device-side convection loop -- adjustment,
    sweeps, layer marking, equilibrium test and temperature step all on the GPU (hx_rt_conv_*; reference
    computation.py:992-1174) -- until its own loop condition turns false; returns the columns' iteration counts.  Columns without
    a super-adiabatic layer, columns with `convection != 1` and aborted columns stay frozen."""
    q0 = quants[0]
    iters = np.zeros(len(quants), np.int64)
    from_table = any(computer._kappa_from_table(q) for q in quants)
    if from_table:    # kappa / c_p follow the profile the radiation loop left behind (computation.py:1037)
        rt.kappa_cp_refresh()
    active = []
    for c, q in enumerate(quants):
        if not (q.singlewalk == 0 and q.convection == 1) or getattr(q, "aborted", False):
            continue
        for n in ("T_lay", "F_net", "F_up_tot", "F_down_tot") + (("kappa_lay", "kappa_int", "c_p_lay") if from_table else ()):
            setattr(q, n, rt.get(n, c))
        q.p_lay, q.p_int = np.asarray(q.p_lay, float), np.asarray(q.p_int, float)
        hsfunc.conv_check(q)
        hsfunc.mark_convective_layers(q, stitching=0)
        q.iter_value = np.int32(0)      # the convection loop counts from zero, also when it has nothing to do
        if sum(q.conv_unstable) > 0:
            active.append(c)
            for name, v, dt in (("kappa_lay", q.kappa_lay, np.float64), ("kappa_int", q.kappa_int, np.float64),
                                ("c_p_lay", q.c_p_lay, np.float64), ("conv_layer", q.conv_layer, np.int32),
                                ("conv_unstable", q.conv_unstable, np.int32)):
                rt.set_state(c, name, np.asarray(v, dt))
            rt.set_state(c, "dampara", np.array([-1.0 if q.input_dampara == "automatic" else float(q.input_dampara)]))
            rt.set_state(c, "done", np.zeros(1, np.int32))
            rt.set_convergence_limit(c, q.rad_convergence_limit)
        if progress and c in active:
            print("\nConvectively unstable layers found. Starting convective adjustment")
        elif progress:
            print("\nAll layers convectively stable. No convective adjustment necessary.\n")
    live = list(active)
    it = 0
    while live:
        if progress and it % 100 == 0:
            for c in live:
                print("\nWe are running \"" + str(quants[c].name) + "\" at iteration step nr. : " + str(it))
        nxt = next_stop(it, q0.max_nr_iterations, q0.crit_relaxation_numbers, coupling_interval=_coupling_interval(q0))
        # (tabulated chemistry follows the temperatures on the device, ahead of the adjustment and for the adjusted profile:
        # k_rt_mmm_from_vmr and the refresh, computation.py:1030-1036, :1056-1061 -- no host step per decade)
        rt.conv_run(it, nxt - it)
        computer.report_diagnostics(q0)
        it = nxt
        done, at = _counts(rt, live, it)
        over = _between_iterations(computer, quants, rt, live, at, write, read)
        for c in live:
            iters[c] = at[c]
        live = [c for c in live if not (done[c] or c in over)]
    for c in active:
        q = quants[c]
        q.iter_value = np.int32(iters[c])
        q.conv_layer, q.conv_unstable = rt.get("conv_layer", c), rt.get("conv_unstable", c)
        q.marked_red = rt.get("marked_red", c)
        for n in ("kappa_lay", "kappa_int", "c_p_lay"):      # what the output files report
            setattr(q, n, rt.get(n, c))
    return iters
