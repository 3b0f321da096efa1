#!/usr/bin/env python3
"""`precision = single` against `double` on one workload, in one process: the same batch built twice, once with fp64 and
once with fp32 coefficient planes (hx_rt_flags.coef_fp32), the same iterations on each.  Prints one JSON line:

    python tools/precision_ab.py [--workload c2] [--steps 9]

per width: k_rt_flux and k_rt_coef averages (hx_rt_profile scopes "rt_flux" / "rt_coef"), ms per step (wall clock over
`steps` iterations without profiling), the traffic model's bytes per step and per refresh and the plane width in use; then
the flux kernel's single/double ratio and the largest differences between the two runs' spectral fluxes (F_up_wg,
relative to its largest value) and total fluxes (relative) after the same iterations."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def one_width(ctx, bench, c, steps):
    rt = bench.make_batch(ctx, c, 1)
    try:
        rt.build_planck_table(1)
        rt.run(0, 1)                     # the first solve: both widths from the same start
        first = {k: rt.get(k) for k in ("F_up_wg", "F_up_tot", "F_down_tot")}
        rt.run(1, 10)                    # the graph captures, ten iterations
        ctx.synchronize()
        t0 = time.perf_counter()
        rt.run(11, steps)                # refresh-free iterations (steps <= 9) or whole decades
        ctx.synchronize()
        ms_step = (time.perf_counter() - t0) * 1e3 / steps
        rt.profile(True)
        rt.run(11 + steps, 10)           # one decade from a refresh boundary or not: both kernels are in it
        rt.profile(False)
        flux = rt.profile_read("matrix_solve" if c.get("flux_calc_method") == "matrix" else "rt_flux")
        coef = rt.profile_read("rt_coef")
        tm = rt.traffic_model()
        out = {"coef_plane_bytes": rt.coef_plane_bytes(), "k_rt_flux_ms": flux[0], "k_rt_flux_launches": flux[1],
               "k_rt_coef_ms": coef[0], "k_rt_coef_launches": coef[1], "ms_per_step": ms_step,
               "traffic_model_step_bytes": tm["step_actual"], "traffic_model_refresh_bytes": tm["refresh_actual"]}
        fluxes = {k: rt.get(k) for k in ("F_up_wg", "F_up_tot", "F_down_tot")}
        return out, (first, fluxes)
    finally:
        rt.close()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--out", default="")
    a = ap.parse_args(argv)
    import bench
    from helios_amd.device import Context
    w = dict(bench.WORKLOADS[a.workload])
    c = bench.build_case(w, 20242, full_tables=False)
    ctx = Context(0)
    res = {"workload": a.workload, "desc": w["desc"], "gpu": ctx.name(), "steps": a.steps}
    runs = {}
    for prec in ("double", "single"):
        c.prec = prec                    # (read when the batch is created)
        res[prec], runs[prec] = one_width(ctx, bench, c, a.steps)
    def differences(d, s):
        spec = float(np.abs(s["F_up_wg"] - d["F_up_wg"]).max() / np.abs(d["F_up_wg"]).max())
        tot = float(max(np.max(np.abs(s[k] - d[k]) / np.maximum(np.abs(d[k]), 1e-300)) for k in ("F_up_tot", "F_down_tot")))
        return {"max_spectral_flux_difference (of the largest F_up_wg)": spec, "max_total_flux_difference (relative)": tot}
    # after the first solve (same temperatures on both sides: the planes' rounding alone), and after all iterations (the
    # temperature steps -- dT ~ |dF|^0.1 -- carry the difference into the trajectories)
    res["first_solve"] = differences(runs["double"][0], runs["single"][0])
    res["after_%d_iterations" % (21 + a.steps)] = differences(runs["double"][1], runs["single"][1])
    res["k_rt_flux_single_over_double"] = res["single"]["k_rt_flux_ms"] / res["double"]["k_rt_flux_ms"]
    res["step_single_over_double"] = res["single"]["ms_per_step"] / res["double"]["ms_per_step"]
    ctx.close()
    line = json.dumps(res)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return res


if __name__ == "__main__":
    main()
