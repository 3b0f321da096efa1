#!/usr/bin/env python3
"""Writes profiles/ro_ny_bench.json: the species loop of one opacity refresh (k_rt_mix_species at 20 Gauss points,
k_rt_species_mix_ny below) at BASELINE config 3's grid and species count as bench.py defines them, with synthetic tables of
8, 10, 16 and 20 Gauss points.

    python tools/ro_ny_bench.py [--parent-lib PATH/libhelios_hip.so] [--ny 8,10,16,20] [--out profiles/ro_ny_bench.json]

Per number of Gauss points: HIP-event time of the species loop per refresh (the batch's own `add_to_mixed_opac` scope), the
median of seven refreshes behind a warm-up one, all in one process.  --parent-lib: the same measurement at 20 points with
another build of the library (the commit before the general mixer), in a child process of its own -- that code path is
unchanged, so the two figures should sit inside the run-to-run spread."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 7


def measure(ny):
    import bench
    from helios_amd.device import Context
    w = dict(bench.WORKLOADS["c3"], ny=ny)
    c = bench.build_case(w, 0, full_tables=False)
    ctx = Context(0)
    rt = bench.make_batch(ctx, c, 1)
    try:
        rt.build_planck_table(1 if c.T_star > 10 else 0)
        rt.profile(True)
        times, total = [], 0.0
        for r in range(RUNS + 1):
            rt.refresh()
            avg, n = rt.profile_read("add_to_mixed_opac")
            times.append(avg * n - total)
            total = avg * n
        times = times[1:]
        opac = rt.get("opac_wg_lay")
        assert np.all(np.isfinite(opac)) and opac.min() > 0
        return dict(ny=ny, species_loop_ms=float(np.median(times)), min_ms=float(min(times)), max_ms=float(max(times)),
                    device=ctx.name())
    finally:
        rt.close()
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ny", default="8,10,16,20")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ro_ny_bench.json"))
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        # another build of the library (HELIOS_HIP_LIB): bind what it exports -- entry points added since are not called here
        import ctypes
        from helios_amd import _lib
        raw = ctypes.CDLL(_lib.LIB_PATH)
        _lib._protos = {k: v for k, v in _lib.prototypes().items() if hasattr(raw, k)}
        print("RESULT " + json.dumps(measure(20)))
        return
    rows = [measure(int(v)) for v in a.ny.split(",")]
    at20 = [r for r in rows if r["ny"] == 20]
    for r in rows:
        if at20:
            r["ratio_to_20"] = r["species_loop_ms"] / at20[0]["species_loop_ms"]
        print("ny = %2d: %.2f ms per refresh (%.2f ... %.2f)%s" % (r["ny"], r["species_loop_ms"], r["min_ms"], r["max_ms"],
                                                                  "  = %.2f of ny = 20" % r["ratio_to_20"] if at20 else ""))
    import bench
    w = bench.WORKLOADS["c3"]
    out = dict(case="%d bins x %d layers, %d absorbers mixed by random overlap (bench.py c3), one refresh"
                    % (w["nbin"], w["nlayer"], w["nspecies"]),
               runs=RUNS, statistic="median of %d refreshes behind a warm-up, HIP events around the species loop" % RUNS, rows=rows)
    if a.parent_lib:
        env = dict(os.environ, HELIOS_HIP_LIB=os.path.abspath(a.parent_lib))
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=env, capture_output=True, text=True,
                           timeout=900)
        if p.returncode != 0:
            raise SystemExit("the parent library's run failed:\n" + p.stderr[-2000:])
        out["parent_library_ny20"] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print("ny = 20, parent library: %.2f ms per refresh (%.2f ... %.2f)"
              % tuple(out["parent_library_ny20"][k] for k in ("species_loop_ms", "min_ms", "max_ms")))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
