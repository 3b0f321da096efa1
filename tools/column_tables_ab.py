#!/usr/bin/env python3
"""What one premixed table set per column costs, on one GPU.  Writes profiles/column_tables_ab.json (or --out):

    python tools/column_tables_ab.py [--parent DIR] [--runs 3] [--repeats 5]

1. `headline` (with --parent DIR, a built checkout of the parent commit): `python bench.py` -- the plain run, ms_per_step of
   config 2 -- here and in DIR, alternating, `--runs` fresh processes each.  The feature must not cost the headline: the
   two sets of runs are to overlap.
2. `batch`: eight columns of config 2's size (10 000 x 100 x 20) over FOUR table sets against the same eight columns over
   ONE, in this process, alternating, `--repeats` timings of five decades each (ms per iteration, the refresh's share
   included).  The bytes read per column are the same, so the two are expected to be equal within the spread of the
   one-table batch.  Also the set-up time of every additional table (its host array handed to
   RTBatch.add_premixed_tables: the host-to-device copy of 0.96 GB)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def bench_ms_per_step(root):
    """one plain bench.py run in a fresh process of the checkout `root`"""
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py")], cwd=root, capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise RuntimeError("bench.py in %s ended with status %d:\n%s" % (root, p.returncode, p.stderr[-2000:]))
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]
    return float(json.loads(line)["ms_per_step"])


def spread(v):
    v = [float(x) for x in v]
    return {"runs": v, "min": min(v), "max": max(v), "median": float(np.median(v))}


def headline(parent, runs):
    here, there = [], []
    for _ in range(runs):                 # alternating: drifts of the box fall on both
        there.append(bench_ms_per_step(parent))
        here.append(bench_ms_per_step(ROOT))
    out = {"this_commit_ms_per_step": spread(here), "parent_ms_per_step": spread(there)}
    out["overlap"] = bool(out["this_commit_ms_per_step"]["min"] <= out["parent_ms_per_step"]["max"]
                          and out["parent_ms_per_step"]["min"] <= out["this_commit_ms_per_step"]["max"])
    return out


def batch(repeats, ncol=8, ntab=4):
    import bench
    from helios_amd import synthetic as syn
    from helios_amd.device import Context
    c = bench.build_case(dict(bench.WORKLOADS["c2"]), 20242, full_tables=False)
    ctx = Context(0)
    setup = []

    def make(ntables):
        rt = bench.make_batch(ctx, c, ncol, sweep=True)
        for t in range(1, ntables):
            # another chemistry on the same grid: its own k-table, Rayleigh cross-sections and mean molecular mass
            k = syn.ktable(np.random.default_rng(20242 + t), c.nbin, c.ny, c.ktemp, c.kpress, c.gauss_y) * (1.0 + t)
            ctx.synchronize()
            t0 = time.perf_counter()
            rt.add_premixed_tables(k, c.opac_scat_cross * (1.0 + 0.5 * t), c.opac_meanmass * (1.0 + 0.1 * t))
            ctx.synchronize()
            setup.append(time.perf_counter() - t0)
            del k
        for col in range(ncol):
            rt.set_column_table(col, col % ntables)
        rt.build_planck_table(1)
        rt.run(0, 20)                     # two decades: both graphs captured
        return rt

    one, four = make(1), make(ntab)
    ms = {"one_table": [], "four_tables": []}
    it = 20
    try:
        for _ in range(repeats):
            for name, rt in (("one_table", one), ("four_tables", four)):
                ctx.synchronize()
                t0 = time.perf_counter()
                rt.run(it, 50)            # five refreshes and fifty iterations
                ctx.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / 50)
            it += 50
        builds = {"one_table": [int(v) for v in one.get("graph_builds")], "four_tables": [int(v) for v in four.get("graph_builds")]}
    finally:
        one.close()
        four.close()
        ctx.close()
    return {"columns": ncol, "nbin": int(c.nbin), "nlayer": int(c.nlayer), "ny": int(c.ny),
            "ms_per_iteration_per_batch": {k: spread(v) for k, v in ms.items()},
            "graph_builds": builds, "setup_s_per_additional_table": spread(setup),
            "table_bytes": int(c.ntemp * c.npress * c.nbin * (c.ny + 1) * 8 + c.ntemp * c.npress * 8)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="a checkout of the parent commit with its library built (for `headline`)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--skip-batch", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "column_tables_ab.json"))
    a = ap.parse_args(argv)
    rec = {}
    if os.path.exists(a.out):             # the two parts may be measured in separate calls
        with open(a.out) as f:
            rec = json.load(f)
    if a.parent:
        rec["headline"] = headline(os.path.abspath(a.parent), a.runs)
    if not a.skip_batch:
        rec["batch"] = batch(a.repeats)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
