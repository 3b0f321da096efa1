#!/usr/bin/env python3
"""Writes profiles/lines_bench.json: a synthetic list of 1e5 lines over 0 - 30000 cm^-1 at dnu = 0.01 cm^-1 with a cut-off of
25 cm^-1, at one low-pressure and one high-pressure node, one node per launch with fp64 rows.  k_lines_prepare_nodes and
k_lines_sum_nodes_fp64 by HIP events (hx_lines_get("timing_ms"); the keys keep the names k_lines_prepare_ms and k_lines_sum_ms of
the single-node kernels they replace), the median of seven runs behind a warm-up, in one process; the pairs (line, point) evaluated, which
is arithmetic, and from them the pairs per second; the numpy backend on the same node with OMP_NUM_THREADS as set, which also
counts the pairs per region of |z|.

    python tools/lines_bench.py [--out FILE] [--no-numpy] [--lines N]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 7
NODES = (("low_pressure", 1000.0, 1e3), ("high_pressure", 1000.0, 1e8))        # K, dyne cm^-2
GRID = (0.0, 0.01, 3000000)
CUTOFF = 25.0
MOLAR_MASS = 18.0153
REGIONS = ("weideman", "eight_levels", "four_levels", "two_levels")


def synthetic_list(n, seed=1):
    rng = np.random.default_rng(seed)
    return dict(nu0=np.sort(rng.uniform(1.0, 30000.0, n)), s_ref=10.0 ** rng.uniform(-28.0, -19.0, n),
                gamma_air=rng.uniform(0.01, 0.1, n), gamma_self=rng.uniform(0.1, 0.5, n), e_low=rng.uniform(0.0, 5000.0, n),
                n_air=rng.uniform(0.4, 0.8, n), delta_air=rng.uniform(-0.01, 0.01, n))


def main(argv):
    from helios_amd import lines
    from helios_amd.device import Context
    n_lines = int(argv[argv.index("--lines") + 1]) if "--lines" in argv else 100000
    line = synthetic_list(n_lines)
    t = np.arange(50.0, 3001.0, 50.0)
    q_table = (t, t ** 1.5)
    q_ref = lines.partition_value(q_table, lines.T_REF)
    out = {"case": "%d lines over 0 - 30000 cm^-1, dnu = %g, cut-off %g cm^-1" % (n_lines, GRID[1], CUTOFF), "lines": n_lines,
           "points": GRID[2], "runs": RUNS, "tile_points": lines.TILE_POINTS, "lds_block": lines.LDS_BLOCK, "nodes": {}}
    ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    out["device"] = ctx.name()
    h = lines.LineOpacity(ctx, n_lines, GRID[2], 1, 1, with_fp64=True)
    kept = {}
    try:
        h.set_lines(line)
        for label, temp, press in NODES:
            q_t = lines.partition_value(q_table, temp)
            ms = []
            for r in range(RUNS + 1):                 # the first run is the warm-up; set_nodes sets the times to zero
                h.set_nodes([temp], [press], [q_t], q_ref, MOLAR_MASS, 0.0, CUTOFF, *GRID)
                h.run_nodes(0, 1)
                ms.append(h.get("timing_ms"))
            ms = np.array(ms)
            pairs = lines.count_pairs(h.get("line_params")[0][0], GRID[0], GRID[1], GRID[2], CUTOFF)
            kept[label] = h.get("kappa64")[0]
            med = np.median(ms[1:], axis=0)
            out["nodes"][label] = {"temperature": temp, "pressure": press, "pairs": pairs,
                                   "k_lines_prepare_ms": {"median": float(med[0]), "min": float(ms[1:, 0].min()),
                                                          "max": float(ms[1:, 0].max()), "warm_up": float(ms[0, 0])},
                                   "k_lines_sum_ms": {"median": float(med[1]), "min": float(ms[1:, 1].min()),
                                                      "max": float(ms[1:, 1].max()), "warm_up": float(ms[0, 1])},
                                   "pairs_per_second": pairs / (float(med[1]) * 1e-3)}
    finally:
        h.close()
        ctx.close()
    if "--no-numpy" not in argv:
        out["numpy_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
        for label, temp, press in NODES:
            timing = {}
            t0 = time.time()
            ref = lines.line_opacity(line, q_table, [temp], [press], GRID, MOLAR_MASS, 0.0, CUTOFF, backend="numpy", timing=timing)[0, 0]
            node = out["nodes"][label]
            node["numpy_seconds"] = time.time() - t0
            node["numpy_pairs_per_second"] = timing["pairs"] / node["numpy_seconds"]
            node["pairs_counted_by_numpy"] = int(timing["pairs"])
            node["share_of_pairs_per_region"] = dict((name, float(c) / timing["pairs"])
                                                     for name, c in zip(REGIONS, timing["pairs_by_region"]))
            with np.errstate(divide="ignore", invalid="ignore"):
                dev = np.abs(kept[label] / ref - 1)
            node["device_vs_numpy"] = float(np.nanmax(np.where(ref > 0, dev, 0.0)))
    path = os.path.join(ROOT, "profiles", "lines_bench.json")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
