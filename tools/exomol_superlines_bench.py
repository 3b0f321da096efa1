#!/usr/bin/env python3
"""Writes profiles/exomol_superlines_bench.json: the case of tools/exomol_bench.py (1e5 states, 1e7 transitions over 0 - 30000
cm^-1, dnu = 0.01 cm^-1, cut-off 25 cm^-1, two broadeners, 500 K and 2000 K x two pressures in one launch of four nodes, S_min = 0)
in plain mode and with super-lines at two thresholds, cells of -dnu.

In one process, the modes alternating launch by launch behind a warm-up of each: by HIP events (hx_exomol_get("timing_ms")) the
ms before the sum (count ... ranges, or classify ... ranges) and in the sum, medians of seven.  Per threshold and node: the share
of the transitions that is weak, the counts (which the device's "superline_counts" must equal), the pairs (list entry, point)
of the launch -- arithmetic on the host from the same classes and cells.  From the fp32 slabs: the largest and the median
relative deviation of kappa from the plain result over the points where that is above 0; and the same for the entries of the
k-table at R = 50 with 20 Gauss points (exomol_ktable on the device, once per mode).

    python tools/exomol_superlines_bench.py [--out FILE] [--states N] [--transitions N] [--no-ktable]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

THRESHOLDS = (1e-24, 1e-21)                    # cm / molecule


def deviation(got, plain):
    lit = plain > 0
    rel = np.abs(got[lit].astype(np.float64) / plain[lit].astype(np.float64) - 1.0)
    return {"largest": float(rel.max()), "median": float(np.median(rel)), "entries": int(lit.sum())}


def main(argv):
    import exomol_bench as eb
    from helios_amd import exomol, ktable, lines
    from helios_amd.device import Context
    n_states = int(argv[argv.index("--states") + 1]) if "--states" in argv else 100000
    n_trans = int(argv[argv.index("--transitions") + 1]) if "--transitions" in argv else 10000000
    grid, cutoff, step = eb.GRID, eb.CUTOFF, eb.GRID[1]
    states, raw = eb.synthetic(n_states, n_trans)
    trans, _ = exomol.sort_transitions({"up": raw[0], "low": raw[1], "A": raw[2]}, states)
    n = len(trans["nu0"])
    rng = np.random.default_rng(2)
    rows = [dict((j, (float(rng.uniform(0.02, 0.12)), float(e + rng.uniform(-0.05, 0.05)))) for j in range(2 * eb.J_MAX + 1))
            for e in (0.45, 0.25)]
    broadening = exomol.broadening_table([("H2", 0.85, rows[0], 0.07, 0.5), ("He", 0.15, rows[1], 0.03, 0.3)], int(states["jidx"].max()))
    t = np.arange(50.0, 3001.0, 50.0)
    q_table = (t, t ** 1.5)
    nodes = [(temp, p, lines.partition_value(q_table, temp)) for temp in eb.TEMPS for p in eb.PRESSURES]
    labels = ["%g K, %g dyne cm^-2" % n_[:2] for n_ in nodes]
    arrays = ([n_[0] for n_ in nodes], [n_[1] for n_ in nodes], [n_[2] for n_ in nodes])
    out = {"case": "%d states, %d transitions over 0 - 30000 cm^-1, dnu = %g, cut-off %g cm^-1, two broadeners, %d nodes in one launch, "
                   "S_min = 0, super-line step %g cm^-1" % (n_states, n_trans, grid[1], cutoff, len(nodes), step),
           "transitions_after_skipping": n, "points": grid[2], "runs": eb.RUNS, "thresholds": list(THRESHOLDS)}
    # classes, cells and pairs: arithmetic on the host
    cell = np.floor(trans["nu0"] / step).astype(np.int64)
    plain_pairs = lines.count_pairs(trans["nu0"], grid[0], grid[1], grid[2], cutoff)
    expected = dict((s_sl, []) for s_sl in THRESHOLDS)
    for temp, p, q_t in nodes:
        s = exomol.strengths(states, trans, temp, q_t)
        for s_sl in THRESHOLDS:
            weak = s < s_sl
            centres = (np.unique(cell[weak]).astype(np.float64) + 0.5) * step
            listed = np.concatenate([trans["nu0"][~weak], centres])
            expected[s_sl].append({"strong": int(n - weak.sum()), "weak": int(weak.sum()), "superlines": len(centres),
                                   "weak_share": float(weak.mean()), "weak_share_of_the_strength": float(s[weak].sum() / s.sum()),
                                   "pairs": lines.count_pairs(listed, grid[0], grid[1], grid[2], cutoff)})
    ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    out["device"] = ctx.name()
    modes = [None] + list(THRESHOLDS)
    ms = dict((m, []) for m in modes)
    slabs, counts = {}, {}
    h = None
    try:
        h = exomol.ExomolOpacity.of(ctx, states, trans, broadening, grid[2], len(nodes), len(nodes))
        for r in range(eb.RUNS + 1):                   # the first run of each mode is its warm-up
            for m in modes:
                h.set_superlines(m, None if m is None else step)
                h.set_nodes(*(arrays + (eb.MOLAR_MASS, cutoff, 0.0) + grid))
                h.run_nodes(0, len(nodes))
                ms[m].append(h.get("timing_ms"))
                if r == eb.RUNS:
                    slabs[m] = h.get("slabs32")
                    counts[m] = h.get("kept").tolist() if m is None else h.get("superline_counts").tolist()
    finally:
        if h is not None:
            h.close()
    out["modes"] = {}
    for m in modes:
        t_ms = np.array(ms[m])
        row = {"before_the_sum_ms": eb.stats(t_ms[:, 0]), "k_exomol_sum_ms": eb.stats(t_ms[:, 1])}
        if m is None:
            row["nodes"] = dict((label, {"kept": int(k), "pairs": int(plain_pairs)}) for label, k in zip(labels, counts[m]))
            row["pairs_of_the_launch"] = int(plain_pairs) * len(nodes)
        else:
            row["nodes"] = dict((label, dict(e, kappa_against_plain=deviation(slabs[m][i], slabs[None][i])))
                                for i, (label, e) in enumerate(zip(labels, expected[m])))
            row["counts_equal_the_hosts"] = [list(c) for c in counts[m]] == [[e["strong"], e["weak"], e["superlines"]]
                                                                            for e in expected[m]]
            row["pairs_of_the_launch"] = int(sum(e["pairs"] for e in expected[m]))
        row["pairs_per_second"] = row["pairs_of_the_launch"] / (row["k_exomol_sum_ms"]["median"] * 1e-3)
        out["modes"]["plain" if m is None else "S_sl = %g" % m] = row
    plain = out["modes"]["plain"]
    for m in THRESHOLDS:
        row = out["modes"]["S_sl = %g" % m]
        row["pairs_against_plain"] = row["pairs_of_the_launch"] / plain["pairs_of_the_launch"]
        row["sum_ms_against_plain"] = row["k_exomol_sum_ms"]["median"] / plain["k_exomol_sum_ms"]["median"]
    del slabs
    if "--no-ktable" not in argv:
        inter = ktable.wavelength_grid("fixed_resolution", "50 0.34 200".split())
        tables = {}
        for m in modes:
            native, _ = exomol.exomol_ktable(states, trans, broadening, q_table, [int(v) for v in eb.TEMPS], ["n300", "p000"], 30000,
                                             grid[1], inter, 20, eb.MOLAR_MASS, cutoff, 0.0, None, "device", ctx, len(nodes),
                                             superline_threshold=m, superline_step=None if m is None else step)
            tables[m] = np.asarray(native["kpoints"], np.float64).reshape(-1)
        for m in THRESHOLDS:
            out["modes"]["S_sl = %g" % m]["ktable_R50_20_points_against_plain"] = deviation(tables[m], tables[None])
    ctx.close()
    path = os.path.join(ROOT, "profiles", "exomol_superlines_bench.json")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
