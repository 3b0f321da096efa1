#!/usr/bin/env python3
"""Writes profiles/exomol_bench.json: a synthetic ExoMol list of 1e5 states and 1e7 transitions over 0 - 30000 cm^-1, written to
`.states` / `.trans` files and read back, at dnu = 0.01 cm^-1 with a cut-off of 25 cm^-1 and two broadeners, at 500 K and 2000 K x
two pressures in one launch of four nodes, with S_min = 0 and S_min = 1e-30.

Recorded: the host's seconds for parsing and for sorting, apart; per node the fraction kept and the pairs (line, point) evaluated,
which is arithmetic on the kept nu_0; by HIP events (hx_exomol_get("timing_ms")) the ms in count + scan + prepare + ranges and in
the sum, medians of seven launches behind a warm-up, in one process.  The baseline is existing code: the same list converted to
lines.py's seven fields (s_ref = S(296), gamma_air = 1.01325 sum_b x_b gamma_b, n_air = the first broadener's n, delta_air = 0)
goes through hx_lines_* with the same four nodes per launch, alternating with the S_min = 0 launches: k_lines_prepare_nodes
against the new prepare path, k_lines_sum_nodes against the new sum.  The numpy backend computes one node on every tenth
transition.

    python tools/exomol_bench.py [--out FILE] [--no-numpy] [--states N] [--transitions N] [--rehearse]
"""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 7
TEMPS, PRESSURES = (500.0, 2000.0), (1e3, 1e6)                 # K; dyne cm^-2 (n300, p000)
GRID = (0.0, 0.01, 3000000)
CUTOFF = 25.0
MOLAR_MASS = 18.0153
S_MINS = (0.0, 1e-30)
J_MAX = 60


def synthetic(n_states, n_trans, seed=1):
    """states with E ascending in 0 ... 30000 cm^-1, and transitions between random pairs of them, upper above lower"""
    rng = np.random.default_rng(seed)
    j = rng.integers(0, J_MAX + 1, n_states).astype(np.float64)
    states = {"E": np.sort(rng.uniform(0.0, 30000.0, n_states)), "g": 2.0 * j + 1.0, "J": j, "jidx": (2 * j).astype(np.int32)}
    a, b = rng.integers(0, n_states, n_trans), rng.integers(0, n_states - 1, n_trans)
    b = b + (b >= a)                                               # never the same state
    return states, (np.maximum(a, b), np.minimum(a, b), 10.0 ** rng.uniform(-6.0, 2.0, n_trans))


def write_files(wd, states, raw):
    st, tr = os.path.join(wd, "bench.states"), os.path.join(wd, "bench.trans")
    ids = np.arange(1, len(states["E"]) + 1)
    np.savetxt(st, np.column_stack([ids, states["E"], states["g"], states["J"]]), fmt="%12d %.17g %d %g")
    with open(tr, "w") as f:
        for lo in range(0, len(raw[0]), 1 << 20):
            sl = slice(lo, lo + (1 << 20))
            f.write("".join("%12d %12d %.10e\n" % row for row in zip((raw[0][sl] + 1).tolist(), (raw[1][sl] + 1).tolist(), raw[2][sl].tolist())))
    return st, tr


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return {"median": float(np.median(ms[1:])), "min": float(ms[1:].min()), "max": float(ms[1:].max()), "warm_up": float(ms[0])}


def main(argv):
    from helios_amd import exomol, lines
    n_states = int(argv[argv.index("--states") + 1]) if "--states" in argv else 100000
    n_trans = int(argv[argv.index("--transitions") + 1]) if "--transitions" in argv else 10000000
    states, raw = synthetic(n_states, n_trans)
    out = {"case": "%d states, %d transitions over 0 - 30000 cm^-1, dnu = %g, cut-off %g cm^-1, two broadeners, %d nodes in one launch"
                   % (n_states, n_trans, GRID[1], CUTOFF, len(TEMPS) * len(PRESSURES)),
           "points": GRID[2], "runs": RUNS, "compact_block": exomol.COMPACT_BLOCK, "tile_points": exomol.TILE_POINTS, "host": {}}
    with tempfile.TemporaryDirectory() as wd:
        t0 = time.time()
        st, tr = write_files(wd, states, raw)
        out["host"]["writing_the_files_seconds"] = time.time() - t0
        out["host"]["trans_file_bytes"] = os.path.getsize(tr)
        t0 = time.time()
        states = exomol.read_states(st)
        out["host"]["parsing_states_seconds"] = time.time() - t0
        t0 = time.time()
        v = exomol._transition_columns(tr, n_states)
        out["host"]["parsing_transitions_seconds"] = time.time() - t0
    t0 = time.time()
    trans, skipped = exomol.sort_transitions({"up": v[:, 0].astype(np.int64) - 1, "low": v[:, 1].astype(np.int64) - 1, "A": v[:, 2]}, states)
    out["host"]["gather_and_sort_seconds"] = time.time() - t0
    del v
    n = len(trans["nu0"])
    out["transitions_after_skipping"] = n
    rng = np.random.default_rng(2)
    rows = [dict((j, (float(rng.uniform(0.02, 0.12)), float(e + rng.uniform(-0.05, 0.05)))) for j in range(2 * J_MAX + 1))
            for e in (0.45, 0.25)]
    broadening = exomol.broadening_table([("H2", 0.85, rows[0], 0.07, 0.5), ("He", 0.15, rows[1], 0.03, 0.3)], int(states["jidx"].max()))
    t = np.arange(50.0, 3001.0, 50.0)
    q_table = (t, t ** 1.5)
    nodes = [(temp, p, lines.partition_value(q_table, temp)) for temp in TEMPS for p in PRESSURES]
    labels = ["%g K, %g dyne cm^-2" % n_[:2] for n_ in nodes]
    # what the counts must be, and the pairs: arithmetic on the host
    expected = {}
    for s_min in S_MINS:
        expected[s_min] = []
        for temp, p, q_t in nodes:
            kept = exomol.strengths(states, trans, temp, q_t) >= s_min
            expected[s_min].append((int(kept.sum()), lines.count_pairs(trans["nu0"][kept], GRID[0], GRID[1], GRID[2], CUTOFF)))
    # the baseline's seven fields
    x, table = broadening
    jx = states["jidx"][trans["low"]]
    q_ref = lines.partition_value(q_table, lines.T_REF)
    line = {"nu0": trans["nu0"], "s_ref": exomol.strengths(states, trans, lines.T_REF, q_ref),
            "gamma_air": 1.01325 * (x[0] * table[0, jx, 0] + x[1] * table[1, jx, 0]), "gamma_self": np.zeros(n),
            "e_low": states["E"][trans["low"]], "n_air": table[0, jx, 1].copy(), "delta_air": np.zeros(n)}
    if "--rehearse" in argv:
        print(json.dumps(dict(out, expected=dict((str(k), v_) for k, v_ in expected.items())), indent=1, sort_keys=True))
        return
    from helios_amd.device import Context
    ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    out["device"] = ctx.name()
    h = base = None
    arrays = ([n_[0] for n_ in nodes], [n_[1] for n_ in nodes], [n_[2] for n_ in nodes])
    try:
        h = exomol.ExomolOpacity.of(ctx, states, trans, broadening, GRID[2], len(nodes), len(nodes))
        base = lines.LineOpacity(ctx, n, GRID[2], len(nodes), len(nodes))
        base.set_lines(line)
        out["runs_by_s_min"] = {}
        for s_min in S_MINS:
            ms, ms_base = [], []
            for r in range(RUNS + 1):                 # the first run is the warm-up; set_nodes starts the sums of timing_ms anew
                h.set_nodes(*(arrays + (MOLAR_MASS, CUTOFF, s_min) + GRID))
                h.run_nodes(0, len(nodes))
                ms.append(h.get("timing_ms"))
                if s_min == 0.0:                      # alternating with the baseline
                    base.set_nodes(*(arrays + (q_ref, MOLAR_MASS, 0.0, CUTOFF) + GRID))
                    base.run_nodes(0, len(nodes))
                    ms_base.append(base.get("timing_ms"))
            ms = np.array(ms)
            kept = h.get("kept")
            row_agrees = kept.tolist() == [e[0] for e in expected[s_min]]      # the host's strengths decide the same set
            pairs = [e[1] for e in expected[s_min]]
            row = {"nodes": dict((label, {"kept": int(k), "kept_fraction": int(k) / n, "pairs": int(p)})
                                 for label, k, p in zip(labels, kept, pairs)),
                   "kept_equals_the_numpy_strengths_count": bool(row_agrees), "pairs_of_the_launch": int(sum(pairs)), "count_scan_prepare_ranges_ms": stats(ms[:, 0]), "k_exomol_sum_ms": stats(ms[:, 1])}
            row["pairs_per_second"] = sum(pairs) / (row["k_exomol_sum_ms"]["median"] * 1e-3)
            if ms_base:
                ms_base = np.array(ms_base)
                row["baseline"] = {"k_lines_prepare_nodes_ms": stats(ms_base[:, 0]), "k_lines_sum_nodes_ms": stats(ms_base[:, 1]),
                                   "pairs_of_the_launch": int(sum(pairs))}
            out["runs_by_s_min"]["%g" % s_min] = row
    finally:
        for obj in (h, base):
            if obj is not None:
                obj.close()
        ctx.close()
    if "--no-numpy" not in argv:
        tenth = dict((k, np.ascontiguousarray(trans[k][::10])) for k in trans)
        temp, p, q_t = nodes[-1]
        timing = {}
        t0 = time.time()
        exomol.exomol_opacity(states, tenth, broadening, q_table, [temp], [p], GRID, MOLAR_MASS, CUTOFF, S_MINS[1], backend="numpy",
                              timing=timing)
        out["numpy_backend"] = {"node": labels[-1], "s_min": S_MINS[1], "transitions": len(tenth["nu0"]), "kept": int(timing["kept"][0, 0]),
                                "pairs": int(timing["pairs"]), "seconds": time.time() - t0,
                                "threads": int(os.environ.get("OMP_NUM_THREADS", "0")) or None}
    path = os.path.join(ROOT, "profiles", "exomol_bench.json")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
