#!/usr/bin/env python3
"""Writes profiles/lines_ktable_bench.json: from a line list to the species' k-table by the two routes -- `lines.py` (files) followed
by `ktable.py`, and `lines.py -ktable yes` -- on tools/lines_bench.py's synthetic list of 1e5 lines over 0 - 30000 cm^-1 at
dnu = 0.01 cm^-1 (3e6 points, cut-off 25 cm^-1), 322 bins x 20 Gauss points, 4 temperatures x 4 pressure codes.  The two-step
route puts 16 files of 12 MB, 192 MB, into the machine's temporary directory; they are removed at the end.

One process.  (a) the whole routes, lines.main + ktable.main against lines.main -ktable yes, by the wall clock, alternating,
medians of five behind a warm-up of each; both read the same `.par` file, whose parsing is part of both.  (b) k_lines_sum_nodes_fp64
per node (one node per launch, the 16 nodes one after the other; the keys keep the name k_lines_sum of the single-node kernel it
replaces) and k_lines_sum_nodes per node (four nodes per launch) by HIP events, seven repeats behind a warm-up, and the spread of
the former's repeats.  (c) the bytes each route moves across PCIe and the disk:
arithmetic on the array shapes, not a measurement.  (d) whether the two routes' tables are equal to the bit.

    python tools/lines_ktable_bench.py [--out FILE] [--lines N]
"""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROUTE_RUNS, KERNEL_RUNS = 5, 7
TEMPS, CODES = "500 1000 1500 2000", "n300 n100 p000 p200"
NUMAX, DNU, CUTOFF = 30000, 0.01, 25.0
GRID, N_GAUSS, PER_LAUNCH = "50 0.34 200", 20, 4
MOLAR_MASS = 18.0153


def quiet(fn, argv):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(argv)


def main(argv):
    import lines_cases as lc
    from lines_bench import synthetic_list
    from helios_amd import _nodes, ktable, lines
    from helios_amd.device import Context
    n_lines = int(argv[argv.index("--lines") + 1]) if "--lines" in argv else 100000
    n_points = _nodes.chunk_limits("lines", 0, NUMAX, DNU)[0][2]
    temps, codes = [int(t) for t in TEMPS.split()], CODES.split()
    n_nodes = len(temps) * len(codes)
    inter = ktable.wavelength_grid("fixed_resolution", GRID.split())
    n_bins = len(inter) - 1
    out = {"case": "%d lines over 0 - %d cm^-1, dnu = %g, cut-off %g cm^-1, %d bins x %d Gauss points, %d x %d nodes, %d nodes per "
                   "launch" % (n_lines, NUMAX, DNU, CUTOFF, n_bins, N_GAUSS, len(temps), len(codes), PER_LAUNCH),
           "lines": n_lines, "points": n_points, "nodes": n_nodes, "bins": n_bins, "gauss_points": N_GAUSS,
           "route_runs": ROUTE_RUNS, "kernel_runs": KERNEL_RUNS}
    wd = tempfile.mkdtemp(prefix="lines_ktable_bench_")
    try:
        line = synthetic_list(n_lines)
        lc.write_par_file(os.path.join(wd, "list.par"), line)
        t = np.arange(50.0, 3001.0, 50.0)
        lc.write_q_file(os.path.join(wd, "q.txt"), (t, t ** 1.5))
        with open(os.path.join(wd, "species.dat"), "w") as f:
            f.write("species path\nH2O %s\n" % os.path.join(wd, "opac"))
        common = ["-name", "H2O", "-line_list", os.path.join(wd, "list.par"), "-partition_function", os.path.join(wd, "q.txt"),
                  "-temperatures", TEMPS, "-pressure_codes", CODES, "-numax", str(NUMAX), "-dnu", repr(DNU), "-cutoff", repr(CUTOFF),
                  "-molar_mass", repr(MOLAR_MASS)]
        table = ["-wavelength_grid", GRID, "-number_of_gaussian_points", str(N_GAUSS), "-container", "npz", "-interpolate", "no"]

        def two_step():
            t0 = time.time()
            quiet(lines.main, common + ["-output_directory", os.path.join(wd, "opac")])
            t1 = time.time()
            quiet(ktable.main, ["-path_to_individual_species_file", os.path.join(wd, "species.dat"),
                                "-directory_with_individual_files", os.path.join(wd, "two_step"), "-points_per_launch",
                                str(PER_LAUNCH)] + table)
            return time.time() - t0, t1 - t0

        def fused():
            t0 = time.time()
            quiet(lines.main, common + ["-ktable", "yes", "-directory_with_individual_files", os.path.join(wd, "fused"),
                                        "-nodes_per_launch", str(PER_LAUNCH)] + table)
            return time.time() - t0

        # ---- (a) the whole routes
        warm = {"two_step_seconds": two_step()[0], "fused_seconds": fused()}
        a, b = [], []
        for _ in range(ROUTE_RUNS):
            a.append(two_step())
            b.append(fused())
        a, b = np.array(a), np.array(b)
        out["routes"] = {"warm_up": warm,
                         "two_step_seconds": {"median": float(np.median(a[:, 0])), "min": float(a[:, 0].min()), "max": float(a[:, 0].max()),
                                              "of_which_lines_main_median": float(np.median(a[:, 1]))},
                         "fused_seconds": {"median": float(np.median(b)), "min": float(b.min()), "max": float(b.max())},
                         "two_step_over_fused": float(np.median(a[:, 0]) / np.median(b))}

        # ---- (d) the tables
        with np.load(os.path.join(wd, "two_step", "H2O_opac_kdistr.npz")) as x, np.load(os.path.join(wd, "fused", "H2O_opac_kdistr.npz")) as y:
            out["tables_equal_to_the_bit"] = bool(sorted(x.files) == sorted(y.files) and all(x[k].tobytes() == y[k].tobytes() for k in x.files))
            out["kpoints_min_max"] = [float(y["kpoints"].min()), float(y["kpoints"].max())]
        out["opacity_files_bytes"] = sum(os.path.getsize(os.path.join(wd, "opac", f)) for f in os.listdir(os.path.join(wd, "opac")))

        # ---- (b) the two sum kernels by HIP events
        line, _ = lines.read_line_list(os.path.join(wd, "list.par"))           # as the routes see it
        q_table = (t, t ** 1.5)
        q_ref = lines.partition_value(q_table, lines.T_REF)
        press = sorted(ktable.pressure_table()[c] for c in codes)
        nodes = [(float(tt), p, lines.partition_value(q_table, tt)) for tt in sorted(temps) for p in press]
        ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
        out["device"] = ctx.name()
        single, batch = np.zeros((KERNEL_RUNS + 1, n_nodes, 2)), np.zeros((KERNEL_RUNS + 1, 2))
        try:
            h = lines.LineOpacity.of(ctx, line, n_points, 1, 1, True)
            try:
                for r in range(KERNEL_RUNS + 1):               # the first repeat is the warm-up
                    for k, (tt, p, q) in enumerate(nodes):
                        h.set_nodes([tt], [p], [q], q_ref, MOLAR_MASS, 0.0, CUTOFF, 0.0, DNU, n_points)
                        h.run_nodes(0, 1)
                        single[r, k] = h.get("timing_ms")
            finally:
                h.close()
            h = lines.LineOpacity.of(ctx, line, n_points, PER_LAUNCH, n_nodes)
            try:
                for r in range(KERNEL_RUNS + 1):
                    h.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], [n[2] for n in nodes], q_ref, MOLAR_MASS, 0.0, CUTOFF,
                                0.0, DNU, n_points)
                    for first in range(0, n_nodes, PER_LAUNCH):
                        h.run_nodes(first, min(PER_LAUNCH, n_nodes - first))
                    batch[r] = h.get("timing_ms") / n_nodes
            finally:
                h.close()
        finally:
            ctx.close()
        per_repeat = single[1:, :, 1].mean(axis=1)          # ms per node, the 16 nodes averaged, per repeat
        out["k_lines_sum_ms_per_node"] = {"median": float(np.median(per_repeat)), "min": float(per_repeat.min()),
                                          "max": float(per_repeat.max()), "spread": float(per_repeat.max() - per_repeat.min()),
                                          "warm_up": float(single[0, :, 1].mean()),
                                          "per_node_median": np.median(single[1:, :, 1], axis=0).tolist()}
        out["k_lines_sum_nodes_ms_per_node"] = {"median": float(np.median(batch[1:, 1])), "min": float(batch[1:, 1].min()),
                                                "max": float(batch[1:, 1].max()), "warm_up": float(batch[0, 1])}
        out["k_lines_prepare_ms_per_node"] = float(np.median(single[1:, :, 0].mean(axis=1)))
        out["k_lines_prepare_nodes_ms_per_node"] = float(np.median(batch[1:, 0]))
        slower = out["k_lines_sum_nodes_ms_per_node"]["median"] - out["k_lines_sum_ms_per_node"]["median"]
        out["batched_minus_single_ms_per_node"] = float(slower)
        out["batched_no_slower_than_single_by_more_than_its_spread"] = bool(slower <= out["k_lines_sum_ms_per_node"]["spread"])

        # ---- (c) bytes: arithmetic on the shapes
        n_tiles = -(-n_points // lines.TILE_POINTS)
        table_bytes = n_nodes * n_bins * N_GAUSS * 8
        out["bytes_by_arithmetic"] = {
            "two_step": {"device_to_host": n_nodes * (n_points * 8 + 4 * len(line["nu0"]) * 8) + table_bytes,      # kappa64, line_params
                         "host_to_device": n_nodes * (n_points * 4 + n_tiles * 8), "disk_written": n_nodes * n_points * 4,
                         "disk_read": n_nodes * n_points * 4},
            "fused": {"device_to_host": table_bytes, "host_to_device": len(press) * n_tiles * 8 + n_nodes * 32, "disk_written": 0,
                      "disk_read": 0},
            "both": "the line list's seven arrays and the k-table's grid go up once, the container is written once; not counted"}
    finally:
        shutil.rmtree(wd, ignore_errors=True)
    path = os.path.join(ROOT, "profiles", "lines_ktable_bench.json")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
