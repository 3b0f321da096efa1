#!/usr/bin/env python3
"""Writes profiles/cia_bench.json: a synthetic CIA table of H2-H2's shape -- one band, 20 ... 10000 cm^-1 at 1 cm^-1, 113
temperatures from 200 to 3000 K -- onto 0 ... 30000 cm^-1 at dnu = 0.01 cm^-1 (3e6 points), 322 bins x 20 Gauss points,
4 temperatures x 4 pressure codes, four nodes per launch.  The two-step route puts 16 files of 12 MB into the machine's temporary
directory; they are removed at the end.

One process, medians of seven runs behind a warm-up.  (a) k_cia_nodes per node by HIP events (four nodes per launch, 16 nodes)
next to a device-to-device copy of one fp32 slab timed the same way, four slabs per event pair: the kernel's least traffic is its
4-byte store per point, the copy reads and writes 4 bytes per point.  (b) k_ktable_bins per node, from the fused route's own
timer.  (c) the whole routes, cia.main + ktable.main against cia.main -ktable yes, by the wall clock, alternating; both parse
the same `.cia` file.  (d) the numpy backend on the same nodes by the wall clock, once.  (e) whether the two routes' tables
are equal to the bit.

    python tools/cia_bench.py [--out FILE]
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

RUNS = 7
TEMPS, CODES = "500 1000 1500 2000", "n300 n100 p000 p200"
NUMAX, DNU = 30000, 0.01
GRID, N_GAUSS, PER_LAUNCH = "50 0.34 200", 20, 4
TABLE_TEMPS = 113


def quiet(fn, argv):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(argv)


def synthetic_blocks():
    """113 blocks on 20, 21, ... 10000 cm^-1: a smooth fall over 15 decades with a ripple, warmer blocks higher"""
    from helios_amd import cia
    nu = np.arange(20.0, 10001.0, 1.0)
    rng = np.random.default_rng(1)
    blocks = []
    for t in np.linspace(200.0, 3000.0, TABLE_TEMPS):
        k = 10.0 ** (-44.0 - 15.0 * nu / 10000.0 * (300.0 / t) ** 0.5 + 0.1 * rng.standard_normal(len(nu)))
        blocks.append(cia.Block(20.0, 10000.0, float(np.round(t, 1)), nu, k))
    return blocks


def stats(a):
    a = np.asarray(a, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def main(argv):
    import cia_cases as cc
    from helios_amd import _nodes, cia, ktable
    from helios_amd.device import Context
    n_points = _nodes.chunk_limits("cia", 0, NUMAX, DNU)[0][2]
    temps, codes = [int(t) for t in TEMPS.split()], CODES.split()
    press = sorted(ktable.pressure_table()[c] for c in codes)
    n_nodes = len(temps) * len(codes)
    inter = ktable.wavelength_grid("fixed_resolution", GRID.split())
    blocks = synthetic_blocks()
    out = {"case": "one band 20 - 10000 cm^-1 at 1 cm^-1, %d temperatures, onto 0 - %d cm^-1 at dnu = %g, %d bins x %d Gauss points, "
                   "%d x %d nodes, %d nodes per launch" % (TABLE_TEMPS, NUMAX, DNU, len(inter) - 1, N_GAUSS, len(temps), len(codes),
                                                           PER_LAUNCH),
           "points": n_points, "nodes": n_nodes, "runs": RUNS, "tabulated_values": int(sum(len(b.nu) for b in blocks))}
    wd = tempfile.mkdtemp(prefix="cia_bench_")
    try:
        path = cc.write_cia_file(os.path.join(wd, "h2h2.cia"), blocks)
        with open(os.path.join(wd, "species.dat"), "w") as f:
            f.write("species path\nCIA_H2H2 %s\n" % os.path.join(wd, "opac"))
        common = ["-name", "CIA_H2H2", "-cia_file", path, "-temperatures", TEMPS, "-pressure_codes", CODES, "-numax", str(NUMAX),
                  "-dnu", repr(DNU), "-nodes_per_launch", str(PER_LAUNCH)]
        table = ["-wavelength_grid", GRID, "-number_of_gaussian_points", str(N_GAUSS), "-container", "npz", "-interpolate", "no"]

        # ---- (a) the kernel and a copy of its output by HIP events
        bands = cia.bands_of(cia.read_cia_file(path)[0])                    # as the routes see it
        nodes = [(float(t), p) for t in sorted(temps) for p in press]
        ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
        out["device"] = ctx.name()
        h = cia.CiaOpacity(ctx, bands, n_points, PER_LAUNCH, n_nodes)
        src, dst = ctx.zeros(PER_LAUNCH * n_points, np.float32), ctx.zeros(PER_LAUNCH * n_points, np.float32)
        try:
            kernel, copy = [], []
            for r in range(RUNS + 1):                                       # the first repeat is the warm-up
                h.set_nodes([n[0] for n in nodes], [n[1] for n in nodes], cc.M_H2, 0.0, DNU, n_points)
                for first in range(0, n_nodes, PER_LAUNCH):
                    h.run_nodes(first, min(PER_LAUNCH, n_nodes - first))
                kernel.append(h.get("timing_ms")[0] / n_nodes)
                ms = 0.0
                for _ in range(n_nodes // PER_LAUNCH):
                    ctx.timer_start()
                    ctx.check(ctx._l.hx_d2d(ctx.handle, dst.d, src.d, PER_LAUNCH * n_points * 4), "hx_d2d")
                    ms += ctx.timer_stop_ms()
                copy.append(ms / n_nodes)
        finally:
            h.close()
            src.free()
            dst.free()
            ctx.close()
        out["k_cia_nodes_ms_per_node"] = dict(stats(kernel[1:]), warm_up=float(kernel[0]))
        out["copy_of_one_slab_ms"] = dict(stats(copy[1:]), warm_up=float(copy[0]))
        k_ms, c_ms = out["k_cia_nodes_ms_per_node"]["median"], out["copy_of_one_slab_ms"]["median"]
        out["bytes_by_arithmetic"] = {"k_cia_nodes_stored_per_node": n_points * 4, "copy_read_and_written_per_slab": n_points * 8}
        out["k_cia_nodes_stored_gb_per_s"] = n_points * 4 / (k_ms * 1e-3) / 1e9
        out["copy_moved_gb_per_s"] = n_points * 8 / (c_ms * 1e-3) / 1e9
        out["k_cia_nodes_over_copy"] = k_ms / c_ms

        # ---- (c) the whole routes, and (b) k_ktable_bins from the fused route's timer
        def two_step():
            t0 = time.time()
            quiet(cia.main, common + ["-output_directory", os.path.join(wd, "opac")])
            t1 = time.time()
            quiet(ktable.main, ["-path_to_individual_species_file", os.path.join(wd, "species.dat"),
                                "-directory_with_individual_files", os.path.join(wd, "two_step"), "-points_per_launch",
                                str(PER_LAUNCH)] + table)
            return time.time() - t0, t1 - t0

        bins_ms = []

        def fused():
            t0 = time.time()
            text = io.StringIO()
            with contextlib.redirect_stdout(text):
                cia.main(common + ["-ktable", "yes", "-directory_with_individual_files", os.path.join(wd, "fused")] + table)
            bins_ms.append(float(text.getvalue().split("k_ktable_bins ")[1].split(" ms")[0]) / n_nodes)
            return time.time() - t0

        warm = {"two_step_seconds": two_step()[0], "fused_seconds": fused()}
        a, b = [], []
        for _ in range(RUNS):
            a.append(two_step())
            b.append(fused())
        a, b = np.array(a), np.array(b)
        out["routes"] = {"warm_up": warm, "two_step_seconds": dict(stats(a[:, 0]), of_which_cia_main_median=float(np.median(a[:, 1]))),
                         "fused_seconds": stats(b), "two_step_over_fused": float(np.median(a[:, 0]) / np.median(b))}
        out["k_ktable_bins_ms_per_node"] = dict(stats(bins_ms[1:]), warm_up=bins_ms[0], source="the tool's own line, one decimal of the sum")

        # ---- (e) the tables
        with np.load(os.path.join(wd, "two_step", "CIA_H2H2_opac_kdistr.npz")) as x, \
                np.load(os.path.join(wd, "fused", "CIA_H2H2_opac_kdistr.npz")) as y:
            out["tables_equal_to_the_bit"] = bool(sorted(x.files) == sorted(y.files) and all(x[k].tobytes() == y[k].tobytes() for k in x.files))
            out["kpoints_min_max"] = [float(y["kpoints"].min()), float(y["kpoints"].max())]
        out["opacity_files_bytes"] = sum(os.path.getsize(os.path.join(wd, "opac", f)) for f in os.listdir(os.path.join(wd, "opac")))

        # ---- (d) the numpy backend, and the device against it
        t0 = time.time()
        host = cia.cia_opacity([b_ for band in bands for b_ in band.blocks], temps, press, (0.0, DNU, n_points), cc.M_H2, backend="numpy")
        out["numpy_backend_seconds"] = time.time() - t0
        out["numpy_backend_ms_per_node"] = out["numpy_backend_seconds"] * 1e3 / n_nodes
        got = np.fromfile(os.path.join(wd, "opac", _nodes.file_name("CIA_H2H2", 0, NUMAX, temps[1], codes[2])), np.float32)
        with np.errstate(under="ignore"):
            want = host[sorted(temps).index(temps[1]), press.index(ktable.pressure_table()[codes[2]])].astype(np.float32)
        out["a_device_file_equals_the_numpy_backend_to_the_bit"] = bool(got.tobytes() == want.tobytes())
    finally:
        shutil.rmtree(wd, ignore_errors=True)
    target = os.path.join(ROOT, "profiles", "cia_bench.json")
    if "--out" in argv:
        target = argv[argv.index("--out") + 1]
    with open(target, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
