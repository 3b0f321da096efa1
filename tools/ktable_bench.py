#!/usr/bin/env python3
"""Times the k-table tool on a synthetic species of HELIOS-K's usual size and writes profiles/ktable_bench.json.

    python tools/ktable_bench.py [--points 8] [--skip-numpy] [--skip-trace]

The species: 0 - 30 000 cm^-1 at 0.01 cm^-1 in three chunks (3e6 fp32 values, 12 MB, per (T, P) point), R = 50 over
0.34 - 200 micron, 20 Gauss points, 8 (T, P) points.  Recorded: (i) the time in k_ktable_bins per (T, P) point from
`rocprofv3 --kernel-trace --stats` in a run of its own, (ii) the wall time per (T, P) point including reading and upload,
(iii) the numpy backend on 16 threads on the same files, and -- read from profiles/ktable_reference_time.json where
tests/golden/make_ktable_golden.py --time-reference left it -- (iv) the reference's big_loop on one (T, P) point.
Every step that uses the GPU is a child process of its own under `timeout`; a step that fails ends the tool.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GRID = (50.0, 0.34, 200.0)
CHUNKS = ((0, 10000), (10000, 20000), (20000, 30000))
RES = 0.01
TEMPS, CODES = (500, 1000, 1500, 2000), ("n100", "p000")


def synthetic_species(n_points, seed=11):
    """file name -> fp32 opacities of the first `n_points` (T, P) points: log-uniform lines over a floor of exact zeros"""
    rng = np.random.default_rng(seed)
    files, done = {}, 0
    for t in TEMPS:
        for c in CODES:
            if done == n_points:
                return files
            for lo, hi in CHUNKS:
                n = int(round((hi - lo) / RES))
                k = (10.0 ** rng.uniform(-12, 3, n)).astype(np.float32)
                k[rng.random(n) < 0.1] = 0.0
                files["Out_%05d_%05d_%05d_%s.bin" % (lo, hi, t, c)] = k
            done += 1
    return files


def write_species(root, n_points):
    os.makedirs(root, exist_ok=True)
    for name, k in synthetic_species(n_points).items():
        k.tofile(os.path.join(root, name))


def run_device(root):
    from helios_amd import ktable
    inter = ktable.wavelength_grid("fixed_resolution", GRID)
    timing = {}
    t0 = time.time()
    ktable.build_species(root, inter, 20, backend="hip", tp_per_launch=4, timing=timing)
    wall = time.time() - t0
    ms = timing["device_ms"]
    return {"wall_seconds_per_tp_point": wall / timing["points"], "kernel_ms_per_tp_point_hip_events": ms[0] / ms[3],
            "launches": int(ms[1]), "points": int(timing["points"]), "bins": len(inter) - 1}


def run_numpy(root, threads=16):
    from helios_amd import ktable
    inter = ktable.wavelength_grid("fixed_resolution", GRID)
    files = ktable.SpeciesFiles(root)
    res = files.resolution()
    lam = ktable.spectral_axis(files.numin[0], files.numax[-1], res)
    start, end = ktable.bin_ranges(lam, inter)
    yg = ktable.grid_datasets(inter, 20)[2]
    pts = [(t, c) for t in files.temps for c in files.codes]
    t0 = time.time()
    with ThreadPoolExecutor(max_workers=threads) as pool:
        list(pool.map(lambda p: ktable.numpy_slab(lam, inter, start, end, files.read_point(p[0], p[1], res), yg), pts))
    return {"numpy_seconds_per_tp_point_16_threads": (time.time() - t0) / len(pts), "threads": threads}


def kernel_trace(root, out_dir, limit):
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir,
           "--", sys.executable, os.path.abspath(__file__), "--child", "device", "--dir", root]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("rocprofv3 run ended with %d: %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
    rows = []
    for path in glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(path)))
    hit = [r for r in rows if "k_ktable_bins" in r.get("Name", "")]
    if not hit:
        raise RuntimeError("no k_ktable_bins row in the kernel statistics")
    return {"total_ns": float(hit[0]["TotalDurationNs"]), "calls": int(hit[0]["Calls"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=8)
    ap.add_argument("--skip-numpy", action="store_true")
    ap.add_argument("--skip-trace", action="store_true")
    ap.add_argument("--child", default=None)
    ap.add_argument("--dir", default=None)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "ktable_bench.json"))
    opt = ap.parse_args()
    if opt.child == "device":
        print(json.dumps(run_device(opt.dir)))
        return
    tmp = tempfile.mkdtemp()
    try:
        root = os.path.join(tmp, "hk")
        write_species(root, opt.points)
        rec = {"species": "synthetic, 0-30000 cm^-1 at 0.01 cm^-1, R = 50 over 0.34-200 micron, 20 Gauss points",
               "bytes_per_tp_point": 12000000}
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "device", "--dir",
                            root], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("device run ended with %d: %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        rec.update(json.loads(r.stdout.strip().splitlines()[-1]))
        if not opt.skip_trace:
            tr = kernel_trace(root, os.path.join(tmp, "trace"), 400)
            rec["kernel_ms_per_tp_point_rocprofv3"] = tr["total_ns"] / 1e6 / rec["points"]
        if not opt.skip_numpy:
            rec.update(run_numpy(root))
        ref = os.path.join(ROOT, "profiles", "ktable_reference_time.json")
        if os.path.exists(ref):
            rec["reference_big_loop_seconds_per_tp_point"] = json.load(open(ref))["seconds_per_tp_point"]
        os.makedirs(os.path.dirname(opt.output), exist_ok=True)
        with open(opt.output, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
        print(json.dumps(rec))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
