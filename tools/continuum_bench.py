#!/usr/bin/env python3
"""Times the analytic containers of ktable.py (H-_bf, H-_ff, He-) on the reference's 120 x 28 (T, P) grid with 20 Gauss points and
adds what it measured to profiles/ktable_continuum.json.

    python tools/continuum_bench.py --device          # R = 50: k_ktable_continuum per container (HIP events around its slabs),
                                                      # container with copy-back, the whole tool with the files written
    python tools/continuum_bench.py --numpy           # the numpy backend at R = 50 and R = 1000, in memory, no GPU

The device part runs as a child process of its own under `timeout`; if it fails the tool ends there.
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
KINDS = ("H-_bf", "H-_ff", "He-")
REPEATS = 7          # medians of this many runs behind a warm-up


def grid(resolution):
    from helios_amd import continuum, ktable
    inter = ktable.wavelength_grid("fixed_resolution", (resolution, 0.34, 200.0))
    return continuum.grid_from(inter, 20, *ktable.default_target_grid())


def run_device(resolution):
    from helios_amd import continuum, ktable
    from helios_amd.device import Context
    g = grid(resolution)
    rec = {"bins": len(g["center wavelengths"]), "container_bytes": 8 * 3360 * 20 * len(g["center wavelengths"])}
    ctx = Context(0)
    try:
        b = continuum.ContinuumBuilder(ctx, g["center wavelengths"], 20, g["temperatures"], g["pressures"])
        out = np.empty(3360 * b.row_len)
        try:
            for name in KINDS:
                b.table(name, out)                                   # warm-up
                kernel, whole = [], []
                for _ in range(REPEATS):
                    before, t0 = b.kernel_ms, time.time()
                    b.table(name, out, timed=True)
                    kernel.append(b.kernel_ms - before)
                    whole.append(time.time() - t0)
                rec[name] = {"kernel_ms_hip_events": float(np.median(kernel)), "kernel_ms_hip_events_min_max": [min(kernel), max(kernel)],
                             "container_seconds_with_copy_back": float(np.median(whole)),
                             "container_seconds_with_copy_back_min_max": [min(whole), max(whole)], "repeats": REPEATS,
                             "nonzero_entries": int(np.count_nonzero(out))}
            rec["slab_rows"] = b.slab_rows
        finally:
            b.close()
    finally:
        ctx.close()
    tmp = tempfile.mkdtemp()
    try:
        for container in ("npz", "h5"):
            t0 = time.time()
            ktable.main(["-continuum_species", "H-,He-", "-rayleigh_species", "H2,He", "-wavelength_grid",
                         "%g 0.34 200" % resolution, "-directory_with_individual_files", os.path.join(tmp, container),
                         "-container", container])
            rec["tool_seconds_three_containers_" + container] = time.time() - t0
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return rec


def run_numpy(resolution):
    from helios_amd import continuum
    g = grid(resolution)
    rec = {"bins": len(g["center wavelengths"])}
    for name in KINDS:
        t0 = time.time()
        continuum.build_continuum(name, g, backend="numpy")
        rec[name + "_seconds"] = time.time() - t0
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--numpy", action="store_true")
    ap.add_argument("--child", type=float, default=None)
    ap.add_argument("--output", default=os.path.join(ROOT, "profiles", "ktable_continuum.json"))
    opt = ap.parse_args()
    if opt.child is not None:
        print(json.dumps(run_device(opt.child)))
        return
    rec = json.load(open(opt.output)) if os.path.exists(opt.output) else {}
    rec["grid"] = "120 x 28 (T, P) nodes, 20 Gauss points, constant R over 0.34 - 200 micron"
    if opt.device:
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", "50"],
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("device run ended with %d: %s" % (r.returncode, (r.stdout + r.stderr)[-2000:]))
        rec["device_R50"] = json.loads(r.stdout.strip().splitlines()[-1])
    if opt.numpy:
        rec["numpy_R50"], rec["numpy_R1000"] = run_numpy(50.0), run_numpy(1000.0)
    os.makedirs(os.path.dirname(opt.output), exist_ok=True)
    with open(opt.output, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
