#!/usr/bin/env python3
"""Set-up time of a cloud sweep with the cloud planes built on the host or on the device, on one GPU.  Writes
profiles/cloud_decks_ab.json (or --out):

    python tools/cloud_sweep_ab.py [--columns 64] [--repeats 3] [--nbin 10000] [--nlayer 100]

A sweep of `--columns` columns over aerosol radius mode x cloud base pressure (one deck, a synthetic LX-MIE directory of 51
radii x 500 wavelengths written to a temporary directory) at BASELINE config 2's grid, synthetic opacities on a small (T, P)
grid -- the cloud set-up does not depend on it.  One fresh process per variant (HELIOS_CLOUD_DECKS=host, =device), each with a
warm-up sweep of two columns first and then `--repeats` timed set-ups: reading and preparing the columns on the host
(`prepare_s`: parameter file, grid, start profile and the clouds -- Cloud.cloud_pre_processing or
Cloud.cloud_deck_description, the Mie cache emptied before every repeat) and building the device batch up to its first refresh
(`batch_s`: RTBatch with tables, profiles and the cloud planes, uploaded or built by the two kernels), the device idle at both
ends.  Medians are reported, every run is kept.  On the device variant the two kernels are then timed by HIP events
(hx_rt_profile) while every column's deck call is issued again."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_mie_directory(path, nw=500, seed=1):
    from helios_amd.clouds import R_VALUES
    rng = np.random.default_rng(seed)
    lam_um = np.geomspace(0.25, 600.0, nw)
    os.makedirs(path, exist_ok=True)
    for r in R_VALUES:
        size = 2 * np.pi * r / lam_um
        geo = np.pi * (r * 1e-4) ** 2
        scat = geo * np.minimum(size ** 4, 2.0 + np.cos(size)) * rng.uniform(0.7, 1.3, nw)
        absorb = geo * np.minimum(size, 1.0) * rng.uniform(0.2, 0.6, nw)
        tab = np.stack([lam_um, size, scat + absorb, scat, absorb, scat / (scat + absorb), rng.uniform(0, 0.9, nw)], axis=1)
        np.savetxt(os.path.join(path, "r{:.6f}.dat".format(r)), tab, fmt="%.17e", header="LX-MIE (synthetic)")
    return path + os.sep


def spread(v):
    v = [float(x) for x in v]
    return {"runs": v, "min": min(v), "max": max(v), "median": float(np.median(v))}


def variant(a):
    """one variant in this (fresh) process; prints its record as one JSON line"""
    from helios_amd import computation, rt as rt_mod
    from helios_amd import sweep as sw
    mode = os.environ["HELIOS_CLOUD_DECKS"]
    side = int(np.ceil(np.sqrt(a.columns)))
    spec = "aerosol_radius_mode=%s;cloud_bottom_pressure=%s" % (
        ",".join("%.4g" % v for v in np.geomspace(0.3, 30.0, side)), ",".join("%.4g" % v for v in np.geomspace(1e6, 1e3, side)))
    overrides = sw.expand_sweep(spec)[:a.columns]
    base = ["-parameter_file", "/nonexistent", "-opacity_mixing", "synthetic", "-synthetic", "%d 6 5 20242" % a.nbin,
            "-number_of_layers", str(a.nlayer), "-convective_adjustment", "no", "-number_of_cloud_decks", "1",
            "-path_to_mie_files", a.mie, "-aerosol_radius_geometric_std_dev", "2", "-cloud_bottom_mixing_ratio", "1e-9",
            "-cloud_to_gas_scale_height_ratio", "0.5"]
    computer = computation.Compute()
    calls = []
    decks = rt_mod.RTBatch.set_column_cloud_decks

    def recording(batch, col, *args):
        calls.append((col, args))
        decks(batch, col, *args)
    rt_mod.RTBatch.set_column_cloud_decks = recording

    def set_up(ovs):
        shared = {"cloud_decks": sw.cloud_deck_mode(ovs)}
        computer.ctx.synchronize()
        t0 = time.perf_counter()
        quants = []
        for k, ov in enumerate(ovs):
            q, _ = sw._prepare_column(base, dict(ov, name="ab_%d" % k), shared)
            q._ctx = computer.ctx
            quants.append(q)
        t1 = time.perf_counter()
        del calls[:]
        rt = computer.make_rt_batch(quants)
        computer.ctx.synchronize()
        return rt, t1 - t0, time.perf_counter() - t1

    rt, _, _ = set_up(overrides[:2])          # warm-up: library, device, code objects, allocator
    rt.close()
    prepare, batch = [], []
    kernels = {}
    for rep in range(a.repeats):
        rt, tp, tb = set_up(overrides)
        prepare.append(tp)
        batch.append(tb)
        if mode == "device" and rep == a.repeats - 1:
            assert len(calls) == len(overrides)
            rt.profile(True)
            for col, args in list(calls):
                decks(rt, col, *args)
            computer.ctx.synchronize()
            for name in ("k_cloud_deck_spectra", "k_cloud_planes"):
                ms, n = rt.profile_read(name)
                kernels[name] = {"launches": int(n), "mean_ms": float(ms)}
            rt.profile(False)
        rt.close()
    rec = {"prepare_s": spread(prepare), "batch_s": spread(batch), "set_up_s": spread(np.add(prepare, batch))}
    if kernels:
        rec["kernels"] = kernels
    print("AB_RECORD " + json.dumps(rec, sort_keys=True))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--columns", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--nbin", type=int, default=10000)
    ap.add_argument("--nlayer", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cloud_decks_ab.json"))
    ap.add_argument("--variant", default="", help=argparse.SUPPRESS)
    ap.add_argument("--mie", default="", help=argparse.SUPPRESS)
    a = ap.parse_args(argv)
    if a.variant:
        return variant(a)
    rec = {"columns": a.columns, "nbin": a.nbin, "nlayer": a.nlayer, "decks": 1, "mie_wavelengths": 500,
           "plane_bytes_per_column": 6 * 8 * a.nbin * (2 * a.nlayer + 1) // 2, "repeats": a.repeats, "variants": {}}
    with tempfile.TemporaryDirectory() as tmp:
        mie = write_mie_directory(os.path.join(tmp, "aerosol"))
        for mode in ("host", "device"):
            env = dict(os.environ, HELIOS_CLOUD_DECKS=mode)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--variant", mode, "--mie", mie, "--columns",
                                str(a.columns), "--repeats", str(a.repeats), "--nbin", str(a.nbin), "--nlayer", str(a.nlayer)],
                               env=env, capture_output=True, text=True)
            if p.returncode != 0:
                raise RuntimeError("variant %s ended with status %d:\n%s" % (mode, p.returncode, p.stderr[-3000:]))
            rec["variants"][mode] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("AB_RECORD ")][-1][10:])
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec, sort_keys=True))


if __name__ == "__main__":
    main()
