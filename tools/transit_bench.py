#!/usr/bin/env python3
"""Writes profiles/transit_bench.json: hx_transit_depth at config 2's shape -- 10 000 bins x 20 Gauss points x 100
non-isothermal layers, 200 half-layer shells, 320 MB of optical depths.  The call (geometry prologue, chord kernel, area
kernel) by HIP events, the median of seven runs behind a warm-up; the bytes it must move (each optical depth once, the
clouds' once, the outputs); a device-to-device copy of one of the two optical-depth arrays timed the same way, and the call's
byte rate as a fraction of that copy's.  The band transmissions that pass through the work buffer are recorded apart.
No threshold: the file records what was measured.

    python tools/transit_bench.py [--out FILE] [--bins N] [--layers N]
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 7


def _arg(argv, name, default):
    return int(argv[argv.index(name) + 1]) if name in argv else default


def column(nbin, ny, nlayer, seed=7):
    """an exponential atmosphere over 25 scale heights with seeded structure per spectral point; the half-layer optical depths
    in the run's layouts, the clouds', the shell boundaries and the Gauss weights"""
    rng = np.random.default_rng(seed)
    R0, H = 7.0e9, 7.0e6
    S = 2 * nlayer
    zb = np.linspace(-2.0 * H, 23.0 * H, S + 1)
    shell = np.exp(-0.5 * (zb[:-1] + zb[1:]) / H) * np.diff(zb)
    strength = 10.0 ** rng.uniform(-9.0, -5.0, (nbin, ny))                  # extinction at z = 0 [1/cm] per spectral point
    halves = []
    for first in (0, 1):                                                      # lower halves: even shells, upper: odd
        a = np.empty((nlayer, nbin, ny))
        for i in range(nlayer):
            a[i] = strength * shell[2 * i + first]
        halves.append(a.reshape(-1))
    cloud = 1e-3 * rng.uniform(0.0, 1.0, (2, nlayer * nbin))
    w = np.polynomial.legendre.leggauss(ny)[1]
    return halves, cloud, zb, w, R0


def main(argv):
    from helios_amd import _lib
    from helios_amd.device import Context
    nbin, ny, nlayer = _arg(argv, "--bins", 10000), 20, _arg(argv, "--layers", 100)
    S = 2 * nlayer
    halves, cloud, zb, w, R0 = column(nbin, ny, nlayer)
    l = _lib.lib()
    ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    out = {"case": "%d bins x %d Gauss points x %d non-isothermal layers (%d shells)" % (nbin, ny, nlayer, S), "runs": RUNS,
           "device": ctx.name().strip(), "chords_per_thread": int(l.hx_transit_chord_block())}
    dev = [ctx.to_gpu(a) for a in halves] + [ctx.to_gpu(cloud[0]), ctx.to_gpu(cloud[1])]
    d_zb, d_w = ctx.to_gpu(zb), ctx.to_gpu(w)
    work = ctx.empty(int(l.hx_transit_work_doubles(S, nbin)))
    d_A, d_floor = ctx.empty(nbin), ctx.empty(nbin)
    null = ctypes.POINTER(ctypes.c_double)()
    ms = []
    for _ in range(RUNS + 1):                         # the first run is the warm-up
        ctx.timer_start()
        ctx.check(l.hx_transit_depth(ctx.handle, dev[0].d, dev[1].d, dev[2].d, dev[3].d, d_zb.d, d_w.d, R0, nbin, ny, S, work.d,
                                     d_A.d, d_floor.d, null), "hx_transit_depth")
        ms.append(ctx.timer_stop_ms())
    A, floor = d_A.get(), d_floor.get()
    out["call_ms"] = {"median": float(np.median(ms[1:])), "min": min(ms[1:]), "max": max(ms[1:]), "warm_up": ms[0]}
    # each optical depth once, the clouds' once, the outputs A and T_floor
    must = 8 * (2 * nlayer * nbin * ny + 2 * nlayer * nbin + 2 * nbin)
    out["bytes_it_must_move"] = must
    # not among them: the band transmissions of every chord, which the call writes to its work buffer and reads back
    out["work_buffer_bytes_written_and_read"] = 8 * 2 * S * nbin
    out["optical_depth_bytes"] = 8 * 2 * nlayer * nbin * ny
    rate = must / (out["call_ms"]["median"] * 1e-3)
    out["achieved_GB_per_s"] = rate / 1e9
    # the work the contract asks for: one multiply and one add per (spectral point, shell >= chord), one division per shell
    out["chord_shell_pairs"] = nbin * ny * S * (S + 1) // 2
    out["pair_updates_per_ns"] = out["chord_shell_pairs"] / (out["call_ms"]["median"] * 1e6)
    scratch = ctx.empty(dev[0].size)
    cms = []
    for _ in range(RUNS + 1):
        ctx.timer_start()
        scratch.copy_from_device(dev[0].ptr, dev[0].nbytes)
        cms.append(ctx.timer_stop_ms())
    copy_rate = 2 * dev[0].nbytes / (float(np.median(cms[1:])) * 1e-3)
    out["copy_ms"] = {"median": float(np.median(cms[1:])), "min": min(cms[1:]), "max": max(cms[1:]), "bytes": dev[0].nbytes}
    out["copy_GB_per_s"] = copy_rate / 1e9
    out["fraction_of_copy_rate"] = rate / copy_rate
    out["transit_radius_minus_R0_in_H"] = {"min": float((np.sqrt((R0 + zb[0]) ** 2 + A) - R0).min() / 7.0e6),
                                           "max": float((np.sqrt((R0 + zb[0]) ** 2 + A) - R0).max() / 7.0e6)}
    out["largest_floor_transmission"] = float(floor.max())
    for d in dev + [d_zb, d_w, work, d_A, d_floor, scratch]:
        d.free()
    ctx.close()
    path = os.path.join(ROOT, "profiles", "transit_bench.json")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
