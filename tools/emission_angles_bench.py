#!/usr/bin/env python3
"""Writes profiles/emission_angles_bench.json: hx_emission_angles at config 2's shape -- 10 000 bins x 20 Gauss points x 100
non-isothermal layers, 200 half-layer shells, beam on -- for N = 1, 8 and 16 emission angles.  The call by HIP events, the
median of seven runs behind a warm-up, one process; next to it the bytes of the arrays the kernel must read once (its traffic
model), the number of exponentials (one exp or expm1 per spectral point, shell and angle), and a device-to-device copy of one
of the arrays timed the same way.  No threshold: the file records what was measured.

    python tools/emission_angles_bench.py [--out FILE] [--bins N] [--layers N]
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RUNS = 7
ANGLES = (1, 8, 16)


def _arg(argv, name, default):
    return int(argv[argv.index(name) + 1]) if name in argv else default


def column(nbin, ny, nlayer, seed=7):
    """a seeded column in the run's layouts: half-layer optical depths falling by 1e7 from the bottom to the top (so the slant
    optical depths lie on both sides of the switch), albedos, Planck values and fluxes of a plausible size"""
    rng = np.random.default_rng(seed)
    nc = nbin * ny
    fall = 10.0 ** (1.0 - 7.0 * np.arange(nlayer) / max(nlayer - 1, 1))
    a = {}
    for n in ("dtau_lower", "dtau_upper"):
        a[n] = (fall[:, None] * rng.uniform(0.5, 2.0, (nlayer, nc))).reshape(-1)
    for n in ("cloud_lower", "cloud_upper"):
        a[n] = 1e-3 * rng.uniform(0.0, 1.0, nlayer * nbin)
    for n in ("w0_lower", "w0_upper"):
        a[n] = rng.uniform(0.0, 0.999, nlayer * nc)
    a["planck_lay"] = rng.uniform(1.0, 2.0, nbin * (nlayer + 2))
    a["planck_int"] = rng.uniform(1.0, 2.0, nbin * (nlayer + 1))
    for n in ("F_up", "F_down", "F_dir"):
        a[n] = np.pi * rng.uniform(0.5, 2.0, (nlayer + 1) * nc)
    for n in ("Fc_up", "Fc_down", "Fc_dir"):
        a[n] = np.pi * rng.uniform(0.5, 2.0, nlayer * nc)
    a["w"] = np.polynomial.legendre.leggauss(ny)[1]
    return a


def main(argv):
    from helios_amd import _lib
    from helios_amd.computation import Compute
    from helios_amd.device import Context
    nbin, ny, nlayer = _arg(argv, "--bins", 10000), 20, _arg(argv, "--layers", 100)
    S = 2 * nlayer
    host = column(nbin, ny, nlayer)
    l = _lib.lib()
    ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    out = {"case": "%d bins x %d Gauss points x %d non-isothermal layers (%d shells), beam on" % (nbin, ny, nlayer, S),
           "runs": RUNS, "device": ctx.name().strip()}
    dev = {n: ctx.to_gpu(v) for n, v in host.items()}
    # what the kernel must read once: every array above
    inputs = sum(d.nbytes for n, d in dev.items() if n != "w")
    out["input_bytes"] = inputs
    d_band = ctx.empty(max(ANGLES) * nbin)
    null = ctypes.POINTER(ctypes.c_double)()
    beta = 1.0 / (4.0 * np.pi * 0.5)
    order = ("dtau_lower", "dtau_upper", "cloud_lower", "cloud_upper", "w0_lower", "w0_upper", "planck_lay", "planck_int", "F_up",
             "F_down", "F_dir", "Fc_up", "Fc_down", "Fc_dir", "w")
    out["angles"] = {}
    for N in ANGLES:
        mu, weight, mu_inv = Compute.emission_quadrature(N)
        d_mu = ctx.to_gpu(mu_inv)
        ms = []
        for _ in range(RUNS + 1):                         # the first run is the warm-up
            ctx.timer_start()
            ctx.check(l.hx_emission_angles(ctx.handle, *[dev[n].d for n in order], d_mu.d, beta, nbin, ny, nlayer, N, d_band.d,
                                           null), "hx_emission_angles")
            ms.append(ctx.timer_stop_ms())
        I = d_band.get()[:N * nbin]
        med = float(np.median(ms[1:]))
        must = inputs + 8 * N * nbin
        exps = nbin * ny * S * N
        out["angles"][str(N)] = {"call_ms": {"median": med, "min": min(ms[1:]), "max": max(ms[1:]), "warm_up": ms[0]},
                                 "bytes_it_must_move": must, "achieved_GB_per_s": must / (med * 1e-3) / 1e9,
                                 "exponentials": exps, "exponentials_per_ns": exps / (med * 1e6),
                                 "intensity_min_max": [float(I.min()), float(I.max())]}
        d_mu.free()
    scratch = ctx.empty(dev["dtau_lower"].size)
    cms = []
    for _ in range(RUNS + 1):
        ctx.timer_start()
        scratch.copy_from_device(dev["dtau_lower"].ptr, dev["dtau_lower"].nbytes)
        cms.append(ctx.timer_stop_ms())
    copy_rate = 2 * dev["dtau_lower"].nbytes / (float(np.median(cms[1:])) * 1e-3)
    out["copy_ms"] = {"median": float(np.median(cms[1:])), "min": min(cms[1:]), "max": max(cms[1:]), "bytes": dev["dtau_lower"].nbytes}
    out["copy_GB_per_s"] = copy_rate / 1e9
    for N in ANGLES:
        r = out["angles"][str(N)]
        r["fraction_of_copy_rate"] = r["achieved_GB_per_s"] * 1e9 / copy_rate
    for d in list(dev.values()) + [d_band, scratch]:
        d.free()
    ctx.close()
    path = os.path.join(ROOT, "profiles", "emission_angles_bench.json")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
