#!/usr/bin/env python3
"""Build time of a premixed table at BASELINE config 3's shape: 10 000 bins x 20 Gauss points, 30 x 20 (T, P) nodes, 20
synthetic species mixed by random overlap, at refine (1, 1) and (2, 2).  Writes per-kernel times and the rate of
k_rt_mix_species in (node, bin) problems per second next to its config-3 refresh rate (2.01 M points in
31.5 ms) to profiles/premix_c3.json.

    python tools/premix_bench.py [--out profiles/premix_c3.json] [--nbin 10000] [--species 20]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C3_POINTS, C3_MS = 2.01e6, 31.5        # (level, bin) points of a config-3 refresh, ms per refresh


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/premix_c3.json")
    ap.add_argument("--nbin", type=int, default=10000)
    ap.add_argument("--species", type=int, default=20)
    ap.add_argument("--ntemp", type=int, default=30)
    ap.add_argument("--npress", type=int, default=20)
    a = ap.parse_args(argv)
    from helios_amd import synthetic as syn
    from helios_amd.device import Context
    from helios_amd.premix import Premixer
    ny = 20
    _iw, wave, _dw = syn.wavelength_grid(a.nbin)
    gy, gw = syn.gauss_points(ny)
    ktemp, kpress = syn.tp_grid(a.ntemp, a.npress)
    rng = np.random.default_rng(20241)
    ctx = Context(0)
    record = {"shape": dict(nbin=a.nbin, ny=ny, ntemp=a.ntemp, npress=a.npress, species=a.species, mixing="random overlap"),
              "device": ctx.name(), "config3_refresh": dict(points=C3_POINTS, ms=C3_MS, points_per_s=C3_POINTS / C3_MS * 1e3),
              "runs": []}
    for refine in ((1, 1), (2, 2)):
        pm = Premixer(ctx, a.nbin, ny, a.ntemp, a.npress, a.species, refine)
        try:
            pm.set_grid(wave, gy, gw, ktemp, kpress)
            srng = np.random.default_rng(7)
            for s in range(a.species):
                vmr = 0.8 if s == 0 else float(10.0 ** srng.uniform(-5.0, -2.0))
                pm.set_species(s, None, None, None, vmr, float(srng.uniform(2.0, 64.0)), True, False)
                kxy, ftp = syn.ktable_factors(rng, a.nbin, ny, ktemp, kpress, gy)
                pm.set_species_separable(s, kxy, ftp)
            for cell_error in (False, True):
                t0 = time.time()
                pm.run(cell_error)
                wall = time.time() - t0
                nodes, cells, ms = pm.nT * pm.nP, (pm.nT - 1) * (pm.nP - 1), pm.get("timing_ms")
                run = dict(refine=list(refine), cell_error=cell_error, nodes=nodes, wall_s=wall,
                           kernel_ms=dict(k_premix_nodes=ms[0], k_rt_mix_species=ms[1], k_premix_scat=ms[2],
                                          cell_error_with_its_mixing_launches=ms[3]),
                           mix_points_per_s=nodes * a.nbin / ms[1] * 1e3,
                           mix_rate_over_config3_refresh=(nodes * a.nbin / ms[1]) / (C3_POINTS / C3_MS))
                if cell_error:
                    e = pm.get("cell_error_max")
                    run["cell_error_largest"], run["cell_error_median"] = float(e.max()), float(np.median(e))
                    run["cell_error_points_per_s"] = cells * a.nbin / ms[3] * 1e3
                record["runs"].append(run)
                print(json.dumps(run))
        finally:
            pm.close()
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(record, f, indent=1)
    return record


if __name__ == "__main__":
    main()
