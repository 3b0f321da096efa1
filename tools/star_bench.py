#!/usr/bin/env python3
"""Times star.py on a synthetic star of PHOENIX's size -- 1 569 128 points, eight corners -- onto the R = 50 grid, for 1 star
and for 16 stars that share the corners, and writes profiles/star_bench.json: the three kernels by HIP events (medians behind a
warm-up), the whole tool with the files read from a temporary directory, and the numpy backend.  Needs a GPU; the reference's
own time for one star is not part of this script (its functions run on the machine that has the reference).

    python tools/star_bench.py [--repeat 7] [--stars 1,16]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N_POINTS = 1569128


def write_fits(path, data):
    """a primary image, written by hand: the bench needs no astropy"""
    data = np.asarray(data)
    bitpix = {np.dtype("f4"): -32, np.dtype("f8"): -64}[data.dtype]
    cards = ["SIMPLE  =                    T", "BITPIX  = %20d" % bitpix, "NAXIS   =                    1",
             "NAXIS1  = %20d" % len(data), "END"]
    head = "".join(c.ljust(80) for c in cards).ljust(2880)
    raw = data.astype(data.dtype.newbyteorder(">")).tobytes()
    with open(path, "wb") as f:
        f.write(head.encode("ascii") + raw + b"\0" * (-len(raw) % 2880))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--repeat", type=int, default=7)
    p.add_argument("--stars", default="1,16")
    opt = p.parse_args(argv)
    from helios_amd import star
    from helios_amd.device import Context
    from helios_amd.ktable import gen_fixed_res_grid
    rng = np.random.default_rng(5)
    lam_A = np.sort(500.0 * (55000.0 / 500.0) ** rng.random(N_POINTS))
    inter = np.asarray(gen_fixed_res_grid(0.34e-4, 200e-4, 50.0))
    out = {"points": N_POINTS, "bins": len(inter) - 1, "repeat": opt.repeat, "cases": {}}
    with tempfile.TemporaryDirectory() as d:
        write_fits(os.path.join(d, star.PHOENIX_WAVE_FILE), lam_A)
        for t in (3000, 3100):
            for g in (4.5, 5.0):
                for m in (0.0, 0.5):
                    write_fits(os.path.join(d, star.corner_name(t, g, m)), (1e14 * (0.2 + rng.random(N_POINTS))).astype(np.float32))
        ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
        try:
            for n in [int(v) for v in opt.stars.split(",")]:
                stars = [{"data_format": "phoenix", "name": "s%d" % k, "temp": 3005.0 + 5 * k, "log_g": 4.6 + 0.02 * k,
                          "m": 0.1 + 0.02 * k} for k in range(n)]
                runs = []
                for r in range(opt.repeat + 1):           # the first run is the warm-up
                    timing = {}
                    star.convert_stars(stars, inter, "automatic", "device", d, ctx=ctx, timing=timing)
                    runs.append(timing)
                runs = runs[1:]
                ms = np.median([t["device_ms"] for t in runs], axis=0)
                t0 = time.time()
                star.convert_stars(stars[:1], inter, "automatic", "numpy", d)
                numpy_one = time.time() - t0
                tool = float(np.median([t["seconds"] for t in runs]))
                out["cases"]["%d_stars" % n] = {
                    "k_star_blend_ms": float(ms[0]), "k_star_planck_bins_ms": float(ms[1]), "k_star_rebin_ms": float(ms[2]),
                    "tool_seconds": tool, "reading_seconds": float(np.median([t["read_seconds"] for t in runs])),
                    "kernels_share_of_tool": float(ms[:3].sum() / 1e3 / tool),
                    "numpy_backend_seconds_one_star": numpy_one, "numpy_over_tool_per_star": numpy_one * n / tool}
        finally:
            ctx.close()
    path = os.path.join(ROOT, "profiles", "star_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
