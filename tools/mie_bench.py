#!/usr/bin/env python3
"""Writes profiles/mie_bench.json: the Mie table of 51 radii x 1000 wavelengths over 0.3 - 200 micron (a smooth synthetic
material).  k_mie by HIP events (hx_mie_get("timing_ms")), the median of seven runs behind a warm-up, with the pairs sorted by
their number of terms, descending, and in the table's own order [radius][wavelength]; the whole tool (mie.py, the 51 files
included) on the device; the numpy backend's series on the same pairs.

    python tools/mie_bench.py [--out FILE] [--no-numpy]
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


def material(lam):
    n = 1.6 - 0.1 * np.log10(lam) + 0.4 * np.exp(-0.5 * (np.log10(lam / 12.0) / 0.15) ** 2)
    k = 1e-3 + 0.8 * np.exp(-0.5 * (np.log10(lam / 10.0) / 0.12) ** 2) + 0.05 * (lam / 250.0)
    return n, k


def main(argv):
    from helios_amd import mie
    from helios_amd.clouds import R_VALUES
    from helios_amd.device import Context
    lam = 0.3 * (200.0 / 0.3) ** (np.arange(1000) / 999.0)
    n, k = material(lam)
    x = (2.0 * np.pi * R_VALUES[:, None] / lam[None, :]).reshape(-1)
    m_re, m_im = np.broadcast_to(n, (51, 1000)).reshape(-1).copy(), np.broadcast_to(k, (51, 1000)).reshape(-1).copy()
    terms = mie.n_terms(x)
    out = {"case": "51 radii x 1000 wavelengths, 0.3 - 200 micron", "pairs": int(len(x)), "terms": int(terms.sum()),
           "longest_pair": int(terms.max()), "median_pair": int(np.median(terms)), "scratch_bytes": mie.SCRATCH_BYTES, "runs": RUNS}
    ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    out["device"] = ctx.name()
    s = mie.MieSeries(ctx, len(x))
    results = {}
    try:
        for label, order in (("sorted_by_terms", None), ("table_order", np.arange(len(x)))):
            ms, launches = [], 0
            for r in range(RUNS + 1):                 # the first run is the warm-up
                s.run(x, m_re, m_im, order)
                t = s.get("timing_ms")
                ms.append(float(t[0]))
                launches = int(t[1])
            results[label] = np.array([s.get("q_ext"), s.get("q_sca"), s.get("g")])
            out["k_mie_ms_" + label] = {"median": float(np.median(ms[1:])), "min": min(ms[1:]), "max": max(ms[1:]),
                                        "warm_up": ms[0], "launches": launches}
        out["guards_intact"] = s.guards_intact()
        out["order_changes_no_bit"] = bool(np.array_equal(results["sorted_by_terms"], results["table_order"]))
    finally:
        s.close()
        ctx.close()
    with tempfile.TemporaryDirectory() as wd:
        nk = os.path.join(wd, "nk.dat")
        with open(nk, "w") as f:
            for row in zip(lam, n, k):
                f.write("%.17g %.17g %.17g\n" % row)
        t0 = time.time()
        mie.main(["-refractive_index_file", nk, "-output_directory", os.path.join(wd, "mie")])
        out["whole_tool_seconds_device"] = time.time() - t0
    if "--no-numpy" not in argv:
        t0 = time.time()
        ref = mie.numpy_series(x, m_re, m_im)
        out["numpy_series_seconds"] = time.time() - t0
        out["numpy_threads"] = int(os.environ.get("OMP_NUM_THREADS", "0")) or None
        dev = results["sorted_by_terms"]
        out["device_vs_numpy"] = {"q_ext": float(np.abs(dev[0] / ref[0] - 1).max()), "q_sca": float(np.abs(dev[1] / ref[1] - 1).max()),
                                  "g": float(np.abs(dev[2] - ref[2]).max())}
    path = os.path.join(ROOT, "profiles", "mie_bench.json")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
