#!/usr/bin/env python3
"""Writes profiles/lines_parity.json: K(x, y) of lines.py against the goldens of tests/golden/lines/voigt.npz (mpmath), per region
of |z| -- the largest relative deviation of the long-double restatement (tests/lines_reference.py), of `plain_fp64`, of the numpy
backend and, with --device, of the kernel's own K (hx_lines_voigt), with the pair it lies at and the bound that
tests/test_lines_reference.py and tests/test_gpu_lines.py hold it to -- and the deviations of plain_fp64, the numpy backend and the
kernel from the restatement, on which the rule max(1e-13, 8 eps) rests.

    python tools/lines_parity.py [--device] [--out FILE]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REGIONS = ("weideman", "eight_levels", "four_levels", "two_levels")


def main(argv):
    import lines_cases as lc
    import lines_reference as lr
    from helios_amd import lines
    g = lc.goldens()
    x, y, gold = g["x"], g["y"], g["k"].astype(np.longdouble)
    ld = lr.voigt_k(x, y, np.longdouble)
    columns = {"restatement": ld, "plain_fp64": lr.voigt_k(x, y, np.float64), "numpy_backend": lines.voigt_k(x, y)}
    if "--device" in argv:
        from helios_amd.device import Context
        ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
        try:
            columns["device"] = lines.device_voigt(ctx, x, y)
        finally:
            ctx.close()
    reg = lr.region(x, y)
    bounds = (lc.GOLDEN_BOUND, lc.GOLDEN_BOUND, lc.GOLDEN_BOUND_OUTER, lc.GOLDEN_BOUND_OUTER)
    out = {"what": "largest relative deviation per region of |z|: vs_golden against mpmath, vs_restatement against the long-double "
                   "restatement", "pairs": int(len(x)), "regions": {}}
    for r, name in enumerate(REGIONS):
        m = reg == r
        row = {"pairs": int(m.sum()), "bound": bounds[r], "vs_golden": {}, "vs_restatement": {}}
        for k, v in columns.items():
            dev = np.abs(np.asarray(v, np.longdouble)[m] / gold[m] - 1)
            j = int(np.argmax(dev))
            row["vs_golden"][k] = {"largest": float(dev[j]), "x": float(x[m][j]), "y": float(y[m][j]),
                                   "within_bound": bool(dev[j] <= bounds[r])}
            if k != "restatement":
                row["vs_restatement"][k] = float(np.abs(np.asarray(v, np.longdouble)[m] / ld[m] - 1).max())
        out["regions"][name] = row
    path = os.path.join(ROOT, "profiles", "lines_parity.json")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
