#!/usr/bin/env python3
"""Writes profiles/mie_parity.json: per golden case of tests/golden/mie/reference.npz the deviation of the long-double restatement
(tests/mie_reference.py) from the golden -- eight times the largest per quantity is what tests/test_mie_reference.py asserts --
and the deviations of `plain_fp64`, of the numpy backend and, with --device, of k_mie from the restatement, on which the bounds of
tests/test_mie.py and tests/test_gpu_mie.py rest.  Relative for Q_ext and Q_sca, absolute for g.

    python tools/mie_parity.py [--device] [--out FILE]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv):
    import mie_cases as mc
    from helios_amd import mie
    g = mc.goldens()
    gold = np.array([g["q_ext"], g["q_sca"], g["g"]])
    ld, f64 = mc.restated(g["m_re"], g["m_im"], g["x"])
    columns = {"restatement_vs_golden": mc.deviations(ld, gold), "plain_fp64": mc.deviations(f64, ld),
               "numpy_backend": mc.deviations(mie.numpy_series(g["x"], g["m_re"], g["m_im"]), ld)}
    if "--device" in argv:
        columns["device"] = mc.deviations(mie.device_series(g["x"], g["m_re"], g["m_im"]), ld)
        columns["device_vs_golden"] = mc.deviations(mie.device_series(g["x"], g["m_re"], g["m_im"]), gold)
    out = {"what": "deviations per golden case: relative for q_ext and q_sca, absolute for g; the columns other than "
                   "restatement_vs_golden and device_vs_golden are against the long-double restatement",
           "x_small": mie.X_SMALL,
           "largest": {k: {mc.NAMES[q]: float(v[q].max()) for q in range(3)} for k, v in columns.items()},
           "asserted_for_the_restatement": {mc.NAMES[q]: max(8.0 * float(columns["restatement_vs_golden"][q].max()), 1e-17)
                                            for q in range(3)},
           "cases": [dict(m_re=float(g["m_re"][p]), m_im=float(g["m_im"][p]), x=float(g["x"][p]), n_terms=int(g["n_terms"][p]),
                          **{k: [float(v[q][p]) for q in range(3)] for k, v in columns.items()}) for p in range(len(g["x"]))]}
    path = os.path.join(ROOT, "profiles", "mie_parity.json")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: out[k] for k in ("largest", "asserted_for_the_restatement")}, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
