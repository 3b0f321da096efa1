#!/usr/bin/env python3
"""Writes profiles/exomol_parity.json: exomol.py against lines.py on one list.  A synthetic ExoMol list with one broadener is
converted to the seven HITRAN-style fields -- s_ref = S(296 K) with Q(296), gamma_air = 1.01325 gamma (a bar against an
atmosphere), n_air = n, delta_air = 0, E'' = E[low] -- and the two long-double restatements (tests/exomol_reference.py,
tests/lines_reference.py) are compared per node: the largest relative deviation of kappa and of the four numbers per line.
tests/test_exomol_reference.py asserts what `measure` returns at the project's floor of 1e-13.

    python tools/exomol_parity.py [--out FILE]
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NODES = ((500.0, 1e3), (1000.0, 1e6), (2000.0, 1e7))


def converted(case):
    """the case's list as lines.FIELDS arrays; S(296) in long double, rounded once"""
    import exomol_reference as er
    import lines_reference as lr
    s_ref = er.strengths(case.states, case.trans, lr.T_REF, case.q(lr.T_REF), np.longdouble).astype(np.float64)
    x, table = case.broadening
    assert len(x) == 1 and x[0] == 1.0
    jx = case.states["jidx"][case.trans["low"]]
    n = len(s_ref)
    return {"nu0": case.trans["nu0"].copy(), "s_ref": s_ref, "gamma_air": 1.01325 * table[0, jx, 0], "gamma_self": np.zeros(n),
            "e_low": case.states["E"][case.trans["low"]], "n_air": table[0, jx, 1].copy(), "delta_air": np.zeros(n)}


def measure():
    import exomol_cases as ec
    import exomol_reference as er
    import lines_reference as lr
    case = ec.build("parity", ec.pattern("all", 300), grid=(1000.0, 0.05, 2000), cutoff=5.0, seed=77, nodes=NODES, s_min=0.0,
                    broadener_list=[("only", 1.0, ec.broad_rows(41, 0.6), 0.07, 0.5)])
    line = converted(case)
    out = {"what": "largest relative deviation between the long-double restatements of exomol.py and of lines.py on one list of "
                   "300 transitions, converted with s_ref = S(296), gamma_air = 1.01325 gamma, n_air = n, delta_air = 0",
           "floor": 1e-13, "nodes": []}
    for temp, press in NODES:
        q_t, q_ref = case.q(temp), case.q(lr.T_REF)
        kappa_e, prm_e, kept = er.long_double(case.states, case.trans, case.broadening, temp, press, q_t, case.molar_mass, 0.0,
                                              case.cutoff, *case.grid)
        assert len(kept) == 300
        kappa_l = lr.long_double(line, temp, press, q_t, q_ref, case.molar_mass, 0.0, case.cutoff, *case.grid)
        prm_l = lr.params(line, temp, press, q_t, q_ref, case.molar_mass, 0.0, np.longdouble)
        assert np.all(kappa_l > 0)
        out["nodes"].append({"T": temp, "P": press, "kappa": float(np.abs(kappa_e / kappa_l - 1).max()),
                             "line_params": [float(np.abs(prm_e[k] / prm_l[k] - 1).max()) for k in range(4)]})
    out["largest"] = max(max([n["kappa"]] + n["line_params"]) for n in out["nodes"])
    return out


def main(argv):
    out = measure()
    path = os.path.join(ROOT, "profiles", "exomol_parity.json")
    if "--out" in argv:
        path = argv[argv.index("--out") + 1]
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
