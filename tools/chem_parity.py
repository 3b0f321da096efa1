#!/usr/bin/env python3
"""Writes profiles/chem_parity.json.  (a) On the CPU: the reference script's own deviation (eps_ref) from the long-double
restatement of chem.py's contract, per species, over the 200 cases of its figure (tests/golden/chem/reference.npz), next to the
numpy backend's; every case is held to max(1e-13, 8 eps_ref) on the way (tests/test_chem.py).  (b) With a GPU: chem.py on the
device and with the numpy backend, both through the device's mixing stage of ktable.py -- the largest relative difference of
kpoints and meanmolmass and the bound the chemistry's tolerance implies (tests/chem_cases.py).

    python tools/chem_parity.py [--out FILE] [--no-device]
"""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv):
    import chem_cases as cc
    import chem_reference as cr
    import test_chem
    from helios_amd import chem
    out = {"case": "800 K and 3000 K at 1 bar, n_O = 5e-4, 100 values of C/O from 0.1 to 10; abundances per H2",
           "rule": "max(1e-13, 8 eps_ref) per entry, all 200 cases"}
    parity = test_chem.golden_parity(chem.GibbsTable(*cr.golden_table()))
    out["eps_ref"] = {k: v[0] for k, v in parity.items()}
    out["numpy_backend"] = {k: v[1] for k, v in parity.items()}
    if "--no-device" not in argv:
        wd = tempfile.mkdtemp(prefix="chem_parity_")
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                diff = cc.chain_difference(wd)
        finally:
            shutil.rmtree(wd, ignore_errors=True)
        k_bound, mu_bound = cc.chain_bound()
        out["chain_device_against_numpy_chemistry"] = {
            "case": "C/O 1.1, 6 x 4 nodes, five absorbers of 4 bins x 3 Gauss points, mixing stage on the device",
            "kpoints": diff["kpoints"], "kpoints_bound": k_bound, "meanmolmass": diff["meanmolmass"], "meanmolmass_bound": mu_bound}
    target = os.path.join(ROOT, "profiles", "chem_parity.json")
    if "--out" in argv:
        target = argv[argv.index("--out") + 1]
    with open(target, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
