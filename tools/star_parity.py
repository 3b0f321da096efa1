#!/usr/bin/env python3
"""Writes profiles/star_parity.json: per golden run of the reference's star tool the black-body temperature it fitted, the
long-double restatement's from the same bin flux, their relative deviation -- eight times the largest is the margin
tests/test_star.py holds the numpy backend's fitted temperature to -- and the numpy backend's own deviation.  No GPU."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import test_star
    runs = test_star.parity_figures()
    out = {"what": "fitted black-body temperatures [K]: reference (numpy 1.26) vs the long-double restatement fed with the same "
                   "bin flux; deviations are relative",
           "margin": 8 * max(v["reference_deviation"] for v in runs.values()), "runs": runs}
    path = os.path.join(ROOT, "profiles", "star_parity.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
