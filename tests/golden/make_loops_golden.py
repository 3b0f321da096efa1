"""Record what the four hand-written host drivers of the device-resident loops did, call for call, on a scripted device
(tests/scripted_device.py): tests/golden/loops/single.json and sweep.json.

The four drivers -- `Compute.radiation_loop`, `Compute._convection_loop_fused`, `sweep._radiation_loop` and
`sweep._convection_loop` -- existed up to the commit that introduced helios_amd/loops.py; this script was run on the commit
before it and refuses to run where they are gone.  tests/test_loops.py holds the one driver that replaced them to these
transcripts.

    python tests/golden/make_loops_golden.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.join(HERE, "..", ".."), os.path.join(HERE, "..")]

import scripted_device as sd                     # noqa: E402
from helios_amd import sweep                      # noqa: E402


def single(computer, quants, rt, write):
    computer.radiation_loop(quants[0], write, None)
    computer.convection_loop(quants[0], write, None)


def swept(computer, quants, rt, write):
    sweep._radiation_loop(computer, quants, rt)
    sweep._convection_loop(computer, quants, rt)


if __name__ == "__main__":
    if not hasattr(sweep, "_radiation_loop"):
        raise SystemExit("the four former drivers are gone from this commit: the transcripts are recorded on the commit "
                         "before helios_amd/loops.py")
    out = os.path.join(HERE, "loops")
    os.makedirs(out, exist_ok=True)
    for name, scenarios, single_run, drive in (("single", sd.SINGLE, True, single), ("sweep", sd.SWEEP, False, swept)):
        rec = {k: sd.transcript(s, single_run, drive) for k, s in scenarios.items()}
        with open(os.path.join(out, name + ".json"), "w") as f:
            json.dump(rec, f, indent=0, sort_keys=True)
            f.write("\n")
        print(name, {k: len(v["calls"]) for k, v in rec.items()})
