#!/usr/bin/env python3
"""Writes profiles/chem_bench.json: the 120 x 28 final grid of the k-table tools (T = 50 ... 6000 K step 50, 1e-6 ... 1e3 bar)
clipped to the Gibbs table's 500 ... 3000 K -- 51 x 28 nodes -- with 1 and with 64 chemistries (C/O from 0.1 to 10 at solar O/H).

One process, medians of seven runs behind a warm-up.  (a) k_chem_nodes by HIP events, one launch per run.  (b) the whole tool,
chem.main with the device backend, by the wall clock: context, kernel, and the `chem.dat` files of 17 digits.  (c) the same with
the numpy backend.  (d) the numpy backend's arithmetic alone (chem.cho_chemistry), and the file writing alone.

    python tools/chem_bench.py [--out FILE]
"""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

RUNS = 7
CHEMISTRIES = (1, 64)


def stats(a):
    a = np.asarray(a, np.float64)
    return {"median": float(np.median(a)), "min": float(a.min()), "max": float(a.max())}


def timed(fn):
    t0 = time.time()
    fn()
    return time.time() - t0


def main(argv):
    import chem_reference as cr
    from helios_amd import chem, ktable
    from helios_amd.device import Context
    table = chem.GibbsTable(*cr.golden_table())
    temp, press = ktable.default_target_grid()
    temp = temp[(temp >= table.temp[0]) & (temp <= table.temp[-1])]
    press = press * 1e-6
    n_nodes = len(temp) * len(press)
    out = {"case": "%d x %d nodes (the final grid clipped to %g ... %g K), %d Gibbs rows" % (len(temp), len(press), table.temp[0],
                                                                                            table.temp[-1], len(table.temp)),
           "nodes": n_nodes, "runs": RUNS}
    wd = tempfile.mkdtemp(prefix="chem_bench_")
    try:
        gibbs = chem.write_gibbs_file(os.path.join(wd, "gibbs.dat"), *cr.golden_table())
        grid = os.path.join(wd, "grid_opac_ip_kdistr.npz")
        np.savez(grid, **{"interface wavelengths": np.array([1e-4, 2e-4]), "center wavelengths": np.array([1.5e-4]),
                          "wavelength width of bins": np.array([1e-4]), "ypoints": np.array([0.5]), "pressures": press * 1e6,
                          "temperatures": temp, "kpoints": np.zeros(n_nodes)})
        ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
        out["device"] = ctx.name()
        try:
            for n_chem in CHEMISTRIES:
                o = np.full(n_chem, chem.O_TO_H_SOLAR)
                c = o * (np.logspace(-1.0, 1.0, n_chem) if n_chem > 1 else 0.55)
                h = chem.ChemDevice(ctx, len(table.temp), n_nodes, n_chem)
                try:
                    h.set_table(table)
                    kernel = []
                    for _ in range(RUNS + 1):                               # the first repeat is the warm-up
                        h.set_nodes(np.repeat(temp, len(press)), np.tile(press, len(temp)))
                        h.run(o, c, 0.085)
                        kernel.append(float(h.get("timing_ms")[0]))
                    vmr = h.get("vmr")
                finally:
                    h.close()
                host = chem.cho_chemistry(table, temp, press, o, c, 0.085, "numpy")
                dev = np.max([np.max(np.abs(vmr[:, j].reshape(host[k].shape) / host[k] - 1)) for j, k in enumerate(chem.KEYS)])
                sweep = [] if n_chem == 1 else ["-sweep", "c_to_o=" + ",".join(repr(float(v)) for v in np.logspace(-1.0, 1.0, n_chem))]

                def tool(backend, tag):
                    with contextlib.redirect_stdout(io.StringIO()):
                        chem.main(["-gibbs_file", gibbs, "-grid_like", grid, "-output_directory", os.path.join(wd, tag),
                                   "-backend", backend] + sweep)
                whole = {b: [timed(lambda: tool(b, "%s_%d" % (b, n_chem))) for _ in range(RUNS + 1)] for b in ("device", "numpy")}
                arithmetic = [timed(lambda: chem.cho_chemistry(table, temp, press, o, c, 0.085, "numpy")) for _ in range(RUNS + 1)]
                files = [timed(lambda: [chem.write_fastchem_directory(os.path.join(wd, "files_%d" % k), temp, press, host, k)
                                        for k in range(n_chem)]) for _ in range(RUNS + 1)]
                k_ms = float(np.median(kernel[1:]))
                out["%d_chemistries" % n_chem] = {
                    "k_chem_nodes_ms": dict(stats(kernel[1:]), warm_up=kernel[0]),
                    "k_chem_nodes_ns_per_node_and_chemistry": k_ms * 1e6 / (n_nodes * n_chem),
                    "bytes_stored_by_arithmetic": n_nodes * n_chem * chem.PLANES * 8,
                    "stored_gb_per_s": n_nodes * n_chem * chem.PLANES * 8 / (k_ms * 1e-3) / 1e9,
                    "tool_device_seconds": dict(stats(whole["device"][1:]), warm_up=whole["device"][0]),
                    "tool_numpy_seconds": dict(stats(whole["numpy"][1:]), warm_up=whole["numpy"][0]),
                    "numpy_backend_arithmetic_seconds": dict(stats(arithmetic[1:]), warm_up=arithmetic[0]),
                    "writing_the_files_seconds": dict(stats(files[1:]), warm_up=files[0]),
                    "device_against_numpy_largest_relative_difference": float(dev)}
        finally:
            ctx.close()
    finally:
        shutil.rmtree(wd, ignore_errors=True)
    target = os.path.join(ROOT, "profiles", "chem_bench.json")
    if "--out" in argv:
        target = argv[argv.index("--out") + 1]
    with open(target, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main(sys.argv[1:])
