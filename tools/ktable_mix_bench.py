#!/usr/bin/env python3
"""Times the mixing stage of ktable.py (helios_amd/ktable_mix.py, csrc/ktable_mix.hip) and writes profiles/ktable_mix.json.

    python tools/ktable_mix_bench.py [-out profiles/ktable_mix.json] [-bins 322] [-tool yes|no]

Workload: 15 synthetic absorbers and 5 scatterers, water vapour among them, on the 120 x 28 grid at 322 bins x 20 Gauss points
(0.17 GB per table); 1 and 8 chemistries on the same resident tables.  One process.  Measured: k_ktmix_sum and k_ktmix_scat by
HIP events (medians of seven runs behind a warm-up), the achieved bytes per second against the (absorbers + 1)-tables traffic
model, a chemistry as the host sees it (mixing ratios up, both tables back), the upload of the tables, the numpy backend on the
same arrays, and -- `-tool yes` -- the whole tool including reading the containers and writing the tables.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from helios_amd import ktable, ktable_mix          # noqa: E402
from helios_amd.device import Context               # noqa: E402

ABSORBERS = ["H2O", "CO2", "CO", "CH4", "NH3", "HCN", "C2H2", "H2S", "PH3", "SO2", "TiO", "VO", "Na", "K", "CIA_H2H2"]
SCATTERERS = ["H2", "He", "H2O", "CO2", "CO"]          # H2O, CO2 and CO also absorb: 17 species in all
REPEATS = 7


def species_text():
    names = ABSORBERS + [n for n in SCATTERERS if n not in ABSORBERS]
    rows = []
    for k, n in enumerate(names):
        ratio = "0.8&0.8" if n.startswith("CIA") else "%.3e" % (0.8 if n == "H2" else 0.15 if n == "He" else 1e-3 / (k + 1))
        rows.append("%s %s %s %s" % (n, "yes" if n in ABSORBERS else "no", "yes" if n in SCATTERERS else "no", ratio))
    return "final species\nname absorbing scattering mixing_ratio\n" + "\n".join(rows) + "\n", names


def median(v):
    return float(np.median(v))


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("-out", default=os.path.join("profiles", "ktable_mix.json"))
    p.add_argument("-bins", type=int, default=322)
    p.add_argument("-tool", default="yes", choices=("yes", "no"))
    opt = p.parse_args(argv)
    temp, press = ktable.default_target_grid()
    nbin, ny = opt.bins, 20
    inter = 0.34e-4 * (200.0 / 0.34) ** (np.arange(nbin + 1) / nbin)
    centre, width, y = ktable.grid_datasets(inter, ny)
    grid = {"interface wavelengths": inter, "center wavelengths": centre, "wavelength width of bins": width, "ypoints": y}
    nodes, nc = len(temp) * len(press), nbin * ny
    text, names = species_text()
    ns = len(names)
    rng = np.random.default_rng(1)
    base = 10.0 ** rng.uniform(-12, 2, nodes * nc)
    rec = {"grid": [len(temp), len(press)], "bins": nbin, "gauss_points": ny, "table_bytes": nodes * nc * 8,
           "absorbers": len(ABSORBERS), "scatterers": len(SCATTERERS), "repeats": REPEATS}
    ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    rec["device"] = ctx.name()
    m = ktable_mix.Mixer(ctx, nbin, ny, len(temp), len(press), ns)
    try:
        m.set_grid(centre, temp, press)
        t0 = time.time()
        for s, n in enumerate(names):
            if n in ABSORBERS:
                m.set_species(s, base)                   # the same values in every slot: the traffic is what is measured
            if n in SCATTERERS:
                m.set_rayleigh(s, None if n == "H2O" else rng.uniform(1e-28, 1e-25, nbin), n == "H2O")
        rec["upload_seconds_15_tables"] = time.time() - t0
        chem = [(rng.uniform(1e-6, 1e-2, (ns, nodes)), rng.uniform(1e-6, 1.0, (ns, nodes))) for _ in range(8)]
        m.run(*chem[0])                                  # warm-up
        ms = []
        for _ in range(REPEATS):
            m.run(*chem[0])
            ms.append(m.get("timing_ms")[:2].copy())
        ms = np.array(ms)
        traffic = (len(ABSORBERS) + 1) * nodes * nc * 8
        rec["k_ktmix_sum_ms"] = {"median": median(ms[:, 0]), "min_max": [float(ms[:, 0].min()), float(ms[:, 0].max())]}
        rec["k_ktmix_scat_ms"] = {"median": median(ms[:, 1]), "min_max": [float(ms[:, 1].min()), float(ms[:, 1].max())]}
        rec["traffic_model_bytes"] = traffic
        rec["k_ktmix_sum_bytes_per_second"] = traffic / (median(ms[:, 0]) * 1e-3)
        for count in (1, 8):
            t = []
            for _ in range(3):
                t0 = time.time()
                for k in range(count):
                    m.run(*chem[k])
                    kp, sc = m.get("kpoints"), m.get("scat_cross")
                t.append(time.time() - t0)
            rec["chemistries_%d_seconds_incl_copy_back" % count] = median(t)
        dev_k, dev_s = kp, sc
    finally:
        m.close()
        ctx.close()
    # the numpy backend on the same arrays (the last chemistry), as a check of the device's result too
    tables = [base if n in ABSORBERS else None for n in names]
    t0 = time.time()
    host_k = ktable_mix.numpy_sum(tables, chem[7][0], nodes, nc)
    rec["numpy_sum_seconds"] = time.time() - t0
    rec["numpy_threads_env"] = os.environ.get("OMP_NUM_THREADS", "")
    rec["device_equals_numpy_bit_for_bit"] = bool(dev_k.tobytes() == host_k.tobytes())
    del host_k, dev_k, dev_s, tables
    if opt.tool == "yes":
        tmp = tempfile.mkdtemp()
        try:
            opac = os.path.join(tmp, "opac")
            os.makedirs(opac)
            with open(os.path.join(tmp, "species.dat"), "w") as f:
                f.write(text)
            t0 = time.time()
            for n in ABSORBERS:
                ktable.write_table(os.path.join(opac, n + "_opac_ip_kdistr.h5"),
                                   dict(grid, temperatures=temp, pressures=press, kpoints=base))
            rec["writing_15_input_containers_seconds"] = time.time() - t0
            argv = ["-mixed_table_production", "yes", "-path_to_final_species_file", os.path.join(tmp, "species.dat"),
                    "-directory_with_individual_files", opac, "-mixed_table_output_directory", os.path.join(tmp, "out")]
            for backend in ("hip", "numpy"):
                t0 = time.time()
                out = ktable.main(argv + ["-backend", backend])
                rec["tool_seconds_%s" % backend] = time.time() - t0
                rec["tool_container"] = os.path.splitext(out[-1])[1][1:]
            t0 = time.time()
            ktable.main(argv + ["-sweep", "path_to_fastchem_output=" + ",".join(["none/"] * 8)])
            rec["tool_seconds_hip_8_chemistries"] = time.time() - t0
        except (IOError, OSError) as e:
            rec["tool_error"] = str(e)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(opt.out) or ".", exist_ok=True)
    with open(opt.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
    print(json.dumps(rec, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
