"""The mixing stage's contract (helios_amd/ktable_mix.py, include/helios_hip.h section 9) restated plainly in np.longdouble:
interpolation weights, mass mixing ratios, the weighted sum and the water formula in extended precision, rounded once.  Of the
project it takes the species' weights and two physical constants, nothing else: no plan, no branch order, no backend.  Also
the seeded inputs of the golden cases (tests/golden/make_mixed_golden.py writes them, tests/test_ktable_mix.py reads them
back) and the directory a case's inputs make."""
import os

import numpy as np

from ktable_reference import LD, reference_regrid, require_extended_precision

from helios_amd import phys_const as pc
from helios_amd.species_data import species_lib

H2O_A = ("0.244257733", "0.974634476e-2", "-0.373234996e-2", "0.268678472e-3", "0.158920570e-2", "0.245934259e-2",
         "0.900704920", "-0.166626219e-1")
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ktable_mix")


def ld(text):
    """a decimal literal as the DOUBLE the contract's arithmetic starts from, held in long double"""
    return LD(np.float64(text))


def is_pair(name):
    return "CIA" in name or name in ("H-_ff", "He-")


def reference_vmr(chem_temp, chem_press, column, temp, press):
    """a chemistry column [p + np_chem * t] on the final grid, long double [nodes]"""
    return reference_regrid(chem_temp, chem_press, np.asarray(column, np.float64), temp, press, 1).reshape(-1)


def reference_h2o(wave, temp, press, f):
    """sigma [node][x] in long double; f[node] long double; 0 beyond 2.5 micron and where f is 0"""
    require_extended_precision()
    wave = np.asarray(wave, np.float64)
    T = np.repeat(np.asarray(temp, np.float64), len(press)).astype(LD)[:, None]
    P = np.tile(np.asarray(press, np.float64), len(temp)).astype(LD)[:, None]
    f = np.asarray(f, LD)[:, None]
    lam = wave.astype(LD)[None, :]
    a = [ld(v) for v in H2O_A]
    kt = LD(np.float64(pc.K_B)) * T
    m = LD(np.float64(species_lib["H2O"].weight)) * LD(np.float64(pc.AMU))
    with np.errstate(all="ignore"):
        delta = f * P * m / kt
        n_ref = f * P / kt
        theta = T / ld("273.15")
        L2 = (lam / ld("0.589e-4")) ** 2
        A = delta * (a[0] + a[1] * delta + a[2] * theta + a[3] * L2 * theta + a[4] / L2 + a[5] / (L2 - ld("0.229202") ** 2)
                     + a[6] / (L2 - ld("5.432937") ** 2) + a[7] * delta ** 2)
        king = (6 + 3 * ld("3e-4")) / (6 - 7 * ld("3e-4"))
        sig = 24 * LD(np.pi) ** 3 / (n_ref ** 2 * lam ** 4) * A ** 2 * king
    return np.where((wave[None, :] <= 2.5e-4) & (f != 0), sig, LD(0))


def reference_sum(tables, mmr, nodes, nc):
    """sum_s m_s k_s in long double, rounded once; `tables`: per species None or the table on the final grid (fp64 or LD)"""
    require_extended_precision()
    acc = np.zeros((nodes, nc), LD)
    for k, m in zip(tables, mmr):
        if k is not None:
            acc += np.asarray(m, LD)[:, None] * np.asarray(k).astype(LD).reshape(nodes, nc)
    return acc.astype(np.float64).reshape(-1)


def reference_scat(sigmas, x, wave, temp, press):
    """`sigmas`: per species None, sigma[nbin] or "H2O"; x[s][node] long double"""
    nodes = len(temp) * len(press)
    acc = np.zeros((nodes, len(wave)), LD)
    for sig, xs in zip(sigmas, x):
        if sig is None:
            continue
        xs = np.asarray(xs, LD)
        if isinstance(sig, str):
            acc += xs[:, None] * reference_h2o(wave, temp, press, xs)
        else:
            acc += xs[:, None] * np.asarray(sig, np.float64).astype(LD)[None, :]
    return acc.astype(np.float64).reshape(-1)


def shuffled(species):
    """the first absorbing species in front"""
    first = [i for i, sp in enumerate(species) if sp[1] == "yes"][0]
    return [species[first]] + species[:first] + species[first + 1:]


def reference_case(case, tables, sigmas):
    """the data sets of the mixed file (CGS) from a case's inputs.  `tables`: name -> ("final", k) or ("native", T, P, k);
    `sigmas`: name -> sigma[nbin] (water needs none).  Returns kpoints, the Rayleigh table and mu as doubles, rounded once."""
    temp, press = case["temperatures"], case["pressures"]
    nodes, nbin = len(temp) * len(press), len(case["center wavelengths"])
    nc = nbin * len(case["ypoints"])
    species = shuffled(case["species"])
    chem = case.get("chem")
    fastchem = any(sp[3] == "FastChem" for sp in species)

    def column(name):
        return reference_vmr(chem["temp"], chem["press"], chem["columns"][name], temp, press)
    x, x2 = [], []
    for name, _a, _s, ratio in species:
        if ratio == "FastChem":
            names = species_lib[name].fc_name.split("&") if is_pair(name) else [species_lib[name].fc_name]
            cols = [column(n) for n in names]
        else:
            cols = [np.full(nodes, LD(np.float64(float(v)))) for v in ratio.split("&")]
        x.append(cols[0])
        x2.append(cols[1] if is_pair(name) else np.ones(nodes, LD))
    if fastchem:
        mu = column("mu")
    else:
        single = [(LD(np.float64(float(sp[3]))), LD(np.float64(species_lib[sp[0]].weight))) for sp in species if "&" not in sp[3]]
        mu = np.full(nodes, sum(a * w for a, w in single) / sum(a for a, w in single))
    mmr = [x[s] * x2[s] * LD(np.float64(species_lib[sp[0]].weight)) / mu for s, sp in enumerate(species)]
    on_grid = []
    for name, absorbing, _s, _r in species:
        if absorbing != "yes":
            on_grid.append(None)
        elif tables[name][0] == "final":
            on_grid.append(tables[name][1])
        else:
            _kind, T, P, k = tables[name]
            on_grid.append(reference_regrid(T, P, k, temp, press, nc).reshape(-1))
    sig = [None if sp[2] != "yes" else ("H2O" if sp[0] == "H2O" else sigmas.get(sp[0])) for sp in species]
    return {"kpoints": reference_sum(on_grid, mmr, nodes, nc),
            "weighted Rayleigh cross-sections": reference_scat(sig, x, case["center wavelengths"], temp, press),
            "meanmolmass": np.asarray(mu, LD).astype(np.float64)}


def relative_deviation(got, want):
    """largest |got - want| / |want| over the entries with want != 0; inf where want is 0 and got is not"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    zero = want == 0
    if np.any(got[zero] != 0):
        return float("inf")
    if zero.all():
        return 0.0
    with np.errstate(all="ignore"):
        return float(np.max(np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])))


# ---- the golden cases' inputs -------------------------------------------------------------------------------------------------------
INTERFACES = np.array([0.4e-4, 0.9e-4, 1.7e-4, 3.3e-4, 12e-4])        # cm; the third bin's centre is 2.5 micron, the limit
N_GAUSS = 3
SPECIES_A = [("H2", "no", "yes", "FastChem"), ("H2O", "yes", "yes", "FastChem"), ("CO2", "yes", "yes", "3.5e-4"),
             ("CIA_H2H2", "yes", "no", "FastChem"), ("He", "no", "yes", "0.15"), ("H-_bf", "yes", "no", "FastChem"),
             ("H-_ff", "yes", "no", "FastChem"), ("He-", "yes", "no", "FastChem")]
SPECIES_C = [("H2", "no", "yes", "0.84"), ("H2O", "yes", "yes", "1e-3"), ("CO2", "yes", "yes", "3.5e-4"),
             ("CIA_H2H2", "yes", "no", "0.84&0.84"), ("He", "no", "yes", "0.15"), ("H-_bf", "yes", "no", "1e-9"),
             ("H-_ff", "yes", "no", "1e-4&1e-8"), ("He-", "yes", "no", "0.15&1e-8")]
CHEM_T = [100.0, 725.0, 2000.0, 3000.0]                 # narrower than the final grid; 100, 2000 and 3000 K are its nodes
CHEM_PBAR = [1e-5, 3e-3, 1.0, 100.0]                    # 1e1, 1e6 and 1e8 dyne cm^-2 are nodes of the final grid
CHEM_COLUMNS = ["H2", "H2O1", "He", "H", "e-", "H1-"]
NATIVE = {"H2O": ([40.0, 1000.0, 7000.0], [0.5, 1e3, 2e9]),            # nodes below, inside and above the final grid
          "CO2": ([300.0, 2500.0], [1e2, 1e7]),
          "CIA_H2H2": ([200.0, 3000.0], [1e0, 1e6])}


def chemistry(seed=11):
    rng = np.random.default_rng(seed)
    n = len(CHEM_T) * len(CHEM_PBAR)
    scale = {"H2": 0.8, "H2O1": 1e-3, "He": 0.15, "H": 1e-4, "e-": 1e-8, "H1-": 1e-10}
    cols = {k: scale[k] * 10 ** rng.uniform(-0.5, 0.05, n) for k in CHEM_COLUMNS}
    cols["mu"] = rng.uniform(2.2, 2.5, n)
    return cols


def chem_text(cols, rows):
    """the text of a FastChem output file holding the rows `rows` (entry p + np * t)"""
    head = "#P(bar) T(k) n_<tot>(cm-3) n_g(cm-3) m(u) " + " ".join(CHEM_COLUMNS)
    lines = [head]
    for r in rows:
        t, p = r // len(CHEM_PBAR), r % len(CHEM_PBAR)
        vals = [CHEM_PBAR[p], CHEM_T[t], 1e15, 1e15, cols["mu"][r]] + [cols[k][r] for k in CHEM_COLUMNS]
        lines.append(" ".join("%.17e" % v for v in vals))
    return "\n".join(lines) + "\n"


def chem_parsed(text_parts):
    """the columns as a reader of the text gets them (17 digits: the doubles themselves)"""
    rows = [[float(v) for v in line.split()] for part in text_parts for line in part.splitlines()[1:] if line.strip()]
    a = np.array(rows)
    cols = {k: a[:, 5 + i] for i, k in enumerate(CHEM_COLUMNS)}
    cols["mu"] = a[:, 4]
    return {"temp": np.array(CHEM_T), "press": np.array([p * 1e6 for p in CHEM_PBAR]), "columns": cols}


def species_text(species):
    return "final species\nname absorbing scattering mixing_ratio\n" + "".join("%s %s %s %s\n" % sp for sp in species)


def native_table(name, nc, seed=5):
    """1e-15 ... 1e3 with exact zeros among them"""
    T, P = NATIVE[name]
    rng = np.random.default_rng(seed + len(name))
    k = 10.0 ** rng.uniform(-15, 3, len(T) * len(P) * nc)
    k[rng.random(k.size) < 0.05] = 0.0
    return k


def cia_ip_table(nodes, nc):
    """a table that is already on the final grid: exact binary fractions, zeros among them"""
    node, e = np.arange(nodes)[:, None], np.arange(nc)[None, :]
    k = ((node * 7 + e * 13) % 1009 + 1) * 2.0 ** -20
    k[(node + e) % 17 == 0] = 0.0
    return k.reshape(-1)


def grid_arrays():
    centre = (INTERFACES[:-1] + INTERFACES[1:]) / 2
    y = np.array([0.5 * v + 0.5 for v in np.polynomial.legendre.leggauss(N_GAUSS)[0]])
    return {"interface wavelengths": INTERFACES, "center wavelengths": centre,
            "wavelength width of bins": INTERFACES[1:] - INTERFACES[:-1], "ypoints": y}


def write_inputs(root, species, chem_files, containers, writer):
    """a species file, FastChem files and containers under `root`; `writer(path_without_extension, datasets)`"""
    os.makedirs(os.path.join(root, "opac"), exist_ok=True)
    os.makedirs(os.path.join(root, "chem"), exist_ok=True)
    with open(os.path.join(root, "final_species.dat"), "w") as f:
        f.write(species_text(species))
    for name, text in chem_files.items():
        with open(os.path.join(root, "chem", name), "w") as f:
            f.write(text)
    for stem, data in containers.items():
        writer(os.path.join(root, "opac", stem), data)
