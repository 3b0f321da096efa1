"""Parameter sweeps: many independent atmosphere columns through ONE device-resident batch per GPU.

The reference runs one column per process (helios.py).  Columns of a sweep share the wavelength grid, the opacity
tables and the physics switches and differ in planet / star / orbit / internal temperature / albedo / start profile --
exactly what `RTBatch` keeps per column -- so a sweep is one batch whose kernels loop over the columns
(BASELINE config 4).  With several GPUs the columns are block-partitioned over the ranks
(`parallel.shard_columns`); the iteration path has no collective, the emission spectra are gathered once at the end.

    python sweep.py -sweep "internal_temperature=100,300,1000;f_factor=0.25,0.5" [helios.py options ...]

Every column gets the full set of output files under `<output>/<name>_<k>/`, exactly as a single run would write them.
"""
import hashlib
import itertools
import os

import numpy as np

from . import additional_heating as add_heat
from . import computation as comp
from . import host_functions as hsfunc
from . import loops
from . import quantities as quant_mod
from . import read as read_mod
from . import write as write_mod

# options that may vary between the columns of one batch (everything else defines the batch itself)
# (directory_with_fastchem_files: every column reads its own chemistry -- a sweep over metallicity or C/O -- and keeps its own
# (T, P) mixing-ratio tables on the device, hx_rt_set_column_vmr_table; path_to_opacity_file: the same sweep on the premixed
# path, one premixed k-table file per chemistry -- every distinct table is resident once per GPU and every column reads its
# own, hx_rt_add_premixed_tables / hx_rt_set_column_table)
# (the cloud options: every column describes its own decks -- aerosol, size distribution, base and vertical profile; several
# decks are space-separated inside one value, as on the command line: "aerosol_radius_mode=1 5,10 5" is two columns of two
# decks.  The number of decks defines the batch.  The planes are built on the device per column from Mie tables resident once
# per batch, hx_rt_add_mie_table / hx_rt_set_column_cloud_decks -- or on the host, HELIOS_CLOUD_DECKS)
CLOUD_OPTIONS = ("path_to_mie_files", "aerosol_radius_mode", "aerosol_radius_geometric_std_dev", "cloud_bottom_pressure",
                 "cloud_bottom_mixing_ratio", "cloud_to_gas_scale_height_ratio", "path_to_file_with_cloud_data", "aerosol_name")
PER_COLUMN_OPTIONS = ("internal_temperature", "f_factor", "stellar_zenith_angle", "surface_albedo", "surface_gravity",
                      "orbital_distance", "radius_planet", "radius_star", "temperature_star",
                      "radiative_equilibrium_criterion", "directory_with_fastchem_files", "path_to_opacity_file",
                      "dataset_in_stellar_spectrum_file", "path_to_stellar_spectrum_file", "name") + CLOUD_OPTIONS

_TABLE_NAMES = ("opacity_mixing", "opac_k", "opac_scat_cross", "opac_meanmass", "opac_wave", "opac_interwave",
                "opac_deltawave", "gauss_y", "ktemp", "kpress", "nbin", "ny", "ntemp", "npress")


def expand_sweep(spec):
    """'key=v1,v2;key2=w1,w2' -> list of {key: value} dicts, the cartesian product in the order given"""
    axes = []
    for part in [p for p in str(spec).split(";") if p.strip()]:
        key, values = part.split("=", 1)
        key = key.strip().lstrip("-")
        if key not in PER_COLUMN_OPTIONS:
            raise ValueError("option '%s' cannot vary inside one batch; allowed: %s" % (key, ", ".join(PER_COLUMN_OPTIONS)))
        axes.append([(key, v.strip()) for v in values.split(",") if v.strip()])
    return [dict(combo) for combo in itertools.product(*axes)] if axes else [{}]


def cloud_deck_mode(overrides_list):
    """where the cloud planes of a sweep's columns are built, HELIOS_CLOUD_DECKS=host|device: on the host by
    Cloud.cloud_pre_processing and uploaded, or on the device from the deck descriptions.  Default: device when a cloud option
    is among the sweep's axes, host otherwise (no result of a sweep without a cloud axis moves)"""
    mode = os.environ.get("HELIOS_CLOUD_DECKS")
    if mode is None:
        return "device" if any(k in CLOUD_OPTIONS for ov in overrides_list for k in ov) else "host"
    if mode not in ("host", "device"):
        raise ValueError("HELIOS_CLOUD_DECKS=%s: the cloud planes are built on 'host' or 'device'" % mode)
    return mode


def _table_entry(keeper):
    """what a table file leaves on the Store that read it, as the entry the Stores of a sweep share: the arrays in the form
    Store.convert_input_list_to_array gives input arrays, made here ONCE, so that host memory holds each table once and
    `make_rt_batch` can tell the distinct tables of a batch by the identity of their arrays"""
    entry = {}
    for n in _TABLE_NAMES:
        if hasattr(keeper, n):
            v = getattr(keeper, n)
            entry[n] = keeper.as_input_array(v) if isinstance(v, (np.ndarray, list, tuple)) else v
    return entry


def _read_star(reader, keeper, shared):
    """Read.read_star with every stellar spectrum file opened once per process: the columns of a sweep over
    dataset_in_stellar_spectrum_file name data sets of the same file (star.py writes them side by side)"""
    files = shared.setdefault("stellar_files", {})

    def opened(path):
        key = os.path.realpath(str(path))
        if key not in files:
            files[key] = read_mod.Read._open_table(path)
        return files[key]
    reader._open_table = opened
    try:
        reader.read_star(keeper)
    finally:
        del reader._open_table


def _prepare_column(base_argv, overrides, shared):
    """the read -> grid -> start-profile part of helios.py:35-83 for one column; every distinct table file is read once per
    process (`shared`, which lives as long as its run_sweep) and its arrays are shared by the Stores that name it"""
    reader = read_mod.Read()
    keeper = quant_mod.Store()
    argv = list(base_argv)
    for k, v in overrides.items():
        argv += ["-" + k, str(v)]
    reader.read_param_file_and_command_line(keeper, reader.cloud, argv)
    reader.check_run_configuration(keeper)
    tables = shared.setdefault("tables", {})
    if keeper.opacity_mixing in ("premixed", "synthetic"):
        # one entry per table FILE (and what is made of it: "no atmosphere" discards the opacities, read.py:445)
        if keeper.opacity_mixing == "synthetic" or str(reader.ktable_path) == "synthetic":
            key = ("synthetic", str(reader.synthetic_spec))
        else:
            key = (os.path.realpath(str(reader.ktable_path)), int(getattr(keeper, "no_atmo_mode", 0)))
        if key not in tables:
            reader.load_premixed_opacity_table(keeper)
            tables[key] = _table_entry(keeper)
    else:
        if "path_to_opacity_file" in overrides:
            raise ValueError("a sweep over path_to_opacity_file varies the PREMIXED table; with opacity mixing = on-the-fly the "
                             "option has no meaning (sweep over directory_with_fastchem_files there)")
        key = "species"
        if key not in tables:
            reader.read_species_file(keeper)
            reader.read_species_opacities(keeper)
            reader.read_species_scat_cross_sections(keeper)
            tables[key] = _table_entry(keeper)
            shared["species_template"] = keeper.species_list
    for n, v in tables[key].items():      # (the Store that read the file too: it takes the entry's arrays)
        setattr(keeper, n, v)
    if keeper.opacity_mixing == "on-the-fly":
        import copy
        keeper.species_list = [copy.copy(sp) for sp in shared["species_template"]]   # tables shared, VMR profiles own
        reader.read_species_mixing_ratios(keeper)
    reader.read_kappa_table_or_use_constant_kappa(keeper)
    reader.read_or_fill_surf_albedo_array(keeper)
    keeper.dimensions()
    _read_star(reader, keeper, shared)
    hsfunc.planet_param(keeper, reader)
    hsfunc.set_up_numerical_parameters(keeper)
    hsfunc.construct_grid(keeper)
    hsfunc.initial_temp(keeper, reader)
    if keeper.approx_f == 1 and keeper.planet_type == "rocky":      # helios.py:70-71
        hsfunc.approx_f_from_formula(keeper, reader)
    hsfunc.calc_F_intern(keeper)
    add_heat.load_heating_terms_or_not(keeper)
    if shared.get("cloud_decks", "host") == "device" and keeper.clouds == 1:
        # the decks' description only: the planes are built on the device (make_rt_batch); a Mie directory is read once per
        # process, as the table files are
        reader.cloud.cloud_deck_description(keeper, shared.setdefault("mie", {}))
    else:
        reader.cloud.cloud_pre_processing(keeper)
    keeper.create_zero_arrays()
    # the table's arrays are in their final form already and stay ONE per process (_table_entry)
    keeper.convert_input_list_to_array(skip=[n for n, v in tables[key].items() if isinstance(v, np.ndarray)])
    return keeper, reader


def _table_grid_digest(q):
    """the sampling of the column's opacity table: wavelength bins, Gauss points and the (T, P) nodes.  A batch has ONE grid
    (hx_rt_set_grid); tables on the same grid may differ from column to column"""
    h = hashlib.sha1()
    for n in ("opac_interwave", "gauss_y", "ktemp", "kpress"):
        v = getattr(q, n, None)
        h.update(b"-" if v is None else np.ascontiguousarray(np.asarray(v, np.float64)).tobytes())
        h.update(b"|")
    return h.hexdigest()


def _batch_signature(q):
    # (the species list and where each species' mixing ratio comes from: a batch shares the opacity tables and hands the
    # device one (T, P) chemistry table per column for the FastChem species -- which species those are must agree)
    chem = tuple((str(getattr(sp, "name", "")), str(getattr(sp, "source_for_vmr", "")))
                 for sp in (getattr(q, "species_list", None) or [])) if str(q.opacity_mixing) == "on-the-fly" else ()
    return (int(q.nbin), int(q.ny), int(q.nlayer), int(q.scat), int(q.dir_beam), int(q.clouds), int(q.scat_corr),
            int(q.smooth), int(q.convection), str(q.opacity_mixing), float(q.g_0), float(q.epsi), str(q.planet_type),
            int(q.iso), int(q.singlewalk), str(q.flux_calc_method), chem, _table_grid_digest(q),
            int(getattr(q, "real_star", 0)))      # (a flag of the whole batch: black-body stars and spectra from a file do not mix)


def _finish_column(computer, q, reader, writer):
    """post-loop diagnostics and output files of one column (helios.py:88-126), on the Store's own device arrays"""
    if getattr(q, "cloud_decks", None) is not None and q.clouds == 1:
        # planes built on the device: the diagnostics and the output files read them from the Store
        for n in ("abs_cross_all_clouds", "scat_cross_all_clouds", "g_0_all_clouds"):
            for lev in ("_lay", "_int"):
                setattr(q, n + lev, q.rt.get(n + lev, q.rt_col))
    tables = {n: getattr(q, n, None) for n in ("opac_k", "opac_scat_cross", "opac_meanmass")}
    for n in tables:                  # the look-up tables live in the batch; the diagnostics do not touch them
        setattr(q, n, np.zeros(1))
    q.copy_host_to_device()
    for n, v in tables.items():
        setattr(q, n, v)
    q.allocate_on_device()
    computer.sync_store_from_rt(q)
    if getattr(q, "conv_layer", None) is not None:
        q.dev_conv_layer.set(np.asarray(q.conv_layer, np.int32))
    q.dev_F_smooth_sum.set(q.rt.get("F_smooth_sum", q.rt_col))
    computer.integrate_optdepth_transmission(q)
    if q.transit_depth_spectrum == 1:
        computer.calculate_transit_depth(q)
    if q.emission_angles > 0:
        computer.calculate_emission_angles(q)
    computer.calculate_contribution_function(q)
    if q.convection == 1:
        computer.interpolate_entropy(q)
        computer.interpolate_phase_state(q)
    computer.calculate_mean_opacities(q)
    computer.integrate_beamflux(q)
    q.copy_device_to_host()
    if q.conv_unstable is None:
        q.conv_unstable = np.zeros(int(q.nlayer) + 1, np.int32)
    hsfunc.calculate_conv_flux(q)
    hsfunc.calc_F_ratio(q)
    if getattr(q, "aborted", False):
        writer.write_abort_file(q, reader)
    writer.write_all(q, reader)
    for name in [n for n in vars(q) if n.startswith("dev_")]:       # give the device memory back before the next column
        arr = getattr(q, name)
        if hasattr(arr, "free"):
            arr.free()
        setattr(q, name, None)


_SWEEP_SEQUENCE = 0      # number of run_sweep calls with a shared work list in this process


def _run_columns(base_argv, overrides_list, cols, computer, writer, shared, columns, timing, write_output):
    """prepare the columns `cols`, run them as device batches (one per batch signature) to the end of both loops, write
    their files and append them to `columns`"""
    import time
    fresh = []
    for k in cols:
        ov = dict(overrides_list[k])
        ov.setdefault("name", "%s_%d" % (_base_name(base_argv), k))
        q, reader = _prepare_column(base_argv, ov, shared)
        q._ctx = computer.ctx
        q.sweep_index = k
        fresh.append((q, reader))
    groups = {}
    for q, reader in fresh:
        why = computer._why_not_fused(q)
        if why is not None:
            raise IOError("sweeps run on the fused device path: flux calculation method 'iteration' or 'matrix' and at most 1024 "
                          "layers (2048 isothermal ones); this one has " + why + " -- run this configuration column by column "
                          "with helios.py")
        groups.setdefault(_batch_signature(q), []).append((q, reader))
    for members in groups.values():
        quants = [q for q, _ in members]
        t0 = time.perf_counter()
        rt = computer.make_rt_batch(quants)
        computer.ctx.synchronize()
        t1 = time.perf_counter()
        loops.radiation(computer, quants, rt)      # (no writer: a sweep hands no profile over during the run, and an
        loops.convection(computer, quants, rt)     # aborted column gets its marker file in _finish_column)
        computer.ctx.synchronize()
        t2 = time.perf_counter()
        timing["batch"] += t1 - t0
        timing["loops"] += t2 - t1
        for q, reader in members:
            if write_output:
                _finish_column(computer, q, reader, writer)
            else:
                q.T_lay = rt.get("T_lay", q.rt_col)
                q.F_up_band = rt.get("F_up_band", q.rt_col)
        timing["finish"] += time.perf_counter() - t2
        for q in quants:
            q.rt = None
        rt.close()
    columns += fresh


def run_sweep(base_argv, overrides_list, dist=None, coll_device="cpu", write_output=True):
    """run every column of `overrides_list` (this rank's share if `dist` is initialised); returns
    (columns of this rank as Stores, emission spectra of ALL columns [ncol_total, nbin] in sweep order)"""
    import os
    from .parallel import column_list, gather_spectra
    rank = dist.get_rank() if dist is not None and dist.is_initialized() else 0
    world = dist.get_world_size() if dist is not None and dist.is_initialized() else 1
    if world > len(overrides_list):
        raise ValueError("%d ranks for %d columns: a sweep needs at least one column per rank" % (world, len(overrides_list)))
    # neighbours in a sweep (similar planets) converge after similar numbers of iterations: dealing the columns out in
    # turn spreads the long-running ones over the ranks; HELIOS_SWEEP_PARTITION=block keeps contiguous blocks
    # HELIOS_SWEEP_PARTITION=dynamic[:chunk]: a shared work list instead -- every rank claims `chunk` columns (default:
    # an eighth of its even share), runs them as one batch, retires them and claims again until the list is empty
    mode = os.environ.get("HELIOS_SWEEP_PARTITION", "cyclic")
    decks_on = cloud_deck_mode(overrides_list)      # (refuses an unknown HELIOS_CLOUD_DECKS before anything is set up)
    computer = comp.Compute()
    writer = write_mod.Write()
    shared = {"cloud_decks": decks_on}
    columns = []
    import time
    timing = dict(batch=0.0, loops=0.0, finish=0.0)
    if mode.startswith("dynamic"):
        from .parallel import WorkList
        chunk = int(mode.split(":")[1]) if ":" in mode else max(1, len(overrides_list) // (8 * world))
        # one counter per sweep: every rank calls run_sweep the same number of times, and a restarted worker group
        # (torchrun --max-restarts) may find the previous attempt's keys still in the agent's store
        global _SWEEP_SEQUENCE
        _SWEEP_SEQUENCE += 1
        key = "%s/restart%s/sweep%d" % (WorkList.KEY, os.environ.get("TORCHELASTIC_RESTART_COUNT", "0"), _SWEEP_SEQUENCE)
        work = WorkList(len(overrides_list), chunk, dist, key=key)
        claims = iter(work.claim, [])
        mine_cols = work.claimed
    else:
        claims = iter([column_list(len(overrides_list), rank, world, mode)])
        mine_cols = None
    for claimed in claims:
        _run_columns(base_argv, overrides_list, claimed, computer, writer, shared, columns, timing, write_output)
    if mine_cols is None:
        mine_cols = [q.sweep_index for q, _ in columns]
    if rank == 0:
        print("\nSweep timing [s]: batch set-up %.2f, iteration loops %.2f, diagnostics + output files %.2f"
              % (timing["batch"], timing["loops"], timing["finish"]))
    if world > 1:
        # columns converge after different numbers of iterations: how unevenly the ranks were loaded
        mine = dict(rank=rank, columns=len(mine_cols), loops=timing["loops"],
                    iterations=int(sum(int(q.iter_value or 0) for q, _ in columns)))
        every = [None] * world
        dist.all_gather_object(every, mine)
        if rank == 0:
            loops = np.array([e["loops"] for e in every])
            print("Load over %d ranks: loop time min %.2f / mean %.2f / max %.2f s (imbalance max/mean = %.2f); "
                  "iterations per rank %s" % (world, loops.min(), loops.mean(), loops.max(),
                                              loops.max() / max(loops.mean(), 1e-30),
                                              [e["iterations"] for e in every]))
    X = int(columns[0][0].nbin) if columns else 0
    local = np.array([np.asarray(q.F_up_band)[-X:] for q, _ in columns]).reshape(len(columns), X)
    spectra = gather_spectra(local, dist, coll_device, columns=mine_cols)
    if spectra.shape[0] != len(overrides_list):
        raise RuntimeError("sweep: %d columns were run, %d were asked for (partition '%s')"
                           % (spectra.shape[0], len(overrides_list), mode))
    return [q for q, _ in columns], spectra


def wavelength_grid(base_argv, overrides):
    """the wavelength grid of a sweep, for a rank that ran none of its columns"""
    q, _ = _prepare_column(base_argv, dict(overrides), {})
    return q.opac_wave


def _base_name(argv):
    argv = list(argv)
    return argv[argv.index("-name") + 1] if "-name" in argv else "sweep"
