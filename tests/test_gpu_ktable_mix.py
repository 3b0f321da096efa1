"""The kernels of the mixing stage (csrc/ktable_mix.hip) at the smallest shapes that reach every path: k_ktmix_sum bit for bit
against the numpy backend (the same two roundings per term, in the same order), the re-gridding into a slot and the water part of
k_ktmix_scat under the rule of tests/test_gpu_ktable_edges.py -- within max(1e-13, 8 eps64) of the long-double restatement,
eps64 the numpy backend's own deviation there -- the error paths by message, the two backends on the whole tool call of golden
case a, and the chain this stage closes: a premixed helios.py run from a file this tool wrote on the hard-coded grid, where
premix.py still refuses the same containers.  Nothing here reads the reference tree."""
import os

import numpy as np
import pytest

import ktable_mix_reference as kr
import ktable_reference as ktr
from ktable_reference import LD, reference_regrid
from test_ktable_mix import case_inputs, final, grid, held, lines, load, restated, tool          # noqa: F401 -- fixtures
from helios_amd import ktable, ktable_mix
from helios_amd._lib import HeliosHipError
from helios_amd._tool import dp, ip

pytestmark = pytest.mark.gpu

G = 16                      # species per launch of k_ktmix_sum (KM_G)
SPAN = 512                  # entries of one workgroup: 256 threads x 2 doubles
GUARD = np.array([0x7ff8dead0badbeef], np.uint64)


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def guards_untouched(m):
    for name in ("kpoints_guard", "scat_cross_guard"):
        assert np.all(m.get(name).view(np.uint64) == GUARD[0]), name


def sum_case(nc, nt, npress, absorbers, seed):
    """slots: the absorbers with a scattering-only species in the middle of the list; the second absorber (where there is
    one) has mixing ratio 0 everywhere"""
    rng = np.random.default_rng(seed)
    nodes = nt * npress
    ns = absorbers + 1
    middle = ns // 2
    tables, mmr = [], rng.uniform(1e-9, 2.0, (ns, nodes))
    for s in range(ns):
        if s == middle:
            tables.append(None)
            continue
        k = 10.0 ** rng.uniform(-15, 3, nodes * nc)
        k[rng.random(k.size) < 0.1] = 0.0
        tables.append(k)
    zeroed = [s for s in range(ns) if s != middle]
    if len(zeroed) > 1:
        mmr[zeroed[1]] = 0.0
    return tables, mmr


def device_sum(ctx, nc, nt, npress, tables, mmr, again=None):
    nbin, ny = (nc, 1) if nc % 3 else (nc // 3, 3)
    m = ktable_mix.Mixer(ctx, nbin, ny, nt, npress, len(tables))
    try:
        m.set_grid(np.linspace(1e-4, 2e-4, nbin), np.linspace(300.0, 900.0, nt), 10.0 ** np.linspace(3, 6, npress))
        for s, k in enumerate(tables):
            m.set_species(s, k)
        out = []
        for r in [mmr] + ([again] if again is not None else []):
            m.run(r, np.zeros_like(r))
            out.append(m.get("kpoints"))
            assert np.all(m.get("scat_cross") == 0)
            guards_untouched(m)
        return out
    finally:
        m.close()


@pytest.mark.parametrize("nc", [1, 3, 20, 60, SPAN - 1, SPAN + 1, 2 * SPAN + 1])
def test_sum_bit_for_bit(ctx, nc):
    """odd nc meets even and odd nodes (2 x 3); 1, 2, G and G + 1 absorbers; either side of one span, and two spans with a
    short last one"""
    for nt, npress in ((1, 1), (2, 3)):
        for absorbers in (1, 2, G, G + 1):
            tables, mmr = sum_case(nc, nt, npress, absorbers, seed=nc + absorbers)
            want = ktable_mix.numpy_sum(tables, mmr, nt * npress, nc)
            got = device_sum(ctx, nc, nt, npress, tables, mmr)[0]
            assert got.tobytes() == want.tobytes(), (nc, nt, npress, absorbers)
            assert nc < 20 or any(k is not None and np.any(k == 0) for k in tables)       # exact zeros among the inputs


def test_second_run_equals_a_fresh_object(ctx):
    nc, nt, npress = SPAN + 1, 2, 3
    tables, mmr = sum_case(nc, nt, npress, G + 1, seed=4)
    other = np.random.default_rng(5).uniform(0.0, 1.0, mmr.shape)
    first, second = device_sum(ctx, nc, nt, npress, tables, mmr, again=other)
    fresh = device_sum(ctx, nc, nt, npress, tables, other)[0]
    assert second.tobytes() == fresh.tobytes() and second.tobytes() != first.tobytes()
    assert second.tobytes() == ktable_mix.numpy_sum(tables, other, nt * npress, nc).tobytes()


def test_no_absorber_gives_zeros(ctx):
    m = ktable_mix.Mixer(ctx, 5, 1, 1, 2, 2)
    try:
        m.set_grid([1e-4] * 5, [300.0], [1e3, 1e4])
        m.run(np.ones((2, 2)), np.ones((2, 2)))
        assert np.all(m.get("kpoints") == 0) and np.all(m.get("scat_cross") == 0)
        guards_untouched(m)
    finally:
        m.close()


# ---- the re-gridding into a slot (k_ktable_regrid) -------------------------------------------------------------------------------
REGRID_T = [100.0, 200.0, 201.0, 450.0, 700.0, 900.0, 2500.0]              # below, on, between and above the nodes
REGRID_P = [1e-2, 1e1, 50.0, 1e3, 1e5, 3e6, 1e8, 1e10]


@pytest.mark.parametrize("source", [([200.0, 900.0], [1e1, 1e8]), ([200.0, 450.0, 900.0], [1e5])])
@pytest.mark.parametrize("nc", [3, 60])
def test_regrid_against_the_restatement(ctx, source, nc):
    T, P = source
    k = 10.0 ** np.random.default_rng(nc).uniform(-15, 3, len(T) * len(P) * nc)
    exact = reference_regrid(T, P, k, REGRID_T, REGRID_P, nc).reshape(-1)
    host = ktable.numpy_regrid(P, T, k, REGRID_T, REGRID_P, nc // 3, 3)
    m = ktable_mix.Mixer(ctx, nc // 3, 3, len(REGRID_T), len(REGRID_P), 2)
    try:
        m.set_grid(np.linspace(1e-4, 2e-4, nc // 3), REGRID_T, REGRID_P)
        m.set_species_native(1, k, T, P)
        got = m.get("species_1")
        with pytest.raises(HeliosHipError, match="species slot 0 holds no table"):
            m.get("species_0")
        assert m.get("timing_ms")[2] > 0
    finally:
        m.close()
    ex64 = exact.astype(np.float64)
    eps64 = np.abs((host.astype(LD) - exact) / exact).astype(np.float64)
    dev = np.abs((got.astype(LD) - exact) / exact).astype(np.float64)
    print("regrid %s, nc %d: device %.3e, numpy %.3e" % (source, nc, dev.max(), eps64.max()))
    assert np.all(dev <= np.maximum(1e-13, 8 * eps64)) and np.all(np.isfinite(ex64))


@pytest.mark.parametrize("nbin,ny", [(1, 3), (7, 5), (3, 20)])
@pytest.mark.parametrize("temps,press", ktr.REGRID_SOURCES, ids=["1x1", "1x3", "3x1", "3x4"])
def test_the_mixer_regrids_bit_for_bit_as_the_builder(ctx, temps, press, nbin, ny):
    """one re-gridding behind both objects: what Mixer.set_species_native leaves in its slot is KTableBuilder.regrid's kpoints_ip
    of the same source, and both are numpy_regrid's, to the bit.  Sources with a single temperature or pressure; the 3 x 4 one
    clamps 4 of the 7 temperatures and 4 of the 9 pressures, so every branch of the kernel runs; rows of 3, 35 and 60 entries"""
    nc = nbin * ny
    k = ktr.regrid_source(temps, press, nc)
    host = ktable.numpy_regrid(press, temps, k, ktr.REGRID_T, ktr.REGRID_P, nbin, ny)
    assert np.all(np.isfinite(host))
    if len(temps) * len(press) == 12:
        assert ktable.regrid_plan(temps, ktr.REGRID_T)[1].sum() == 4 and ktable.regrid_plan(press, ktr.REGRID_P)[1].sum() == 4
    b = ktable.KTableBuilder(ctx, 8, nbin, ny, len(temps) * len(press))
    try:
        ctx.check(b._l.hx_ktable_put(b.handle, dp(np.ascontiguousarray(k, np.float64))), "hx_ktable_put")
        b.regrid(temps, press, ktr.REGRID_T, ktr.REGRID_P)
        built = b.get("kpoints_ip")
    finally:
        b.close()
    m = ktable_mix.Mixer(ctx, nbin, ny, len(ktr.REGRID_T), len(ktr.REGRID_P), 2)
    try:
        m.set_grid(np.linspace(1e-4, 2e-4, nbin), ktr.REGRID_T, ktr.REGRID_P)
        m.set_species_native(1, k, temps, press)
        mixed = m.get("species_1")
    finally:
        m.close()
    np.testing.assert_array_equal(mixed, built)
    np.testing.assert_array_equal(built, host)


# ---- k_ktmix_scat ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbin", [1, 63, 65, 257])
def test_scat_constant_part_bit_for_bit_and_water_to_the_rule(ctx, nbin):
    rng = np.random.default_rng(nbin)
    temp, press = [300.0, 2000.0], [1e2, 1e5, 1e8]
    nodes = 6
    at = 2.5e-4                                                            # the limit itself, and its two neighbours
    wave = np.sort(np.concatenate(([np.nextafter(at, 0), at, np.nextafter(at, 1)][:nbin],
                                   10.0 ** rng.uniform(np.log10(0.35e-4), np.log10(20e-4), max(0, nbin - 3)))))
    sig = [rng.uniform(1e-30, 1e-24, nbin), None, rng.uniform(1e-30, 1e-24, nbin), None]
    x = rng.uniform(1e-6, 1.0, (4, nodes))
    x[3] = [1e-12, 1.0, 1e-3, 1.0, 0.0, 1e-12]                             # the water: slot 3; slot 1 does not scatter
    m = ktable_mix.Mixer(ctx, nbin, 2, 2, 3, 4)
    try:
        m.set_grid(wave, temp, press)
        m.set_rayleigh(0, sig[0])
        m.set_rayleigh(2, sig[2])
        m.run(np.zeros_like(x), x)
        const = m.get("scat_cross")
        assert const.tobytes() == ktable_mix.numpy_scat(sig, x, wave, temp, press).tobytes()
        m.set_rayleigh(0, None)
        m.set_rayleigh(2, None)
        m.set_rayleigh(3, None, is_h2o=True)
        m.run(np.zeros_like(x), x)
        water = m.get("scat_cross")
        guards_untouched(m)
        assert np.all(m.get("kpoints") == 0)
    finally:
        m.close()
    only = [None, None, None, "H2O"]
    host = ktable_mix.numpy_scat(only, x, wave, temp, press)
    exact = (x[3].astype(LD)[:, None] * kr.reference_h2o(wave, temp, press, x[3].astype(LD))).reshape(-1)
    zero = exact == 0
    assert np.all(water[zero] == 0) and np.all(host[zero] == 0)
    assert zero.reshape(nodes, nbin)[4].all() and np.array_equal(zero.reshape(nodes, nbin)[0], wave > at)
    eps64 = np.abs((host[~zero].astype(LD) - exact[~zero]) / exact[~zero]).astype(np.float64)
    dev = np.abs((water[~zero].astype(LD) - exact[~zero]) / exact[~zero]).astype(np.float64)
    print("water, %d bins: device %.3e, numpy %.3e" % (nbin, dev.max(), eps64.max()))
    assert np.all(dev <= np.maximum(1e-13, 8 * eps64))


# ---- the error paths ---------------------------------------------------------------------------------------------------------------
def test_error_paths_by_message(ctx):
    asked = ((1 << 12) * ((1 << 11) - 1) + 1) * (1 << 26) * 8               # kpoints and its guard row: 4.5e15 bytes
    with pytest.raises(HeliosHipError, match=r"kpoints needs %d bytes, the device has \d+ free" % asked):
        ktable_mix.Mixer(ctx, 1 << 20, 64, 1 << 12, (1 << 11) - 1, 1)
    with pytest.raises(HeliosHipError, match="bins, Gauss points, temperatures, pressures and species are >= 1"):
        ktable_mix.Mixer(ctx, 4, 0, 2, 2, 1)
    m = ktable_mix.Mixer(ctx, 4, 3, 2, 2, 2)
    try:
        with pytest.raises(HeliosHipError, match="hx_ktmix_run: set the grid first"):
            m.run(np.ones((2, 4)), np.ones((2, 4)))
        m.set_grid([1e-4, 2e-4, 3e-4, 4e-4], [100.0, 200.0], [1e3, 1e4])
        with pytest.raises(HeliosHipError, match="hx_ktmix_set_species: species slot 2 out of range, the object has 2"):
            m.set_species(2, np.ones(48))
        with pytest.raises(HeliosHipError, match="hx_ktmix_set_rayleigh: species slot -1 out of range"):
            m.set_rayleigh(-1, np.ones(4))
        with pytest.raises(HeliosHipError, match="water vapour's cross-section is computed per node"):
            m.set_rayleigh(0, np.ones(4), is_h2o=True)
        with pytest.raises(HeliosHipError, match="hx_ktmix_get: run first"):
            m.get("kpoints")
        m.run(np.ones((2, 4)), np.ones((2, 4)))
        out = np.zeros(47)
        rc = m._l.hx_ktmix_get(m.handle, b"kpoints", out.ctypes.data, out.nbytes)
        assert rc != 0
        with pytest.raises(HeliosHipError, match=r"hx_ktmix_get\(kpoints\): 384 bytes expected, got 376"):
            ctx.check(rc, "hx_ktmix_get")
        with pytest.raises(HeliosHipError, match="unknown name 'species_x'"):
            m.get("species_x")
        with pytest.raises(HeliosHipError, match="unknown name 'nothing'"):
            m.get("nothing")
        with pytest.raises(HeliosHipError, match="hx_ktmix_get: species slot 7 out of range"):
            m.get("species_7")
        with pytest.raises(HeliosHipError, match="temperature plan out of range"):
            bad = np.array([5, 5], np.int32)
            ok = np.zeros(2, np.int32)
            a = np.array([100.0, 200.0])
            m.ctx.check(m._l.hx_ktmix_set_species_native(m.handle, 0, dp(np.ones(48)), 2, 2, ip(bad),
                                                         ip(ok), ip(ok), ip(ok),
                                                         *[dp(a)] * 4), "hx_ktmix_set_species_native")
    finally:
        m.close()


# ---- the tool ---------------------------------------------------------------------------------------------------------------------
def test_the_two_backends_on_golden_case_a(ctx, tmp_path, grid, lines, final, restated):     # noqa: F811
    g = load("a")
    host_root, dev_root = os.path.join(str(tmp_path), "host"), os.path.join(str(tmp_path), "dev")
    for root in (host_root, dev_root):
        case_inputs(root, "a", grid, lines, final)
    host = np.load(tool(host_root)[-1])
    dev = np.load(tool(dev_root, "-backend", "hip")[-1])
    for k in ("pressures", "temperatures", "meanmolmass", "wavelengths", "ypoints", "center wavelengths",
              "interface wavelengths", "wavelength width of bins"):
        assert dev[k].tobytes() == host[k].tobytes(), k
    for k, want in restated["a"].items():
        held(dev[k], want, float(g["eps_ref " + k]), "device, case a, %s" % k)
    # the containers written on the way: the re-gridded ones as k_ktable_regrid's rule asks, the existing one untouched
    for n in ("H2O", "CO2"):
        d = np.load(os.path.join(dev_root, "opac", n + "_opac_ip_kdistr.npz"))["kpoints"]
        h = np.load(os.path.join(host_root, "opac", n + "_opac_ip_kdistr.npz"))["kpoints"]
        exact = reference_regrid(lines["native %s temperatures" % n], lines["native %s pressures" % n],
                                 lines["native %s kpoints" % n], final[0], final[1], 12).reshape(-1)
        nz = exact != 0
        assert np.all(d[~nz] == 0)
        eps64 = np.abs((h[nz].astype(LD) - exact[nz]) / exact[nz]).astype(np.float64)
        devn = np.abs((d[nz].astype(LD) - exact[nz]) / exact[nz]).astype(np.float64)
        assert np.all(devn <= np.maximum(1e-13, 8 * eps64)), n


def test_the_chain_to_a_premixed_run(tmp_path):
    """synthetic containers of 8 bins x 20 Gauss points on 6 x 5 native nodes -> ktable.py -mixed_table_production yes on the
    hard-coded 120 x 28 grid (device) -> helios.py -opacity_mixing premixed, 12 layers: it ends within 2000 iterations with
    finite fluxes and its global energy imbalance inside its criterion.  premix.py on the same containers is refused: the
    hard-coded pressures are not uniform in log10 P."""
    import helios
    import ktable as ktable_tool
    import premix as premix_tool
    from helios_amd import host_functions as hsfunc, synthetic as syn
    from test_gpu_ktable import _otf_argv
    wd = str(tmp_path)
    opac = os.path.join(wd, "opac")
    os.makedirs(opac)
    inter, wave, width = syn.wavelength_grid(8)
    y, _w = syn.gauss_points(20)
    T, P = syn.tp_grid(6, 5)
    g = {"interface wavelengths": inter, "center wavelengths": wave, "wavelength width of bins": width, "ypoints": y,
         "temperatures": T, "pressures": P}
    mu = (1e-3 * 18.0153 + 0.85 * 2.01588 + 0.15 * 4.0026) / (1e-3 + 0.85 + 0.15)
    k = syn.ktable(np.random.default_rng(11), 8, 20, T, P, y) * (mu / (1e-3 * 18.0153))      # so that the mix is syn.ktable
    np.savez(os.path.join(opac, "H2O_opac_kdistr.npz"), kpoints=k, **g)
    species = "species      absorbing       scattering         mixing_ratio\n\nH2O  yes no 1e-3\nH2   no  yes  0.85\nHe  no yes 0.15\n"
    with open(os.path.join(wd, "species.dat"), "w") as f:
        f.write(species)
    written = ktable_tool.main(["-mixed_table_production", "yes", "-path_to_final_species_file", os.path.join(wd, "species.dat"),
                                "-directory_with_individual_files", opac, "-mixed_table_output_directory", wd,
                                "-container", "npz"])
    assert [os.path.basename(p) for p in written] == ["H2O_opac_ip_kdistr.npz", "scat_cross_sections.npz",
                                                      "mixed_opac_kdistr.npz"]
    t = np.load(written[-1])
    assert t["kpoints"].shape == (120 * 28 * 8 * 20,) and np.all(t["kpoints"] > 0) and np.all(t["meanmolmass"] == mu)
    criterion = 1e-4
    run = helios.run_helios(["-parameter_file", "/nonexistent", "-opacity_mixing", "premixed", "-path_to_opacity_file",
                             written[-1], "-name", "mixed", "-output_directory", wd + "/", "-number_of_layers", "12",
                             "-maximum_number_of_iterations", "2000", "-radiative_equilibrium_criterion", "%g" % criterion,
                             "-convective_adjustment", "no", "-toa_pressure", "1e3", "-boa_pressure", "1e7"])
    imbalance = float(hsfunc.global_energy_imbalance(run))
    print("iterations %d, T %.1f ... %.1f, global energy imbalance %.3e" % (run.iter_value, run.T_lay.min(), run.T_lay.max(),
                                                                          imbalance))
    assert int(run.nbin) == 8 and int(run.ny) == 20 and int(run.nlayer) == 12
    assert 3 < int(run.iter_value) < 2000
    assert np.all(np.isfinite(run.F_net)) and np.all(np.isfinite(run.F_up_band)) and np.all(np.isfinite(run.T_lay))
    assert abs(imbalance) <= criterion
    with pytest.raises(IOError, match="log10 pressure nodes are not uniform"):
        premix_tool.main(_otf_argv(wd) + ["-premix_output", os.path.join(wd, "premix.npz")])
