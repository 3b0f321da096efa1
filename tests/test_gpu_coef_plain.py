"""k_rt_coef_plain -- k_rt_coef's source compiled with a plain column's flags as constants (no clouds, no beam, no I2S
correction, g_0 = 0, the sweeps over half-layers) -- against k_rt_coef itself, which HELIOS_RT_COEF_GENERAL=1 keeps for such
a column: the coefficient planes byte for byte, padding slots included, and the band fluxes and temperatures of the
iteration that follows.  The profiling scope rt_coef_plain tells which of the two kernels a refresh launched.

Without a GPU: the code-object notes of the specialised kernels (no scratch, no spill, fewer VGPRs than the general
kernel at BASELINE config 2's tiling)."""
import contextlib
import os

import numpy as np
import pytest

import cases
import coef_cases as cc
from helios_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("HELIOS_RT_K", "HELIOS_RT_GENERIC_SCANS", "HELIOS_RT_MAXTHREADS", "HELIOS_RT_COEF_TPB", "HELIOS_RT_CLOUD_LDS",
         "HELIOS_RT_COEF_GENERAL", "HELIOS_RT_FUSED_LOOKUP")
# name -> (the column, (k, ROWS) of its tiling)
COLUMNS = {
    "edges_L9": (lambda: cc.make("plain", "L9"), None),
    "edges_L100": (lambda: cc.make("plain", "L100"), (16, 13)),
    "L2": (lambda: cases.make_case(nbin=5, nlayer=2), (8, 1)),             # 4 half-layers on 8 lanes
    "L7": (lambda: cases.make_case(nbin=5, nlayer=7), (16, 1)),
    "L100_x3": (lambda: cases.make_case(nbin=3, nlayer=100), (16, 13)),    # config 2's tiling, the last tile partly empty
}


def _library_has(word):
    with open(_lib.LIB_PATH, "rb") as f:
        return word in f.read()


@pytest.fixture(scope="module")
def specialised():
    """a library from before k_rt_coef_plain has neither the kernel nor the knob: nothing to compare there"""
    if not (_library_has(b"k_rt_coef_plain") and _library_has(b"HELIOS_RT_COEF_GENERAL")):
        pytest.skip("this library has no k_rt_coef_plain")


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    c = Context(0)
    yield c


@contextlib.contextmanager
def _knobs(env):
    """exactly these tuning knobs while a batch is created (hx_rt_create reads them), the others unset"""
    saved = {k: os.environ.get(k) for k in KNOBS}
    try:
        for k in KNOBS:
            os.environ.pop(k, None)
        for k, v in env.items():
            os.environ[k] = str(v)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _run(ctx, c, env, onthefly):
    """one refresh, then one iteration: (tiling, planes of the refresh, launches of the specialised kernel in that refresh,
    band fluxes and temperatures after step(0))"""
    from helios_amd.rt import batch_from_case
    c = c.copy()
    if onthefly:
        cases.add_species(c, nspecies=1, with_h2o=False)      # one absorber and the H2 scatterer
    species = c.get("species")
    with _knobs(env):
        rt = batch_from_case(ctx, c, nspecies=len(species) if species else 0)
    try:
        if species:
            for k, sp in enumerate(species):
                rt.set_species(k, sp["pretab"], sp["scat"], sp["weight"], is_h2o=0, is_cia=0, in_mu=1)
            rt.set_column_vmr(-1, *cases.species_vmr_arrays(c))
        rt.build_planck_table(1 if c.T_star > 10 else 0)
        rt.profile(True)
        rt.refresh()
        launches = rt.profile_read("rt_coef_plain")[1]
        assert rt.profile_read("rt_coef")[1] == 1
        planes = rt.coef_planes(0)
        rt.step(0)
        return dict(tiling=rt.flux_tiling(), planes=planes, launches=launches,
                    out={k: rt.get(k) for k in ("F_up_band", "F_down_band", "T_lay")})
    finally:
        rt.close()


@pytest.mark.gpu
@pytest.mark.parametrize("onthefly", [0, 1], ids=["premixed", "onthefly"])
@pytest.mark.parametrize("name", list(COLUMNS))
def test_plain_columns_get_the_general_kernels_bits(ctx, specialised, name, onthefly):
    """premixed: the k-table look-up inside the kernel (FROM_TABLE); one on-the-fly absorber: the mixed opacities.  Default
    tiles per workgroup and 1, 2 and 8"""
    make, tiling = COLUMNS[name]
    c = make()
    for tpb in (None, 1, 2, 8):
        env = {} if tpb is None else dict(HELIOS_RT_COEF_TPB=tpb)
        new = _run(ctx, c, env, onthefly)
        old = _run(ctx, c, dict(env, HELIOS_RT_COEF_GENERAL=1), onthefly)
        t = new["tiling"]
        assert t == old["tiling"] and t["coef_bytes"] == 8 and (tpb is None or t["coef_tpb"] == tpb), (t, old["tiling"])
        if tiling is not None:
            assert (t["k"], t["ROWS"]) == tiling, t
        assert (new["launches"], old["launches"]) == (1, 0), (tpb, new["launches"], old["launches"])
        assert np.all(np.isfinite(new["planes"]))
        assert new["planes"].tobytes() == old["planes"].tobytes(), "tpb %s: %d of %d plane slots differ" % (
            tpb, int(np.sum(new["planes"].view(np.uint64) != old["planes"].view(np.uint64))), new["planes"].size)
        for k, v in new["out"].items():
            assert np.all(np.isfinite(v)), k
            assert v.tobytes() == old["out"][k].tobytes(), (tpb, k)


@pytest.mark.gpu
@pytest.mark.parametrize("flagset,shape", [("clouds", "L9"), ("beam_glimit", "L9"), ("matrix", "L9"), ("plain", "iso20")])
def test_other_columns_keep_the_general_kernel(ctx, specialised, flagset, shape):
    """clouds with the I2S correction, the beam, the matrix method and isothermal layers are not what the specialised
    kernel was compiled for: k_rt_coef runs, with the knob or without"""
    c = cc.make(flagset, shape)
    new, old = _run(ctx, c, {}, 0), _run(ctx, c, dict(HELIOS_RT_COEF_GENERAL=1), 0)
    assert (new["launches"], old["launches"]) == (0, 0)
    assert new["planes"].tobytes() == old["planes"].tobytes()


# ---- the code objects (no GPU needed) -----------------------------------------------------------------------------------

def _kernel_notes():
    import importlib.util
    spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(ROOT, "tools", "code_object_notes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return {k["name"]: k for k in mod.kernel_notes()}


def test_the_specialised_kernels_use_no_scratch_and_fewer_registers(specialised):
    notes = _kernel_notes()
    plain = {n: k for n, k in notes.items() if "k_rt_coef_plain<" in n}
    general = {n: k for n, k in notes.items() if "k_rt_coef<" in n}
    # both look-up modes of every (rows, tiles per workgroup) pair the general fp64 kernel has
    assert general and len(plain) == 2 * len(general), (len(plain), len(general))
    for n in general:
        rows_tpb = n.split("k_rt_coef<")[1].split(">")[0]
        for mode in ("true", "false"):
            assert sum("k_rt_coef_plain<%s, %s>" % (rows_tpb, mode) in p for p in plain) == 1, (rows_tpb, mode)
    bad = sorted(n for n, k in plain.items() if k["private_segment_fixed_size"] != 0 or k["vgpr_spill_count"] != 0)
    assert not bad, bad
    config2 = [k for n, k in plain.items() if "k_rt_coef_plain<13, 4, true>" in n]
    was = [k for n, k in general.items() if "k_rt_coef<13, 4>" in n]
    assert len(config2) == 1 and len(was) == 1
    print("k_rt_coef_plain<13, 4, true>: %d VGPRs, k_rt_coef<13, 4>: %d" % (config2[0]["vgpr_count"], was[0]["vgpr_count"]))
    assert config2[0]["vgpr_count"] < was[0]["vgpr_count"]
