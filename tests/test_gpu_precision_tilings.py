"""`precision = single` at every tiling: the fp32 coefficient kernels (k_rt_coef_f32<ROWS, TPB>) and flux kernels
(k_rt_flux_f32<ROWS, K>) of rt_fused_f32.hip, each instantiation run and held to the fp64 planes of the same column.

The tilings come from the library (hx_rt_flux_geometry): for every (rows, k) the selection picks over 1-416 layers and
1-832 isothermal ones, the smallest and the largest layer count of its range (the largest fills the last lane, the
smallest leaves it partly empty), and the tilings reached only through the knobs (HELIOS_RT_K, HELIOS_RT_GENERIC_SCANS,
HELIOS_RT_MAXTHREADS, HELIOS_RT_COEF_TPB, HELIOS_RT_CLOUD_LDS).  Every case reads back the tiling that ran
(RTBatch.flux_tiling) and asserts it is the one it names.  The flags rotate over the cases -- beam on and off, clouds with
scat_corr (the v' plane), isothermal layers, zenith correction, ny = 1, thin top layers -- so that every plane layout and
both of the flux kernel's decode branches (v' stored, or K * rest) run at every K."""
import contextlib
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest

import cases
import fused_helpers as fh
from plane_coding import decode_slot, encode_planes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOBS = ("HELIOS_RT_K", "HELIOS_RT_GENERIC_SCANS", "HELIOS_RT_MAXTHREADS", "HELIOS_RT_COEF_TPB", "HELIOS_RT_CLOUD_LDS")
SIX = ["F_up_wg", "F_down_wg", "Fc_up_wg", "Fc_down_wg", "F_up_band", "F_down_band"]
TOTALS = ["F_up_tot", "F_down_tot"]


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


def _geometry(nlayer, iso):
    from helios_amd import _lib
    k, r = ctypes.c_int(), ctypes.c_int()
    with _knobs({}):
        assert _lib.lib().hx_rt_flux_geometry(nlayer, iso, 1, 20, 3, 1, ctypes.byref(k), ctypes.byref(r)) == 0
    return r.value, k.value


def _has_fp32_tiling(rows, k, generic_scans=False):
    """rt_fused_f32.hip's coef_fp32_tiling"""
    return rows <= 13 or (rows == 14 and k == 16 and not generic_scans)


def _notes():
    spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(ROOT, "tools", "code_object_notes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return [k["name"] for k in mod.kernel_notes()]


def _instantiations(pattern):
    return {tuple(int(v) for v in m.groups()) for m in (re.search(pattern, n) for n in _notes()) if m}


# ---- the cases ---------------------------------------------------------------------------------------------------------

def _flags(i):
    """the flags of the i-th case: the four plane layouts (v' plane, beam) in turn, the rest on other periods"""
    has_vp, beam = [(0, 0), (1, 0), (0, 1), (1, 1)][i % 4]
    kw = dict(nbin=2 + i % 2, dir_beam=beam)
    if beam:
        kw["albedo"] = 0.2
        if (i // 4) % 2:
            kw.update(geom_zenith_corr=1, zenith_deg=80.0)
    if has_vp:
        kw.update(clouds=1, scat_corr=1, g_0=0.2)
    if i % 7 == 3:
        kw["ny"] = 1
    if i % 5 == 2:
        kw["thin_top"] = True
    return kw


def _make(nlayer, iso, kw, prec):
    kw = dict(kw, nlayer=nlayer, iso=iso)
    if nlayer <= 4:
        kw["p_boa"] = 1e11     # (the height integration needs a layer centre below 10 bar: tests/test_gpu_fused.py "L3")
    c = cases.make_case(**kw)
    c.prec = prec
    return c


def _selected_ranges():
    """{(rows, k, iso): (smallest, largest layer count)} of the selection over 1-416 layers and 1-832 isothermal ones"""
    ranges = {}
    for iso, top in ((0, 416), (1, 832)):
        for L in range(1, top + 1):
            r, k = _geometry(L, iso)
            lo, hi = ranges.get((r, k, iso), (L, L))
            ranges[(r, k, iso)] = (min(lo, L), max(hi, L))
    return ranges


# (name, layers, knobs): tilings only the knobs reach -- forced lane counts at row counts the selection does not pick, the
# generic-scan kernel where a compile-time one exists, and both workgroup shapes at a deep column
KNOB_CASES = [("k8_rows5", 20, {"HELIOS_RT_K": 8}), ("k8_rows13", 52, {"HELIOS_RT_K": 8}),
              ("k32_rows1", 10, {"HELIOS_RT_K": 32}), ("k32_rows7", 100, {"HELIOS_RT_K": 32}),
              ("k64_rows1", 30, {"HELIOS_RT_K": 64}), ("k64_rows6", 180, {"HELIOS_RT_K": 64}),
              ("generic_k16", 100, {"HELIOS_RT_GENERIC_SCANS": 1}), ("generic_k32", 150, {"HELIOS_RT_GENERIC_SCANS": 1}),
              ("generic_k64", 400, {"HELIOS_RT_GENERIC_SCANS": 1}),
              ("threads64_k64", 416, {"HELIOS_RT_MAXTHREADS": 64}), ("threads320_k64", 385, {"HELIOS_RT_MAXTHREADS": 320}),
              ("threads64_rows14", 105, {"HELIOS_RT_MAXTHREADS": 64})]


def _expected(nlayer, iso, env):
    """(rows, k, generic scans) the batch must run"""
    H = nlayer if iso else 2 * nlayer
    if "HELIOS_RT_K" in env:
        k = int(env["HELIOS_RT_K"])
        return -(-H // k), k, 0
    r, k = _geometry(nlayer, iso)
    return r, k, int(env.get("HELIOS_RT_GENERIC_SCANS", 0))


def _first_solve_cases():
    """[(name, layers, iso, knobs, flags)]: both ends of every selected range, then the knob cases; 1 layer is left out (the
    synthetic case needs two for its heights)"""
    out = []
    for (r, k, iso), (lo, hi) in sorted(_selected_ranges().items(), key=lambda kv: (kv[0][2], kv[0][1], kv[0][0])):
        for L in sorted({max(2, lo), hi}):
            threads = {"HELIOS_RT_MAXTHREADS": 64} if (len(out) // 2) % 2 else {}
            out.append(("%s%d_rows%d_k%d_L%d" % ("iso_" if iso else "", len(out), r, k, L), L, iso, threads))
    for name, L, env in KNOB_CASES:
        out.append((name, L, 0, env))
    return [(n, L, iso, env, _flags(i)) for i, (n, L, iso, env) in enumerate(out)]


# ---- running a batch ---------------------------------------------------------------------------------------------------

def _run(ctx, c, env, n_iter=1, ncol=1, T_per_col=None, keys=SIX + TOTALS):
    """{tiling, planck_grid, cols: [{flux key: array, "planes": coefficient planes}]} after n_iter iterations (0: one
    refresh and no iteration)"""
    from helios_amd.rt import batch_from_case
    with _knobs(env):
        rt = batch_from_case(ctx, c, ncol=ncol)
    try:
        out = dict(tiling=rt.flux_tiling())
        rt.keep_down_fluxes(True)
        for i, T in enumerate(T_per_col or []):
            rt.set_temperatures(i, T)
        rt.build_planck_table(1 if c.T_star > 10 else 0)
        if n_iter:
            rt.run(0, n_iter)
            out["planck_grid"] = rt.get("planck_grid")
        else:
            rt.refresh()
        out["cols"] = [dict({k: rt.get(k, col) for k in (keys if n_iter else ())}, planes=rt.coef_planes(col))
                       for col in range(ncol)]
        return out
    finally:
        rt.close()


def _check_tiling(t, want, bytes_, what):
    rows, k, generic = want
    assert (t["ROWS"], t["k"], t["generic_scans"], t["coef_bytes"]) == (rows, k, generic, bytes_), (what, t)


def _padding(t, nbin, H):
    """mask (tiles, ROWS, 64) of the slots that hold no half-layer of a spectral point: alpha = 1, beta = 0, zeros"""
    ntiles = -(-nbin // t["nxb"]) * t["nparts"] * t["NW"]
    tile = np.arange(ntiles)[:, None, None]
    row = np.arange(t["ROWS"])[None, :, None]
    lane = np.arange(64)[None, None, :]
    wv, bx = tile % t["NW"], tile // (t["NW"] * t["nparts"])
    s_local = (wv * 64 + lane) // t["k"]
    x = bx * t["nxb"] + s_local // t["ypb"]
    h = (lane % t["k"]) * t["ROWS"] + row
    return (s_local >= t["nxb"] * t["ypb"]) | (x >= nbin) | (h >= H)


_CACHE = {}


def _first_solves(ctx):
    """per case: the fp64-plane and the fp32-plane run of the same column, one iteration (computed once per module)"""
    if "first" not in _CACHE:
        res = []
        for name, L, iso, env, kw in _first_solve_cases():
            d = _run(ctx, _make(L, iso, kw, "double"), env)
            s = _run(ctx, _make(L, iso, kw, "single"), env)
            res.append((name, L, iso, env, kw, d, s))
        _CACHE["first"] = res
    return _CACHE["first"]


# ---- (a) the coefficient kernel's fp32 store ------------------------------------------------------------------------

def test_fp32_planes_are_the_fp64_planes_coded_once_at_every_tiling(ctx):
    """k_rt_coef_f32 against k_rt_coef on the same column, slot by slot and bit for bit: the fp32 image is
    tests/plane_coding.py's encode_planes of the fp64 image (both translation units compile rt_coef_kernel.inc with
    -ffp-contract=off, so the values before the rounding are the same), and every slot without a half-layer of a spectral
    point reads alpha = 1, beta = 0 as rest = -0.0, beta = +0.0, zeros"""
    flux_ran = set()
    for name, L, iso, env, kw, d, s in _first_solves(ctx):
        want = _expected(L, iso, env)
        _check_tiling(s["tiling"], want, 4, name)
        _check_tiling(d["tiling"], want, 8, name)
        assert {k: v for k, v in d["tiling"].items() if k != "coef_bytes"} == \
            {k: v for k, v in s["tiling"].items() if k != "coef_bytes"}, name
        t = s["tiling"]
        p64, p32 = d["cols"][0]["planes"], s["cols"][0]["planes"]
        assert p32.dtype == np.float32 and p64.dtype == np.float64 and p32.shape == p64.shape, name
        assert t["nplane"] == 3 + int(kw.get("scat_corr", 0)) + 2 * kw["dir_beam"] and t["has_vp"] == kw.get("scat_corr", 0)
        enc = encode_planes(p64, t)
        bad = np.nonzero(enc.view(np.uint32).ravel() != p32.view(np.uint32).ravel())[0]
        if bad.size:
            i = bad[0]
            raise AssertionError("%s: %d of %d slots differ; first at %s: fp64 %r, coded %r (%08x), stored %r (%08x)" % (
                name, bad.size, p32.size, decode_slot(t, i, kw["nbin"]), float(p64.ravel()[i]), float(enc.ravel()[i]),
                enc.view(np.uint32).ravel()[i], float(p32.ravel()[i]), p32.view(np.uint32).ravel()[i]))
        pad = _padding(t, kw["nbin"], L if iso else 2 * L)
        p64_pad, p32_pad = p64.transpose(1, 0, 2, 3)[:, pad], p32.view(np.uint32).transpose(1, 0, 2, 3)[:, pad]
        assert np.all(p64_pad[0] == 1.0) and np.all(p64_pad[1:] == 0.0), name
        assert np.all(p32_pad[0] == 0x80000000) and np.all(p32_pad[1:] == 0), name
        assert np.any(~pad), name
        flux_ran.add((t["ROWS"], t["k"] if t["k"] >= 16 and not t["generic_scans"] else 0))
    print("\n(a) fp32 flux instantiations (ROWS, K) run by the first-solve cases: %d" % len(flux_ran))


# ---- (b) tiles per coefficient workgroup ----------------------------------------------------------------------------

def test_tiles_per_coefficient_workgroup_do_not_change_the_planes(ctx):
    """HELIOS_RT_COEF_TPB = 1, 2, 4, 8 against the batch's own choice, in both plane widths and both workgroup shapes, at
    the largest column of every tiling the selection picks: the same bits in every plane.  A value the batch clamps
    (flux_tiling()["coef_tpb"] says which ran) is recorded and left out, not the tiling.  One clouded case runs with the
    clouds' half-layer terms in LDS and from the bin-major rows (HELIOS_RT_CLOUD_LDS), since their image adds to the LDS
    that bounds the tiles per workgroup.  Every k_rt_coef_f32<ROWS, TPB> of the code object runs."""
    runs = []
    for i, ((r, k, iso), (lo, hi)) in enumerate(sorted(_selected_ranges().items())):
        if not iso:
            runs.append(("rows%d_k%d_L%d" % (r, k, hi), hi, 0, {"HELIOS_RT_MAXTHREADS": 64 if i % 2 else 320}, _flags(i)))
    clouds = dict(nbin=3, clouds=1, scat_corr=1, g_0=0.2, dir_beam=1, albedo=0.2)
    for lds in (1, 0):
        runs.append(("clouds_lds%d" % lds, 200, 0, {"HELIOS_RT_CLOUD_LDS": lds}, clouds))
    ran, clamped = set(), []
    ref_clouds = {}
    for name, L, iso, env, kw in runs:
        for prec in ("double", "single"):
            c = _make(L, iso, kw, prec)
            base = _run(ctx, c, dict(env), n_iter=0)
            t0 = base["tiling"]
            _check_tiling(t0, _expected(L, iso, env), 4 if prec == "single" else 8, name)
            ref = base["cols"][0]["planes"]
            if name.startswith("clouds"):         # (both cloud paths against the default of the first)
                ref = ref_clouds.setdefault(prec, ref)
                np.testing.assert_array_equal(base["cols"][0]["planes"].view(np.uint8), ref.view(np.uint8), err_msg=name)
            ran.add((prec, t0["ROWS"], t0["coef_tpb"]))
            for tpb in (1, 2, 4, 8):
                if tpb == t0["coef_tpb"]:
                    continue
                got = _run(ctx, c, dict(env, HELIOS_RT_COEF_TPB=tpb), n_iter=0)
                t = got["tiling"]
                assert {a: b for a, b in t.items() if a != "coef_tpb"} == {a: b for a, b in t0.items() if a != "coef_tpb"}
                if t["coef_tpb"] != tpb:
                    clamped.append((name, prec, tpb, t["coef_tpb"]))
                    continue
                np.testing.assert_array_equal(got["cols"][0]["planes"].view(np.uint8), ref.view(np.uint8),
                                              err_msg="%s, %s, %d tiles per workgroup" % (name, prec, tpb))
                ran.add((prec, t["ROWS"], tpb))
    coef32 = {(r, t) for p, r, t in ran if p == "single"}
    print("\n(b) k_rt_coef_f32 (ROWS, TPB) run: %d, k_rt_coef (ROWS, TPB) run: %d; clamped: %s"
          % (len(coef32), len({(r, t) for p, r, t in ran if p == "double"}), clamped or "none"))
    assert coef32 == _instantiations(r"k_rt_coef_f32<(\d+), (\d+)>")


# ---- (c) the fp32 first solve against fp64 planes and the oracle ----------------------------------------------------

def _excess(a, b, keys):
    """worst |a - b| over test_gpu_precision_single.py's bound (<= 1 passes), the spectral and band fluxes, and the totals"""
    worst = 0.0
    for k in keys:
        bound = 1e-5 * np.abs(b[k]) + 1e-7 * np.abs(b[k]).max()
        worst = max(worst, float(np.max(np.abs(a[k] - b[k]) / np.maximum(bound, 1e-300))))
    tot = 0.0
    for k in TOTALS:
        bound = 2e-6 * np.abs(b[k]) + 1e-12 * np.abs(b[k]).max()
        tot = max(tot, float(np.max(np.abs(a[k] - b[k]) / np.maximum(bound, 1e-300))))
    return worst, tot


def test_fp32_first_solve_against_the_fp64_planes_and_the_oracle_at_every_tiling(ctx, port):
    """k_rt_flux_f32 at every tiling: the first solve on fp32 planes within test_first_solve_against_the_double_planes'
    bound (1e-5 |b| + 1e-7 max|b| on the spectral and band fluxes, 2e-6 on the totals) of the same column on fp64 planes,
    and of the CPU oracle fed the batch's Planck grid; finite, and not the fp64 result"""
    rows_out, failures = [], []
    for name, L, iso, env, kw, d, s in _first_solves(ctx):
        c = _make(L, iso, kw, "double")
        keys = fh.keys_for(c, SIX)
        a, b = s["cols"][0], d["cols"][0]
        o = fh.run_oracle(port, c, 1, planck_grid=d["planck_grid"])
        nwg = c.ny * c.nbin * c.nlayer
        o = {k: (o[k][:nwg] if k.startswith("Fc_") else o[k]) for k in keys + TOTALS}
        a_o = {k: (a[k][:nwg] if k.startswith("Fc_") else a[k]) for k in keys + TOTALS}
        for k in keys + TOTALS:
            assert np.all(np.isfinite(a[k])), (name, k)
        assert any(np.any(a[k] != b[k]) for k in keys), name
        e_d, e_o = _excess(a, b, keys), _excess(a_o, o, keys)
        rel = max(float(np.max(np.abs(a[k] - b[k]))) / float(np.abs(b[k]).max()) for k in keys)
        t = s["tiling"]
        rows_out.append("%-28s rows %2d k %2d%s  max|f32 - f64| / max|f64| %.1e  of the bound: fp64 %.3f / %.3f, oracle "
                        "%.3f / %.3f" % (name, t["ROWS"], t["k"], " generic" if t["generic_scans"] else "", rel,
                                         e_d[0], e_d[1], e_o[0], e_o[1]))
        if max(e_d + e_o) > 1.0:
            failures.append(rows_out[-1])
    print("\n(c) worst first-solve error per tiling (spectral / totals, as a fraction of the bound):\n" + "\n".join(rows_out))
    assert not failures, failures


# ---- (d) one column on every tiling ---------------------------------------------------------------------------------

FLUX_INSTANTIATION = r"k_rt_flux_f32<(\d+), (\d+), false>"


def _tilings_of(nlayer):
    """[(knobs, (rows, K))] of every fp32 tiling a column of nlayer layers can be forced onto: k = 8, 16, 32, 64 and the
    generic-scan kernel at k = 16, 32, 64 (K = 0: the runtime-k kernel)"""
    out = []
    for k in (8, 16, 32, 64):
        rows = -(-2 * nlayer // k)
        for generic in ((0, 1) if k >= 16 else (0,)):
            if rows <= 16 and _has_fp32_tiling(rows, k, generic):
                env = {"HELIOS_RT_K": k}
                if generic:
                    env["HELIOS_RT_GENERIC_SCANS"] = 1
                out.append((env, (rows, 0 if generic or k == 8 else k)))
    return out


def _cross_layer_counts():
    """layer counts that together put a column on every fp32 (ROWS, K): greedily, the count that adds most"""
    want = {(r, K) for K in (0, 16, 32, 64) for r in range(1, 14)} | {(14, 16)}
    chosen, have = [], set()
    while want - have:
        best = max(range(2, 417), key=lambda L: (len({t for _, t in _tilings_of(L)} - have), -L))
        new = {t for _, t in _tilings_of(best)} - have
        assert new, sorted(want - have)
        chosen.append(best)
        have |= new
    return sorted(chosen), want


def test_one_column_on_every_tiling_agrees_as_closely_in_fp32_as_in_fp64(ctx):
    """the sharp check: a plane value of (bin, Gauss point, half-layer) does not depend on the tiling, and the sweeps are
    fp64 in every kernel, so one column's first solve on two tilings may differ in fp32 only about as much as in fp64 (the
    association of the scans).  A kernel that read a wrong row, lane, plane or beam group in one instantiation would be
    orders of magnitude off, inside the 1e-5 of the test above.  For every pair of tilings A, B of a column, elementwise
    on the spectral and band fluxes:

        |f32_A - f32_B| <= max(8 |f64_A - f64_B|, 1e-14 max|f64|)

    Measured on an MI355X over these 26 columns and 126 tilings: the largest |f32_A - f32_B| is 5.5e-16 of max|f64|, the
    scans' rounding as in fp64, so no element comes near the floor (set 18 times above it; 1e-13 was the first estimate)
    and the factor 8 never binds.  The ratio itself is not small: max|f32_A - f32_B| / max|f64_A - f64_B| reaches 512 for
    a key and pair, because both are rounding noise of a different association and the fp64 pair can agree to an ulp of a
    small flux by chance.  The floor is the sharp part: a misread row, lane or plane is off by the plane value itself.
    And the compile-time scans against the generic kernel, after three iterations: the same bits at K = 16 and
    32, fluxes within 1e-12 at K = 64 -- what test_every_row_count_of_the_compile_time_kernels requires of the fp64 kernels.
    The layer counts together run every k_rt_flux_f32 instantiation of the code object."""
    layer_counts, want = _cross_layer_counts()
    ran, worst_ratio, worst_floor, worst_max_ratio, fails = set(), 0.0, 0.0, 0.0, []
    for i, L in enumerate(layer_counts):
        kw = _flags(i)
        c32, c64 = _make(L, 0, kw, "single"), _make(L, 0, kw, "double")
        keys = fh.keys_for(c32, SIX)
        runs = []
        for env, inst in _tilings_of(L):
            s, d = _run(ctx, c32, env), _run(ctx, c64, env)
            t = s["tiling"]
            assert t["coef_bytes"] == 4 and d["tiling"]["coef_bytes"] == 8, (L, env, t)
            assert (t["ROWS"], t["k"] if t["k"] >= 16 and not t["generic_scans"] else 0) == inst, (L, env, t)
            assert t["k"] == env["HELIOS_RT_K"]
            ran.add(inst)
            runs.append((env, s["cols"][0], d["cols"][0]))
        for ia in range(len(runs)):
            for ib in range(ia + 1, len(runs)):
                (ea, sa, da), (eb, sb, db) = runs[ia], runs[ib]
                for k in keys:
                    d32, d64 = np.abs(sa[k] - sb[k]), np.abs(da[k] - db[k])
                    floor = 1e-14 * np.abs(da[k]).max()
                    over = d32 > floor
                    if np.any(over):
                        worst_ratio = max(worst_ratio, float(np.max(d32[over] / np.maximum(d64[over], 1e-300))))
                    worst_floor = max(worst_floor, float(d32.max() / max(np.abs(da[k]).max(), 1e-300)))
                    if d64.max() > 0.0:
                        worst_max_ratio = max(worst_max_ratio, float(d32.max() / d64.max()))
                    if np.any(d32 > np.maximum(8.0 * d64, floor)):
                        fails.append((L, ea, eb, k, float(d32.max()), float(d64.max()), float(np.abs(da[k]).max())))
        # the compile-time scans against the runtime-k kernel on the same lanes, three iterations
        for k in (16, 32, 64):
            pair = [env for env, _ in _tilings_of(L) if env["HELIOS_RT_K"] == k]
            if len(pair) != 2:
                continue
            a, b = (_run(ctx, c32, env, n_iter=3, keys=SIX + ["F_net"])["cols"][0] for env in pair)
            for key in keys + ["F_net"]:
                msg = "%s, k = %d, %d layers, fp32 planes" % (key, k, L)
                if k == 64:
                    np.testing.assert_allclose(a[key], b[key], rtol=1e-12, atol=1e-13 * np.abs(b[key]).max(), err_msg=msg)
                else:
                    np.testing.assert_array_equal(a[key], b[key], err_msg=msg)
    print("\n(d) layer counts %s: %d fp32 flux instantiations (ROWS, K); largest |f32_A - f32_B| / |f64_A - f64_B| above "
          "the floor %.3g; largest |f32_A - f32_B| / max|f64| %.3g; largest max|f32_A - f32_B| / max|f64_A - f64_B| %.3g"
          % (layer_counts, len(ran), worst_ratio, worst_floor, worst_max_ratio))
    assert not fails, fails[:5]
    assert ran == want
    assert ran == {(r, K) for r, K in _instantiations(FLUX_INSTANTIATION)}


# ---- (e) batches ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nlayer,k", [(300, 64), (150, 32)])
def test_a_deep_batch_equals_single_columns_bit_for_bit(ctx, nlayer, k):
    """three columns with different temperature profiles in one fp32 batch against each column alone, with the v' plane and
    the beam: the same planes (coef_col is a stride in fp32 elements) and the same fluxes after 12 iterations"""
    c = _make(nlayer, 0, dict(nbin=3, clouds=1, scat_corr=1, g_0=0.2, dir_beam=1, albedo=0.2), "single")
    Ts = [c.T_lay, c.T_lay * 1.05, c.T_lay * 0.9 + 30.0]
    keys = ["T_lay", "F_up_band", "F_down_band", "F_up_wg", "F_down_wg", "F_net"]
    batch = _run(ctx, c, {}, n_iter=12, ncol=3, T_per_col=Ts, keys=keys)
    t = batch["tiling"]
    assert (t["k"], t["coef_bytes"], t["has_vp"], t["nplane"]) == (k, 4, 1, 6), t
    for i, T in enumerate(Ts):
        one = _run(ctx, c, {}, n_iter=12, ncol=1, T_per_col=[T], keys=keys)
        assert one["tiling"] == t
        for key in keys + ["planes"]:
            np.testing.assert_array_equal(batch["cols"][i][key], one["cols"][0][key], err_msg="%s column %d" % (key, i))
    assert np.any(batch["cols"][0]["planes"] != batch["cols"][1]["planes"])


# ---- (f) where the fp32 planes stop -----------------------------------------------------------------------------------

def test_where_the_fp32_planes_stop(ctx):
    """at every layer count of the device-resident loop (1-1024, isothermal 1-2048) the selected tiling has fp32 kernels
    exactly up to 832 half-layers -- 416 layers, 832 isothermal -- and the driver's message agrees; batches with
    `precision = single` at the edges and the transitions get the plane width that says"""
    from helios_amd.computation import Compute
    from helios_amd.rt import batch_from_case

    class Q(object):
        flux_calc_method = "iteration"
    for iso, top in ((0, 1024), (1, 2048)):
        Q.iso = iso
        for L in range(1, top + 1):
            r, k = _geometry(L, iso)
            Q.nlayer = L
            fp32 = _has_fp32_tiling(r, k)
            assert fp32 == ((L if iso else 2 * L) <= 832), (iso, L, r, k)
            assert fp32 == ("layers" not in Compute._why_fp64_planes(Q())), (iso, L)

    def width(nlayer, iso=0, env=None):
        c = _make(nlayer, iso, dict(nbin=2), "single")
        with _knobs(env or {}):
            rt = batch_from_case(ctx, c)
        try:
            return rt.coef_plane_bytes(), rt.flux_tiling()
        finally:
            rt.close()
    for nlayer, iso, env, want, tiling in [
            (2, 0, {}, 4, None), (416, 0, {}, 4, (13, 64)), (417, 0, {}, 8, (14, 64)), (1024, 0, {}, 8, (32, 64)),
            (2, 1, {}, 4, None), (832, 1, {}, 4, (13, 64)), (833, 1, {}, 8, (14, 64)), (2048, 1, {}, 8, (32, 64)),
            (105, 0, {}, 4, (14, 16)), (112, 0, {}, 4, (14, 16)),
            (105, 0, {"HELIOS_RT_GENERIC_SCANS": 1}, 8, (14, 16)), (112, 0, {"HELIOS_RT_GENERIC_SCANS": 1}, 8, (14, 16)),
            (220, 0, {"HELIOS_RT_K": 32}, 8, (14, 32)), (104, 0, {"HELIOS_RT_K": 16}, 4, (13, 16))]:
        b, t = width(nlayer, iso, env)
        assert b == want == t["coef_bytes"], (nlayer, iso, env, b, t)
        if tiling:
            assert (t["ROWS"], t["k"]) == tiling, (nlayer, iso, env, t)
