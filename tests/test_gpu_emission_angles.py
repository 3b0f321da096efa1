"""hx_emission_angles on the GPU held to the contract's restatement (tests/emission_reference.py), and the feature end to end.

The rule: every I_wg and I_band entry within max(1e-13, 8 eps) relative of the long-double restatement, eps being the
deviation of the plain fp64 evaluation of the contract from its long-double evaluation at that entry."""
import ctypes
import json
import os

import numpy as np
import pytest

import emission_reference as er

pytestmark = pytest.mark.gpu

LD = np.longdouble
TS = np.float64(er.T_SWITCH)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


def _depth_with_slant(target, mu_inv):
    """(dtau, m) with dtau * mu_inv[m] == target in fp64, searched a few ulp around target / mu_inv[m]"""
    for m in range(len(mu_inv)):
        d = target / mu_inv[m]
        cands = [d]
        for _ in range(6):
            cands = [np.nextafter(cands[0], 0)] + cands + [np.nextafter(cands[-1], np.inf)]
        for c in cands:
            if c * mu_inv[m] == target:
                return float(c), m
    raise AssertionError("no optical depth reaches %r along any angle" % (target,))


def _inputs(iso, X, Y, L, N, beam, seed, enclosure=None):
    """seeded column in shell-major arrays (the restatement's) plus the Planck arrays per layer and interface.  Optical
    depths 1e-7 ... 50; spread over the column: a shell of optical depth 0 exactly, shells whose slant optical depth is one ulp
    below / at / one ulp above the switch along an angle, a shell of 800, a cloud-only shell (gas 0), albedo 0 and
    1 - 1e-10.  `enclosure` = ("any" | "opaque"): B one value per bin, F_up = F_down = pi B, no beam."""
    rng = np.random.default_rng(seed)
    S = L if iso else 2 * L
    mu, mw, mu_inv = er.angles(N)
    dtau = 10.0 ** rng.uniform(-7, 1.7, (S, X, Y))
    cloud = 10.0 ** rng.uniform(-5, 0.5, (S, X)) * (rng.uniform(size=(S, X)) < 0.4)
    w0 = rng.uniform(0.0, 0.999, (S, X, Y))
    special = []
    edge = [_depth_with_slant(t, mu_inv) for t in (float(np.nextafter(TS, 0)), float(TS), float(np.nextafter(TS, 1)))]
    # one special value per (shell, bin) slot, dealt round the column
    kinds = ["zero", "below", "at", "above", "thick", "cloud_only", "w_zero", "w_one"]
    slots = [(s, x) for x in range(X) for s in range(S)]
    for n, (s, x) in enumerate(slots if S * X < 16 else slots[::2]):          # every other slot keeps its seeded values
        kind = kinds[(n + seed) % len(kinds)]
        special.append(kind)
        if kind == "zero":
            dtau[s, x, :], cloud[s, x] = 0.0, 0.0
        elif kind in ("below", "at", "above"):
            dtau[s, x, :], cloud[s, x] = edge[("below", "at", "above").index(kind)][0], 0.0
        elif kind == "thick":
            dtau[s, x, :], cloud[s, x] = 800.0, 0.0
        elif kind == "cloud_only":
            dtau[s, x, :], cloud[s, x] = 0.0, 10.0 ** rng.uniform(-3, 0.5)
        elif kind == "w_zero":
            w0[s, x, :] = 0.0
        else:
            w0[s, x, :] = 1.0 - 1e-10
    planck_lay = rng.uniform(1.0, 3.0, (L + 2, X)) * 10.0 ** rng.uniform(-3, 3, X)[None, :]
    planck_int = rng.uniform(1.0, 3.0, (L + 1, X)) * planck_lay[0][None, :] / 2.0
    shape_i, shape_c = (L + 1, X, Y), (L, X, Y)
    scale = np.pi * planck_lay[0][None, :, None]
    F = {n: scale * rng.uniform(0.2, 1.5, shape_i) for n in ("F_up", "F_down")}
    F.update({n: scale * rng.uniform(0.2, 1.5, shape_c) for n in ("Fc_up", "Fc_down")})
    # the beam's flux with either sign: the contract takes its modulus
    F["F_dir"] = scale * rng.uniform(-1.0, 1.0, shape_i)
    F["Fc_dir"] = scale * rng.uniform(-1.0, 1.0, shape_c)
    if enclosure:
        beam = False
        B = rng.uniform(1.2, 1.8, X)                       # one binade: an ulp of B is one number per bin
        planck_lay[:], planck_int[:] = B[None, :], B[None, :]
        for n in ("F_up", "F_down", "Fc_up", "Fc_down"):
            F[n][:] = (np.pi * B)[None, :, None]
        if enclosure == "opaque":
            dtau = rng.uniform(40.0, 900.0, (S, X, Y))     # t >= 40 along every angle: e < 5e-18
    w = np.polynomial.legendre.leggauss(Y)[1]
    return dict(iso=iso, X=X, Y=Y, L=L, N=N, beam=beam, dtau=dtau, cloud=cloud, w0=w0, planck_lay=planck_lay,
                planck_int=planck_int, F=F, w=w, mu=mu, mw=mw, mu_inv=mu_inv, beta=1.0 / (4.0 * np.pi * 0.7), special=special)


def _restatement_args(c):
    if c["iso"]:
        B_bot, B_top = er.planck_ends(c["planck_lay"][:c["L"]])
        Fk = [c["F"][n] for n in ("F_up", "F_down", "F_dir")]
    else:
        B_bot, B_top = er.planck_ends(c["planck_lay"][:c["L"]], c["planck_int"])
        Fk = [er.boundaries_of(c["F"][n], c["F"]["Fc" + n[1:]]) for n in ("F_up", "F_down", "F_dir")]
    return (c["dtau"], c["cloud"], c["w0"], B_bot, B_top, Fk[0], Fk[1], Fk[2] if c["beam"] else None, c["w"], c["mu_inv"],
            c["beta"])


def _run_kernel(ctx, c, want_wg=True):
    """hx_emission_angles through the C-ABI, the arrays in the layouts of the run: [c + ny*nbin*i] per spectral point,
    [x + nbin*i] the clouds', layer-fastest Planck arrays; half-layer shells as lower / upper halves of layer i"""
    from helios_amd import _lib
    l = _lib.lib()
    X, Y, L, N = c["X"], c["Y"], c["L"], c["N"]
    null = ctypes.POINTER(ctypes.c_double)()
    up = lambda a: ctx.to_gpu(np.ascontiguousarray(a, np.float64).ravel())
    dev = {}
    if c["iso"]:
        for k, n in (("dtau", "dtau"), ("cloud", "cloud"), ("w0", "w0")):
            dev[k] = up(c[n])
    else:
        for k, n in (("dtau", "dtau"), ("cloud", "cloud"), ("w0", "w0")):
            dev[k] = up(c[n][0::2])
            dev[k + "_up"] = up(c[n][1::2])
        dev["planck_int"] = up(c["planck_int"].T)
    dev["planck_lay"] = up(c["planck_lay"].T)
    for n in ("F_up", "F_down") + (("F_dir",) if c["beam"] else ()):
        dev[n] = up(c["F"][n])
        if not c["iso"]:
            dev["Fc" + n[1:]] = up(c["F"]["Fc" + n[1:]])
    dev["w"], dev["mu_inv"] = up(c["w"]), up(c["mu_inv"])
    guard = 8
    d_band = ctx.to_gpu(np.full(N * X + guard, -7.0))
    d_wg = ctx.to_gpu(np.full(N * X * Y + guard, -7.0)) if want_wg else None
    p = lambda k: dev[k].d if k in dev else null
    args = (ctx.handle, p("dtau"), p("dtau_up"), p("cloud"), p("cloud_up"), p("w0"), p("w0_up"), p("planck_lay"), p("planck_int"),
            p("F_up"), p("F_down"), p("F_dir"), p("Fc_up"), p("Fc_down"), p("Fc_dir"), p("w"), p("mu_inv"), float(c["beta"]),
            X, Y, L, N, d_band.d, d_wg.d if want_wg else null)
    ctx.check(l.hx_emission_angles(*args), "hx_emission_angles")
    band = d_band.get()
    ctx.check(l.hx_emission_angles(*args), "hx_emission_angles")          # a repeated launch repeats its bits
    assert np.array_equal(band, d_band.get())
    assert np.all(band[N * X:] == -7.0)                                   # nothing is written behind any array
    out = {"I_band": band[:N * X].reshape(N, X), "I_wg": None}
    if want_wg:
        wg = d_wg.get()
        assert np.all(wg[N * X * Y:] == -7.0)
        out["I_wg"] = wg[:N * X * Y].reshape(N, X, Y)
    for d in list(dev.values()) + [d_band, d_wg]:
        if d is not None:
            d.free()
    return out


def _hold(name, got, ref, plain):
    """the rule of the module docstring, figures first"""
    got, ref, plain = np.asarray(got, LD), np.asarray(ref, LD), np.asarray(plain, LD)
    bound = er.bound(ref, plain)
    err = np.abs(got - ref)
    scale = np.where(ref != 0, np.abs(ref), 1)
    print("%-7s max relative error %.2e (plain fp64: %.2e), worst error / bound %.2f"
          % (name, float((err / scale).max()), float((np.abs(plain - ref) / scale).max()),
             float((err / np.where(bound > 0, bound, 1)).max())))
    bad = np.nonzero(~(err <= bound))
    assert not len(bad[0]), (name, [tuple(int(i) for i in b) for b in zip(*bad)][:5], got[bad][:5], ref[bad][:5])


# (iso, nbin, ny, nlayer, N, beam): ny 1 / 7 (does not divide 256) / 20 (idle lanes); nbin 1 / 12 / 13 / 25 around the 12 bins
# of 20 points a workgroup holds, 37 and 74 past one workgroup of 7 and of 1; nlayer 1 / 2 / 5 / 33 (S = 1 and S = 2
# included); N 1 / 2 / 8 / 16 -- each value with each layer mode at least once
CASES = [(1, 1, 1, 1, 1, 0), (1, 12, 7, 2, 2, 1), (1, 13, 20, 5, 8, 0), (1, 25, 20, 33, 16, 1), (1, 37, 7, 5, 16, 0),
         (1, 300, 1, 2, 8, 1),
         (0, 1, 20, 1, 16, 1), (0, 12, 20, 2, 8, 0), (0, 13, 7, 5, 2, 1), (0, 25, 1, 33, 1, 0), (0, 25, 20, 33, 8, 1),
         (0, 37, 7, 2, 16, 0), (0, 13, 20, 1, 1, 1)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%s-x%d-y%d-l%d-n%d-%s" % (("half", "iso")[c[0]], c[1], c[2], c[3], c[4],
                                                                               ("dark", "beam")[c[5]]))
def test_kernel_against_the_restatement(ctx, case):
    iso, X, Y, L, N, beam = case
    c = _inputs(bool(iso), X, Y, L, N, bool(beam), seed=100 * X + 10 * L + N)
    out = _run_kernel(ctx, c)
    args = _restatement_args(c)
    ref, plain = er.emission(*args), er.plain_fp64(*args)
    _hold("I_wg", out["I_wg"], ref["I_wg"], plain["I_wg"])
    _hold("I_band", out["I_band"], ref["I_band"], plain["I_band"])
    # without I_wg asked for the band intensities are the same bits
    assert np.array_equal(_run_kernel(ctx, c, want_wg=False)["I_band"], out["I_band"])


def test_the_seeded_columns_hold_every_edge_value():
    """what the cases above are built from, asserted once: every kind of special shell in both layer modes, the slant optical
    depth one ulp on either side of the switch in fp64"""
    for N in (1, 2, 8, 16):
        mu_inv = er.angles(N)[2]
        for t in (np.nextafter(TS, 0), TS, np.nextafter(TS, 1)):
            d, m = _depth_with_slant(float(t), mu_inv)
            assert d * mu_inv[m] == t
    for iso in (True, False):
        kinds = set()
        for case in CASES:
            if bool(case[0]) == iso:
                kinds |= set(_inputs(iso, *case[1:5], bool(case[5]), seed=100 * case[1] + 10 * case[3] + case[4])["special"])
        assert kinds == {"zero", "below", "at", "above", "thick", "cloud_only", "w_zero", "w_one"}, (iso, kinds)


# An enclosure returns B.  Worst case in fp64, in ulps of B: the start F_up / pi is one off; a shell adds at most 2.5
# (the weights sum to 1 within half an ulp, three products and two sums) + 2.5 (a + b) for the source (J = B within one ulp,
# 1 - w0, two products, one sum), and passes e times the deviation it received.  So 8 ulps hold for one or two shells of any
# optical depth (1 + 2 * 2.5 = 6), and for any number of opaque shells (t >= 40: e < 5e-18, 5 ulps from the last one alone).
ENCLOSURES = [(1, 13, 20, 1, 16, "any"), (1, 25, 7, 2, 8, "any"), (0, 13, 20, 1, 16, "any"), (1, 13, 20, 33, 16, "opaque"),
              (0, 25, 20, 33, 8, "opaque"), (0, 12, 1, 5, 2, "opaque")]


@pytest.mark.parametrize("case", ENCLOSURES, ids=lambda c: "%s-x%d-y%d-l%d-n%d-%s" % ((("half", "iso")[c[0]],) + tuple(c[1:])))
def test_enclosure_on_the_device(ctx, case):
    iso, X, Y, L, N, kind = case
    c = _inputs(bool(iso), X, Y, L, N, False, seed=7 * X + L, enclosure=kind)
    out = _run_kernel(ctx, c)
    B = c["planck_lay"][0]
    ulps = np.abs(out["I_wg"] - B[None, :, None]) / np.spacing(B)[None, :, None]
    print("enclosure %s: largest deviation %.1f ulp" % (kind, ulps.max()))
    assert ulps.max() <= 8


def test_a_bins_result_does_not_depend_on_its_place(ctx):
    """the same bin alone (nbin = 1), as the last of 13 (the first of the second workgroup at 20 Gauss points) and inside 25"""
    base = _inputs(False, 25, 20, 5, 8, True, seed=3)

    def with_bin_at(X, at):
        c = _inputs(False, X, 20, 5, 8, True, seed=40 + X)
        for n in ("dtau", "w0"):
            c[n][:, at, :] = base[n][:, 4, :]
        c["cloud"][:, at] = base["cloud"][:, 4]
        c["planck_lay"][:, at], c["planck_int"][:, at] = base["planck_lay"][:, 4], base["planck_int"][:, 4]
        for n in c["F"]:
            c["F"][n][:, at, :] = base["F"][n][:, 4, :]
        return c
    alone = _run_kernel(ctx, with_bin_at(1, 0))
    last = _run_kernel(ctx, with_bin_at(13, 12))
    inside = _run_kernel(ctx, with_bin_at(25, 17))
    assert np.array_equal(alone["I_band"][:, 0], last["I_band"][:, 12]) and np.array_equal(alone["I_band"][:, 0], inside["I_band"][:, 17])
    assert np.array_equal(alone["I_wg"][:, 0], last["I_wg"][:, 12]) and np.array_equal(alone["I_wg"][:, 0], inside["I_wg"][:, 17])
    assert np.all(alone["I_band"] > 0) and np.ptp(alone["I_band"][:, 0]) > 0


def test_refused_arguments(ctx):
    from helios_amd import _lib
    l = _lib.lib()
    null = ctypes.POINTER(ctypes.c_double)()
    a = ctx.zeros(64)
    def call(ny=2, nlayer=1, nangle=1, upper=False, w0_upper=None):
        u = a.d if upper else null
        wu = u if w0_upper is None else (a.d if w0_upper else null)
        return l.hx_emission_angles(ctx.handle, a.d, u, a.d, u, a.d, wu, a.d, u, a.d, a.d, null, u, u, null, a.d, a.d, 0.0, 2, ny,
                                    nlayer, nangle, a.d, null)
    assert call() == 0 and call(upper=True) == 0
    assert call(nangle=0) == 1 and call(nangle=17) == 1
    assert b"emission angles" in l.hx_last_error(ctx.handle)
    assert call(nlayer=0) == 1 and call(upper=True, w0_upper=False) == 1
    assert call(ny=257) == 3
    a.free()


def test_the_kernel_keeps_nothing_in_scratch():
    """read from the code object's notes: no private segment, no spilled vector register, 32 KB of LDS.  (The notes also
    count 4 and 2 scalar registers that the compiler keeps in lanes of a vector register: no memory is involved, and they are
    not held to zero here -- DESIGN.md section 6 says so.)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("code_object_notes", os.path.join(ROOT, "tools", "code_object_notes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mine = [k for k in mod.kernel_notes() if "k_emission_angles" in k["name"]]
    assert len(mine) == 2
    for k in mine:
        print(k["name"], {n: k[n] for n in ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")})
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["group_segment_fixed_size"] == 32768


# ---- end to end ---------------------------------------------------------------------------------------------------------------
BASE = ["-parameter_file", "/nonexistent", "-opacity_mixing", "synthetic", "-synthetic", "20 6 5 11", "-number_of_layers", "12",
        "-maximum_number_of_iterations", "20000", "-radiative_equilibrium_criterion", "1e-4", "-convective_adjustment", "no"]
# the device-resident loop with the sweeps (beam on), with isothermal layers, with the matrix method; and the per-stage loop
# (isothermal layers), after which the Store's own fluxes are used as they are
MODES = {"loop": ["-direct_irradiation_beam", "yes"], "iso": ["-isothermal_layers", "yes"],
         "matrix": ["-direct_irradiation_beam", "yes", "-flux_calculation_method", "matrix"],
         "stage": ["-isothermal_layers", "yes"]}
FLUX_TOLERANCE = 1e-6          # the project's tolerance for fluxes


def _read_file(path, N):
    lines = open(path).read().split("\n")
    assert lines[3].split() == ["bin", "cent_lambda[um]", "angular_flux", "two_stream_flux"] + ["I(mu_%d)" % m for m in range(N)]
    head = [[float(v) for v in ln.split()[1:]] for ln in lines[1:3]]
    return np.array([[float(v) for v in ln.split()] for ln in lines[4:]]), head, lines


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """the same small synthetic run with the option on and off, in every mode"""
    import helios
    from helios_amd import computation
    out = {}
    init = computation.Compute.__init__

    def per_stage(self, ctx=None):
        init(self, ctx)
        self.use_fused = False
    for mode, extra in MODES.items():
        for on in (True, False):
            wd = str(tmp_path_factory.mktemp("em_%s_%d" % (mode, on)))
            if mode == "stage":
                computation.Compute.__init__ = per_stage
            try:
                q = helios.run_helios(BASE + extra + (["-emission_angles", "4"] if on else []) + ["-name", "em_0", "-output_directory", wd + "/"])
            finally:
                computation.Compute.__init__ = init
            out[(mode, on)] = (q, os.path.join(wd, "em_0"))
    return out


@pytest.mark.parametrize("mode", sorted(MODES))
def test_single_run_writes_the_restatement_of_its_own_column(runs, mode):
    q, out = runs[(mode, True)]
    iso = mode in ("iso", "stage")
    # only the per-stage run ends with the last flux solve on the Store; the others bring the loop's state over and re-solve
    assert (q.rt is None) == (mode == "stage") and q.spectral_fluxes_current
    assert q.flux_calc_method == ("matrix" if mode == "matrix" else "iteration")
    assert int(q.iso) == int(iso) and int(q.dir_beam) == int(not iso) and int(q.emission_angles) == 4
    L, X, Y, N = int(q.nlayer), int(q.nbin), int(q.ny), 4
    table, head, _lines = _read_file(os.path.join(out, "em_0_emission_angles.dat"), N)
    mu, mw, mu_inv = er.angles(N)
    assert L == 12 and table.shape == (X, 4 + N) and np.array_equal(table[:, 0], np.arange(X))
    # the file's numbers are the Store's
    assert head[0] == mu.tolist() and head[1] == mw.tolist()
    assert np.array_equal(q.emission_mu, mu) and np.array_equal(q.emission_weight, mw)
    assert np.array_equal(table[:, 2], q.emission_angular_flux) and np.array_equal(table[:, 4:].T, q.emission_intensity)
    assert np.array_equal(table[:, 3], np.asarray(q.F_up_band)[L * X:(L + 1) * X])
    # two_stream_flux is the column of the TOA flux file
    toa = [ln.split() for ln in open(os.path.join(out, "em_0_TOA_flux_eclipse.dat")).read().split("\n")[3:]]
    assert [float(r[5]) for r in toa] == [float("%g" % v) for v in table[:, 3]]
    # the restatement on the Store's own arrays
    get = lambda n: getattr(q, "dev_" + n).get()
    gas = lambda n: get(n)[:L * X * Y].reshape(L, X, Y)
    cl = lambda n: get(n)[:L * X].reshape(L, X)
    flux = lambda n, k: get(n)[:k * X * Y].reshape(k, X, Y)
    planck_lay = get("planckband_lay").reshape(X, L + 2).T
    if iso:
        shells = (gas("delta_tau_wg"), cl("delta_tau_all_clouds"), gas("w_0"))
        B_bot, B_top = er.planck_ends(planck_lay[:L])
        F = [flux(n, L + 1) for n in ("F_up_wg", "F_down_wg", "F_dir_wg")]
    else:
        shells = tuple(er.shells_of_layers(f(n + "_lower"), f(n + "_upper")) for f, n in
                       ((gas, "delta_tau_wg"), (cl, "delta_tau_all_clouds"), (gas, "w_0")))
        B_bot, B_top = er.planck_ends(planck_lay[:L], get("planckband_int").reshape(X, L + 1).T)
        F = [er.boundaries_of(flux(n, L + 1), flux("Fc" + n[1:], L)) for n in ("F_up_wg", "F_down_wg", "F_dir_wg")]
    beta = 1.0 / (4.0 * np.pi * abs(float(q.mu_star)))
    args = shells + (B_bot, B_top, F[0], F[1], None if iso else F[2], q.gauss_weight, mu_inv, beta)
    ref, plain = er.emission(*args, mu=mu, mu_weight=mw), er.plain_fp64(*args, mu=mu, mu_weight=mw)
    _hold("I_band", q.emission_intensity, ref["I_band"], plain["I_band"])
    _hold("F", q.emission_angular_flux, ref["F"], plain["F"])
    assert np.all(q.emission_intensity > 0) and (iso or np.abs(F[2]).max() > 0)
    # the TOA up-fluxes the kernel read, summed over y, against the run's own band flux
    band = np.zeros(X)
    for y in range(Y):
        band = band + (0.5 * q.gauss_weight[y]) * F[0][-1][:, y]
    toa_band = np.asarray(q.F_up_band)[L * X:(L + 1) * X]
    dev = float(np.abs(band / toa_band - 1).max())
    ratio = q.emission_angular_flux / toa_band
    print("%s: TOA up-flux read by the kernel against F_up_band: max relative deviation %.2e; angular / two-stream flux %.4f ... %.4f"
          % (mode, dev, ratio.min(), ratio.max()))
    if os.environ.get("EMISSION_PARITY_JSON"):
        path = os.environ["EMISSION_PARITY_JSON"]
        rec = json.load(open(path)) if os.path.exists(path) else {}
        rec[mode] = {"case": " ".join(BASE[2:] + MODES[mode] + ["-emission_angles", "4"]), "iterations": int(q.iter_value),
                     "toa_up_flux_max_relative_deviation": dev, "tolerance": FLUX_TOLERANCE,
                     "angular_over_two_stream_flux": [float(ratio.min()), float(ratio.max())]}
        with open(path, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
            f.write("\n")
    assert dev <= FLUX_TOLERANCE


@pytest.mark.parametrize("mode", sorted(MODES))
def test_option_off_changes_no_other_file(runs, mode):
    (_q, on), (q, off) = runs[(mode, True)], runs[(mode, False)]
    assert q.emission_intensity is None and int(q.emission_angles) == 0
    files = sorted(os.listdir(off))
    assert "em_0_emission_angles.dat" not in files and len(files) > 15
    assert sorted(os.listdir(on)) == sorted(files + ["em_0_emission_angles.dat"])
    for f in files:
        with open(os.path.join(on, f), "rb") as fa, open(os.path.join(off, f), "rb") as fb:
            assert fa.read() == fb.read(), f


def test_a_sweeps_column_writes_the_single_runs_file(runs, tmp_path):
    """the same case as one column of a two-column sweep: the same bytes"""
    import sweep
    single, sdir = runs[("loop", True)]
    wd = str(tmp_path)
    cols, _spectra = sweep.main(["-sweep", "radius_planet=1,1.3"] + BASE + MODES["loop"] +
                                ["-emission_angles", "4", "-name", "em", "-output_directory", wd + "/batch/"])
    assert len(cols) == 2 and int(cols[0].iter_value) == int(single.iter_value)
    with open(os.path.join(wd, "batch", "em_0", "em_0_emission_angles.dat"), "rb") as fa, \
            open(os.path.join(sdir, "em_0_emission_angles.dat"), "rb") as fb:
        assert fa.read() == fb.read()
    for n in ("emission_mu", "emission_weight", "emission_intensity", "emission_angular_flux"):
        assert np.array_equal(getattr(cols[0], n), getattr(single, n)), n
    # the other column (a larger radius leaves this plane-parallel column as it is) wrote its own Store's numbers
    table, _head, _lines = _read_file(os.path.join(wd, "batch", "em_1", "em_1_emission_angles.dat"), 4)
    assert np.array_equal(table[:, 4:].T, cols[1].emission_intensity) and np.array_equal(table[:, 2], cols[1].emission_angular_flux)
