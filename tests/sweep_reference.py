"""TEST INFRASTRUCTURE: the iteration sweeps of k_rt_flux<ROWS, K> (csrc/rt_flux_kernel.inc, the non-MATRIX branch) restated
in numpy.  Host only, no GPU here.

  restate            the pair of affine recurrences over the half-layers, sequential over the nodes 0 ... H and vectorised
                     over the spectral points, in long double; beside every value its companion magnitude m
  scan_twin          the same sweeps in plain fp64 in the KERNEL's association (local composition per lane, Hillis-Steele
                     composition over the k lanes, the boundary value, the replay); `fault` injects the mutants of
                     tests/test_sweep_reference.py
  check / holds      the rule  |got - ref| <= max(FLOOR, R 2^-53) m
  inputs_from_batch  the inputs of both from what an RTBatch serves, so that the device's own planes are restated
  slots / planes_of  where a (bin, Gauss point, half-layer) lies in the plane image

The recurrences.  A column has H half-layers (isothermal layers: one per layer) and the nodes 0 ... H, node 0 the surface;
half-layer h lies between its bottom node h and its top node h + 1.  With the planes alpha, beta, u', v' (dd, du with the
beam) and the Planck function B at the nodes

    sd = u' B[h] + v' B[h+1] (+ dd)         su = u' B[h+1] + v' B[h] (+ du)        isothermal layers: B[h] in both places

a sweep is
    D[H] = (1 - dir_beam) f (R*/a)^2 pi B_star,     D[h] = tiny(alpha D[h+1] + beta U_prev[h] + sd),   h = H-1 ... 0
    U[0] = albedo (Fdir0 + D[0]) + (1 - albedo) pi boaK B_surf
    U[h+1] = alpha U[h] + beta D[h+1] + su, h = 0 ... H-1, tiny() where the layers are isothermal or node h + 1 is an interface
with tiny(v) = |v| where |v| < 1e-100 (two_stream.h).  A step is nsweep sweeps; U carries over from sweep to sweep and from
step to step.  Where the tiling stores no v' plane, v' = Kconst ((1 - alpha) - beta) - u' with Kconst = 2 pi epsi.

The companion magnitude m is the same recurrence with every operand and every result replaced by its absolute value, so
that |a| + |b| stands for a +- b: a first-order bound of any evaluation's error is (its count of roundings) 2^-53 m.  One
place is sharper than that and still a bound: 1 - alpha, (1 - alpha) - beta and 1 - albedo subtract numbers that both
evaluations are GIVEN (the planes are fp64 on both sides), so each rounds relative to its own result and nothing before it
is amplified; their magnitudes are |1 - alpha| + |(1 - alpha) - beta| and |1 - albedo|, not 2 + |beta| and 1 + |albedo|
-- and where alpha >= 1/2 the difference 1 - alpha is exact in fp64 and in long double alike (Sterbenz), so only
|(1 - alpha) - beta| is left: a nearly conservative scatterer (beta = 1 - alpha up to 1e-5 of it) would otherwise carry a
magnitude 1e5 times its sources, and the rule would say nothing about them.
(With 1 + alpha in that place m would be 2 Kconst B in a thin half-layer whose sources are 1e-6 of that: the rule would not
see a wrong v' there.)  For a column without negative sources m is the value itself, v' derived from the planes aside.

R, the count of roundings.  One sweep direction of the kernel, for the value that leaves a lane's last row (every fma is one
rounding, -ffp-contract=off forms no others):
    local pass     t = fma(beta, U, s) and Bc = fma(alpha, Bc, t) per row, A *= alpha beside it      rows + 1 on Bc's chain
    scan           log2(k) combines, each Bc = fma(A, B2, Bc) and A *= A2                            log2(k), A's chain as long
    boundary       fma(A, D_toa, Bc), or fma(A, U[0], Bc)                                            1
    replay         per row fma(alpha, D, fma(beta, U, s)): the outer fma is on the chain, the inner
                   one feeds it                                                                      rows (+ rows beside it)
That is a chain of 2 rows + log2(k) + 2 roundings; counting also the roundings that FEED the chain at each of its links -- the
inner fma of the replay rows, A's products at the combines -- gives at most 3 rows + 2 log2(k) + 4 per direction.  The surface
value adds 3 on the way from D[0] to U[0] ((Fdir0 + D) albedo + ...), inside the + 4 of the up direction.  A sweep is two
directions, the second built on the first; the sources are formed once per launch: v' (4 roundings where it is derived), two
products and a sum, the beam term: 7; D_toa: 5.  So

    R = 2 nsweep n_steps (3 rows + 2 log2(k) + 4) + 8,

the figure the rule was asked to use; the chain alone counts nsweep n_steps (4 rows + 2 log2(k) + 9) + 7, less for every
tiling, so the rule's R is not short.  What R is NOT is the worst case over all roundings that reach a value: the relative
errors of BOTH operands of a product add, A after the scan is a product of up to H alphas with H - 1 roundings, and a source
H half-layers away reaches a value through all of them -- as it does in a sequential sweep.  That worst case is about
2 nsweep (H + 2 rows) 2^-53 m, 1.9e-12 m at 1024 layers, and needs every rounding of a transparent column to fall the same
way.  The rule asks for the depth instead and tests/test_sweep_reference.py proves on the CPU that the twin, which rounds
where the kernel rounds, keeps it at every tiling.  R is derived here and nowhere measured; the code under test never sets
it.  For every tiling of the GPU case list max(FLOOR, R 2^-53) <= 2e-13 (1.004e-13 at 32 rows on 64 lanes, FLOOR elsewhere).

Entries with |ref| < 1e-90 are compared by absolute value: tiny() decides their sign at 1e-100 on a rounding."""
import numpy as np

import lines_cases

LD = np.longdouble
FLOOR = lines_cases.FLOOR
TINY = 1e-100
SMALL = 1e-90
FAULTS = ("neighbour", "drop_widest", "stale_down", "pad_alpha0", "tiny_parity", "no_Fdir0", "zero_second_step")
FLUX_KEYS = ("F_up_wg", "F_down_wg", "Fc_up_wg", "Fc_down_wg")


# ---- where a half-layer of a spectral point lies in the plane image ------------------------------------------------

def slots(t, nbin, ny, H):
    """(x, y, h, padding) per slot, each (tiles, ROWS, 64): plane_coding.decode_slot's arithmetic on whole arrays"""
    ntiles = -(-nbin // t["nxb"]) * t["nparts"] * t["NW"]
    tile = np.arange(ntiles)[:, None, None]
    row = np.arange(t["ROWS"])[None, :, None]
    lane = np.arange(64)[None, None, :]
    wv, part, bx = tile % t["NW"], (tile // t["NW"]) % t["nparts"], tile // (t["NW"] * t["nparts"])
    s_local = (wv * 64 + lane) // t["k"]
    xl, yl = s_local // t["ypb"], s_local % t["ypb"]
    x, y = bx * t["nxb"] + xl, part * t["ypb"] + yl
    h = (lane % t["k"]) * t["ROWS"] + row
    pad = (s_local >= t["nxb"] * t["ypb"]) | (x >= nbin) | (y >= ny) | (h >= H)
    shape = np.broadcast(x, y, h).shape
    return tuple(np.broadcast_to(a, shape) for a in (x, y, h, pad))


def planes_of(c, t, p64):
    """the six planes per slot as k_rt_flux reads them: v' from its plane, or 2 pi epsi ((1 - alpha) - beta) - u'"""
    out = dict(alpha=p64[:, 0], beta=p64[:, 1], up=p64[:, 2])
    out["vp"] = p64[:, t["pl_vp"]] if t["has_vp"] else 2.0 * np.pi * c.epsi * ((1.0 - out["alpha"]) - out["beta"]) - out["up"]
    if c.dir_beam:
        out["dd"], out["du"] = p64[:, t["pl_dd"]], p64[:, t["pl_dd"] + 1]
    return out


# ---- the rule --------------------------------------------------------------------------------------------------------

def rounding_count(rows, k, nsweep, n_steps=1):
    """R of the module's docstring"""
    log2k = int(k).bit_length() - 1
    assert 1 << log2k == k
    return 2 * nsweep * n_steps * (3 * rows + 2 * log2k + 4) + 8


def rel_bound(rows, k, nsweep, n_steps=1):
    return max(FLOOR, rounding_count(rows, k, nsweep, n_steps) * 2.0 ** -53)


def deviations(got, ref, m):
    """(|got - ref|, m) in float64; where |ref| < 1e-90 the absolute values are compared"""
    got, ref, m = np.asarray(got, LD), np.asarray(ref, LD), np.asarray(m, LD)
    err = np.where(np.abs(ref) < SMALL, np.abs(np.abs(got) - np.abs(ref)), np.abs(got - ref))
    return err.astype(np.float64), m.astype(np.float64)


def holds(got, ref, m, bound):
    """bool per entry: the rule, and finite"""
    err, mm = deviations(got, ref, m)
    return np.isfinite(np.asarray(got, np.float64)) & (err <= bound * mm)


def check(got, ref, m, bound, label=""):
    """prints the largest err / bound and err / m over the entries and returns (largest err / bound, largest err / m, the
    flat indices that break the rule)"""
    err, mm = deviations(got, ref, m)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(err == 0.0, 0.0, err / mm)            # (m = 0 with err != 0: inf)
    rel = np.where(np.isfinite(np.asarray(got, np.float64)), rel, np.inf)
    worst = float(rel.max()) if rel.size else 0.0
    print("%-44s largest err / bound %.3f, largest err / m %.2e (bound %.2e)" % (label, worst / bound, worst, bound))
    return worst / bound, worst, np.nonzero(rel.ravel() > bound)[0]


def cancelled_fraction(ref, m):
    """the share of entries with m > 100 |ref|: where the rule says little"""
    ref, m = np.abs(np.asarray(ref, LD)), np.asarray(m, LD)
    return float(np.mean(m > 100 * ref)) if ref.size else 0.0


# ---- the restatement -------------------------------------------------------------------------------------------------

def _tiny(v):
    a = np.abs(v)
    return np.where(a < TINY, a, v)


def _sources(inp, T):
    """(alpha, beta, sd, su) and the magnitudes (m_sd, m_su), each [H][points] of dtype T"""
    al, be, up = (np.asarray(inp[k], T) for k in ("alpha", "beta", "up"))
    H = al.shape[0]
    B = np.asarray(inp["B"], T)
    Bb = B[:H]
    Bt = Bb if inp["iso"] else B[1:H + 1]
    if inp.get("vp") is not None:
        vp = np.asarray(inp["vp"], T)
        m_vp = np.abs(vp)
    else:
        K = T(inp["Kconst"])
        one_minus = T(1) - al
        rest = one_minus - be
        vp = K * rest - up
        # (1 - alpha is exact for alpha >= 1/2 -- Sterbenz -- in both evaluations: nothing of it to carry)
        m_vp = K * (np.where(al < T(0.5), np.abs(one_minus), T(0)) + np.abs(rest)) + np.abs(up)
    sd, su = up * Bb + vp * Bt, up * Bt + vp * Bb
    m_sd, m_su = np.abs(up) * np.abs(Bb) + m_vp * np.abs(Bt), np.abs(up) * np.abs(Bt) + m_vp * np.abs(Bb)
    if inp["dir_beam"]:
        dd, du = np.asarray(inp["dd"], T), np.asarray(inp["du"], T)
        sd, su, m_sd, m_su = sd + dd, su + du, m_sd + np.abs(dd), m_su + np.abs(du)
    return al, be, sd, su, m_sd, m_su


def _boundaries(inp, T):
    rs = T(inp["R_star"]) / T(inp["a"])
    D_toa = T(1.0 - inp["dir_beam"]) * T(inp["f_factor"]) * (rs * rs) * T(np.pi) * np.asarray(inp["Bstar"], T)
    albedo = np.asarray(inp["albedo"], T)
    emit = (T(1) - albedo) * T(np.pi) * np.asarray(inp["boaK"], T) * np.asarray(inp["Bsurf"], T)
    return D_toa, albedo, np.asarray(inp["Fdir0"], T), emit


def restate(inputs, nsweep, n_steps, T=LD):
    """dict(U, D, mU, mD), each [n_steps][H + 1][points] of dtype T: the fluxes at the nodes after each step and their
    companion magnitudes.  `inputs`: alpha, beta, up, vp (None: derived with Kconst), dd, du (with dir_beam) as [H][points];
    B [H + 1][points]; Bstar, Bsurf, albedo, boaK, Fdir0 [points]; f_factor, R_star, a, dir_beam, iso, Kconst; and
    U [H + 1][points], the up-flux state before the first step."""
    al, be, sd, su, m_sd, m_su = _sources(inputs, T)
    aal, abe = np.abs(al), np.abs(be)
    H, iso = al.shape[0], bool(inputs["iso"])
    D_toa, albedo, Fdir0, emit = _boundaries(inputs, T)
    U = np.array(inputs["U"], T)
    mU = np.abs(U)
    D, mD = np.zeros_like(U), np.zeros_like(U)
    out = dict(U=[], D=[], mU=[], mD=[])
    for _ in range(n_steps):
        for _ in range(nsweep):
            D[H], mD[H] = D_toa, np.abs(D_toa)
            for h in range(H - 1, -1, -1):              # U[h], mU[h]: the previous sweep's
                D[h] = _tiny(al[h] * D[h + 1] + be[h] * U[h] + sd[h])
                mD[h] = aal[h] * mD[h + 1] + abe[h] * mU[h] + m_sd[h]
            U[0] = albedo * (Fdir0 + D[0]) + emit
            mU[0] = np.abs(albedo) * (np.abs(Fdir0) + mD[0]) + np.abs(emit)
            for h in range(H):
                v = al[h] * U[h] + be[h] * D[h + 1] + su[h]
                U[h + 1] = _tiny(v) if (iso or (h + 1) % 2 == 0) else v
                mU[h + 1] = aal[h] * mU[h] + abe[h] * mD[h + 1] + m_su[h]
        for key, v in (("U", U), ("D", D), ("mU", mU), ("mD", mD)):
            out[key].append(v.copy())
    return {k: np.array(v) for k, v in out.items()}


# ---- the twin: fp64 in the kernel's association ------------------------------------------------------------------------

def _on_lanes(a, rows, k, fill):
    """[H][points] -> [k lanes][rows][points], half-layer h in lane h // rows, row h % rows; `fill` in the padding rows"""
    H, P = a.shape
    out = np.full((k * rows, P), fill, np.float64)
    out[:H] = a
    return out.reshape(k, rows, P)


def _from_above(v, n, edge):
    """per lane j the value of lane j + n; `edge` where there is none"""
    out = np.empty_like(v)
    out[:v.shape[0] - n] = v[n:]
    out[v.shape[0] - n:] = edge
    return out


def _from_below(v, n, edge):
    out = np.empty_like(v)
    out[n:] = v[:v.shape[0] - n]
    out[:n] = edge
    return out


def scan_twin(inputs, rows, k, nsweep, n_steps, fault=None):
    """dict(U, D), each [n_steps][H + 1][points] float64: the sweeps as k_rt_flux<rows, k> associates them -- per lane the
    local composition (A, Bc) over its rows, a Hillis-Steele composition over the k lanes of a spectral point, the
    boundary value applied in one step, the replay through the rows; padding rows are the identity (alpha = 1, beta = 0,
    no sources).  numpy has no fma: a product and a sum stand for one, two roundings for one.  `fault`: one of FAULTS."""
    assert fault is None or fault in FAULTS, fault
    f64 = np.float64
    al_h, be_h, sd_h, su_h, _, _ = _sources(inputs, f64)
    H, P = al_h.shape
    assert k * rows >= H and k & (k - 1) == 0, (H, rows, k)
    iso = bool(inputs["iso"])
    al = _on_lanes(al_h, rows, k, 0.0 if fault == "pad_alpha0" else 1.0)
    be, sd, su = (_on_lanes(a, rows, k, 0.0) for a in (be_h, sd_h, su_h))
    D_toa, albedo, Fdir0, emit = _boundaries(inputs, f64)
    if fault == "no_Fdir0":
        Fdir0 = np.zeros_like(Fdir0)
    reach = 2 if fault == "neighbour" else 1               # the lane the boundary values are taken from
    steps = [n for n in (1, 2, 4, 8, 16, 32) if n < k]
    if fault == "drop_widest":
        steps = steps[:-1]
    node = np.arange(k * rows).reshape(k, rows, 1) + 1      # the top node of each row
    flip_up = np.ones_like(node, bool) if iso else (node % 2 == (1 if fault == "tiny_parity" else 0))
    state = np.asarray(inputs["U"], f64)
    U0 = state[0].copy()
    Uo = _on_lanes(state[1:], rows, k, 0.0)
    Do = np.zeros_like(Uo)
    D_edge = np.broadcast_to(D_toa, (reach, P))
    out = dict(U=[], D=[])
    for step in range(n_steps):
        if fault == "zero_second_step" and step == 1:
            U0, Uo = np.zeros_like(U0), np.zeros_like(Uo)
        for _ in range(nsweep):
            D_prev = Do
            # ---- down
            Ubelow = _from_below(Uo[:, rows - 1], 1, U0)
            A, Bc = np.ones((k, P)), np.zeros((k, P))
            for r in range(rows - 1, -1, -1):
                Uh = Uo[:, r - 1] if r > 0 else Ubelow
                Bc = al[:, r] * Bc + (be[:, r] * Uh + sd[:, r])
                A = A * al[:, r]
            for n in steps:                                 # inclusive suffix composition over the lanes
                A2, B2 = _from_above(A, n, 1.0), _from_above(Bc, n, 0.0)
                Bc = A * B2 + Bc
                A = A * A2
            D = _from_above(A * D_toa + Bc, reach, D_edge)
            Do = np.empty_like(Uo)
            for r in range(rows - 1, -1, -1):
                Uh = Uo[:, r - 1] if r > 0 else Ubelow
                D = _tiny(al[:, r] * D + (be[:, r] * Uh + sd[:, r]))
                Do[:, r] = D
            # ---- surface
            U0 = albedo * (Fdir0 + Do[0, 0]) + emit
            # ---- up
            Dsrc = D_prev if fault == "stale_down" else Do
            Dabove = _from_above(Dsrc[:, 0], 1, D_toa)
            A, Bc = np.ones((k, P)), np.zeros((k, P))
            for r in range(rows):
                Dh = Dsrc[:, r + 1] if r < rows - 1 else Dabove
                Bc = al[:, r] * Bc + (be[:, r] * Dh + su[:, r])
                A = A * al[:, r]
            for n in steps:                                 # inclusive prefix composition
                A2, B2 = _from_below(A, n, 1.0), _from_below(Bc, n, 0.0)
                Bc = A * B2 + Bc
                A = A * A2
            U = _from_below(A * U0 + Bc, reach, np.broadcast_to(U0, (reach, P)))
            Unew = np.empty_like(Uo)
            for r in range(rows):
                Dh = Dsrc[:, r + 1] if r < rows - 1 else Dabove
                U = al[:, r] * U + (be[:, r] * Dh + su[:, r])
                U = np.where(flip_up[:, r], _tiny(U), U)
                Unew[:, r] = U
            Uo = Unew
        out["U"].append(np.concatenate([U0[None], Uo.reshape(k * rows, P)[:H]]))
        out["D"].append(np.concatenate([Do.reshape(k * rows, P)[:H], D_toa[None] * np.ones((1, P))]))
    return {key: np.array(v) for key, v in out.items()}


# ---- between the nodes and the reference's flux arrays ---------------------------------------------------------------------

def to_wg(U, D, iso, nlayer):
    """F_up_wg, F_down_wg, Fc_up_wg, Fc_down_wg in the reference's layout [level][bin][Gauss point] (flat, the centre
    arrays as long as the interface ones) from the nodes [H + 1][points]; with isothermal layers there are no centre
    fluxes"""
    P, I = U.shape[1], nlayer + 1
    zero = np.zeros((I, P), U.dtype)
    if iso:
        return dict(F_up_wg=U.reshape(-1), F_down_wg=D.reshape(-1), Fc_up_wg=zero.reshape(-1), Fc_down_wg=zero.reshape(-1))
    cu, cd = zero.copy(), zero.copy()
    cu[:nlayer], cd[:nlayer] = U[1::2], D[1::2]
    return dict(F_up_wg=U[0::2].reshape(-1), F_down_wg=D[0::2].reshape(-1), Fc_up_wg=cu.reshape(-1), Fc_down_wg=cd.reshape(-1))


def nodes_of_wg(F_wg, Fc_wg, iso, nlayer, npoints):
    """[H + 1][points] from an interface array and its centre array as RTBatch.get returns them"""
    I = nlayer + 1
    F = np.asarray(F_wg).reshape(I, npoints)
    if iso:
        return F.copy()
    out = np.empty((2 * nlayer + 1, npoints), F.dtype)
    out[0::2], out[1::2] = F, np.asarray(Fc_wg).reshape(I, npoints)[:nlayer]
    return out


def planck_nodes(planckband_lay, planckband_int, iso, nbin, ny, nlayer):
    """(B [H + 1][points], the star row, the surface value [points]) from the two band arrays ([bin][layer, star, surface]
    and [bin][interface]); points are y + ny x"""
    lay = np.asarray(planckband_lay).reshape(nbin, nlayer + 2)
    H = nlayer if iso else 2 * nlayer
    B = np.zeros((H + 1, nbin), lay.dtype)
    if iso:
        B[:H] = lay[:, :nlayer].T          # (the node above the top layer is not read)
    else:
        B[1::2] = lay[:, :nlayer].T
        B[0::2] = np.asarray(planckband_int).reshape(nbin, nlayer + 1).T
    rep = lambda a: np.repeat(a, ny, axis=-1)
    return rep(B), rep(lay[:, nlayer]), rep(lay[:, nlayer + 1])


def inputs_from_batch(rt, c, col=0, column=None):
    """the inputs of restate / scan_twin from what batch `rt` of case `c` serves for column `col`: the coefficient planes of
    the last refresh, the Planck nodes, the beam at the surface, boa_source_factor, the up-flux state as it is NOW, and the
    column's parameters (`column`: what differs from the case's, as batch_from_case's `columns`, and `surf_albedo`)"""
    t, p = rt.flux_tiling(), rt.coef_planes(col)
    assert p.dtype == np.float64, "fp64 planes only"
    X, Y, L, iso = c.nbin, c.ny, c.nlayer, int(c.iso)
    H = L if iso else 2 * L
    x, y, h, pad = slots(t, X, Y, H)
    where = (h[~pad], (y + Y * x)[~pad])
    inp = dict(iso=iso, dir_beam=int(c.dir_beam), Kconst=2.0 * np.pi * c.epsi)
    names = dict(alpha=0, beta=1, up=2)
    if t["has_vp"]:
        names["vp"] = t["pl_vp"]
    if c.dir_beam:
        names.update(dd=t["pl_dd"], du=t["pl_dd"] + 1)
    for name, plane in names.items():
        cube = np.full((H, X * Y), np.nan)
        cube[where] = p[:, plane][~pad]
        assert not np.isnan(cube).any(), name
        inp[name] = cube
    if not t["has_vp"]:
        inp["vp"] = None
    inp["B"], inp["Bstar"], inp["Bsurf"] = planck_nodes(rt.get("planckband_lay", col), rt.get("planckband_int", col), iso, X, Y, L)
    inp["Fdir0"] = rt.get("F_dir_wg", col)[:X * Y]
    inp["boaK"] = rt.get("boa_source_factor", col)
    par = dict(c, **(column or {}))
    inp["albedo"] = np.repeat(np.asarray(par["surf_albedo"], np.float64), Y)
    inp["f_factor"], inp["R_star"], inp["a"] = float(par["f_factor"]), float(par["R_star"]), float(par["a"])
    inp["U"] = nodes_of_wg(rt.get("F_up_wg", col), rt.get("Fc_up_wg", col), iso, L, X * Y)
    inp["pad_share"] = float(pad.mean())
    return inp
