"""add_to_mixed_opac (kernels.cu:3283-3397) restated in numpy for ANY number of Gauss points: 20 -> ny, 400 -> ny^2,
399 -> ny^2 - 1, 19 -> ny - 1, everything else in the reference's own order of operations.  Vectorised over the problems
(one per bin and level); the sort is numpy's stable one on the fill-ordered sums (the reference's adjacent-swap passes with
a strict '<' are a stable sort), the re-binning walk an explicit left-to-right loop over the sorted sums.

At ny = 20 it equals the oracle's port of the kernel bit for bit (tests/test_ro_reference.py); the device's general mixer
(csrc/random_overlap_ny.h) is held to it for ny < 20 (tests/test_gpu_ro_ny.py).  Also here: the problems both tests use."""
import numpy as np


def fill_order(ny, yx, mix_first):
    """(y1, y2) per fill position: y1 indexes the running mix, y2 the new absorber (:3332-3365)"""
    y1 = np.empty(ny * ny, np.int64)
    y2 = np.empty(ny * ny, np.int64)
    for outer in range(ny):                 # first region: the curve that is stronger at y = 0 on the outer loop
        for inner in range(yx):
            pos = inner + yx * outer
            y1[pos], y2[pos] = (outer, inner) if mix_first else (inner, outer)
    for outer in range(yx, ny):             # second region: the other curve on the outer loop
        for inner in range(ny):
            pos = inner + ny * outer
            y1[pos], y2[pos] = (inner, outer) if mix_first else (outer, inner)
    return y1, y2


def mix_problems(mixed, new, gw, gy, with_skipped=False):
    """mixed, new: (problems, ny), the running mix and the scaled coefficients of the new absorber -> the new mix; with_skipped:
    and per problem whether a Gauss point met the interval of its predecessor and was read off the next one, by
    extrapolation (the reference prints "malfunctioning" there, :3384; it happens with few points and coarse weights)"""
    mixed = np.asarray(mixed, np.float64)
    new = np.asarray(new, np.float64)
    nprob, ny = mixed.shape
    skipped = np.zeros(nprob, bool)
    if ny == 1:                                                                    # :3302
        return (mixed + new, skipped) if with_skipped else mixed + new
    n = ny * ny
    out = mixed.copy()
    negligible = (0.01 * mixed[:, 0] > new[:, ny - 1]) | (0.01 * new[:, 0] > mixed[:, ny - 1])      # :3297
    out[negligible] = mixed[negligible] + new[negligible]
    above = mixed > new
    yx = np.full(nprob, ny)
    for y in range(1, ny):                                                         # the LAST crossing (:3323-3329)
        yx[above[:, y] != above[:, y - 1]] = y
    mix_first = mixed[:, 0] > new[:, 0]
    hw = 0.5 * gw
    K = np.empty((nprob, n))
    G = np.empty((nprob, n))
    for x in np.unique(yx):
        for first in (False, True):
            sel = np.nonzero((yx == x) & (mix_first == first) & ~negligible)[0]
            if sel.size:
                y1, y2 = fill_order(ny, int(x), first)
                K[sel] = mixed[sel][:, y1] + new[sel][:, y2]
                G[sel] = (hw[y1] * hw[y2])[None, :]
    live = np.nonzero(~negligible)[0]
    K, G = K[live], G[live]
    order = np.argsort(K, axis=1, kind="stable")                                   # sort_array (:3152-3171)
    K = np.take_along_axis(K, order, axis=1)
    G = np.take_along_axis(G, order, axis=1)
    Y = np.empty_like(K)
    Y[:, 0] = 0.5 * G[:, 0]
    for w in range(1, n):                                                          # :3371-3376
        Y[:, w] = Y[:, w - 1] + 0.5 * G[:, w - 1] + 0.5 * G[:, w]
    res = mixed[live].copy()              # an entry the walk does not reach stays what it was
    y = np.zeros(live.size, np.int64)
    going = np.ones(live.size, bool)
    rows = np.arange(live.size)
    for w in range(1, n):                                                          # :3381-3396
        q = gy[y]
        hit = going & (Y[:, w] > q)
        h = rows[hit]
        skipped[live[h[Y[h, w - 1] > q[h]]]] = True
        res[h, y[h]] = (K[h, w - 1] * (Y[h, w] - q[h]) + K[h, w] * (q[h] - Y[h, w - 1])) / (Y[h, w] - Y[h, w - 1])
        going[h[y[h] == ny - 1]] = False
        y[h[y[h] < ny - 1]] += 1
    out[live] = res
    return (out, skipped) if with_skipped else out


def add_to_mixed_opac(vmr, opac_spec, opac_wg, meanmolmass, gauss_weight, gauss_y, mass_spec, s, ro_method, ny, nbin, nlev):
    """the kernel's argument list (oracle/helios_oracle.h); opac_wg is updated in place"""
    n = nlev * nbin * ny            # (the arrays may be longer: a caller's buffers for the interfaces serve its layers too)
    spec = np.asarray(opac_spec)[:n].reshape(nlev, nbin, ny)
    mixed = opac_wg[:n].reshape(nlev, nbin, ny)
    new = (vmr * mass_spec / meanmolmass)[:, None, None] * spec                    # :3293
    if ro_method == 0 or s == 0 or ny == 1:
        mixed += new
        return
    mixed[...] = mix_problems(mixed.reshape(-1, ny), new.reshape(-1, ny), np.asarray(gauss_weight), np.asarray(gauss_y)).reshape(mixed.shape)


FAC = 1e-3 * 18.0 / 2.3        # vmr * mass / mu of the calls below


def call(impl, ny, mix0, spec, gw, gy):
    """one add_to_mixed_opac of `impl` (the oracle's signature) on problems (nlev, nbin, ny); returns the new mix"""
    from helios_amd import phys_const as pc
    nlev, nbin = mix0.shape[:2]
    mix = np.ascontiguousarray(mix0.reshape(-1)).copy()
    impl.add_to_mixed_opac(np.full(nlev, 1e-3), np.ascontiguousarray(spec.reshape(-1)), mix, np.full(nlev, 2.3 * pc.AMU), gw, gy,
                           18.0 * pc.AMU, 1, 1, ny, nbin, nlev)
    return mix.reshape(mix0.shape)


def cases(ny, nbin=48, nlev=3, seed=17):
    """the problem kinds of tests/test_gpu_stages.py::_ro_cases at any ny: name -> (mix, species coefficients)"""
    rng = np.random.default_rng(seed + ny)
    shape = (nlev, nbin, ny)
    generic = np.sort(10.0 ** rng.uniform(-4, 0, shape), axis=2)
    out = {}
    out["generic"] = (generic, np.sort(10.0 ** rng.uniform(-4, 0, shape), axis=2) / FAC)
    out["wide"] = (np.sort(10.0 ** rng.uniform(-12, 6, shape), axis=2), np.sort(10.0 ** rng.uniform(-12, 6, shape), axis=2) / FAC)
    out["coarse"] = (np.round(generic, 1) + 0.1, (np.round(generic[::-1], 1) + 0.1) / FAC)          # exact ties
    out["flat_mix"] = (np.full(shape, 0.25), out["generic"][1])
    out["flat_both"] = (np.full(shape, 0.25), np.full(shape, 0.5) / FAC)
    out["unsorted"] = (10.0 ** rng.uniform(-2, 0, shape), 10.0 ** rng.uniform(-2, 0, shape) / FAC)
    curve = np.sort(10.0 ** rng.uniform(-3, 1, shape), axis=2)
    out["same_shape"] = (curve, curve * (1.0 + 1e-9 * rng.uniform(-1, 1, shape)) / FAC)
    out["narrow"] = (1.0 + 1e-5 * np.sort(rng.uniform(0, 1, shape), axis=2), (1.0 + 1e-5 * np.sort(rng.uniform(0, 1, shape), axis=2)) / FAC)
    out["tiny_min"] = (np.sort(10.0 ** rng.uniform(-300, 6, shape), axis=2), np.sort(10.0 ** rng.uniform(-300, 6, shape), axis=2) / FAC)
    out["dominated"] = (generic, np.sort(generic[..., ::-1] * 0.03, axis=2) / FAC)                  # just above the 1 % threshold
    return out


def crossing_rows(ny, seed=77):
    """two ascending curves that cross once behind Gauss point yx - 1 for every yx = 1 ... ny - 1, either curve the stronger
    one at y = 0, over 1.5 and 14 decades; curves that cross several times; rows of the tableau that touch exactly and by
    one ulp, and rows far apart.  (1, problems, ny) each."""
    rng = np.random.default_rng(seed + ny)
    rows = []
    for decades in (1.5, 14.0):
        for yx in range(1, ny):
            for first in (0, 1):
                a = np.sort(10.0 ** rng.uniform(-3.0, -3.0 + decades, ny))
                b = np.where(np.arange(ny) < yx, a * rng.uniform(0.55, 0.95, ny), a * rng.uniform(1.05, 1.8, ny))
                b = np.maximum.accumulate(b)
                rows.append((a, b) if first else (b, a))
        for _ in range(12):
            a = np.sort(10.0 ** rng.uniform(-3.0, -3.0 + decades, ny))
            rows.append((a, np.maximum.accumulate(a * np.where(rng.uniform(size=ny) < 0.5, 0.8, 1.25))))
    inner = np.linspace(1.0, 2.0, ny)
    outer = 4.0 + np.arange(ny) * 1.0
    rows.append((outer, inner))
    rows.append((outer, inner * (1.0 + np.where(np.arange(ny) == ny - 1, 2.3e-16, 0.0))))
    rows.append((outer * 64.0, inner))
    mix0 = np.array([r[0] for r in rows])[None]
    spec = np.array([r[1] for r in rows])[None] / FAC
    return mix0, spec
