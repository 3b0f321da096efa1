"""The per-iteration kernels around the sweeps, restated in numpy bit for bit: the order of the wavelength sum
(k_rt_totals_a, k_rt_totals_b) and the Planck values at the nodes (k_rt_nodes).  How these kernels batch their loads is
free; what they add, and in which order, is not.

The wavelength sum: per chunk of per = ceil(X / nchunk) bins, (F_dir + F_down) * dl (down) and F_up * dl (up) are added
serially in bin order, the product rounded before the addition; the chunks are added serially inside four segments of
ceil(nchunk / 4) chunks, the segments combined as ((s0 + s1) + s2) + s3; F_net = up - down."""
import contextlib
import os

import numpy as np
import pytest

import cases

pytestmark = pytest.mark.gpu
KNOBS = ("HELIOS_RT_NCHUNK",)


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    c = Context(0)
    yield c


@contextlib.contextmanager
def _knobs(env):
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


def _batch(ctx, c, nchunk=None, ncol=1):
    from helios_amd.rt import batch_from_case
    with _knobs({} if nchunk is None else dict(HELIOS_RT_NCHUNK=nchunk)):
        rt = batch_from_case(ctx, c, ncol=ncol)
    rt.build_planck_table(1 if c.T_star > 10 else 0)
    return rt


def restated_totals(f_up, f_down, f_dir, dl, nchunk):
    """(F_up_tot, F_down_tot, F_net) from band fluxes [I][X] in the kernels' order"""
    I, X = f_up.shape
    per = -(-X // nchunk)
    part = np.zeros((nchunk, 2, I))
    for chunk in range(nchunk):
        down, up = np.zeros(I), np.zeros(I)
        for x in range(chunk * per, min(X, chunk * per + per)):
            down = down + (f_dir[:, x] + f_down[:, x]) * dl[x]
            up = up + f_up[:, x] * dl[x]
        part[chunk, 0], part[chunk, 1] = down, up
    cper = (nchunk + 3) // 4
    seg = np.zeros((4, 2, I))
    for s in range(4):
        for chunk in range(s * cper, min(nchunk, s * cper + cper)):
            seg[s] = seg[s] + part[chunk]
    tot = ((seg[0] + seg[1]) + seg[2]) + seg[3]
    return tot[1], tot[0], tot[1] - tot[0]


def _check_totals(rt, c, col=0):
    X, I = c.nbin, c.nlayer + 1
    band = {k: rt.get(k, col).reshape(I, X) for k in ("F_up_band", "F_down_band", "F_dir_band")}
    if not c.dir_beam:
        assert not band["F_dir_band"].any()
    want = restated_totals(band["F_up_band"], band["F_down_band"], band["F_dir_band"], np.asarray(c.opac_deltawave, np.float64),
                           rt.totals_chunks())
    assert np.all(np.isfinite(want[0])) and np.any(want[0] != 0.0) and np.any(want[1] != 0.0)
    for k, w in zip(("F_up_tot", "F_down_tot", "F_net"), want):
        got = rt.get(k, col)
        bad = np.nonzero(got.view(np.uint64) != w.view(np.uint64))[0]
        print("%s: %d of %d interfaces differ" % (k, bad.size, I))
        assert np.array_equal(got, w) and bad.size == 0, (k, bad[:5], got[bad[:5]], w[bad[:5]])


# X = 97: one chunk; two chunks of 49 (a batch of loads one bin long behind 48); five chunks in segments of 2, 2, 1, 0; more
# chunks than bins.  X = 230: the chunking of the formula.  2 I = 6, 256 (one pass of the kernels' 256-wide loop) and 258
@pytest.mark.parametrize("nbin,nlayer,nchunk,beam", [(97, 2, 1, 0), (97, 127, 2, 0), (97, 128, 5, 1), (97, 2, 4096, 0),
                                                     (230, 2, None, 1), (230, 127, None, 0), (230, 128, None, 0)])
def test_wavelength_sum_in_the_kernels_order(ctx, nbin, nlayer, nchunk, beam):
    c = cases.make_case(nbin=nbin, nlayer=nlayer, ny=4, dir_beam=beam, albedo=0.2 if beam else 0.0)
    rt = _batch(ctx, c, nchunk)
    try:
        assert nchunk is None or rt.totals_chunks() == nchunk
        rt.step(0)
        _check_totals(rt, c)
    finally:
        rt.close()


def test_wavelength_sum_leaves_a_finished_column_alone(ctx):
    """two columns; column 1's loop has ended before the second iteration: its totals stay those of the first"""
    c = cases.make_case(nbin=97, nlayer=9, ny=4)
    rt = _batch(ctx, c, ncol=2)
    try:
        rt.set_temperatures(1, c.T_lay * 1.1)
        rt.step(0)
        for col in (0, 1):
            _check_totals(rt, c, col)
        kept = {k: rt.get(k, 1) for k in ("F_up_tot", "F_down_tot", "F_net", "F_up_band", "T_lay")}
        rt.set_state(1, "done", np.ones(1, np.int32))
        rt.step(1)
        assert int(rt.get("done", 1)[0]) == 1 and int(rt.get("done", 0)[0]) == 0
        _check_totals(rt, c, 0)
        for k, v in kept.items():
            assert rt.get(k, 1).tobytes() == v.tobytes(), k
    finally:
        rt.close()


# ---- node Planck values ---------------------------------------------------------------------------------------------------

def planck_lookup(grid, T, dim, step):
    """two_stream.h's planck_lookup for every bin: grid [dim + 1][X], T [n] -> [n][X]"""
    t = (np.asarray(T, np.float64) - 1.0) / float(step)
    t = np.maximum(0.001, np.minimum(dim - 1.001, t))
    td, tu = np.floor(t).astype(int), np.ceil(t).astype(int)
    blend = grid[td] * (tu - t)[:, None] + grid[tu] * (t - td)[:, None]
    return np.where((td != tu)[:, None], blend, grid[td]), td, tu


@pytest.mark.parametrize("nlayer", [2, 15])      # H + 3 = 7 and 33 nodes: inside one 32-wide tile, and one over
def test_node_planck_values_bit_for_bit(ctx, nlayer):
    """33 bins (one over a tile).  Temperatures exactly on a table row, below the first row and above the last"""
    X, L = 33, nlayer
    c = cases.make_case(nbin=X, nlayer=L, ny=4)
    dim, step = c.plancktable_dim, c.plancktable_step
    on_row, below, above = 1.0 + step * 50, 0.5, 1.0 + step * dim + 100.0
    c.T_lay[[0, 1, L] if L == 2 else [3, 7, 11]] = [on_row, below, above]
    rt = _batch(ctx, c)
    try:
        rt.refresh()
        T = rt.get("T_lay")
        assert T.tobytes() == np.asarray(c.T_lay, np.float64).tobytes()
        grid = rt.get("planck_grid").reshape(dim + 1, X)
        T_int = np.empty(L + 1)
        T_int[0] = T[0] - 0.5 * (T[1] - T[0])
        T_int[L] = T[L - 1] + 0.5 * (T[L - 1] - T[L - 2])
        T_int[1:L] = T[0:L - 1] + 0.5 * (T[1:L] - T[0:L - 1])
        assert rt.get("T_int").tobytes() == T_int.tobytes()
        lay, td, tu = planck_lookup(grid, T, dim, step)                 # layers 0 .. L-1 and the surface, T_lay[L]
        assert (td == tu).any() and (td == 0).any() and (tu == dim - 1).any() and (td != tu).any()
        got_lay = rt.get("planckband_lay").reshape(X, L + 2)
        assert np.all(np.isfinite(got_lay))
        assert got_lay[:, :L].T.tobytes() == lay[:L].tobytes(), "layer centres"
        assert got_lay[:, L + 1].tobytes() == lay[L].tobytes(), "surface"
        inter = planck_lookup(grid, T_int, dim, step)[0]
        got_int = rt.get("planckband_int").reshape(X, L + 1)
        assert got_int.T.tobytes() == inter.tobytes(), "interfaces"
    finally:
        rt.close()
