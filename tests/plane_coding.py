"""A numpy restatement of the fp32 coefficient planes' coding (csrc/plane_code.h and the fp32 store of
csrc/rt_coef_kernel.inc), written from the header's description and not from its code: the fp32 image the coefficient
kernel must store, given the fp64 planes the same kernel stores with `precision = double`."""
import numpy as np


def _nonneg(v):
    """v > 0 ? v : 0 -- negative values, -0.0 and NaN become +0.0"""
    v = np.asarray(v, np.float64)
    return np.where(v > 0.0, v, 0.0)


def code_alpha_beta(alpha, beta):
    """planes 0 and 1: the smaller of alpha and rest = (1 - alpha) - beta (both clamped to >= +0.0), alpha as +alpha and
    rest as -rest (ties go to alpha); beta, or -(1 - beta) when beta > 1/2.  Each value formed in fp64, rounded once."""
    alpha, beta = np.asarray(alpha, np.float64), np.asarray(beta, np.float64)
    a, rest = _nonneg(alpha), _nonneg((1.0 - alpha) - beta)
    with np.errstate(over="ignore"):                     # (beyond fp32's range: inf, as the C conversion gives)
        c0 = np.where(a <= rest, a.astype(np.float32), -rest.astype(np.float32))
        c1 = np.where(beta > 0.5, -_nonneg(1.0 - beta).astype(np.float32), _nonneg(beta).astype(np.float32))
    return c0.astype(np.float32), c1.astype(np.float32)


def encode_planes(p64, tiling):
    """the fp32 plane image of the fp64 one, both shaped (tiles, planes, ROWS, 64) as RTBatch.coef_planes returns them;
    `tiling` is RTBatch.flux_tiling(): which planes hold v' (has_vp, pl_vp) and the beam (pl_dd, pl_dd + 1)"""
    p64 = np.asarray(p64, np.float64)
    out = np.empty(p64.shape, np.float32)
    out[:, 0], out[:, 1] = code_alpha_beta(p64[:, 0], p64[:, 1])
    out[:, 2] = p64[:, 2].astype(np.float32)                          # u'
    beam_from = 3
    if tiling["has_vp"]:
        vp = tiling["pl_vp"]
        out[:, vp] = (p64[:, 2] + p64[:, vp]).astype(np.float32)      # u' + v', summed in fp64
        beam_from = tiling["pl_dd"]
    if p64.shape[1] > beam_from:                                      # dd, du
        out[:, beam_from:] = p64[:, beam_from:].astype(np.float32)
    return out


def decode_slot(tiling, flat_index, nbin=None):
    """(tile, plane, row, lane) of a flat plane-image index, with the (bin, Gauss point, half-layer) the slot holds --
    a finding's address for a message"""
    rows, nplane = tiling["ROWS"], tiling["nplane"]
    tile, rem = divmod(int(flat_index), nplane * rows * 64)
    plane, rem = divmod(rem, rows * 64)
    row, lane = divmod(rem, 64)
    NW, nparts, k, ypb, nxb = tiling["NW"], tiling["nparts"], tiling["k"], tiling["ypb"], tiling["nxb"]
    wv, part, bx = tile % NW, (tile // NW) % nparts, tile // (NW * nparts)
    s_local, j = (wv * 64 + lane) // k, lane % k
    xl, yl = divmod(s_local, ypb)
    x, y = bx * nxb + xl, part * ypb + yl
    where = "tile %d plane %d row %d lane %d: bin %d Gauss point %d half-layer %d" % (tile, plane, row, lane, x, y,
                                                                                     j * rows + row)
    if s_local >= nxb * ypb or (nbin is not None and x >= nbin):
        where += " (no spectral point: padding)"
    return where
