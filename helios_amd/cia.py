"""Collision-induced absorption of one pair from a HITRAN CIA file, on the device (include/helios_hip.h section 12, csrc/cia.hip).

The species loop and ktable_mix.py take `CIA_<pair>_opac_ip_kdistr` as they take a line absorber's container.  This tool makes
it: the files `Out_<name>_<numin>_<numax>_<T>_<pcode>.bin` that `ktable.py` reads, or with `-ktable yes` the containers
themselves, without the files.

The input.  A header line in fixed columns (0-based, end exclusive): symbol 0:20, numin 20:30, numax 30:40 [cm^-1], number of
points 40:47, temperature 47:54 [K]; the rest of the header is ignored.  That many data lines follow, each split on blanks, the
first two numbers nu [cm^-1] and k [cm^5 molecule^-2].  A block is one header with its data; blocks whose header numin and numax
are the same doubles form a band; inside a band the blocks are ordered by T, and the bands by numin.  A negative k counts as 0.
Refused, with the line number or the value: a header shorter than 54 characters, a field that is not a finite number, fewer data
lines than announced, a block of fewer than 2 points, nu that does not strictly ascend, two blocks of one band at the same T,
more than one symbol in the file; selected bands that overlap or touch (numax_a >= numin_b): choose with `-bands`.

The contract.  All arithmetic is fp64 and nothing is contracted; K_B and N_A are phys_const's; every statement left to right.
A block's value at nu is 0 for nu < nu_b[0] or nu > nu_b[n-1]; otherwise, with i the last index with nu_b[i] <= nu, at most n - 2,
    d = nu_b[i+1] - nu_b[i],    u = (nu - nu_b[i]) / d,    u' = (nu_b[i+1] - nu) / d,    v = u' * k[i] + u * k[i+1].
Both weights come from differences: the tables fall by orders of magnitude from point to point and hold zeros, and neither
`1 - u` nor `k_i + u (k_{i+1} - k_i)` keeps every digit there.  A band at T, its blocks at T_0 < ... < T_{m-1}: block 0's value
for T <= T_0, block m-1's for T >= T_{m-1} (constant extrapolation); otherwise with j the last index with T_j <= T
    D = T_{j+1} - T_j,    w = (T - T_j) / D,    w' = (T_{j+1} - T) / D,    sigma = w' * v_j + w * v_{j+1}.
sigma(nu, T) is the value of the one band with numin <= nu <= numax and 0 outside every band, and
    kappa = sigma * (P / (K_B * T)) * N_A / M_partner    [cm^2 per gram of the second partner],
rounded once to fp32 when written, at nu_i = nu_first + i * dnu.  It is the quantity that `x_a x_b w_partner / mu` of the species
loop and of ktable_mix.py turns into the mixture's opacity; M_partner is by default the weight of `-name` in species_data.py.

Not modelled: no far wing and no temperature dependence beyond the constant extrapolation, no dimer features beyond what the
file holds, one file per call.

`backend="device"`: k_cia_nodes takes the node as a grid dimension and gives a workgroup a tile of TILE_POINTS consecutive
points.  The workgroup finds on the tile's first and last nu the index windows of the node's two blocks; windows of up to WINDOW
entries each are staged through LDS and searched there, larger ones and tiles that meet several bands are searched in global
memory by the same statements, a tile outside every band stores zeros.  `backend="numpy"` computes the same contract on the CPU,
and the device equals it bit for bit, in the fp64 rows and in the fp32 slabs.

`-ktable yes`: as `lines.py -ktable yes`.  The fp32 slabs stay on the device, where k_ktable_bins (ktable.KTableBuilder.run_device)
sorts them on the same stream.  The containers are the ones `cia.py` followed by `ktable.py` writes, to the bit: one chunk
0 ... numax, the nodes sorted ascending and de-duplicated (node = p + np t), the kernel's step the `-dnu` given and the k-table's
axis numax / points.  Refused with `-ktable yes`: `-numin` other than 0, `-chunk_width`, `-output_format text`, `-output_directory`.

The frame around the reader and the contract is _nodes.py's, shared with lines.py and exomol.py.
"""
import argparse
import time

import numpy as np

from . import _nodes
from . import phys_const as pc
from ._tool import dp, ip

HEADER_MIN = 54
_HEADER = (("numin", 20, 30), ("numax", 30, 40), ("points", 40, 47), ("temperature", 47, 54))
# csrc/cia.hip: CIA_THREADS, CIA_PPT, CIA_WINDOW (tests/test_gpu_cia.py derives its sizes from these)
THREADS = 256
POINTS_PER_THREAD = 4
TILE_POINTS = THREADS * POINTS_PER_THREAD
WINDOW = 256
GRID_TOOL = "lines"                   # the refusals of the grid and of the node lists came from lines.py with its word, and keep it


# ---- the input -----------------------------------------------------------------------------------------------------------
class Block(object):
    """one header with its data: nu strictly ascending, k >= 0"""
    __slots__ = ("symbol", "numin", "numax", "temp", "nu", "k", "line")

    def __init__(self, numin, numax, temp, nu, k, symbol="", line=0):
        self.symbol, self.numin, self.numax, self.temp, self.line = symbol, float(numin), float(numax), float(temp), line
        self.nu, self.k = np.ascontiguousarray(nu, np.float64).reshape(-1), np.ascontiguousarray(k, np.float64).reshape(-1)


class Band(object):
    """the blocks of one spectral range, ordered by T"""
    __slots__ = ("numin", "numax", "blocks")

    def __init__(self, numin, numax, blocks):
        self.numin, self.numax, self.blocks = numin, numax, blocks

    def temps(self):
        return np.array([b.temp for b in self.blocks])

    def describe(self, index):
        t = self.temps()
        pts = sorted(set(len(b.nu) for b in self.blocks))
        return "band %d: %.17g ... %.17g cm^-1, %d temperatures %.17g ... %.17g K, %s points" % (
            index, self.numin, self.numax, len(t), t[0], t[-1], "%d" % pts[0] if len(pts) == 1 else "%d ... %d" % (pts[0], pts[-1]))


def _header_number(text, where, name, lo, hi):
    try:
        v = float(text[lo:hi])
    except ValueError:
        v = np.nan
    if not np.isfinite(v):
        raise IOError("cia: %s: %s = %r (columns %d:%d) is not a finite number" % (where, name, text[lo:hi], lo, hi))
    return v


def read_cia_file(path):
    """(blocks in the order of the file, negative values set to 0) of a HITRAN `.cia` file"""
    blocks, negatives, symbols = [], 0, []
    with open(path) as f:
        rows = [r.rstrip("\r\n") for r in f]
    nr = 0
    while nr < len(rows):
        head = rows[nr]
        nr += 1
        if not head.strip():
            continue
        where = "line %d of %s (%r)" % (nr, path, head[:HEADER_MIN])
        if len(head) < HEADER_MIN:
            raise IOError("cia: %s holds %d characters, a header needs %d" % (where, len(head), HEADER_MIN))
        v = dict((name, _header_number(head, where, name, lo, hi)) for name, lo, hi in _HEADER)
        n = int(v["points"])
        if n != v["points"] or n < 2:
            raise IOError("cia: %s: a block of %.17g points; a block has a whole number of at least 2" % (where, v["points"]))
        symbol = head[0:20].strip()
        if symbol not in symbols:
            symbols.append(symbol)
        if len(symbols) > 1:
            raise IOError("cia: %s: the file holds more than one symbol (%r and %r); one pair per call" % (where, symbols[0], symbol))
        nu, k = _data_lines(rows[nr:nr + n])
        if nu is None or len(nu) != n:
            _refuse_data_lines(rows, nr, n, where, path)
        nr += n
        negatives += int(np.count_nonzero(k < 0))
        blocks.append(Block(v["numin"], v["numax"], v["temperature"], nu, np.where(k < 0, 0.0, k), symbol, nr - n))
    if not blocks:
        raise IOError("cia: %s holds no block" % path)
    return blocks, negatives


def _data_lines(lines):
    """(nu, k) of data lines that are all sound -- two finite numbers first, nu strictly ascending -- else (None, None)"""
    try:
        pairs = np.array([r.split()[:2] for r in lines], dtype=np.float64)
    except ValueError:
        return None, None
    if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.all(np.isfinite(pairs)) or np.any(np.diff(pairs[:, 0]) <= 0):
        return None, None
    return np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])


def _refuse_data_lines(rows, nr, n, where, path):
    """the data lines of a block that _data_lines did not take, one by one, up to the one to name"""
    last = None
    for j in range(n):
        if nr >= len(rows) or not rows[nr].strip():
            raise IOError("cia: %s announces %d data lines, %d follow (line %d)" % (where, n, j, nr + 1))
        col = rows[nr].split()
        nr += 1
        try:
            pair = [float(c) for c in col[:2]]
        except ValueError:
            pair = []
        if len(pair) < 2 or not np.all(np.isfinite(pair)):
            raise IOError("cia: %s announces %d data lines, %d follow: line %d (%r) does not hold the finite numbers nu and k"
                          % (where, n, j, nr, rows[nr - 1][:HEADER_MIN]))
        if j and not pair[0] > last:
            raise IOError("cia: line %d of %s: nu = %.17g does not lie above %.17g: nu strictly ascends" % (nr, path, pair[0], last))
        last = pair[0]
    raise IOError("cia: %s: the %d data lines cannot be read" % (where, n))


def group_bands(blocks):
    """the bands of `blocks`, ordered by numin; a band's blocks by T"""
    by_range = {}
    for b in blocks:
        check_block(b)
        by_range.setdefault((b.numin, b.numax), []).append(b)
    bands = []
    for (numin, numax), group in sorted(by_range.items()):
        group = sorted(group, key=lambda b: b.temp)
        for a, b in zip(group[:-1], group[1:]):
            if a.temp == b.temp:
                raise IOError("cia: the band %.17g ... %.17g cm^-1 holds two blocks at T = %.17g K (headers in lines %d and %d)"
                              % (numin, numax, a.temp, a.line, b.line))
        bands.append(Band(numin, numax, group))
    return bands


def check_block(b):
    if len(b.nu) < 2 or len(b.nu) != len(b.k):
        raise IOError("cia: a block of %d values of nu and %d of k; a block has at least 2 points" % (len(b.nu), len(b.k)))
    if not (np.all(np.isfinite(b.nu)) and np.all(np.isfinite(b.k)) and np.all(b.k >= 0)):
        raise IOError("cia: the block at T = %.17g K holds a value that is not a finite number, or k < 0" % b.temp)
    if np.any(np.diff(b.nu) <= 0):
        j = int(np.argmax(np.diff(b.nu) <= 0)) + 1
        raise IOError("cia: the block at T = %.17g K: nu = %.17g does not lie above %.17g: nu strictly ascends" % (b.temp, b.nu[j],
                                                                                                                  b.nu[j - 1]))
    if not (np.isfinite(b.temp) and b.temp > 0 and np.isfinite(b.numin) and np.isfinite(b.numax) and b.numax >= b.numin):
        raise IOError("cia: a block at T = %r K over %r ... %r cm^-1" % (b.temp, b.numin, b.numax))


def select_bands(bands, indices=None):
    """the bands chosen by their index in the list, in ascending order; refuses bands that overlap or touch"""
    if indices is not None:
        for i in indices:
            if not 0 <= i < len(bands):
                raise IOError("cia: -bands %d: the file holds the bands 0 ... %d" % (i, len(bands) - 1))
        chosen = sorted(set(indices))
    else:
        chosen = list(range(len(bands)))
    if not chosen:
        raise IOError("cia: -bands holds no index")
    for a, b in zip(chosen[:-1], chosen[1:]):
        if bands[a].numax >= bands[b].numin:
            raise IOError("cia: band %d (%.17g ... %.17g cm^-1) and band %d (%.17g ... %.17g cm^-1) overlap or touch: choose the bands "
                          "to take with -bands" % (a, bands[a].numin, bands[a].numax, b, bands[b].numin, bands[b].numax))
    return [bands[i] for i in chosen]


def bands_of(blocks):
    """the non-overlapping bands of a list of blocks (the library functions' `blocks`)"""
    return select_bands(group_bands(blocks))


def outside_counts(bands, temps):
    """per band how many of `temps` lie below its first or above its last temperature"""
    temps = np.asarray(temps, np.float64)
    return [int(np.count_nonzero((temps < b.blocks[0].temp) | (temps > b.blocks[-1].temp))) for b in bands]


def pack(bands):
    """the arrays hx_cia_set_blocks takes: block_off, nu, k, block_temp, band_first, band_numin, band_numax"""
    blocks = [b for band in bands for b in band.blocks]
    off = np.concatenate(([0], np.cumsum([len(b.nu) for b in blocks]))).astype(np.int32)
    first = np.concatenate(([0], np.cumsum([len(band.blocks) for band in bands]))).astype(np.int32)
    return (off, np.concatenate([b.nu for b in blocks]), np.concatenate([b.k for b in blocks]), np.array([b.temp for b in blocks]),
            first, np.array([band.numin for band in bands]), np.array([band.numax for band in bands]))


# ---- the contract in numpy ---------------------------------------------------------------------------------------------
def block_value(block, nu):
    """the block's value at the points nu"""
    a, k = block.nu, block.k
    n = len(a)
    i = np.clip(np.searchsorted(a, nu, side="right") - 1, 0, n - 2)
    d = a[i + 1] - a[i]
    u, up = (nu - a[i]) / d, (a[i + 1] - nu) / d
    v = up * k[i] + u * k[i + 1]
    return np.where((nu >= a[0]) & (nu <= a[n - 1]), v, 0.0)


def band_value(band, nu, temp):
    """the band's value at the points nu and the temperature temp"""
    t = band.temps()
    m = len(t)
    if temp <= t[0]:
        return block_value(band.blocks[0], nu)
    if temp >= t[m - 1]:
        return block_value(band.blocks[m - 1], nu)
    j = int(np.searchsorted(t, temp, side="right")) - 1
    big_d = t[j + 1] - t[j]
    w, wp = (temp - t[j]) / big_d, (t[j + 1] - temp) / big_d
    return wp * block_value(band.blocks[j], nu) + w * block_value(band.blocks[j + 1], nu)


def numpy_sigma(bands, temp, nu):
    """sigma [cm^5 molecule^-2] at the points nu"""
    sigma = np.zeros(len(nu))
    for band in bands:
        inside = (nu >= band.numin) & (nu <= band.numax)
        if inside.any():
            sigma[inside] = band_value(band, nu[inside], float(temp))
    return sigma


def numpy_node(bands, temp, press, nu_first, dnu, n_points, partner_mass, sigma=None):
    """kappa64 [n_points] of one node; `sigma`: numpy_sigma of the node's temperature on this grid, where the caller kept it"""
    if sigma is None:
        sigma = numpy_sigma(bands, temp, nu_first + np.arange(n_points, dtype=np.float64) * dnu)
    return sigma * (press / (pc.K_B * temp)) * pc.N_A / partner_mass


# ---- device ------------------------------------------------------------------------------------------------------------
class CiaOpacity(_nodes.NodeOpacity):
    """hx_cia: the resident blocks of the selected bands, nodes of up to n_points_max spectral points, nodes_per_launch per
    launch into fp32 slabs that stay on the device; `with_fp64`: the rows before rounding as well"""

    PREFIX = "hx_cia"

    def __init__(self, ctx, bands, n_points_max, nodes_per_launch, n_nodes_max, with_fp64=False):
        arr = pack(bands)
        self.n_points_max, self.nodes_per_launch, self.n_nodes_max = int(n_points_max), int(nodes_per_launch), int(n_nodes_max)
        self.with_fp64 = bool(with_fp64)
        self.n_nodes = self.n_points = self.rows_run = 0
        self._create(ctx, len(arr[1]), len(arr[3]), self.n_points_max, self.nodes_per_launch, self.n_nodes_max, int(self.with_fp64))
        try:
            self.set_blocks(*arr)
        except Exception:
            self.close()
            raise

    def set_blocks(self, block_off, nu, k, block_temp, band_first, band_numin, band_numax):
        off, first = np.ascontiguousarray(block_off, np.int32), np.ascontiguousarray(band_first, np.int32)
        a = [np.ascontiguousarray(v, np.float64).reshape(-1) for v in (nu, k, block_temp, band_numin, band_numax)]
        assert len(a[0]) == len(a[1]) and len(off) == len(a[2]) + 1 and len(first) == len(a[3]) + 1 == len(a[4]) + 1
        self._reset_nodes()
        self._call("set_blocks", len(a[2]), ip(off), dp(a[0]), dp(a[1]), dp(a[2]), len(a[3]), ip(first), dp(a[3]), dp(a[4]))

    def set_nodes(self, temps, pressures, partner_mass, nu_first, dnu, n_points):
        """T and P per node and what the nodes share"""
        arr = [np.ascontiguousarray(a, np.float64).reshape(-1) for a in (temps, pressures)]
        assert len(arr[0]) == len(arr[1])
        self._reset_nodes()
        self._call("set_nodes", len(arr[0]), dp(arr[0]), dp(arr[1]), float(partner_mass), float(nu_first), float(dnu), int(n_points))
        self.n_nodes, self.n_points = len(arr[0]), int(n_points)

    def _results(self):
        return {"slabs32": ((self.rows_run, self.n_points), np.float32), "kappa64": (self.rows_run, self.n_points), "timing_ms": 2}


# ---- the library functions -----------------------------------------------------------------------------------------------
def _check_node_inputs(temps, pressures, nu_grid, partner_mass):
    return _nodes.check_node_inputs("cia", temps, pressures, nu_grid, partner_mass, "partner")


def cia_opacity(blocks, temps, pressures_cgs, nu_grid, partner_mass, backend="device", ctx=None, nodes_per_launch=4, handle=None,
                timing=None):
    """kappa [T][P][nu] in cm^2 per gram of the partner, fp64.  `blocks`: the Blocks of the bands to take; `nu_grid`: (nu of point
    0, dnu, points); `handle`: a CiaOpacity with fp64 rows that already holds the blocks.  `timing` receives nodes_ms, summed"""
    _nodes.check_backend("cia", backend)
    temps, pressures, (nu_first, dnu, n_points) = _check_node_inputs(temps, pressures_cgs, nu_grid, partner_mass)
    bands = bands_of(blocks) if handle is None or backend == "numpy" else None
    out = np.empty((len(temps), len(pressures), n_points))
    ms = 0.0
    if backend == "numpy":
        nu = nu_first + np.arange(n_points, dtype=np.float64) * dnu
        for it, t in enumerate(temps):
            sigma = numpy_sigma(bands, t, nu)
            for jp, p in enumerate(pressures):
                out[it, jp] = numpy_node(bands, t, p, nu_first, dnu, n_points, partner_mass, sigma)
    else:
        nodes = [(t, p) for t in temps for p in pressures]
        flat = out.reshape(len(nodes), n_points)

        def collect(h, rows):
            flat[rows] = h.get("kappa64")
        ms = float(_nodes.nodes_in_turns(
            ctx, handle, lambda c: CiaOpacity(c, bands, n_points, max(1, min(int(nodes_per_launch), len(nodes))), len(nodes), True), nodes,
            lambda h, part: h.set_nodes([n[0] for n in part], [n[1] for n in part], partner_mass, nu_first, dnu, n_points), collect)[0])
    if timing is not None:
        timing["nodes_ms"] = timing.get("nodes_ms", 0.0) + ms
    return out


# ---- from the file to the k-table ------------------------------------------------------------------------------------------
class CiaSlabs(_nodes.NodeSlabs):
    """ktable.build_table's slabs from the blocks of a CIA file (_nodes.NodeSlabs); `ms` holds the kernel's time once the table is
    built"""

    TOOL, KERNEL = "cia", "kernel's"

    def __init__(self, bands, temps, pressures, numax, dnu, n_points, partner_mass, nodes_per_launch=4):
        _nodes.NodeSlabs.__init__(self, temps, pressures, numax, dnu, n_points, nodes_per_launch)
        self.bands, self.partner_mass = bands, partner_mass
        self._sigma = (None, None)                                   # (it, numpy_sigma of temps[it]): the pressures of a T share it

    def host_slab(self, it, t, p):
        if self._sigma[0] != it:
            self._sigma = (it, numpy_sigma(self.bands, t, 0.0 + np.arange(self.n_points, dtype=np.float64) * self.dnu))
        return numpy_node(self.bands, t, p, 0.0, self.dnu, self.n_points, self.partner_mass, self._sigma[1])

    def open_handle(self, ctx, per, nodes):
        self.handle = h = CiaOpacity(ctx, self.bands, self.n_points, per, len(nodes))
        h.set_nodes([n[1] for n in nodes], [n[2] for n in nodes], self.partner_mass, 0.0, self.dnu, self.n_points)


def cia_ktable(blocks, temps, pressure_codes, numax, dnu, inter, n_gauss, partner_mass, target=None, backend="device", ctx=None,
               nodes_per_launch=4, lds_points=None, timing=None):
    """the data sets of `<name>_opac_kdistr` and, with `target` = (temperatures, pressures), of `<name>_opac_ip_kdistr`, as
    ktable.build_species returns them for the directory cia.py would write for the same arguments -- to the bit -- without the
    files.  `temps`: integers in K; `pressure_codes`: keys of ktable.pressure_table(); the range is 0 ... numax in one chunk.
    `timing` receives nodes_ms and build_table's entries"""
    out, source = _nodes.node_ktable(
        "cia", backend, temps, pressure_codes, numax, dnu, lambda t, p, nu_grid: _check_node_inputs(t, p, nu_grid, partner_mass),
        lambda t, p, n_points: CiaSlabs(bands_of(blocks), t, p, numax, dnu, n_points, partner_mass, nodes_per_launch),
        inter, n_gauss, target, ctx, lds_points, timing, GRID_TOOL)
    if timing is not None:
        timing["nodes_ms"] = float(source.ms[0])
    return out


# ---- the tool ----------------------------------------------------------------------------------------------------------
def parse_args(argv=None):
    p = argparse.ArgumentParser(prog="cia.py", description="collision-induced absorption of a pair from a HITRAN CIA file")
    p.add_argument("-name", required=True, help="of the species, as in species_data.py: CIA_H2H2, CIA_H2He, ...")
    p.add_argument("-cia_file", required=True)
    _nodes.add_node_options(p)
    p.add_argument("-partner_mass", type=float, default=None, help="g/mol; by default the weight of -name in species_data.py")
    p.add_argument("-bands", default=None, help="indices in the printed list of the bands to take, separated by blanks")
    _nodes.add_ktable_options(p)
    return _nodes.parse_node_args(p, argv)


def parse_bands(text):
    if text is None:
        return None
    try:
        return [int(w) for w in str(text).split()]
    except ValueError:
        raise IOError("cia: -bands %r: indices in the printed list, separated by blanks" % (text,))


def main(argv=None):
    """cia.py: the directory of one pair, or with -ktable yes its k-table; returns the paths written"""
    opt = parse_args(argv)
    t0 = time.time()
    temps = _nodes.parse_temperatures(GRID_TOOL, opt.temperatures)
    codes, pressures = _nodes.parse_pressure_codes(GRID_TOOL, opt.pressure_codes)
    if opt.ktable == "yes":
        _nodes.refuse_with_ktable("cia", opt)
    chunks = _nodes.chunk_limits(GRID_TOOL, opt.numin, opt.numax, opt.dnu, opt.chunk_width)
    partner_mass = _nodes.mass_of("cia", opt.name, opt.partner_mass, "partner")
    wanted = parse_bands(opt.bands)
    blocks, negatives = read_cia_file(opt.cia_file)
    listed = group_bands(blocks)
    print("cia: %s of %s: %d blocks in %d bands, %d negative values taken as 0" % (blocks[0].symbol, opt.cia_file, len(blocks),
                                                                                   len(listed), negatives))
    for i, band in enumerate(listed):
        print("cia:   " + band.describe(i))
    bands = select_bands(listed, wanted)
    for band, n in zip(bands, outside_counts(bands, temps)):
        if n:
            print("cia: %d of the %d node temperatures lie outside %.17g ... %.17g K of band %d: the band is constant in T there"
                  % (n, len(temps), band.blocks[0].temp, band.blocks[-1].temp, listed.index(band)))
    kept = [b for band in bands for b in band.blocks]
    if opt.ktable == "yes":
        return _nodes.main_ktable(
            "cia", opt,
            lambda inter, target, timing: cia_ktable(kept, temps, codes, opt.numax, opt.dnu, inter, opt.number_of_gaussian_points,
                                                     partner_mass, target, opt.backend, None, opt.nodes_per_launch, None, timing),
            lambda timing: "k_cia_nodes %.1f ms, k_ktable_bins %.1f ms" % (timing["nodes_ms"], timing["device_ms"][0]), t0)
    n_nodes = len(temps) * len(codes)
    return _nodes.main_files(
        "cia", opt, chunks, temps, codes,
        lambda ctx, n_points_max: CiaOpacity(ctx, bands, n_points_max, max(1, min(opt.nodes_per_launch, n_nodes)), n_nodes, True),
        lambda nu_grid, ctx, handle, timing: cia_opacity(kept, temps, pressures, nu_grid, partner_mass, opt.backend, ctx,
                                                         opt.nodes_per_launch, handle, timing),
        lambda timing: "k_cia_nodes %.1f ms" % timing["nodes_ms"], t0)
