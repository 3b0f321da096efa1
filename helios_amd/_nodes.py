"""What the node tools share: lines.py, cia.py and exomol.py each take a list of (T, P) nodes and a grid numin ... numax at dnu, and
write the files `Out_<name>_<numin>_<numax>_<T>_<pcode>.bin` that ktable.py reads or, with `-ktable yes`, the species' k-table
from fp32 slabs that stay on the device.  Here is that frame, once: the grid, the file names and the node lists; the checks of
the nodes; the handle that runs nodes into slabs and the loop that gives it its nodes in turns; the slab source and the front
of ktable.build_table; the options, their refusals, and the two ends of a tool's main.  A tool keeps its reader, its contract
in numpy, its device object's setters, its own options and its report lines.

`tool` is the word before the colon of a message: "lines", "cia" or "exomol"."""
import contextlib
import ctypes
import os
import time

import numpy as np

from ._tool import DeviceObject

MAX_TABLE_POINTS = 1 << 28            # hx_ktable_create


# ---- the grid, the files and the node lists ------------------------------------------------------------------------------
def file_name(name, numin, numax, temp, code, ending=".bin"):
    return "Out_%s_%05d_%05d_%05d_%s%s" % (name, numin, numax, temp, code, ending)


def chunk_limits(tool, numin, numax, dnu, chunk_width=None):
    """[(numin, numax, points)] of the files"""
    if not (np.isfinite(dnu) and dnu > 0):
        raise IOError("%s: -dnu %r is not > 0" % (tool, dnu))
    if numax <= numin:
        raise IOError("%s: -numax %d is not above -numin %d" % (tool, numax, numin))
    width = numax - numin if chunk_width is None else int(chunk_width)
    if width <= 0:
        raise IOError("%s: -chunk_width %r is not > 0" % (tool, chunk_width))
    out = []
    for lo in range(numin, numax, width):
        hi = min(lo + width, numax)
        n = (hi - lo) / dnu
        if abs(n - round(n)) > 1e-9 * max(n, 1.0) or round(n) < 1:
            raise IOError("%s: dnu = %.17g does not divide the chunk %d ... %d cm^-1 into a whole number of points (%.17g)"
                          % (tool, dnu, lo, hi, n))
        out.append((lo, hi, int(round(n))))
    return out


def write_file(path, nu, kappa64, output_format):
    k32 = np.asarray(kappa64).astype(np.float32)
    if output_format == "binary":
        k32.astype("<f4").tofile(path)
    else:
        with open(path, "w") as f:
            for row in zip(nu, k32):
                f.write("%.12g %.9g\n" % row)


def parse_temperatures(tool, text):
    out = []
    for word in str(text).split():
        try:
            t = int(word)
        except ValueError:
            raise IOError("%s: the temperature %r is not an integer in K (the file name carries it)" % (tool, word))
        if t <= 0:
            raise IOError("%s: the temperature %r is not > 0 K" % (tool, word))
        out.append(t)
    if not out:
        raise IOError("%s: -temperatures holds no temperature" % tool)
    return out


def parse_pressure_codes(tool, text):
    from .ktable import pressure_table
    table = pressure_table()
    codes = str(text).split()
    for c in codes:
        if c not in table:
            raise IOError("%s: pressure code %r is not in the table (n800 ... p400)" % (tool, c))
    if not codes:
        raise IOError("%s: -pressure_codes holds no code" % tool)
    return codes, [table[c] for c in codes]


# ---- the checks of a library function --------------------------------------------------------------------------------------
def check_backend(tool, backend):
    if backend not in ("device", "numpy"):
        raise ValueError("%s: backend is device or numpy (got %r)" % (tool, backend))


def check_node_inputs(tool, temps, pressures, nu_grid, mass, kind="molar"):
    """(temperatures, pressures, (nu_first, dnu, points)) as fp64 arrays and numbers; `mass` is the `kind` mass in g/mol.  What
    else a tool checks of a call runs after this"""
    temps = np.asarray(temps, np.float64).reshape(-1)
    pressures = np.asarray(pressures, np.float64).reshape(-1)
    if len(temps) == 0 or not np.all(np.isfinite(temps) & (temps > 0)):
        raise ValueError("%s: every temperature is a finite number > 0 (got %r)" % (tool, temps.tolist()))
    if len(pressures) == 0 or not np.all(np.isfinite(pressures) & (pressures > 0)):
        raise ValueError("%s: every pressure is a finite number > 0 dyne cm^-2 (got %r)" % (tool, pressures.tolist()))
    nu_first, dnu, n_points = float(nu_grid[0]), float(nu_grid[1]), int(nu_grid[2])
    if not (np.isfinite(dnu) and dnu > 0):
        raise ValueError("%s: dnu = %r is not > 0" % (tool, dnu))
    if n_points < 1 or not np.isfinite(nu_first):
        raise ValueError("%s: the grid (nu_first, dnu, points) = %r needs a finite start and at least one point" % (tool, tuple(nu_grid)))
    if mass is None or not (np.isfinite(mass) and mass > 0):
        raise ValueError("%s: no %s mass (got %r): give one > 0 g/mol" % (tool, kind, mass))
    return temps, pressures, (nu_first, dnu, n_points)


# ---- device ------------------------------------------------------------------------------------------------------------
class NodeOpacity(DeviceObject):
    """a handle that runs up to nodes_per_launch of its n_nodes nodes per launch into fp32 slabs that stay on the device.  A
    class has set_nodes, and every setter begins with _reset_nodes"""

    def _reset_nodes(self):
        """what was set before does not outlive a setter that fails"""
        self.n_nodes = self.rows_run = 0

    def run_nodes(self, first, n):
        """queues nodes first ... first + n - 1 into slab rows 0 ... n - 1; returns at once"""
        self._call("run_nodes", int(first), int(n))
        self.rows_run = int(n)

    def slab_pointer(self):
        """device address of the fp32 slabs [nodes_per_launch][...], rows of the last run_nodes with the stride n_points"""
        p = ctypes.c_void_p()
        self._call("device_ptr", b"slabs32", ctypes.byref(p))
        return p


@contextlib.contextmanager
def opened(ctx, handle, make_handle):
    """the handle of a call: the one given, which stays open; else make_handle(ctx), closed at the end, on the context given or
    on one that is opened here and closed after it"""
    own_ctx = ctx is None and handle is None
    if own_ctx:
        from .device import Context
        ctx = Context(int(os.environ.get("HELIOS_DEVICE", "0")))
    try:
        made = make_handle(ctx) if handle is None else None
        try:
            yield handle if made is None else made
        finally:
            if made is not None:
                made.close()
    finally:
        if own_ctx:
            ctx.close()


def nodes_in_turns(ctx, handle, make_handle, nodes, set_nodes, collect):
    """runs the list `nodes` through the handle of opened(): set_nodes(handle, part) sets up to n_nodes_max of them, and after
    every launch collect(handle, rows) takes what the handle holds of the nodes `rows`, a slice of the list.  Returns timing_ms
    summed over the turns"""
    ms = np.zeros(2)
    with opened(ctx, handle, make_handle) as h:
        per = h.nodes_per_launch
        for lo in range(0, len(nodes), h.n_nodes_max):                       # a handle made for fewer nodes takes them in turns
            part = nodes[lo:lo + h.n_nodes_max]
            set_nodes(h, part)
            for first in range(0, len(part), per):
                n = min(per, len(part) - first)
                h.run_nodes(first, n)
                collect(h, slice(lo + first, lo + first + n))
            ms += h.get("timing_ms")
    return ms


# ---- from the nodes to the k-table -----------------------------------------------------------------------------------------
class NodeSlabs(object):
    """ktable.build_table's slabs from a tool's input: one chunk 0 ... numax of `n_points` points, the nodes sorted ascending and
    de-duplicated as ktable.SpeciesFiles does (node = p + np * t).  On the device the slabs never leave it; `ms` holds the kernel
    times once the table is built.  A class gives TOOL, host_slab(it, t, p), the fp64 row of the node of temps[it], and
    open_handle(ctx, per, nodes), which makes self.handle and then gives it the input and the nodes [(it, t, p)]"""

    TOOL = None
    KERNEL = "line kernel's"

    def __init__(self, temps, pressures, numax, dnu, n_points, nodes_per_launch):
        self.numax, self.dnu, self.n_points = int(numax), float(dnu), int(n_points)
        self.temps, self.press = sorted(set(temps)), sorted(set(pressures))
        self.nodes_per_launch = max(1, int(nodes_per_launch))
        self.handle, self.ms = None, np.zeros(2)

    def axis(self):
        return 0, self.numax, self.numax / self.n_points           # ktable.SpeciesFiles.resolution() of the file not written

    def _check(self, n_points):
        if n_points != self.n_points:
            raise IOError("%s: the k-table's axis 0 ... %d cm^-1 at %.17g cm^-1 has %d points, the %s grid at -dnu %.17g has %d"
                          % (self.TOOL, self.numax, self.numax / self.n_points, n_points, self.KERNEL, self.dnu, self.n_points))

    def host_slabs(self, pool, n_points):
        self._check(n_points)
        for it, t in enumerate(self.temps):
            for p in self.press:
                yield self.host_slab(it, float(t), p).astype(np.float32)

    def feed(self, b, pool, n_points):
        self._check(n_points)
        nodes = [(it, float(t), p) for it, t in enumerate(self.temps) for p in self.press]
        per = min(self.nodes_per_launch, b.max_tp)
        self.open_handle(b.ctx, per, nodes)
        h = self.handle
        slabs = h.slab_pointer()
        for first in range(0, len(nodes), per):
            n = min(per, len(nodes) - first)
            h.run_nodes(first, n)
            b.run_device(slabs, n, first)
            self.after_launch(h)

    def after_launch(self, h):
        """what a tool reads of a launch, after the launch's sort is queued"""

    def close(self):
        h, self.handle = self.handle, None
        if h is not None:
            try:
                self.ms = h.get("timing_ms")
            finally:
                h.close()


def node_ktable(tool, backend, temps, pressure_codes, numax, dnu, check, make_source, inter, n_gauss, target, ctx, lds_points, timing,
                grid_tool=None):
    """the front of a tool's k-table function: (what ktable.build_table returns, the source).  `temps`: integers in K;
    `pressure_codes`: keys of ktable.pressure_table(); the range is 0 ... numax in one chunk.  check(temps, pressures, nu_grid)
    is the tool's check of a call's nodes; make_source(temps, pressures, n_points) its NodeSlabs.  `grid_tool`: the word of
    chunk_limits' refusals where it is not the tool's"""
    from . import ktable
    check_backend(tool, backend)
    table = ktable.pressure_table()
    for c in pressure_codes:
        if c not in table:
            raise IOError("%s: pressure code %r is not in the table (n800 ... p400)" % (tool, c))
    for t in temps:
        if int(t) != t:
            raise IOError("%s: the temperature %r is not an integer in K" % (tool, t))
    temps, pressures = [int(t) for t in temps], [table[c] for c in pressure_codes]
    n_points = chunk_limits(grid_tool or tool, 0, int(numax), dnu)[0][2]
    check(temps, pressures, (0.0, dnu, n_points))
    if n_points > MAX_TABLE_POINTS:
        raise IOError("%s: %d spectral points, the k-table's kernel takes 1 ... %d" % (tool, n_points, MAX_TABLE_POINTS))
    source = make_source(temps, pressures, n_points)
    out = ktable.build_table(source, inter, n_gauss, "hip" if backend == "device" else "numpy", ctx, source.nodes_per_launch,
                             ktable.LDS_POINTS if lds_points is None else lds_points, target, timing)
    return out, source


# ---- the tool ----------------------------------------------------------------------------------------------------------
def add_node_options(p):
    """the nodes, the grid and the files"""
    p.add_argument("-temperatures", required=True, help="integers in K, separated by blanks")
    p.add_argument("-pressure_codes", required=True, help="HELIOS-K's codes, n800 ... p400, separated by blanks")
    p.add_argument("-numin", type=int, default=0)
    p.add_argument("-numax", type=int, required=True)
    p.add_argument("-dnu", type=float, required=True)
    p.add_argument("-output_directory", default=None, help="of the files; required without -ktable yes")
    p.add_argument("-chunk_width", type=int, default=None)
    p.add_argument("-output_format", default="binary", choices=("binary", "text"))
    p.add_argument("-backend", default="device", choices=("device", "numpy"))


def add_ktable_options(p):
    p.add_argument("-ktable", default="no", choices=("yes", "no"),
                   help="the species' k-table in place of the files; the options below are ktable.py's")
    p.add_argument("-grid_format", default="fixed_resolution")
    p.add_argument("-wavelength_grid", default="50 0.34 200")
    p.add_argument("-path_to_grid_file", default=None)
    p.add_argument("-number_of_gaussian_points", type=int, default=20)
    p.add_argument("-directory_with_individual_files", default="./output/")
    p.add_argument("-interpolate", default="yes", choices=("yes", "no"))
    p.add_argument("-temperature_grid", default=None)
    p.add_argument("-pressure_grid", default=None)
    p.add_argument("-container", default="h5", choices=("h5", "npz"))
    p.add_argument("-nodes_per_launch", type=int, default=4)


def parse_node_args(p, argv):
    opt = p.parse_args(argv)
    if opt.ktable == "no" and opt.output_directory is None:
        p.error("the following arguments are required: -output_directory")
    return opt


def refuse_with_ktable(tool, opt):
    if opt.numin != 0:
        raise IOError("%s: -ktable yes with -numin %d: the k-table's wavelength axis starts at 0 cm^-1, and ktable.py refuses a "
                      "directory whose first chunk does not" % (tool, opt.numin))
    if opt.chunk_width is not None:
        raise IOError("%s: -ktable yes with -chunk_width %d: the table is built from the one chunk 0 ... numax; a chunk's points "
                      "are lo + i dnu, which are other bits than 0 + i dnu" % (tool, opt.chunk_width))
    if opt.output_format != "binary":
        raise IOError("%s: -ktable yes with -output_format %s: no opacity file is written, the fp32 opacities stay on the device"
                      % (tool, opt.output_format))
    if opt.output_directory is not None:
        raise IOError("%s: -ktable yes with -output_directory %s: a call writes the files or the table, not both; the table goes "
                      "to -directory_with_individual_files" % (tool, opt.output_directory))
    if opt.number_of_gaussian_points < 1:
        raise IOError("%s: -number_of_gaussian_points is an integer >= 1" % tool)
    if opt.nodes_per_launch < 1:
        raise IOError("%s: -nodes_per_launch is an integer >= 1" % tool)


def mass_of(tool, name, given, kind="molar"):
    """the `kind` mass in g/mol: the one given with -<kind>_mass, else the weight of `name` in species_data.py"""
    mass = given
    if mass is None:
        from .species_data import species_lib
        if name not in species_lib:
            raise IOError("%s: no %s mass: %r is not in species_data.py, give -%s_mass" % (tool, kind, name, kind))
        mass = species_lib[name].weight
    if not (np.isfinite(mass) and mass > 0):
        raise IOError("%s: no %s mass: -%s_mass %r is not > 0 g/mol" % (tool, kind, kind, mass))
    return mass


def _how(opt, timing, kernels, pairs):
    """the middle of a summary line: the pairs where the tool counts them, and the kernels' times or `numpy`"""
    return ("%d pairs, " % timing["pairs"] if pairs else "") + ("numpy" if opt.backend == "numpy" else kernels(timing))


def main_ktable(tool, opt, build, kernels, t0, pairs=False):
    """-ktable yes: `<name>_opac_kdistr` and, with -interpolate yes, `<name>_opac_ip_kdistr`.  build(inter, target, timing) is
    the tool's k-table function; kernels(timing) names the device's times in the summary line"""
    from . import ktable
    inter = ktable.wavelength_grid(opt.grid_format, opt.wavelength_grid.split(), opt.path_to_grid_file)
    target = ktable.target_grid(opt.temperature_grid, opt.pressure_grid) if opt.interpolate == "yes" else None
    timing = {}
    native, ip = build(inter, target, timing)
    stem = os.path.join(opt.directory_with_individual_files, opt.name)
    written = [ktable.write_table("%s_opac_kdistr.%s" % (stem, opt.container), native)]
    if ip is not None:
        written.append(ktable.write_table("%s_opac_ip_kdistr.%s" % (stem, opt.container), ip))
    print("%s: %d nodes of %d points into %d bins x %d Gauss points, %s, %.2f s -> %s" % (
        tool, timing["points"], chunk_limits(tool, 0, opt.numax, opt.dnu)[0][2], len(inter) - 1, opt.number_of_gaussian_points,
        _how(opt, timing, kernels, pairs), time.time() - t0, ", ".join(written)))
    return written


def main_files(tool, opt, chunks, temps, codes, make_handle, opacity, kernels, t0, pairs=False):
    """the files of every (chunk, T, P).  make_handle(ctx, n_points_max) is the handle of the device backend, which holds the
    tool's input; opacity(nu_grid, ctx, handle, timing) the tool's library function, kappa [T][P][nu]"""
    if opt.numin != 0:
        print("%s: -numin %d is not 0: ktable.py will refuse the directory" % (tool, opt.numin))
    directory = os.path.join(str(opt.output_directory), "")
    os.makedirs(directory, exist_ok=True)
    ending = ".bin" if opt.output_format == "binary" else ".dat"
    timing, written = {}, []
    on_device = opened(None, None, lambda ctx: make_handle(ctx, max(c[2] for c in chunks))) if opt.backend == "device" else None
    with on_device or contextlib.nullcontext() as handle:            # one context and one handle for every chunk
        for lo, hi, n in chunks:
            kappa = opacity((float(lo), opt.dnu, n), handle.ctx if handle is not None else None, handle, timing)
            nu = float(lo) + np.arange(n, dtype=np.float64) * opt.dnu
            for it, t in enumerate(temps):
                for jp, code in enumerate(codes):
                    written.append(directory + file_name(opt.name, lo, hi, t, code, ending))
                    write_file(written[-1], nu, kappa[it, jp], opt.output_format)
    print("%s: %d nodes x %d chunks, %s, %.2f s -> %d files in %s" % (
        tool, len(temps) * len(codes), len(chunks), _how(opt, timing, kernels, pairs), time.time() - t0, len(written), directory))
    return written
