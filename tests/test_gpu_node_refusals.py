"""The refusals that hx_lines, hx_cia and hx_exomol share around their kernels (csrc/hx_tool.h), each with its full text, the
function's name included: the ranges of create, the counts and a node's value at set_nodes, the three of run_nodes, the name
device_ptr does not know and the fp64 rows a handle was made without.  The handles are tiny: 10 spectral points, 2 nodes per
launch, 3 nodes."""
import ctypes

import pytest

import cia_cases as cc
import exomol_cases as ec
import lines_cases as lc
from helios_amd import cia, exomol, lines
from helios_amd._lib import HeliosHipError

pytestmark = pytest.mark.gpu

POINTS, PER, NODES = 10, 2, 3


@pytest.fixture(scope="module")
def ctx():
    from helios_amd.device import Context
    return Context(0)


class Lines(object):
    prefix = "hx_lines"
    no_fp64 = "(want_fp64 of hx_lines_create)"

    def make(self, ctx, points=POINTS, per=PER, nodes=NODES, fp64=False, load=True):
        h = lines.LineOpacity(ctx, 10, points, per, nodes, fp64)
        if load:
            h.set_lines(lc.synthetic_lines(10, 1000.0, 1002.0, seed=3))
        return h

    def set_nodes(self, h, temps, press, n_points=POINTS, dnu=0.25):
        h.set_nodes(temps, press, [1.0] * len(temps), 1.0, lc.M_H2O, 0.0, 2.0, 1000.0, dnu, n_points)


class Cia(object):
    prefix = "hx_cia"
    no_fp64 = "(hx_cia_create, with_fp64)"

    def make(self, ctx, points=POINTS, per=PER, nodes=NODES, fp64=False, load=True):
        return cia.CiaOpacity(ctx, cia.bands_of(cc.edge_blocks()), points, per, nodes, fp64)

    def set_nodes(self, h, temps, press, n_points=POINTS, dnu=0.25):
        h.set_nodes(temps, press, cc.M_H2, 30.0, dnu, n_points)


class Exomol(object):
    prefix = "hx_exomol"
    no_fp64 = "(want_fp64 of hx_exomol_create)"

    def make(self, ctx, points=POINTS, per=PER, nodes=NODES, fp64=False, load=True):
        case = ec.make("count: 63")
        if not load:
            return exomol.ExomolOpacity(ctx, len(case.states["E"]), 63, 1, points, per, nodes, fp64)
        return exomol.ExomolOpacity.of(ctx, case.states, case.trans, case.broadening, points, per, nodes, fp64)

    def set_nodes(self, h, temps, press, n_points=POINTS, dnu=0.25):
        h.set_nodes(temps, press, [1.0] * len(temps), lc.M_H2O, 2.0, 0.0, 0.0, dnu, n_points)


TOOLS = {"lines": Lines(), "cia": Cia(), "exomol": Exomol()}


def said(call):
    """what the library says: the text behind `<function> failed with status <n>: `"""
    with pytest.raises(HeliosHipError) as e:
        call()
    return str(e.value).split(": ", 1)[1]


def check_frame(ctx, tool, create="create"):
    p = tool.prefix
    for sizes, text in [(dict(per=0), "1 ... 65535 nodes per launch"), (dict(nodes=0), "1 ... 2^24 nodes"),
                        (dict(points=0), "1 ... 2^30 spectral points")]:
        assert said(lambda: tool.make(ctx, load=False, **sizes)) == "%s_%s: %s" % (p, create, text)
    h = tool.make(ctx)
    try:
        assert said(lambda: h.run_nodes(0, 1)) == "%s_run_nodes: no nodes (%s_set_nodes)" % (p, p)
        assert said(lambda: tool.set_nodes(h, [300.0] * 4, [1e5] * 4)) == "%s_set_nodes: 4 nodes, the handle holds 1 ... 3" % p
        assert said(lambda: tool.set_nodes(h, [300.0], [1e5], 11)) == "%s_set_nodes: 11 spectral points, the handle holds 1 ... 10" % p
        assert said(lambda: tool.set_nodes(h, [300.0, 400.0], [1e5, -5.0])) == (
            "%s_set_nodes: node 1: P = -5 is not a finite number > 0" % p)
        assert said(lambda: tool.set_nodes(h, [300.0], [1e5], dnu=0.0)) == "%s_set_nodes: dnu = 0 is not a finite number > 0" % p
        tool.set_nodes(h, [300.0, 400.0, 500.0], [1e5, 1e5, 1e6])
        assert said(lambda: h.run_nodes(0, 3)) == "%s_run_nodes: 3 nodes in one call, the handle holds 1 ... 2 per launch" % p
        assert said(lambda: h.run_nodes(2, 2)) == "%s_run_nodes: nodes 2 ... 3, %s_set_nodes gave 0 ... 2" % (p, p)
        assert said(lambda: h.run_nodes(-1, 1)) == "%s_run_nodes: nodes -1 ... -1, %s_set_nodes gave 0 ... 2" % (p, p)
        where = ctypes.c_void_p()
        assert said(lambda: h._call("device_ptr", b"kappa64", ctypes.byref(where))) == "%s_device_ptr: unknown name 'kappa64'" % p
        assert said(lambda: h.get("slabs32")) == "%s_get: no nodes have been run (%s_run_nodes)" % (p, p)
        h.run_nodes(1, 2)
        assert h.get("slabs32").shape == (2, POINTS) and h.slab_pointer().value
        if tool.no_fp64:
            assert said(lambda: h.get("kappa64")) == "%s_get: the handle keeps no fp64 rows %s" % (p, tool.no_fp64)
    finally:
        h.close()


@pytest.mark.parametrize("name", sorted(TOOLS))
def test_the_frames_refusals_with_their_full_text(ctx, name):
    check_frame(ctx, TOOLS[name])
