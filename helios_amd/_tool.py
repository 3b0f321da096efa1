"""What the device objects of the off-line tools share: the pointers ctypes wants, and the handle with its checked calls,
get(name) and close().  A class names its C object (`PREFIX`, as in hx_ktable_create) and the results it returns (`_results`)."""
import ctypes

import numpy as np


def dp(a):
    """a contiguous float64 array as const double*; None is NULL.  The pointer keeps the array alive."""
    return None if a is None else a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def ip(a):
    """a contiguous int32 array as const int*"""
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class DeviceObject(object):
    PREFIX = None

    def _create(self, ctx, *args, **how):
        """`constructor`: another of the object's constructors than <PREFIX>_create"""
        from . import _lib
        self.ctx, self._l = ctx, _lib.lib()
        h = ctypes.c_void_p()
        name = "%s_%s" % (self.PREFIX, how.get("constructor", "create"))
        ctx.check(getattr(self._l, name)(ctx.handle, *(args + (ctypes.byref(h),))), name)
        self.handle = h

    def _call(self, what, *args):
        self.ctx.check(getattr(self._l, "%s_%s" % (self.PREFIX, what))(self.handle, *args), "%s_%s" % (self.PREFIX, what))

    def _results(self):
        """{name: shape of float64, or (shape, dtype)}"""
        raise NotImplementedError

    def get(self, name):
        spec = self._results().get(name, 1)         # a name the class does not know is the library's to refuse
        shape, dtype = spec if isinstance(spec, tuple) and isinstance(spec[-1], type) else (spec, np.float64)
        out = np.zeros(shape, dtype)
        self.ctx.check(getattr(self._l, self.PREFIX + "_get")(self.handle, name.encode(), vp(out), out.nbytes),
                       "%s_get(%s)" % (self.PREFIX, name))
        return out

    def close(self):
        if self.handle:
            getattr(self._l, self.PREFIX + "_destroy")(self.handle)
            self.handle = None
