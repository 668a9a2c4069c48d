"""What the coding modules' Python objects share: a typed array in device memory and an object that owns a C handle."""
import ctypes as C

import numpy as np

from . import _lib


class DeviceArray:
    """`n` elements of the subclass's `DTYPE` in device memory, uploaded from `host` (converted to DTYPE) when given.  What
    a call writes there is stream-ordered; `to_host()` waits for it."""

    DTYPE = None

    def __init__(self, ctx, n, host=None):
        self.ctx, self.n = ctx, int(n)
        self.ptr = ctx.alloc(max(self.n, 1) * self.DTYPE.itemsize)
        if host is not None and self.n:
            ctx.upload(self.ptr, np.ascontiguousarray(host, self.DTYPE))

    def __len__(self):
        return self.n

    def __del__(self):
        try:
            if self.ptr and self.ctx.h:                              # a closed context has freed its memory itself
                self.ctx.free(self.ptr)
                self.ptr = None
        except Exception:
            pass

    def to_host(self):
        out = np.empty(self.n, self.DTYPE)
        if self.n:
            self.ctx.download(self.ptr, out)
        return out

    def _p(self):
        return C.c_void_p(self.ptr)


class Handle:
    """An object made on a context by a create call of the library: `ctx`, `_lib` and the C handle `h`, which the subclass's
    create call fills and `close()` (or the last reference) gives to the function named `DESTROY`, once."""

    DESTROY = None
    NEEDS_CONTEXT = True            # destroy waits for the context's stream: skipped when the context has been closed

    def __init__(self, ctx):
        self.ctx, self._lib, self.h = ctx, _lib.load(), C.c_void_p()

    def close(self):
        if getattr(self, "h", None) and self.h.value:
            if self.ctx.h or not self.NEEDS_CONTEXT:
                getattr(self._lib, self.DESTROY)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
