"""What the record reductions (sync, mov) share on the Python side: an array of records on the device and the number of
records a call produces."""
import ctypes as C

import numpy as np

from .context import DeviceVec


def n_blocks(n, block):
    """records a call over n samples in blocks of `block` (0: one block) produces"""
    n, block = int(n), int(block)
    return -(-n // (block if block else max(n, 1)))


def _vec(ctx, x):
    return x if isinstance(x, DeviceVec) else ctx.vec(x)


class DeviceRecordArray:
    """`count` records of the subclass's `DTYPE` on the device, filled by a call (stream-ordered, no wait)."""

    DTYPE = None

    def __init__(self, ctx, count):
        self.ctx, self.n = ctx, int(count)
        self.ptr = ctx.alloc(max(self.n, 1) * self.DTYPE.itemsize)

    def __len__(self):
        return self.n

    def __del__(self):
        try:
            if self.ptr and self.ctx.h:
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
