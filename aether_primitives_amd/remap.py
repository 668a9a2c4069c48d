"""Rate matching on the device: periodic byte maps for puncturing and interleaving (include/aether_hip.h, aeth_remap_*).

The reference has nothing of the kind.  A `Remap` is an input period r_in, an output period r_out and a table of r_out
entries, each -1 or an index below r_in:

    out[q r_out + i] = fill if map[i] < 0 else in[q r_in + map[i]]

Puncturing, depuncturing to erasures, block interleaving and any chain of them are this one gather; the tables come from
the library's host builders (the functions below need no context), and a chain composed with `.then` is still one pass
over one-byte data.  Bytes are never interpreted: `exec` takes and returns `DeviceBits` or `DeviceSoft`."""
import ctypes as C

import numpy as np

from . import _lib
from ._device import Handle
from ._lib import check
from .modulation import DeviceBits, DeviceSoft

ROUTE_TILE, ROUTE_GATHER = 1, 2                 # AETH_REMAP_ROUTE_*
MAX_PERIOD = 1 << 20


def _i32(a):
    return np.ascontiguousarray(a, np.int32)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def puncture_map(keep):
    """keep[i] & 1: coded bit i of a period of len(keep) is sent -> (map of the kept positions ascending, r_in = len(keep))"""
    keep = np.ascontiguousarray(keep, np.uint8)
    out = np.empty(max(keep.size, 1), np.int32)
    r_out = C.c_size_t(0)
    check(_lib.load().aeth_remap_puncture(_p(keep), keep.size, _p(out), out.size, C.byref(r_out)))
    return out[:r_out.value].copy(), int(keep.size)


def invert_map(map, r_in):
    """inv[j] = the smallest i with map[i] == j, or -1 -> (inv, r_in of the inverse = len(map))"""
    map = _i32(map)
    inv = np.empty(max(int(r_in), 1), np.int32)
    check(_lib.load().aeth_remap_invert(_p(map), map.size, int(r_in), _p(inv)))
    return inv[:int(r_in)].copy(), int(map.size)


def compose_maps(a, a_in, b, b_in):
    """b applied to the output of a -> (map, r_in)"""
    a, b = _i32(a), _i32(b)
    out = np.empty(MAX_PERIOD, np.int32)
    r_out, r_in = C.c_size_t(0), C.c_size_t(0)
    check(_lib.load().aeth_remap_compose(_p(a), a.size, int(a_in), _p(b), b.size, int(b_in), _p(out), out.size, C.byref(r_out),
                                         C.byref(r_in)))
    return out[:r_out.value].copy(), int(r_in.value)


def rows_cols_map(rows, cols):
    """written row by row, read column by column: map[c rows + r] = r cols + c -> (map, r_in = rows cols)"""
    n = int(rows) * int(cols)
    out = np.empty(min(max(n, 1), MAX_PERIOD), np.int32)
    check(_lib.load().aeth_remap_rows_cols(int(rows), int(cols), _p(out)))
    return out, n


def bicm16_map(n_cbps, n_bpsc):
    """the interleaver of 802.11a 17.3.5.6 in gather form: map[j] = k -> (map, r_in = n_cbps)"""
    out = np.empty(min(max(int(n_cbps), 1), MAX_PERIOD), np.int32)
    check(_lib.load().aeth_remap_bicm16(int(n_cbps), int(n_bpsc), _p(out)))
    return out, int(n_cbps)


class Remap(Handle):
    """Remap(ctx, map, r_in): the object owns the device copy of its table."""

    DESTROY = "aeth_remap_destroy"

    def __init__(self, ctx, map, r_in):
        super().__init__(ctx)
        self.map = _i32(map).copy()
        self.r_in = int(r_in)
        check(self._lib.aeth_remap_create(ctx.h, _p(self.map), self.map.size, self.r_in, C.byref(self.h)))

    @classmethod
    def puncture(cls, ctx, keep):
        return cls(ctx, *puncture_map(keep))

    @classmethod
    def rows_cols(cls, ctx, rows, cols):
        return cls(ctx, *rows_cols_map(rows, cols))

    @classmethod
    def bicm16(cls, ctx, n_cbps, n_bpsc):
        return cls(ctx, *bicm16_map(n_cbps, n_bpsc))

    def inverse(self):
        """the depuncturer of a puncturer, the deinterleaver of an interleaver, the first copy of a repetition"""
        return Remap(self.ctx, *invert_map(self.map, self.r_in))

    def then(self, other):
        """`other` applied to the output of this map, as one map"""
        return Remap(self.ctx, *compose_maps(self.map, self.r_in, other.map, other.r_in))

    @property
    def r_out(self):
        return int(self._lib.aeth_remap_out_period(self.h))

    @property
    def route(self):
        return int(self._lib.aeth_remap_route(self.h))

    @property
    def tile(self):
        """periods per tile on the tile route, 0 on the gather route"""
        return int(self._lib.aeth_remap_tile(self.h))

    def in_count(self, n_out):
        """input bytes a call that writes n_out bytes reads"""
        return int(self._lib.aeth_remap_in_count(self.h, int(n_out)))

    def out_count(self, n_in):
        """the most outputs n_in input bytes serve"""
        q = int(n_in) // self.r_in
        lo, hi = q * self.r_out, (q + 1) * self.r_out                # in_count(lo) <= n_in < in_count(hi), in_count is monotone
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if self.in_count(mid) <= n_in else (lo, mid)
        return lo

    def exec(self, x, fill=0, out=None, n_out=None):
        """-> a buffer of x's kind holding `n_out` bytes (default: all that x serves; out.n when `out` is given)"""
        if not isinstance(x, (DeviceBits, DeviceSoft)):
            x = np.asarray(x)
            x = DeviceSoft(self.ctx, x.size, x) if x.dtype == np.int8 else DeviceBits(self.ctx, x.size, x)
        if out is None:
            out = type(x)(self.ctx, self.out_count(x.n) if n_out is None else int(n_out))
        check(self._lib.aeth_remap_exec(self.h, C.c_void_p(x.ptr), x.n, C.c_void_p(out.ptr), out.n, int(fill) & 0xff))
        return out
