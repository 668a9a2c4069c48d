"""Streaming correlator: the reference's open item "Add Correlation by Freq. Domain Convolution" (README.md:95), built
from the chain of its "correlator inplace" benchmark (benches/benches.rs:394-416) run as overlap-save over a stream.

    c[j] = sum_{k<M} conj(ref[M-1-k]) * x[j-k]

is the causal matched filter: an occurrence of `ref` that starts at stream index p peaks at j = p + M - 1."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check
from .context import DeviceF32, DeviceVec, LEVEL_NORM


class _CorrPeak(C.Structure):
    _fields_ = [("index", C.c_size_t), ("norm", C.c_float), ("n_nan", C.c_uint)]


# one record of aeth_corr_search as numpy sees it (struct aeth_corr_peak: 16 bytes, no padding)
PEAK_DTYPE = np.dtype([("index", np.uint64), ("norm", np.float32), ("n_nan", np.uint32)])


class CorrPeak:
    """index: output index of the largest |c|^2 (lowest index among equals; n when every sample had a NaN component),
    lag = index - (nref - 1): where the occurrence starts; norm: |c| there; n_nan: samples with a NaN component."""
    __slots__ = ("index", "lag", "norm", "n_nan")

    def __init__(self, index, norm, n_nan, nref):
        self.index, self.norm, self.n_nan = int(index), float(norm), int(n_nan)
        self.lag = self.index - (nref - 1)

    def __repr__(self):
        return f"CorrPeak(index={self.index}, lag={self.lag}, norm={self.norm!r}, n_nan={self.n_nan})"


class Corr:
    def __init__(self, ctx, ref, fft_len=2048):
        self.ctx = ctx
        self._lib = _lib.load()
        ref = np.ascontiguousarray(ref, dtype=np.complex64)
        h = C.c_void_p()
        check(self._lib.aeth_corr_create(ctx.h, ref.ctypes.data_as(C.c_void_p), ref.size, fft_len, C.byref(h)))
        self.h = h

    def __del__(self):
        try:
            if self.h and self.ctx.h:
                self._lib.aeth_corr_destroy(self.h)
                self.h = None
        except Exception:
            pass

    @property
    def nref(self): return self._lib.aeth_corr_nref(self.h)
    @property
    def fft_len(self): return self._lib.aeth_corr_fft_len(self.h)
    @property
    def hop(self): return self._lib.aeth_corr_hop(self.h)

    def n_blocks(self, n):
        """peak records `search` produces for a stream of n samples"""
        return -(-int(n) // self.hop)

    def correlate(self, x, out=None, hist=None):
        """c[j] for every sample of the DeviceVec x; zero initial state unless `hist` (the nref-1 samples before x[0])."""
        out = DeviceVec(self.ctx, x.n) if out is None else out
        check(self._lib.aeth_corr_exec(self.h, hist._p() if hist is not None else None, x._p(), x.n, out._p()))
        return out

    def levels(self, x, kind=LEVEL_NORM, out=None, hist=None):
        """level of c[j] (LEVEL_NORM / LEVEL_DB / LEVEL_POWER_DB) -> DeviceF32, in one pass: c itself is never written."""
        out = DeviceF32(self.ctx, x.n) if out is None else out
        check(self._lib.aeth_corr_exec_levels(self.h, hist._p() if hist is not None else None, x._p(), x.n, int(kind),
                                              out._p(), out.n))
        return out

    def search(self, x, hist=None, blocks=False):
        """The best CorrPeak of the stream in one pass (nothing of c is written).  blocks=True: (best, records) with one
        record per `hop` outputs as a structured array (PEAK_DTYPE), for thresholding on the host."""
        best = _CorrPeak()
        hp = hist._p() if hist is not None else None
        if not blocks:
            check(self._lib.aeth_corr_search(self.h, hp, x._p(), x.n, None, 0, C.byref(best)))
            return CorrPeak(best.index, best.norm, best.n_nan, self.nref)
        nb = self.n_blocks(x.n)
        dev = self.ctx.alloc(max(nb, 1) * PEAK_DTYPE.itemsize)
        try:
            check(self._lib.aeth_corr_search(self.h, hp, x._p(), x.n, C.c_void_p(dev), nb, C.byref(best)))
            rec = np.empty(nb, PEAK_DTYPE)
            if nb:
                self.ctx.download(dev, rec)
        finally:
            self.ctx.free(dev)
        return CorrPeak(best.index, best.norm, best.n_nan, self.nref), rec
