"""Context + the VecOps mirror (reference: src/vecops.rs:39-89).

`DeviceVec` is the device-resident receiver: the same chainable
method set as the trait, each call one stream-ordered kernel launch, no host
traffic.  `HostVec` is the literal host-slice receiver: every call stages
through the GPU and returns with the numpy array updated (one H2D + D2H per
call, as a drop-in `impl VecOps for [cf32]` would).
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


def _c64(a):
    a = np.ascontiguousarray(a, dtype=np.complex64)
    return a


# level kinds of aeth_vec_levels / aeth_fft_exec_levels (include/aether_hip.h, AETH_LEVEL_*)
LEVEL_NORM, LEVEL_DB, LEVEL_POWER_DB = 0, 1, 2


class _VecStats(C.Structure):
    # struct aeth_vec_stats
    _fields_ = [("n", C.c_size_t), ("n_nan", C.c_size_t), ("min_index", C.c_size_t), ("max_index", C.c_size_t),
                ("min_norm", C.c_float), ("max_norm", C.c_float), ("mean_re", C.c_double), ("mean_im", C.c_double),
                ("power", C.c_double)]


class VecStats:
    """What `stats()` returns (the reference's open item "VecStats": Min(index), Max(index), Mean, Power).  min / max are
    by |c|^2 in f64, ties to the lowest index; samples with a NaN component are counted in `n_nan` and skipped (all NaN:
    both indices are `n`).  `raw` is the C struct, byte for byte."""
    __slots__ = ("n", "n_nan", "min_index", "max_index", "min_norm", "max_norm", "mean", "power", "raw")

    def __init__(self, c):
        self.n, self.n_nan, self.min_index, self.max_index = c.n, c.n_nan, c.min_index, c.max_index
        self.min_norm, self.max_norm = np.float32(c.min_norm), np.float32(c.max_norm)
        self.mean = complex(c.mean_re, c.mean_im)
        self.power = c.power
        self.raw = bytes(c)

    def __repr__(self):
        return (f"VecStats(n={self.n}, n_nan={self.n_nan}, min={self.min_norm!r}@{self.min_index}, "
                f"max={self.max_norm!r}@{self.max_index}, mean={self.mean!r}, power={self.power!r})")


class Context:
    """One device + one HIP stream (aeth_ctx).  Not thread-safe, like `&mut self`."""

    def __init__(self, device=0, stream=None):
        self._lib = _lib.load()
        h = C.c_void_p()
        if stream is None:
            check(self._lib.aeth_ctx_create(device, C.byref(h)))
        else:
            check(self._lib.aeth_ctx_create_on_stream(device, C.c_void_p(stream), C.byref(h)))
        self.h = h
        self.device = device

    def close(self):
        if getattr(self, "h", None):
            self._lib.aeth_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._lib.aeth_ctx_sync(self.h))

    def trim(self):
        """Give back what the context retains between calls (host pipeline: stage streams, device slots, pinned staging
        elements, copy threads; the device scratch of the host-slice flavours)."""
        check(self._lib.aeth_ctx_trim(self.h))

    def set_overlap(self, enable=True):
        """Let consecutive independent `Fir.filter` launches alternate between two HIP queues (the end of one
        launch then runs beside the start of the next); everything else stays ordered as on one stream."""
        check(self._lib.aeth_ctx_set_overlap(self.h, 1 if enable else 0))

    @property
    def overlap(self):
        return bool(self._lib.aeth_ctx_overlap(self.h))

    def lane_counts(self):
        """(packets, joins) the overlap lane has spent on ordering so far: event packets in front of its launches, and
        chains it ended by joining the two queues."""
        p, j = C.c_uint64(), C.c_uint64()
        check(self._lib.aeth_ctx_lane_counts(self.h, C.byref(p), C.byref(j)))
        return p.value, j.value

    @property
    def stream(self):
        """hipStream_t of the context for interop.  SIDE EFFECT: handing the stream out parks the overlap lane (every
        later launch stays on this one stream, `overlap` reads False) until `set_overlap(True)` re-arms it."""
        return self._lib.aeth_ctx_stream(self.h)

    # ---- device memory ----
    def alloc(self, nbytes):
        p = C.c_void_p()
        check(self._lib.aeth_dev_alloc(self.h, nbytes, C.byref(p)))
        return p.value

    def free(self, ptr):
        check(self._lib.aeth_dev_free(self.h, C.c_void_p(ptr)))

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        check(self._lib.aeth_upload(self.h, C.c_void_p(dptr), arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def download(self, dptr, arr):
        assert arr.flags["C_CONTIGUOUS"]
        check(self._lib.aeth_download(self.h, arr.ctypes.data_as(C.c_void_p), C.c_void_p(dptr), arr.nbytes))

    # ---- constructors ----
    def vec(self, host_array):
        """Upload a complex64 array -> DeviceVec."""
        a = _c64(host_array).reshape(-1)
        v = DeviceVec(self, a.size)
        if a.size:
            self.upload(v.ptr, a)
        return v

    def empty(self, n):
        return DeviceVec(self, n)

    # ---- averaged spectra (aeth_vec_frame_sums / aeth_vec_sum_levels; no body in the reference) ----
    def frame_sums(self, vec, len, block=0, chunk=32, want=("sum", "max")):
        """`vec` as frames of `len` samples: the per-column sum and maximum of q = re^2 + im^2 (f64) over rows of `block`
        frames (0: one row over the whole call), frames added in chunks of `chunk` in ascending order -> (sum, max) as
        DeviceF64 of rows * len values; a plane that `want` does not name is None."""
        if not isinstance(vec, DeviceVec):
            vec = self.vec(vec)
        ln, block = int(len), int(block)
        frames = vec.n // ln if ln else 0
        rows = -(-frames // block) if 0 < block < frames else 1
        s = DeviceF64(self, rows * ln) if "sum" in want else None
        m = DeviceF64(self, rows * ln) if "max" in want else None
        check(self._lib.aeth_vec_frame_sums(self.h, vec._p(), vec.n, ln, block, int(chunk), s._p() if s else None, m._p() if m else None,
                                            rows * ln))
        return s, m

    def sum_levels(self, plane, count, kind=LEVEL_NORM, out=None):
        """what a plot draws of a plane: the level (LEVEL_*) of q / count -> DeviceF32.  `count` is the number of frames
        of a row for a sum plane, 1 for a max plane."""
        out = DeviceF32(self, plane.n) if out is None else out
        check(self._lib.aeth_vec_sum_levels(self.h, plane._p(), plane.n, float(count), int(kind), out._p()))
        return out

    # ---- events (bench) ----
    def event(self):
        return Event(self)


class Event:
    def __init__(self, ctx):
        self.ctx = ctx
        h = C.c_void_p()
        check(ctx._lib.aeth_event_create(ctx.h, C.byref(h)))
        self.h = h

    def record(self):
        check(self.ctx._lib.aeth_event_record(self.h))

    def sync(self):
        check(self.ctx._lib.aeth_event_sync(self.h))

    def elapsed_ms(self, stop):
        ms = C.c_float()
        check(self.ctx._lib.aeth_event_elapsed_ms(self.h, stop.h, C.byref(ms)))
        return ms.value

    def __del__(self):
        try:
            if self.h:
                self.ctx._lib.aeth_event_destroy(self.h)
                self.h = None
        except Exception:
            pass


class DeviceF32:
    """Device-resident `[f32]`: the levels of a vector or of a batch of spectra."""

    def __init__(self, ctx, n, ptr=None, offset=0, owner=None):
        self.ctx, self.n, self._owner = ctx, int(n), owner
        if ptr is None:
            self._base = ctx.alloc(max(self.n, 1) * 4)
            self.ptr, self._owns = self._base, True
        else:
            self._base, self.ptr, self._owns = ptr, ptr + offset * 4, False

    def __len__(self):
        return self.n

    def __del__(self):
        try:
            if self._owns and self._base and self.ctx.h:
                self.ctx.free(self._base)
                self._base = None
        except Exception:
            pass

    def slice(self, start, stop):
        assert 0 <= start <= stop <= self.n
        return DeviceF32(self.ctx, stop - start, ptr=self.ptr, offset=start, owner=self)

    def to_host(self):
        out = np.empty(self.n, np.float32)
        if self.n:
            self.ctx.download(self.ptr, out)
        return out

    def _p(self):
        return C.c_void_p(self.ptr)


class DeviceF64:
    """Device-resident `[f64]`: the sum and max planes of averaged spectra."""

    def __init__(self, ctx, n, ptr=None, offset=0, owner=None):
        self.ctx, self.n, self._owner = ctx, int(n), owner
        if ptr is None:
            self._base = ctx.alloc(max(self.n, 1) * 8)
            self.ptr, self._owns = self._base, True
        else:
            self._base, self.ptr, self._owns = ptr, ptr + offset * 8, False

    def __len__(self):
        return self.n

    def __del__(self):
        try:
            if self._owns and self._base and self.ctx.h:
                self.ctx.free(self._base)
                self._base = None
        except Exception:
            pass

    def slice(self, start, stop):
        assert 0 <= start <= stop <= self.n
        return DeviceF64(self.ctx, stop - start, ptr=self.ptr, offset=start, owner=self)

    def to_host(self):
        out = np.empty(self.n, np.float64)
        if self.n:
            self.ctx.download(self.ptr, out)
        return out

    def _p(self):
        return C.c_void_p(self.ptr)


class DeviceVec:
    """Device-resident `[cf32]` with the VecOps method set (src/vecops.rs:39-89)."""

    def __init__(self, ctx, n, ptr=None, offset=0, owner=None):
        self.ctx = ctx
        self.n = int(n)
        self._owner = owner
        if ptr is None:
            self._base = ctx.alloc(max(self.n, 1) * 8)
            self.ptr = self._base
            self._owns = True
        else:
            self._base = ptr
            self.ptr = ptr + offset * 8
            self._owns = False

    def __len__(self):
        return self.n

    def __del__(self):
        try:
            if self._owns and self._base and self.ctx.h:
                self.ctx.free(self._base)
                self._base = None
        except Exception:
            pass

    def slice(self, start, stop):
        """Borrowed sub-slice `self[start..stop]` (keeps the parent alive)."""
        assert 0 <= start <= stop <= self.n
        return DeviceVec(self.ctx, stop - start, ptr=self.ptr, offset=start, owner=self)

    def to_host(self):
        out = np.empty(self.n, np.complex64)
        if self.n:
            self.ctx.download(self.ptr, out)
        return out

    def _p(self):
        return C.c_void_p(self.ptr)

    def fused(self):
        """A chain of the element-wise methods as ONE pass over memory (`aeth_vec_chain`): record the links with the
        usual names, `run()` (or leaving a `with` block) executes them -- bit-identical to the separate calls:
            v.fused().vec_add(a).vec_mul(b).vec_conj().run()         # BASELINE config 1: one launch, 32 B per sample"""
        return _Chain(self)

    def _other(self, other):
        if isinstance(other, DeviceVec):
            return other
        return self.ctx.vec(other)      # host slice given: stage it (AsRef<[cf32]>)

    # ---- numbers and levels (aeth_vec_stats / aeth_vec_levels; no body in the reference yet) ----
    def stats(self):
        """One read-only pass: count, NaN count, min / max by norm with their indices, mean, power -> VecStats.
        Waits for the 64-byte record; nothing else leaves the device."""
        c = _VecStats()
        check(self.ctx._lib.aeth_vec_stats(self.ctx.h, self._p(), self.n, C.byref(c)))
        return VecStats(c)

    def levels(self, kind=LEVEL_NORM, out=None):
        """norm() (LEVEL_NORM), the reference's DB::from(norm).db() (LEVEL_DB: 10 * log10 of the amplitude, its quirk)
        or the power in dB (LEVEL_POWER_DB) of every sample (util/plot.rs:65,127) -> DeviceF32; self is not modified."""
        out = DeviceF32(self.ctx, self.n) if out is None else out
        check(self.ctx._lib.aeth_vec_levels(self.ctx.h, self._p(), self.n, int(kind), out._p(), out.n))
        return out

    # ---- trait VecOps ----
    def vec_scale(self, scale):                                   # vecops.rs:41
        check(self.ctx._lib.aeth_vec_scale(self.ctx.h, self._p(), self.n, float(np.float32(scale)))); return self

    def vec_mul(self, other):                                     # vecops.rs:44
        o = self._other(other); check(self.ctx._lib.aeth_vec_mul(self.ctx.h, self._p(), self.n, o._p(), o.n)); return self

    def vec_div(self, other):                                     # vecops.rs:47
        o = self._other(other); check(self.ctx._lib.aeth_vec_div(self.ctx.h, self._p(), self.n, o._p(), o.n)); return self

    def vec_conj(self):                                           # vecops.rs:50
        check(self.ctx._lib.aeth_vec_conj(self.ctx.h, self._p(), self.n)); return self

    def vec_mirror(self):                                         # vecops.rs:54
        check(self.ctx._lib.aeth_vec_mirror(self.ctx.h, self._p(), self.n)); return self

    def vec_mul_frames(self, sig, frame_len=None):
        """every frame of `frame_len` samples *= sig (one launch; benches.rs:410-416's vec_mul per chunk)"""
        o = self._other(sig); L = frame_len or o.n
        check(self.ctx._lib.aeth_vec_mul_frames(self.ctx.h, self._p(), L, self.n // L if L else 0, o._p(), o.n)); return self

    def vec_mirror_frames(self, frame_len):
        check(self.ctx._lib.aeth_vec_mirror_frames(self.ctx.h, self._p(), frame_len, self.n // frame_len)); return self

    def vec_clone(self, other):                                   # vecops.rs:58
        o = self._other(other); check(self.ctx._lib.aeth_vec_clone(self.ctx.h, self._p(), self.n, o._p(), o.n)); return self

    def vec_zero(self):                                           # vecops.rs:61
        check(self.ctx._lib.aeth_vec_zero(self.ctx.h, self._p(), self.n)); return self

    def vec_mutate(self, f):                                      # vecops.rs:64
        """Closure per element, in order: cannot cross the FFI -> D2H, apply, H2D (slow by design)."""
        h = self.to_host()
        for i in range(h.size):
            r = f(h[i])
            if r is not None:
                h[i] = r
        if self.n:
            self.ctx.upload(self.ptr, h)
        return self

    def vec_add(self, other):                                     # vecops.rs:67
        o = self._other(other); check(self.ctx._lib.aeth_vec_add(self.ctx.h, self._p(), self.n, o._p(), o.n)); return self

    def vec_sub(self, other):                                     # vecops.rs:70
        o = self._other(other); check(self.ctx._lib.aeth_vec_sub(self.ctx.h, self._p(), self.n, o._p(), o.n)); return self

    def vec_fft(self, scale):                                     # vecops.rs:74, :185-189 (the reference plans per call; the context caches)
        check(self.ctx._lib.aeth_vec_fft(self.ctx.h, self._p(), self.n, +1, scale.kind, scale.x)); return self

    def vec_ifft(self, scale):                                    # vecops.rs:78, :191-196
        check(self.ctx._lib.aeth_vec_fft(self.ctx.h, self._p(), self.n, -1, scale.kind, scale.x)); return self

    def vec_rfft(self, fft, scale):                               # vecops.rs:83, :198-202
        fft.ifwd(self, scale); return self

    def vec_rifft(self, fft, scale):                              # vecops.rs:88, :203-207
        fft.ibwd(self, scale); return self


class _VecStep(C.Structure):
    # struct aeth_vec_step
    _fields_ = [("op", C.c_int), ("other_dev", C.c_void_p), ("n_other", C.c_size_t), ("scale", C.c_float)]


class _Chain:
    """links recorded for DeviceVec.fused(); AETH_VEC_*: scale 0, mul 1, div 2, conj 3, add 4, sub 5, clone 6, zero 7"""

    def __init__(self, vec):
        self.vec, self.steps, self._keep = vec, [], []

    def _bin(self, op, other):
        o = self.vec._other(other)
        self._keep.append(o)
        self.steps.append(_VecStep(op, o.ptr, o.n, 0.0)); return self

    def vec_scale(self, s): self.steps.append(_VecStep(0, None, 0, float(np.float32(s)))); return self
    def vec_mul(self, o): return self._bin(1, o)
    def vec_div(self, o): return self._bin(2, o)
    def vec_conj(self): self.steps.append(_VecStep(3, None, 0, 0.0)); return self
    def vec_add(self, o): return self._bin(4, o)
    def vec_sub(self, o): return self._bin(5, o)
    def vec_clone(self, o): return self._bin(6, o)
    def vec_zero(self): self.steps.append(_VecStep(7, None, 0, 0.0)); return self

    def run(self):
        arr = (_VecStep * max(len(self.steps), 1))(*self.steps)
        check(self.vec.ctx._lib.aeth_vec_chain(self.vec.ctx.h, self.vec._p(), self.vec.n, arr, len(self.steps)))
        self.steps, self._keep = [], []
        return self.vec

    def __enter__(self): return self
    def __exit__(self, et, ev, tb):
        if et is None: self.run()


class HostVec:
    """Host slice receiver: numpy complex64 array mutated in place through the GPU."""

    def __init__(self, ctx, array):
        assert isinstance(array, np.ndarray) and array.dtype == np.complex64 and array.flags["C_CONTIGUOUS"]
        self.ctx = ctx
        self.a = array

    def _p(self):
        return self.a.ctypes.data_as(C.c_void_p)

    def _bin(self, name, other):
        o = _c64(other)
        check(getattr(self.ctx._lib, name)(self.ctx.h, self._p(), self.a.size, o.ctypes.data_as(C.c_void_p), o.size))
        return self

    def stats(self):
        """VecStats of the host slice, computed on the device (the same record, bit for bit, as DeviceVec.stats())"""
        c = _VecStats()
        check(self.ctx._lib.aeth_host_vec_stats(self.ctx.h, self._p(), self.a.size, C.byref(c)))
        return VecStats(c)

    def vec_scale(self, s):
        check(self.ctx._lib.aeth_host_vec_scale(self.ctx.h, self._p(), self.a.size, float(np.float32(s)))); return self

    def vec_mul(self, o): return self._bin("aeth_host_vec_mul", o)
    def vec_div(self, o): return self._bin("aeth_host_vec_div", o)
    def vec_add(self, o): return self._bin("aeth_host_vec_add", o)
    def vec_sub(self, o): return self._bin("aeth_host_vec_sub", o)
    def vec_clone(self, o): return self._bin("aeth_host_vec_clone", o)

    def vec_conj(self):
        check(self.ctx._lib.aeth_host_vec_conj(self.ctx.h, self._p(), self.a.size)); return self

    def vec_mirror(self):
        check(self.ctx._lib.aeth_host_vec_mirror(self.ctx.h, self._p(), self.a.size)); return self

    def vec_zero(self):
        check(self.ctx._lib.aeth_host_vec_zero(self.ctx.h, self._p(), self.a.size)); return self

    def vec_mutate(self, f):
        for i in range(self.a.size):
            r = f(self.a[i])
            if r is not None:
                self.a[i] = r
        return self

    def vec_fft(self, scale):
        check(self.ctx._lib.aeth_host_vec_fft(self.ctx.h, self._p(), self.a.size, +1, scale.kind, scale.x)); return self

    def vec_ifft(self, scale):
        check(self.ctx._lib.aeth_host_vec_fft(self.ctx.h, self._p(), self.a.size, -1, scale.kind, scale.x)); return self

    def vec_rfft(self, fft, scale):
        fft.ifwd(self.a, scale); return self

    def vec_rifft(self, fft, scale):
        fft.ibwd(self.a, scale); return self
