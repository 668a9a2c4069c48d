"""CPU: what the coding chain's Python objects do with a context, on a stub context that logs every call.  The eight
typed device arrays (bytes allocated, the dtype an upload arrives in, what `to_host()` answers, one free, none on a closed
context) and the six objects with a C handle (destroy once, and whether a closed context keeps them from it)."""
import ctypes as C
import gc

import numpy as np
import pytest

from aether_primitives_amd import cc, crc, ldpc, modulation, polar, remap, rs


class StubContext:
    """alloc / free / upload / download over a bytearray, every call logged; `h` is what the objects look at before they free"""

    def __init__(self):
        self.h = C.c_void_p(0x1000)
        self.mem = bytearray(1 << 12)
        self.top = 64
        self.log = []

    def alloc(self, nbytes):
        p, self.top = self.top, self.top + (int(nbytes) + 63) // 64 * 64
        self.log.append(("alloc", int(nbytes), p))
        return p

    def free(self, ptr):
        self.log.append(("free", ptr))

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        self.log.append(("upload", dptr, arr.dtype, arr.nbytes))
        self.mem[dptr:dptr + arr.nbytes] = arr.tobytes()

    def download(self, dptr, arr):
        self.log.append(("download", dptr, arr.nbytes))
        arr.reshape(-1).view(np.uint8)[:] = np.frombuffer(self.mem, np.uint8, arr.nbytes, dptr)

    def calls(self, kind):
        return [e for e in self.log if e[0] == kind]


# class, dtype, constructor takes n, constructor takes host=
ARRAYS = ((modulation.DeviceBits, np.dtype(np.uint8), True, True),
          (modulation.DeviceSoft, np.dtype(np.int8), True, True),
          (crc.DeviceU64, np.dtype(np.uint64), True, True),
          (crc.CrcSummary, np.dtype(np.uint64), False, False),
          (ldpc.DeviceRecords, ldpc.RECORD, True, False),
          (rs.DeviceRecords, rs.RECORD, True, False),
          (rs.DeviceSummary, rs.SUMMARY, False, False),
          (polar.DeviceFlips, np.dtype(np.uint32), True, True))
FIXED = {crc.CrcSummary: 2, rs.DeviceSummary: 1}                         # elements of the two that take no count
IDS = [f"{a[0].__module__.rsplit('.', 1)[-1]}.{a[0].__name__}" for a in ARRAYS]


def make(cls, ctx, n, sized, **kw):
    return cls(ctx, n, **kw) if sized else cls(ctx)


@pytest.mark.parametrize("cls,dtype,sized,hosted", ARRAYS, ids=IDS)
def test_bytes_allocated_and_freed_once(cls, dtype, sized, hosted):
    for n in (0, 1, 5) if sized else (FIXED[cls],):
        ctx = StubContext()
        a = make(cls, ctx, n, sized)
        assert [e[1] for e in ctx.calls("alloc")] == [max(n, 1) * dtype.itemsize], (n, ctx.log)
        ptr = ctx.calls("alloc")[0][2]
        assert a.ptr == ptr
        assert a.n == n and a.ctx is ctx and len(a) == n and a._p().value == ptr
        assert not ctx.calls("upload") and not ctx.calls("free")
        del a
        gc.collect()
        assert ctx.calls("free") == [("free", ptr)], (n, ctx.log)


@pytest.mark.parametrize("cls,dtype,sized,hosted", ARRAYS, ids=IDS)
def test_a_closed_context_is_not_asked_to_free(cls, dtype, sized, hosted):
    ctx = StubContext()
    a = make(cls, ctx, 3, sized)
    ctx.h = None
    del a
    gc.collect()
    assert not ctx.calls("free"), ctx.log


@pytest.mark.parametrize("cls,dtype,sized,hosted", [a for a in ARRAYS if a[3]], ids=[i for i, a in zip(IDS, ARRAYS) if a[3]])
def test_host_values_arrive_in_the_dtype_of_the_class(cls, dtype, sized, hosted):
    for host in ([1.0, 0.0, 3.0, 2.0, 1.0], np.array([1, 0, 3, 2, 1], np.int64)):
        ctx = StubContext()
        a = cls(ctx, 5, host=host)
        assert ctx.calls("upload") == [("upload", a.ptr, dtype, 5 * dtype.itemsize)], ctx.log
        assert np.frombuffer(ctx.mem, dtype, 5, a.ptr).tolist() == [1, 0, 3, 2, 1]
        assert a.to_host().tolist() == [1, 0, 3, 2, 1]
    ctx = StubContext()                                                   # nothing to upload at n = 0: no byte moves
    cls(ctx, 0, host=np.zeros(0, np.float32))
    assert sum(e[3] for e in ctx.calls("upload")) == 0, ctx.log


COUNTED = [(i, a) for i, a in zip(IDS, ARRAYS) if a[2]]


@pytest.mark.parametrize("cls,dtype,sized,hosted", [a for i, a in COUNTED], ids=[i for i, a in COUNTED])
def test_to_host_of_a_counted_array(cls, dtype, sized, hosted):
    for n in (0, 1, 5):
        ctx = StubContext()
        a = cls(ctx, n)
        want = np.frombuffer(bytes(range(1, 1 + 5 * dtype.itemsize)), dtype)[:n]
        ctx.mem[a.ptr:a.ptr + want.nbytes] = want.tobytes()
        got = a.to_host()
        assert isinstance(got, np.ndarray) and got.dtype == dtype and got.shape == (n,)
        assert got.tobytes() == want.tobytes()
        assert ctx.calls("download") == ([("download", a.ptr, n * dtype.itemsize)] if n else []), ctx.log


def test_the_two_summaries_answer_values_not_arrays():
    ctx = StubContext()
    s = crc.CrcSummary(ctx)
    ctx.mem[s.ptr:s.ptr + 16] = np.array([7, 1 << 40], np.uint64).tobytes()
    got = s.to_host()
    assert got == (7, 1 << 40) and all(type(v) is int for v in got)
    assert ctx.calls("download") == [("download", s.ptr, 16)]
    ctx = StubContext()
    s = rs.DeviceSummary(ctx)
    ctx.mem[s.ptr:s.ptr + 16] = np.array([3, 1 << 33], np.uint64).tobytes()
    got = s.to_host()
    assert got.dtype == rs.SUMMARY and got.shape == () and (int(got["n_failed"]), int(got["n_corrected"])) == (3, 1 << 33)
    assert ctx.calls("download") == [("download", s.ptr, 16)]


class StubLib:
    """every function of the library, recorded by name"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def f(*args):
            self.calls.append((name, args))
            return 0
        return f


# class, its destroy function, does destroy wait for a live context
HANDLES = ((cc.ConvCode, "aeth_cc_destroy", False), (remap.Remap, "aeth_remap_destroy", True), (crc.Crc, "aeth_crc_destroy", True),
           (ldpc.Ldpc, "aeth_ldpc_destroy", True), (rs.Rs, "aeth_rs_destroy", True), (polar.Polar, "aeth_polar_destroy", True))


def handle(cls):
    obj = cls.__new__(cls)
    obj.ctx, obj._lib, obj.h = StubContext(), StubLib(), C.c_void_p(0x5500)
    return obj


@pytest.mark.parametrize("cls,destroy,bound", HANDLES, ids=[h[0].__name__ for h in HANDLES])
def test_close_twice_destroys_once(cls, destroy, bound):
    obj = handle(cls)
    lib, h = obj._lib, obj.h
    obj.close()
    assert [c[0] for c in lib.calls] == [destroy] and lib.calls[0][1][0] is h
    assert not obj.h.value
    obj.close()
    del obj
    gc.collect()
    assert [c[0] for c in lib.calls] == [destroy]
    obj = handle(cls)                                                     # dropped without close(): the same one call
    lib = obj._lib
    del obj
    gc.collect()
    assert [c[0] for c in lib.calls] == [destroy]


@pytest.mark.parametrize("cls,destroy,bound", HANDLES, ids=[h[0].__name__ for h in HANDLES])
def test_close_after_the_context_has_gone(cls, destroy, bound):
    obj = handle(cls)
    obj.ctx.h = None
    obj.close()
    assert [c[0] for c in obj._lib.calls] == ([] if bound else [destroy])
    assert not obj.h.value
    obj.close()
    assert len(obj._lib.calls) == (0 if bound else 1)


def test_an_object_whose_create_failed_has_nothing_to_destroy():
    for cls, destroy, bound in HANDLES:
        obj = cls.__new__(cls)                                            # __init__ raised before `h` was set
        obj.close()
        obj = cls.__new__(cls)
        obj.ctx, obj._lib, obj.h = StubContext(), StubLib(), C.c_void_p()  # ... or create left it null
        obj.close()
        assert not obj._lib.calls
