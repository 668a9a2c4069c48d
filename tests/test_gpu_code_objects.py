"""GPU: the six coding objects at the smallest code each accepts, through the Python classes they share a base with: a call
with zero codewords, a round trip of one codeword and of group + 1 codewords (the first count that needs a second
workgroup), close() twice, and an object dropped after its context was closed.  Seconds in total; nothing here is refused."""
import gc

import numpy as np
import pytest

import aether_primitives_amd as ap
from aether_primitives_amd import crc, ldpc, polar, rs

pytestmark = pytest.mark.gpu
U8, I8 = np.dtype(np.uint8), np.dtype(np.int8)


def soft_of(bits):
    """noise-free soft values: positive for a 0"""
    return np.where(np.asarray(bits) == 0, 64, -64).astype(np.int8)


class PolarCase:
    """n = 3, K = 4"""
    def make(self, ctx):
        return ap.Polar(ctx, 3, polar.mask(3, 4))

    def unit(self, obj):
        return 4, obj.group

    def trip(self, obj, data):
        coded = obj.encode(data)
        out, rec = obj.decode(soft_of(coded.to_host()))
        return coded, out, {"records": (rec, polar.RECORD, data.size // 4)}


class LdpcCase:
    """staircase(2, 4, z=2): N = 8, K = 4"""
    def make(self, ctx):
        return ap.Ldpc(ctx, ldpc.staircase(2, 4, z=2), 2)

    def unit(self, obj):
        return 4, obj.group

    def trip(self, obj, data):
        coded = obj.encode(data)
        out, rec = obj.decode(soft_of(coded.to_host()), payload=True)
        got = rec.to_host()
        assert (got["unsatisfied"] == 0).all()
        return coded, out, {"records": (rec, ldpc.RECORD, data.size // 4)}


class RsCase:
    """m = 3, n = 7, nroots = 2, depth 1: five data symbols of three bits"""
    def make(self, ctx):
        return ap.Rs(ctx, (3, 0xb, 0, 1, 2, 7))

    def unit(self, obj):
        return 5, obj.group

    def trip(self, obj, data):
        coded = obj.encode(data)
        out, rec, summ = obj.decode(coded, payload=True)
        got, total = rec.to_host(), summ.to_host()
        assert (got["status"] == 0).all() and (got["corrected"] == 0).all()
        assert total.dtype == rs.SUMMARY and (int(total["n_failed"]), int(total["n_corrected"])) == (0, 0)
        return coded, out, {"records": (rec, rs.RECORD, data.size // 5)}


class CrcCase:
    """r = 3, g = x^3 + x + 1, frames of five bits"""
    L = 5

    def make(self, ctx):
        return ap.Crc(ctx, 3, 0x3)

    def unit(self, obj):
        return self.L, obj.frames_per_workgroup(self.L + 3)

    def trip(self, obj, data):
        framed = obj.attach(data, self.L)
        diff, out, summ = obj.check(framed, self.L)
        assert not diff.to_host().any()
        n_bad, first_bad = summ.to_host()
        assert n_bad == 0
        assert obj.registers(data, self.L).to_host().dtype == np.uint64
        return framed, out, {"diff": (diff, np.dtype(np.uint64), data.size // self.L)}


class CcCase:
    """k = 3, n = 2, block 8: a 'codeword' is one output block"""
    def make(self, ctx):
        return ap.ConvCode(ctx, 3, (0o7, 0o5), block=8, warmup=16, traceback=16)

    def unit(self, obj):
        return 8, 64 >> (obj.k - 1)

    def trip(self, obj, data):
        coded = obj.encode(data)
        return coded, obj.decode_stream(soft_of(coded.to_host())), {}


class RemapCase:
    """the identity map of period 2"""
    def make(self, ctx):
        return ap.Remap(ctx, [0, 1], 2)

    def unit(self, obj):
        return 2, max(obj.tile, 1)

    def trip(self, obj, data):
        out = obj.exec(data)
        return out, out, {}


CASES = (PolarCase(), LdpcCase(), RsCase(), CrcCase(), CcCase(), RemapCase())
IDS = [type(c).__name__[:-4].lower() for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_zero_one_and_group_plus_one_codewords(ctx, case):
    obj = case.make(ctx)
    per, group = case.unit(obj)
    assert per >= 1 and group >= 1
    rng = np.random.default_rng(per * 1000 + group)
    for count in (0, 1, group + 1):
        data = rng.integers(0, 2, count * per).astype(np.uint8)
        mid, out, extra = case.trip(obj, data)
        for buf in (mid, out):
            got = buf.to_host()
            assert got.dtype in (U8, I8) and got.ndim == 1
        got = out.to_host()
        assert got.shape == (count * per,) and got.dtype == U8 and got.tobytes() == data.tobytes(), (count, got, data)
        for name, (arr, dtype, n) in extra.items():
            rec = arr.to_host()
            assert rec.dtype == dtype and rec.shape == (n,) and n == count, (name, count, rec)
    obj.close()
    assert not obj.h.value
    obj.close()


def test_objects_dropped_after_their_context_was_closed():
    own = ap.Context(0)
    objs = [case.make(own) for case in CASES]
    bufs = [ap.DeviceBits(own, 8, np.ones(8)), ap.DeviceSoft(own, 0), crc.DeviceU64(own, 3), crc.CrcSummary(own), ldpc.DeviceRecords(own, 2),
            rs.DeviceRecords(own, 2), rs.DeviceSummary(own), polar.DeviceFlips(own, 2, [1, polar.NONE]), polar.DeviceRecords(own, 1)]
    assert bufs[0].to_host().tolist() == [1] * 8
    own.sync()
    own.close()
    for obj in objs:
        obj.close()
        assert not obj.h.value
    del objs, bufs, obj
    gc.collect()
