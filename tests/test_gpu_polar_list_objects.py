"""GPU: a `PolarList` through the trip tests/test_gpu_code_objects.py gives every code object: zero, one and G + 1
codewords of the (3, 4) code at L = 2, encoded by `Polar` and decoded back from noise-free soft values, with the record
array's type and length; close twice; an object, its records and a `pick` result dropped after their context closed."""
import gc

import numpy as np
import pytest

import aether_primitives_amd as ap
from aether_primitives_amd import polar

pytestmark = pytest.mark.gpu
U8 = np.dtype(np.uint8)


def test_zero_one_and_group_plus_one_codewords(ctx):
    msk = polar.mask(3, 4)
    enc, obj = ap.Polar(ctx, 3, msk), ap.PolarList(ctx, 3, msk, 2)
    assert (obj.n, obj.k, obj.paths) == (8, 4, 2) and obj.group >= 1
    rng = np.random.default_rng(4002)
    for count in (0, 1, obj.group + 1):
        data = rng.integers(0, 2, count * 4).astype(np.uint8)
        soft = np.where(enc.encode(data).to_host() == 0, 64, -64).astype(np.int8)
        out, rec = obj.decode(soft)
        got = out.to_host()
        assert got.shape == (count * 4,) and got.dtype == U8 and got.tobytes() == data.tobytes(), (count, got, data)
        rec = rec.to_host()
        assert rec.dtype == polar.LIST_RECORD and rec.shape == (count,)
        assert (rec["metric"][:, 0] == 0).all() and (rec["metric"][:, 1] > 0).all() and (rec["metric"][:, 2:] == polar.NONE).all()
        rows, none = obj.decode(soft, all=True, codeword=True, records=False)
        assert none is None and rows.to_host().shape == (count * 2 * 8,)
        diff = np.zeros(count * 2, np.uint64)
        picked, which = polar.pick(ctx, obj.decode(soft, all=True)[0], 4, 2, diff)
        assert picked.to_host().tobytes() == data.tobytes() and which.to_host().tolist() == [0] * count
    obj.close()
    assert not obj.h.value
    obj.close()
    enc.close()


def test_objects_dropped_after_their_context_was_closed():
    own = ap.Context(0)
    obj = ap.PolarList(own, 3, polar.mask(3, 4), 2)
    out, rec = obj.decode(np.full(8, 64, np.int8), all=True)
    picked, which = polar.pick(own, out, 4, 2, np.zeros(2, np.uint64))
    bufs = [out, rec, picked, which, polar.DeviceListRecords(own, 2), polar.DeviceWhich(own, 0)]
    assert picked.to_host().tolist() == [0] * 4 and which.to_host().tolist() == [0]
    own.sync()
    own.close()
    obj.close()
    assert not obj.h.value
    del obj, bufs, out, rec, picked, which
    gc.collect()
