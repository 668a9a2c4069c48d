"""GPU: the context's scratch buffers (the two staging slots of the host-slice calls, the slab of aeth_vec_stats, the
slab of aeth_corr_search) stay separate and alive while they are in use.

Four calls that each hold one or two of them are run in several orders, around a trim and around a larger size that makes
every buffer regrow; every repeat must give the bytes of the first run of the same call and size.  Nothing new is
asserted about values: an aliased or prematurely freed buffer shows as a repeat that differs.

fft_len 1024 with a 64-sample template: hop 960, so 40 000 samples are 42 blocks with a ragged last one, and their
320 000 bytes are above the zero-copy limit of the host-slice calls (256 KiB), which therefore stage on the device."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import aether_primitives_amd as ap                                        # noqa: E402
from helpers import bits_equal, rand_c64                                   # noqa: E402

pytestmark = pytest.mark.gpu
FFT_LEN, M = 1024, 64
N_SMALL, N_BIG = 40_000, 120_000


def test_scratch_users_do_not_disturb_each_other(ctx):
    ref = rand_c64(301, M)
    corr = ap.Corr(ctx, ref, FFT_LEN)
    fir = ap.Fir(ctx, rand_c64(302, M), FFT_LEN)
    assert corr.hop == 960 and corr.n_blocks(N_SMALL) == 42 and N_SMALL % corr.hop != 0
    host = {n: rand_c64(303 + n, n) for n in (N_SMALL, N_BIG)}
    dev = {n: ctx.vec(x) for n, x in host.items()}

    def search(n):
        best, rec = corr.search(dev[n], blocks=True)
        return rec.tobytes() + np.array([(best.index, best.norm, best.n_nan)], rec.dtype).tobytes()

    calls = {
        "search": search,
        "stats": lambda n: corr.correlate(dev[n]).stats().raw,
        "levels": lambda n: corr.levels(dev[n], ap.LEVEL_DB).to_host().tobytes(),
        "host_filter": lambda n: fir.filter(host[n]).tobytes(),
    }
    first = {}

    def run(n, order, trim_before=None):
        for name in order:
            if name == trim_before:
                ctx.trim()
            got = calls[name](n)
            print(f"n={n} {name}: {len(got)} bytes, {'first run' if (name, n) not in first else 'repeat'}")
            assert first.setdefault((name, n), got) == got, f"{name}, n={n}: differs from its first run (order {order})"

    run(N_SMALL, ("search", "stats", "levels", "host_filter"))
    run(N_SMALL, ("host_filter", "levels", "stats", "search"))
    run(N_BIG, ("search", "stats", "levels", "host_filter"))                  # every buffer regrows
    run(N_SMALL, ("stats", "host_filter", "search", "levels"), trim_before="search")
    run(N_BIG, ("host_filter", "search", "levels", "stats"))
    for n in (N_SMALL, N_BIG):
        want = fir.filter(dev[n]).to_host()
        assert bits_equal(np.frombuffer(first[("host_filter", n)], np.complex64), want), f"host-slice filter, n={n}"
        assert bits_equal(dev[n].to_host(), host[n])
