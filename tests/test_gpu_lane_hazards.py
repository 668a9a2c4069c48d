"""GPU: the overlap lane orders its launches by buffer hazards (csrc/aeth_lane_hazards.h, ctx_fir_lane), not by an event
pair in front of every kernel.  Every scenario below is run twice on fresh contexts, with set_overlap(False) and with
set_overlap(True), and every buffer it touches must come out bit for bit the same; aeth_ctx_lane_counts says what the
lane spent on ordering.

FFT-2048, 64 taps, hop 1984 throughout.  A "long" launch filters 2^22 samples (about 13 us on the device), long enough
to be still running when the launches behind it are enqueued, so that a missing order would show in the bits.  These
are checks of the protocol when the race is lost, not proofs of it: tests/test_lane_hazards_host.py and a reading of
ctx_fir_lane's callers carry those."""
import numpy as np
import pytest

import aether_primitives_amd as ap
from aether_primitives_amd import Fir, HipFft, modulation
from helpers import bits_equal, rand_c64

pytestmark = pytest.mark.gpu

FFT, NTAPS, HOP = 2048, 64, 1984
LONG = 1 << 22
B3 = 3 * HOP                      # three overlap-save blocks


@pytest.fixture(scope="module")
def taps(oracle):
    return oracle.synth_lowpass_taps(NTAPS, 0.25)


def both(scenario):
    """scenario(ctx) -> (list of host arrays, anything) on a one-queue context and on one with the lane: the arrays
    agree bit for bit; returns what the lane run reported"""
    res = []
    for overlap in (False, True):
        c = ap.Context(0)
        c.set_overlap(overlap)
        assert c.overlap == overlap
        res.append(scenario(c))
        c.close()
    (want, _), (got, info) = res
    assert len(want) == len(got)
    for k, (a, b) in enumerate(zip(want, got)):
        assert a.dtype == b.dtype and a.size == b.size
        assert bits_equal(a, b) if a.dtype == np.complex64 else (a == b).all(), f"buffer {k} differs from the one-queue run"
    return info


@pytest.mark.parametrize("npairs", [3, 6])
def test_independent_chain_costs_no_packets_after_its_start(npairs, taps):
    """13 launches rotating over 3 buffer pairs (an odd set: every pair meets both lanes) and over 6 (the benchmark's
    set), three blocks and a ragged one each: launches 3 ... 13 put no event packet on either queue and join nothing."""
    n = B3 + 17

    def scenario(c):
        f = Fir(c, taps, FFT)
        assert f.hop == HOP
        ins = [c.vec(rand_c64(300 + i, n)) for i in range(npairs)]
        outs = [c.empty(n) for _ in range(npairs)]
        counts = []
        for k in range(13):
            f.filter(ins[k % npairs], out=outs[k % npairs])
            counts.append(c.lane_counts())
        return [o.to_host() for o in outs], counts

    counts = both(scenario)
    (p2, j2), (p13, j13) = counts[1], counts[12]
    print("lane counts per launch:", counts)
    assert p2 <= 2                          # at most: one record in front of the head, one wait on the other lane
    assert p13 == p2 and j13 == 0 and j2 == 0


def test_idle_context_chain_costs_no_packets_at_all(taps):
    n = B3 + 17

    def scenario(c):
        f = Fir(c, taps, FFT)
        ins = [c.vec(rand_c64(320 + i, n)) for i in range(4)]
        outs = [c.empty(n) for _ in range(4)]
        c.sync()
        before = c.lane_counts()
        for k in range(8):
            f.filter(ins[k % 4], out=outs[k % 4])
        return [o.to_host() for o in outs], (before, c.lane_counts())

    before, after = both(scenario)
    assert after == before


def _distance3(taps, last):
    """a -> b (long), c -> d, e -> f, then `last(bufs)`: a small launch that meets the long one three launches later,
    on the other lane of a plain alternation"""
    def scenario(c):
        f = Fir(c, taps, FFT)
        v = {"a": c.vec(rand_c64(400, LONG)), "b": c.empty(LONG), "c": c.vec(rand_c64(401, B3)), "d": c.empty(B3),
             "e": c.vec(rand_c64(402, B3)), "f": c.empty(B3), "g": c.empty(B3), "h": c.vec(rand_c64(403, B3))}
        c.sync()
        f.filter(v["a"], out=v["b"])
        f.filter(v["c"], out=v["d"])
        f.filter(v["e"], out=v["f"])
        last(f, v)
        counts = c.lane_counts()
        return [v[k].to_host() for k in sorted(v)], counts
    return both(scenario)


def test_read_after_write_at_distance_three(taps):
    """the consumer reads the last three blocks of what the long producer is still writing"""
    _distance3(taps, lambda f, v: f.filter(v["b"].slice(LONG - B3, LONG), out=v["g"]))


def test_write_after_read_at_distance_three(taps):
    """a small launch overwrites the last three blocks of the long launch's input"""
    _distance3(taps, lambda f, v: f.filter(v["h"], out=v["a"].slice(LONG - B3, LONG)))


def test_write_after_write_at_distance_three(taps):
    """a small launch overwrites the last three blocks of the long launch's output: its samples are the ones that stay"""
    _distance3(taps, lambda f, v: f.filter(v["h"], out=v["b"].slice(LONG - B3, LONG)))


def test_hazards_on_both_lanes_join(taps):
    """long launches on BOTH lanes, then one that reads the first's output and overwrites the second's: no lane orders
    it behind both, so the chain ends in a join -- and the next chain starts behind it"""
    def scenario(c):
        f = Fir(c, taps, FFT)
        a, b = c.vec(rand_c64(410, LONG)), c.empty(LONG)
        p, q = c.vec(rand_c64(411, LONG)), c.empty(LONG)
        e, g = c.vec(rand_c64(412, B3)), c.empty(B3)
        c.sync()
        f.filter(a, out=b)
        f.filter(p, out=q)
        j0 = c.lane_counts()[1]
        f.filter(b.slice(LONG - B3, LONG), out=q.slice(LONG - B3, LONG))
        j1 = c.lane_counts()[1]
        f.filter(e, out=g)                                                  # beside it, on the aux lane: behind the join
        f.filter(q.slice(LONG - B3, LONG), out=a.slice(0, B3))              # reads the joiner's output, overwrites a
        return [x.to_host() for x in (a, b, q, g)], (j0, j1)

    j0, j1 = both(scenario)
    assert j1 == j0 + 1


def test_upload_right_before_the_chain(taps):
    """work enqueued on the main stream before a chain stays in front of ALL its launches, the aux lane's included: an
    upload into the second launch's input, and a long device copy into it that is still running when the chain starts"""
    def scenario(c):
        f = Fir(c, taps, FFT)
        h1, h2, h3 = rand_c64(420, B3), rand_c64(421, B3), rand_c64(422, LONG)
        x1, x2, y1, y2 = c.empty(B3), c.empty(B3), c.empty(B3), c.empty(B3)
        src, x3, x4, y3, y4 = c.vec(h3), c.empty(LONG), c.vec(rand_c64(423, B3)), c.empty(B3), c.empty(B3)
        c.sync()
        c.upload(x1.ptr, h1); c.upload(x2.ptr, h2)
        f.filter(x1, out=y1)
        f.filter(x2, out=y2)                                                # aux lane
        c.sync()
        x3.vec_clone(src)                                                   # asynchronous, on the main stream
        f.filter(x4, out=y4)
        f.filter(x3.slice(LONG - B3, LONG), out=y3)                         # aux lane: the copy's last samples
        return [v.to_host() for v in (y1, y2, y3, y4)], None

    both(scenario)


def test_more_buffer_pairs_than_the_tracker_holds(taps):
    """one block and a ragged one per launch, 70 distinct pairs in one chain: a lane's record fills (32 entries), the
    chain is joined rather than a record dropped, and every output is right"""
    n, npairs = HOP + 5, 70

    def scenario(c):
        f = Fir(c, taps, FFT)
        big = c.vec(rand_c64(430, n * npairs))
        outs = c.empty(n * npairs)
        c.sync()
        j0 = c.lane_counts()[1]
        for k in range(npairs):
            f.filter(big.slice(k * n, (k + 1) * n), out=outs.slice(k * n, (k + 1) * n))
        return [outs.to_host()], c.lane_counts()[1] - j0

    assert both(scenario) >= 1


@pytest.mark.parametrize("frames", [4, 2048])
def test_writing_the_reference_signal_behind_correlate_demod(frames, taps):
    """aeth_fft_mul_ifft_demod reads `sig` in every workgroup until it ends; a launch right behind it that writes `sig`
    must wait -- with one demodulating launch in flight (same lane) and with one on each lane (a join).  frames = 4 is
    the recorded case; 2048 frames keep the kernel busy long enough for the write to matter."""
    def scenario(c):
        f = Fir(c, taps, FFT)
        fft = HipFft(c, FFT, max_batch=frames)
        mod = modulation.qpsk(c)
        fr = [c.vec(rand_c64(440 + i, frames * FFT, scale=0.5)) for i in range(3)]
        sig = c.vec(rand_c64(445, FFT))
        news = c.vec(rand_c64(446, FFT))
        bits = [modulation.DeviceBits(c, frames * FFT * 2) for _ in range(3)]
        c.sync()
        mod.correlate_demod(fft, fr[0], sig, out=bits[0])
        f.filter(news, out=sig)                                            # write-after-read on sig
        mod.correlate_demod(fft, fr[1], sig, out=bits[1])                  # reads the new sig
        mod.correlate_demod(fft, fr[2], sig, out=bits[2])                  # beside it
        f.filter(fr[0].slice(0, FFT), out=sig)                             # sig is read on both lanes now
        return [b.to_host() for b in bits] + [sig.to_host()], None

    both(scenario)


def test_stream_hand_out_and_event_in_mid_chain(taps):
    """aeth_event_record and aeth_ctx_stream in the middle of a chain are ordered behind both lanes: another context
    (its own queue) that waits for the event only sees finished outputs, and foreign work on the handed-out stream
    reads what both lanes wrote.  Long launches on both lanes in front, three blocks behind."""
    def scenario(c):
        f = Fir(c, taps, FFT)
        ins = [c.vec(rand_c64(450 + i, LONG)) for i in range(2)] + [c.vec(rand_c64(452 + i, B3)) for i in range(2)]
        outs = [c.empty(LONG), c.empty(LONG), c.empty(B3), c.empty(B3)]
        other = ap.Context(0)
        ev = c.event()
        c.sync()
        for i in range(4):
            f.filter(ins[i], out=outs[i])
        ev.record()                                                        # mid-chain: behind both lanes
        for i in (2, 3):
            f.filter(ins[i], out=outs[i])                                  # same results again; the chain goes on
        ev.sync()
        seen = []
        for o in outs[:2]:                                                 # read through a context that never joined c
            got = np.empty(B3, np.complex64)
            other.download(o.ptr + 8 * (LONG - B3), got)
            seen.append(got)
        other.close()
        for i in range(4):
            f.filter(ins[i], out=outs[i])
        foreign = ap.Context(0, stream=c.stream)                           # the hand-over, mid-chain
        assert not c.overlap                                               # parked (and never on in the one-queue run)
        from aether_primitives_amd._lib import check
        check(f._lib.aeth_vec_add(foreign.h, outs[1]._p(), LONG, outs[0]._p(), LONG))
        check(f._lib.aeth_vec_add(foreign.h, outs[3]._p(), B3, outs[2]._p(), B3))
        foreign.sync()
        summed = [np.empty(LONG, np.complex64), np.empty(B3, np.complex64)]
        foreign.download(outs[1].ptr, summed[0]); foreign.download(outs[3].ptr, summed[1])
        foreign.close()
        return seen + summed, None

    both(scenario)
