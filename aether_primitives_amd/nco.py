"""Numerically controlled oscillator: frequency shift, tone and chirp on the device (include/aether_hip.h, aeth_nco_*).

The reference has no oscillator.  An `Nco` multiplies a stream by e^{j phi(n)} (`mix`) or writes amp * e^{j phi(n)}
(`tone`), with the phase of sample n a 64-bit integer word: w(n) = phase + n * step + n (n - 1) / 2 * rate modulo 2^64,
each word a fraction of a turn scaled by 2^64.  The output is defined bit for bit, so chunks of a stream concatenate
exactly at any stream position."""
import ctypes as C

from . import _lib
from ._lib import check
from .context import DeviceVec

_MASK = (1 << 64) - 1


class _Words(C.Structure):
    # struct aeth_nco_words
    _fields_ = [("phase", C.c_uint64), ("step", C.c_uint64), ("rate", C.c_uint64)]


def word(cycles):
    """the 64-bit word of `cycles` turns: frac(cycles) * 2^64 truncated; a negative value is its two's complement.
    Needs no context."""
    return int(_lib.load().aeth_nco_word(float(cycles)))


def word_at(words, n):
    """w(n) of the words (phase, step, rate) at stream position n.  Needs no context."""
    w = _Words(*(int(v) & _MASK for v in words))
    return int(_lib.load().aeth_nco_word_at(C.byref(w), int(n) & _MASK))


def phasor(w):
    """(cos, sin) of one word as the kernels compute it -> Python complex holding two float32 values.  Needs no context."""
    out = _lib.Cf32()
    check(_lib.load().aeth_nco_phasor(int(w) & _MASK, C.byref(out)))
    return complex(out.re, out.im)


class Nco:
    """Nco(ctx, freq, phase, rate, position): `freq` in cycles per sample, `phase` in cycles, `rate` in cycles per sample
    per sample (a chirp), each turned into a word by `word()`.  `mix` and `tone` start at stream position `position` and
    advance it by the samples they handled."""

    def __init__(self, ctx, freq=0.0, phase=0.0, rate=0.0, position=0):
        self.ctx = ctx
        self._lib = _lib.load()
        self._w = _Words(word(phase), word(freq), word(rate))
        self.position = int(position)

    @classmethod
    def from_words(cls, ctx, phase=0, step=0, rate=0, position=0):
        """the three words given as integers (taken modulo 2^64)"""
        o = cls(ctx, position=position)
        o._w = _Words(int(phase) & _MASK, int(step) & _MASK, int(rate) & _MASK)
        return o

    @property
    def words(self):
        """(phase, step, rate)"""
        return self._w.phase, self._w.step, self._w.rate

    def seek(self, position):
        self.position = int(position)
        return self

    def mix(self, x, out=None):
        """x[i] * phasor(w(position + i)) -> DeviceVec; `out=x` runs in place"""
        if not isinstance(x, DeviceVec):
            x = self.ctx.vec(x)
        if out is None:
            out = DeviceVec(self.ctx, x.n)
        if out.n != x.n:
            raise _lib.LengthMismatch(_lib.E_LEN, f"output holds {out.n} samples, input {x.n}")
        check(self._lib.aeth_nco_mix(self.ctx.h, C.byref(self._w), self.position, x._p(), out._p(), x.n))
        self.position += x.n
        return out

    def tone(self, n, amp=1.0, out=None):
        """amp * phasor(w(position + i)) for i < n -> DeviceVec"""
        n = int(n)
        if out is None:
            out = DeviceVec(self.ctx, n)
        if out.n != n:
            raise _lib.LengthMismatch(_lib.E_LEN, f"output holds {out.n} samples, {n} asked for")
        check(self._lib.aeth_nco_tone(self.ctx.h, C.byref(self._w), self.position, float(amp), out._p(), n))
        self.position += n
        return out
