"""Truth for the LFSR sequence tests: restatements of sequence::generate (reference: src/sequence.rs:47-53) for the
generator `|n, s| (sum s[n - d]) % 2`, written here and nowhere else (not the library, not the oracle).

  plain(delays, init, n)          the loop of the reference, one element at a time
  block(delays, init, n)          the same values by numpy blocks: seq[n] = XOR seq[n - 2^j d] also holds for
                                  n >= 2^j * order (over GF(2), f(x)^(2^j) = f(x^(2^j))), and with every delay >= 1024
                                  a block of 1024 elements depends only on finished ones
  py_window(delays, init, skip)   the 64 values at skip by powers of the 64 x 64 step matrix, in Python integers
  truth(regs, inits, skip, n)     XOR over the registers of their values at [skip, skip + n)"""
import numpy as np

M64 = (1 << 64) - 1


def plain(delays, init, n):
    order = max(delays)
    s = [(init >> i) & 1 for i in range(order)]
    while len(s) < n:
        k = len(s)
        v = 0
        for d in delays:
            v += s[k - d]
        s.append(v % 2)
    return np.array(s[:n], np.uint8)


def block(delays, init, n, state=None):
    """state: 64 consecutive values to continue from instead of the init bits (any 64 in a row determine the rest)"""
    order = max(delays)
    j = 0
    while (min(delays) << j) < 1024:
        j += 1
    if state is None:
        start = plain(delays, init, min(n, order << j))
    else:                                                       # the recurrence as a loop over the given 64 values
        s = [int(b) for b in state]
        while len(s) < min(n, 64 + (order << j)):
            s.append(sum(s[len(s) - d] for d in delays) % 2)
        start = np.array(s[:n], np.uint8)
    if start.size >= n:
        return start[:n]
    out = np.empty(n, np.uint8)
    out[:start.size] = start
    big = [d << j for d in delays]
    step = min(big)
    p = start.size
    while p < n:
        m = min(step, n - p)
        acc = np.zeros(m, np.uint8)
        for d in big:
            acc ^= out[p - d:p - d + m]
        out[p:p + m] = acc
        p += m
    return out


def _apply(rows, w):
    o = 0
    for r in range(64):
        o |= (bin(rows[r] & w).count("1") & 1) << r
    return o


def _square(rows):
    out = []
    for r in range(64):
        acc, bits, i = 0, rows[r], 0
        while bits:
            if bits & 1:
                acc ^= rows[i]
            bits >>= 1
            i += 1
        out.append(acc)
    return out


def py_window(delays, init, skip):
    order = max(delays)
    mask = 0
    for d in delays:
        mask |= 1 << (64 - d)
    w = ((init & ((1 << order) - 1)) << (64 - order)) & M64
    for _ in range(64 - order):
        w = (w >> 1) | ((bin(w & mask).count("1") & 1) << 63)
    rows = [1 << (r + 1) for r in range(63)] + [mask]
    while skip:
        if skip & 1:
            w = _apply(rows, w)
        skip >>= 1
        if skip:
            rows = _square(rows)
    return w


def one(delays, init, skip, n):
    """values of one register at [skip, skip + n)"""
    if skip + n <= (1 << 21):
        return block(delays, init, skip + n)[skip:]
    w = py_window(delays, init, skip)
    state = [(w >> i) & 1 for i in range(64)]
    return block(delays, 0, max(n, 64), state=state)[:n]


def truth(regs, inits, skip, n):
    acc = np.zeros(n, np.uint8)
    for delays, init in zip(regs, inits):
        acc ^= one(tuple(delays), int(init), skip, n)
    return acc


def m_sequence_bits():
    """the 127 values of delays (6, 7) from init 0x7f: one period"""
    return plain((6, 7), 0x7f, 127)
