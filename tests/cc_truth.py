"""numpy restatement of the three definitions of include/aether_hip.h the convolutional-code tests compare bytes with:
the encoder (aeth_cc_encode), the block-wise Viterbi decoder (aeth_cc_decode) and the soft demodulator
(aeth_demod_soft).  The decoder is vectorised over states and over the output blocks of a call."""
import numpy as np

PARITY = np.array([bin(x).count("1") & 1 for x in range(1 << 9)], np.uint8)

# (k, polys, D, A, T): the small decode shapes, run with N = 5 D + 3
SMALL_SHAPES = ((7, (0o171, 0o133), 64, 16, 24),
                (3, (0o7, 0o5), 8, 3, 5),
                (5, (0o23, 0o35), 32, 0, 10),
                (7, (0o133, 0o171, 0o165), 48, 20, 0),
                (4, (0o15, 0o17, 0o13, 0o11), 16, 7, 9),
                (6, (0o53, 0o75), 1, 10, 10))


def encode(k, polys, bits, hist=None):
    """c[n t + j] = parity(reg_t & poly[j]), reg_t = sum_{i < k} u[t - i] 2^(k - 1 - i); hist = u[-(k-1)] .. u[-1]"""
    bits = np.asarray(bits, np.uint8) & 1
    h = np.zeros(k - 1, np.uint8) if hist is None else (np.asarray(hist, np.uint8) & 1)
    assert h.size == k - 1
    u = np.concatenate([h, bits]).astype(np.uint32)             # u[t] sits at index t + k - 1
    N = bits.size
    reg = np.zeros(N, np.uint32)
    for i in range(k):
        reg |= u[k - 1 - i:k - 1 - i + N] << np.uint32(k - 1 - i)
    out = np.empty((N, len(polys)), np.uint8)
    for j, p in enumerate(polys):
        out[:, j] = PARITY[reg & np.uint32(p)]
    return out.reshape(-1)


def _signs(k, polys):
    """(2, n, S): 1 - 2 c_q(u, p_d) for destination state j, d = 0, 1"""
    S = 1 << (k - 1)
    j = np.arange(S)
    u, p0 = j >> (k - 2), (2 * j) % S
    out = np.empty((2, len(polys), S), np.int64)
    for d in (0, 1):
        reg = (u << (k - 1)) | (p0 + d)
        for q, p in enumerate(polys):
            out[d, q] = 1 - 2 * PARITY[reg & p].astype(np.int64)
    return out


def _windows(k, polys, A, vw, first_out, dlen, D, out):
    """vw: (blocks, W, n) soft values of the windows; block b writes out[first_out + b D + sd] for sd < dlen"""
    nb, W, _ = vw.shape
    S = 1 << (k - 1)
    sg = _signs(k, polys)
    j = np.arange(S)
    p0 = (2 * j) % S
    m = np.zeros((nb, S), np.int64)                               # every window starts with all metrics at 0
    dec = np.zeros((W, nb, S), bool)
    for w in range(W):
        c0 = m[:, p0] + vw[:, w, :] @ sg[0]
        c1 = m[:, p0 + 1] + vw[:, w, :] @ sg[1]
        dec[w] = c1 > c0                                          # a tie takes p0
        m = np.where(dec[w], c1, c0)
    assert np.abs(m).max(initial=0) <= 8192 * 4 * 128
    s = np.argmax(m, axis=1)                                      # the largest metric, ties to the smallest state
    rows = np.arange(nb)
    for w in range(W - 1, A - 1, -1):                             # the first A steps store no decisions
        sd = w - A                                                # the decision for step b D - T + sd is out[b D + sd]
        if sd < dlen:
            out[first_out + rows * D + sd] = s >> (k - 2)
        s = ((s << 1) & (S - 1)) | dec[w, rows, s]


def decode(k, polys, D, A, T, soft, hist=None):
    """aeth_cc_decode: out[o] = the decision for step o - T, block by block"""
    n = len(polys)
    soft = np.asarray(soft, np.int8)
    assert soft.size % n == 0
    N = soft.size // n
    h = np.zeros((A + T) * n, np.int8) if hist is None else np.asarray(hist, np.int8)
    assert h.size == (A + T) * n
    v = np.concatenate([h, soft]).astype(np.int64).reshape(-1, n)          # step t sits at row t + A + T
    out = np.zeros(N, np.uint8)
    nfull, tail = N // D, N % D
    if nfull:
        W = A + T + D
        idx = (np.arange(nfull) * D)[:, None] + np.arange(W)[None, :]      # block b: rows b D .. b D + W - 1
        _windows(k, polys, A, v[idx], 0, D, D, out)
    if tail:
        W = A + T + tail
        _windows(k, polys, A, v[None, nfull * D:nfull * D + W], nfull * D, tail, D, out)
    return out


def decode_stream(k, polys, D, A, T, soft, known_start=True):
    """ConvCode.decode_stream: +127 history, T steps of erasures behind the stream, the T leading outputs dropped"""
    n = len(polys)
    hist = np.full((A + T) * n, 127, np.int8) if known_start else None
    padded = np.concatenate([np.asarray(soft, np.int8), np.zeros(T * n, np.int8)])
    return decode(k, polys, D, A, T, padded, hist)[T:]


def demod_soft(table, sym, scale):
    """aeth_demod_soft: every operation f32 and rounded on its own; minima start at +Inf, `d < best ? d : best`"""
    table = np.asarray(table, np.complex64)
    sym = np.asarray(sym, np.complex64)
    bps = int(table.size).bit_length() - 1
    assert table.size == 1 << bps
    b = np.full((2, bps, sym.size), np.inf, np.float32)
    with np.errstate(all="ignore"):
        for idx in range(table.size):
            dre = sym.real - table.real[idx]
            dim = sym.imag - table.imag[idx]
            d = dre * dre + dim * dim
            assert d.dtype == np.float32
            for i in range(bps):
                best = b[(idx >> i) & 1, i]
                best[...] = np.where(d < best, d, best)
        L = (b[1] - b[0]) * np.float32(scale)                              # (bps, nsym)
        r = np.clip(np.rint(L), -127, 127)
    r = np.where(np.isnan(L), np.float32(0), r)
    return r.T.astype(np.int8).reshape(-1)                                 # out[bps s + i]
