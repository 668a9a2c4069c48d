"""The numpy restatement of aeth_remap_exec and plain-loop versions of the five table builders (include/aether_hip.h,
aeth_remap_*), written from the definitions and independently of csrc/aeth_remap.hip."""
import math

import numpy as np


def in_count(map, r_in, n_out):
    map = np.asarray(map, np.int64)
    q, rem = divmod(int(n_out), map.size)
    head = map[:rem]
    head = head[head >= 0]
    return q * int(r_in) + (int(head.max()) + 1 if head.size else 0)


def remap(x, map, r_in, n_out, fill=0):
    """out[q r_out + i] = fill if map[i] < 0 else x[q r_in + map[i]], n_out bytes of x's dtype"""
    x = np.asarray(x)
    map = np.asarray(map, np.int64)
    r_out, r_in = map.size, int(r_in)
    q, rem = divmod(int(n_out), r_out)
    assert x.size >= in_count(map, r_in, n_out)
    fillv = np.array([fill & 0xff], np.uint8).view(x.dtype)[0]
    whole = np.where(map < 0, fillv, x[:q * r_in].reshape(q, r_in)[:, np.maximum(map, 0)]).reshape(-1)
    last = np.empty(rem, x.dtype)
    for i in range(rem):                                             # the partial period, element by element
        last[i] = fillv if map[i] < 0 else x[q * r_in + map[i]]
    return np.concatenate([whole.astype(x.dtype), last])


def puncture(keep):
    out = []
    for i, k in enumerate(keep):
        if int(k) & 1:
            out.append(i)
    return np.array(out, np.int32), len(keep)


def invert(map, r_in):
    inv = [-1] * int(r_in)
    for i, t in enumerate(map):
        if t >= 0 and inv[t] < 0:
            inv[t] = i
    return np.array(inv, np.int32), len(map)


def compose(a, a_in, b, b_in):
    """b applied to the output of a, by following every output of one common period back through both tables"""
    a_out, b_out = len(a), len(b)
    m = a_out * b_in // math.gcd(a_out, b_in)
    r_in, r_out = a_in * m // a_out, b_out * m // b_in
    out = []
    for o in range(r_out):
        t = b[o % b_out]
        if t < 0:
            out.append(-1)
            continue
        mid = (o // b_out) * b_in + int(t)
        s = a[mid % a_out]
        out.append(-1 if s < 0 else (mid // a_out) * a_in + int(s))
    return np.array(out, np.int32), r_in


def rows_cols(rows, cols):
    out = [0] * (rows * cols)
    for r in range(rows):
        for c in range(cols):
            out[c * rows + r] = r * cols + c
    return np.array(out, np.int32), rows * cols


def bicm16_scatter(n_cbps, n_bpsc):
    """where coded bit k goes: 802.11a 17.3.5.6, both steps"""
    s = max(n_bpsc // 2, 1)
    to = []
    for k in range(n_cbps):
        i = (n_cbps // 16) * (k % 16) + k // 16
        to.append(s * (i // s) + (i + n_cbps - (16 * i) // n_cbps) % s)
    return to


def bicm16(n_cbps, n_bpsc):
    out = [-1] * n_cbps
    for k, j in enumerate(bicm16_scatter(n_cbps, n_bpsc)):
        out[j] = k
    return np.array(out, np.int32), n_cbps
