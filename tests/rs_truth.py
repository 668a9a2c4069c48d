"""A restatement of the Reed-Solomon definition of include/aether_hip.h (aeth_rs_*) that shares nothing with the
library: field products by shift-and-reduce (no tables), encoding by polynomial long division, and two decoders --
(a) an exhaustive search over all codewords by the definition, for codes with at most 4096 codewords, and (b) Euclid's
algorithm on the key equation (Sugiyama), whose candidate is accepted only when it is a codeword inside the bound, which
the definition's own count decides.  A code is a tuple (m, poly, fcr, prim, nroots, n)."""
import itertools

import numpy as np


def mul(a, b, m, poly):
    """a b in GF(2^m): shift and reduce"""
    p = 0
    while b:
        if b & 1:
            p ^= a
        b >>= 1
        a <<= 1
        if a >> m:
            a ^= poly
    return p


def power(a, e, m, poly):
    r = 1
    while e:
        if e & 1:
            r = mul(r, a, m, poly)
        a = mul(a, a, m, poly)
        e >>= 1
    return r


def inverse(a, m, poly):
    return power(a, (1 << m) - 2, m, poly)


def vmul(a, b, m, poly):
    """elementwise product of arrays (or an array and a scalar), shift and reduce"""
    a = np.array(a, np.uint32)
    b = np.broadcast_to(np.asarray(b, np.uint32), a.shape).copy()
    p = np.zeros_like(a)
    for _ in range(m):
        p ^= np.where(b & 1, a, 0).astype(np.uint32)
        b >>= 1
        a = a << 1
        a ^= np.where(a >> m, poly, 0).astype(np.uint32)
    return p


class Truth:
    def __init__(self, code):
        self.m, self.poly, self.fcr, self.prim, self.r, self.n = (int(v) for v in code)
        self.N0 = (1 << self.m) - 1
        self.k = self.n - self.r
        self.beta = power(2, self.prim, self.m, self.poly)
        self.roots = [power(self.beta, self.fcr + j, self.m, self.poly) for j in range(self.r)]
        self._all = None

    def mul(self, a, b):
        return mul(a, b, self.m, self.poly)

    # polynomials are lists, lowest coefficient first
    def generator(self):
        g = [1]
        for root in self.roots:
            g = [(g[i - 1] if i else 0) ^ (self.mul(g[i], root) if i < len(g) else 0) for i in range(len(g) + 1)]
        return g

    def encode_words(self, data):
        """[W][k] symbols -> [W][n]: data & N0, then the remainder of d(x) x^r modulo g, highest coefficient first, by
        long division on all words at once"""
        g = np.asarray(self.generator(), np.uint32)
        data = np.asarray(data, np.uint32).reshape(-1, self.k) & self.N0
        work = np.concatenate([data, np.zeros((data.shape[0], self.r), np.uint32)], axis=1)
        gdesc = g[self.r - 1::-1][None, :]                               # g is monic: subtract c g x^(...)
        for i in range(self.k):
            work[:, i + 1:i + 1 + self.r] ^= vmul(np.repeat(work[:, i:i + 1], self.r, axis=1), gdesc, self.m, self.poly)
        return np.concatenate([data, work[:, self.k:]], axis=1).astype(np.uint8)

    def encode_word(self, data):
        return [int(v) for v in self.encode_words(np.asarray(data)[None, :])[0]]

    def encode(self, data, depth=1):
        data = np.asarray(data, np.uint8).reshape(-1, self.k, depth)
        F = data.shape[0]
        words = self.encode_words(data.transpose(0, 2, 1).reshape(F * depth, self.k))
        return np.ascontiguousarray(words.reshape(F, depth, self.n).transpose(0, 2, 1)).ravel()

    def syndromes(self, words):
        """words [W][n] -> [W][r]: the word evaluated at every root, by Horner"""
        words = np.asarray(words, np.uint32) & self.N0
        S = np.zeros((words.shape[0], self.r), np.uint32)
        rt = np.asarray(self.roots, np.uint32)[None, :]
        for j in range(self.n):
            S = vmul(S, rt, self.m, self.poly) ^ words[:, j:j + 1]
        return S

    def all_codewords(self):
        assert (self.N0 + 1) ** self.k <= 4096
        if self._all is None:
            self._all = self.encode_words(np.array(list(itertools.product(range(self.N0 + 1), repeat=self.k)), np.uint8))
        return self._all

    def verdict(self, word, era, cand):
        """the definition's count for a candidate codeword: inside the bound?"""
        e = int(((cand != word) & ~era).sum())
        return 2 * e + int(era.sum()) <= self.r

    def decode_exhaustive(self, word, era=None):
        """(a): -> (n symbols, corrected, status)"""
        word = np.asarray(word, np.uint8) & self.N0
        era = np.zeros(self.n, bool) if era is None else np.asarray(era) != 0
        C = self.all_codewords()
        e = ((C != word[None, :]) & ~era[None, :]).sum(axis=1)
        hit = np.nonzero(2 * e + int(era.sum()) <= self.r)[0]
        assert hit.size <= 1, "two codewords inside the bound"
        if hit.size == 0:
            return word.copy(), 0, 1
        c = C[hit[0]]
        return c.copy(), int((c != word).sum()), 0

    # ---- (b): Euclid on the key equation ----
    def _pmul(self, a, b):
        out = [0] * (len(a) + len(b) - 1)
        for i, x in enumerate(a):
            if x:
                for j, y in enumerate(b):
                    out[i + j] ^= self.mul(x, y)
        return out

    @staticmethod
    def _deg(a):
        for i in range(len(a) - 1, -1, -1):
            if a[i]:
                return i
        return -1

    def _divmod(self, a, b):
        a = list(a)
        db = self._deg(b)
        q = [0] * max(len(a) - db, 1)
        ib = inverse(b[db], self.m, self.poly)
        while self._deg(a) >= db:
            da = self._deg(a)
            c = self.mul(a[da], ib)
            q[da - db] = c
            for i in range(db + 1):
                a[da - db + i] ^= self.mul(c, b[i])
        return q, a

    def _eval(self, p, x):
        v = 0
        for c in reversed(p):
            v = self.mul(v, x) ^ c
        return v

    def decode_euclid(self, word, era=None, S=None):
        """(b): -> (n symbols, corrected, status)"""
        word = np.asarray(word, np.uint8) & self.N0
        era = np.zeros(self.n, bool) if era is None else np.asarray(era) != 0
        f = int(era.sum())
        fail = (word.copy(), 0, 1)
        if f > self.r:
            return fail
        if S is None:
            S = self.syndromes(word[None, :])[0]
        S = [int(v) for v in S]
        if f == 0 and not any(S):
            return word.copy(), 0, 0
        X = lambda j: power(self.beta, self.n - 1 - j, self.m, self.poly)        # noqa: E731
        gamma = [1]
        for j in np.nonzero(era)[0]:
            gamma = self._pmul(gamma, [1, X(int(j))])
        T = self._pmul(S, gamma)[:self.r]                                # modified syndromes
        # r0 = x^r, r1 = T; stop when 2 deg r1 < r + f
        r0, r1 = [0] * self.r + [1], T + [0]
        t0, t1 = [0], [1]
        while 2 * self._deg(r1) >= self.r + f:
            q, rem = self._divmod(r0, r1)
            qt = self._pmul(q, t1)
            t2 = [(t0[i] if i < len(t0) else 0) ^ (qt[i] if i < len(qt) else 0) for i in range(max(len(t0), len(qt)))]
            r0, r1, t0, t1 = r1, rem, t1, t2
        if not t1[0]:
            return fail
        lam = self._pmul(t1, gamma)                                      # the errata locator, up to a constant
        omega = r1
        dl = self._deg(lam)
        dlam = [lam[i + 1] if i % 2 == 0 else 0 for i in range(dl)]     # the derivative: d/dx x^i = i x^(i-1) over GF(2)
        cand = word.copy()
        found = 0
        for j in range(self.n):
            xi = inverse(X(j), self.m, self.poly)
            if self._eval(lam, xi):
                continue
            found += 1
            den = self._eval(dlam, xi)
            if not den:
                return fail
            # e = Omega(X^-1) X^(1 - fcr) / Lambda'(X^-1)
            xf = power(X(j), (1 - self.fcr) % self.N0, self.m, self.poly)
            cand[j] ^= self.mul(self.mul(self._eval(omega, xi), xf), inverse(den, self.m, self.poly))
        if found != dl:
            return fail
        # accepted only as what the definition asks for: a codeword inside the bound
        if self.syndromes(cand[None, :]).any() or not self.verdict(word, era, cand):
            return fail
        return cand, int((cand != word).sum()), 0

    def decode(self, coded, era=None, depth=1, payload=False, exhaustive=False):
        """frames -> (bytes, corrected [W], status [W]) in the layout of aeth_rs_decode"""
        coded = np.asarray(coded, np.uint8).reshape(-1, self.n, depth)
        eras = None if era is None else np.asarray(era, np.uint8).reshape(-1, self.n, depth)
        F = coded.shape[0]
        nb = self.k if payload else self.n
        out = np.zeros((F, nb, depth), np.uint8)
        words = coded.transpose(0, 2, 1).reshape(F * depth, self.n)
        S = self.syndromes(words)
        corrected, status = np.zeros(F * depth, np.uint32), np.zeros(F * depth, np.uint32)
        for w in range(F * depth):
            f, i = divmod(w, depth)
            e = None if eras is None else eras[f, :, i]
            c, corrected[w], status[w] = self.decode_exhaustive(words[w], e) if exhaustive else self.decode_euclid(words[w], e, S[w])
            out[f, :, i] = c[:nb]
        return out.ravel(), corrected, status


def damage(rng, truth, words, weights, era_counts, overlap=False):
    """words [W][n] -> (damaged copy, erasure flags): per word `weights[w]` symbols changed at random positions outside the
    erased ones (inside them too with overlap=True) and `era_counts[w]` positions erased"""
    words = np.array(words, np.uint8)
    era = np.zeros_like(words)
    for w in range(words.shape[0]):
        pos = rng.permutation(truth.n)
        ne, nw = int(era_counts[w]), int(weights[w])
        era[w, pos[:ne]] = 1
        hit = pos[:nw] if overlap else pos[ne:ne + nw]
        for j in hit:
            words[w, j] ^= rng.integers(1, truth.N0 + 1)
    return words, era
