"""rdsp_channelizer_t (include/rdsp.h "channelizer") restated in numpy, for tests/test_channelizer.py and
tests/test_channelizer_gpu.py: the rate, the prototype, the twiddles, the placement, and the arithmetic of a call operation for
operation (fold, then direct DFT, every fused operation an exact float32 fma) beside a float64 evaluation of the same
definition.  The float32 fma, the table of values and the prototype's design are tests/engine_sources_model.py's.  CONFIGS are
the six configurations of the tests, EDGE the accepted ones at the edges they do not reach."""
import math

import numpy as np

from engine_sources_model import F32, fma32, taps_of, values

CONFIGS = [(16, 1, 16, 4), (16, 1, 16, 3), (640, 147, 8, 2), (8000, 147, 32, 5), (8000, 147, 64, 3), (20480, 441, 32, 4)]
REFUSED = [(8000, 147, 32, 4), (2500, 441, 8, 2), (10240, 441, 32, 3)]
# the edges CONFIGS does not reach, each accepted; EDGE_FACTS has per entry Tb, T mod M after 1, 2 and 3 blocks, and why it is here
EDGE = [(320, 147, 16, 2), (640, 147, 16, 3), (2, 1, 8, 2), (4, 1, 64, 4), (4, 1, 32, 2), (64, 1, 64, 3), (1536, 49, 64, 2), (64, 1, 8, 16)]
EDGE_FACTS = [(32, (6, 13, 3), "M = 16 with T mod M != 0"),
              (32, (13, 10, 7), "M = 16 with T mod M != 0, Q1 = 441"),
              (16, (0, 0, 0), "P1 = Q1: no rate change, Tb = 2 M"),
              (16, (0, 0, 0), "Tb < M: the waves 1 to 3 fold nothing"),
              (32, (0, 0, 0), "Tb = M: one tap a chain"),
              (352, (0, 0, 0), "the top rate and the largest LDS plan"),
              (256, (44, 24, 5), "M = 64 at D2 = 2, T mod M != 0"),
              (64, (0, 0, 0), "D2 = 16")]


def rate(P, Q, D2):
    """P / (Q D2) in lowest terms"""
    g = math.gcd(P, Q)
    P, Q = P // g, Q // g
    g = math.gcd(P, Q * D2)
    return P // g, Q * D2 // g


def accepted(P, Q, M, D2):
    g = math.gcd(P, Q)
    P, Q = P // g, Q // g
    P1, Q1 = rate(P, Q, D2)
    return (Q <= 441 and Q <= P <= 64 * Q and M in (8, 16, 32, 64) and 2 <= D2 <= 64 and P1 >= Q1 and Q1 <= 441
            and 44100 * P <= 2 * M * Q * 12000 * (D2 - 1))          # fs / (2 M) + 12000 <= 12000 D2, in integers


def taps(P, Q, D2):
    """the prototype: the polyphase pass's taps at P1 / Q1 and unit gain, times 2^-15 (exact)"""
    P1, Q1 = rate(P, Q, D2)
    return taps_of(P1, Q1, 1.0) * F32(2.0 ** -15)


def twiddles(M):
    """float32 [M, 2]: the first octant of (cos, sin)(2 pi m / M) by libm in double, rounded; the rest by symmetry"""
    quarter, eighth = M // 4, M // 8
    out = np.zeros((M, 2), F32)
    for m in range(M):
        turn, rem = divmod(m, quarter)
        b = rem if rem <= eighth else quarter - rem
        a = 2.0 * 3.14159265358979323846 * float(b) / float(M)
        c, s = F32(math.cos(a)), F32(math.sin(a))
        if b == 0:
            c, s = F32(1.0), F32(0.0)
        if b == eighth:
            s = c
        if rem > eighth:
            c, s = s, c
        x, y = [(c, s), (-s, c), (-c, -s), (s, -c)][turn]
        out[m] = (x + F32(0.0), y + F32(0.0))
    return out


def place(P, Q, M, station):
    fs = (float(P) * 44100.0) / float(Q)
    spacing = fs / float(M)
    x = station / spacing
    kk = math.floor(abs(x))
    if abs(x) - kk >= 0.5:
        kk += 1
    kk = kk if x >= 0 else -kk
    return kk % M, station - float(kk) * spacing


def centre_hz(P, Q, M, k):
    return ((k + M // 2) % M - M // 2) * ((float(P) * 44100.0) / float(Q)) / float(M)


class Model:
    """the object's state and one call after another: per source the last Tb values, frac, T (kept whole; only T mod M
    enters)"""

    def __init__(self, n_sources, P, Q, M, D2):
        assert accepted(P, Q, M, D2)
        self.S, self.M, self.D2 = n_sources, M, D2
        self.P1, self.Q1 = rate(P, Q, D2)
        self.Tb = 16 * -(-self.P1 // self.Q1)
        self.hb = np.ascontiguousarray(taps(P, Q, D2).reshape(self.Tb, self.Q1).T)      # [Q1][Tb]
        self.tw = twiddles(M)
        self.reset()

    def reset(self):
        self.frac, self.T = 0, 0
        self.hist = np.zeros((self.S, self.Tb, 2), F32)

    def source_pairs(self, n_blocks):
        return (self.frac + n_blocks * 128 * self.D2 * self.P1) // self.Q1

    def _schedule(self, i):
        """(n, r) of the output instants i of the next call, in 64 bits"""
        t = self.frac + (np.asarray(i, np.int64) + 1) * self.P1
        return t // self.Q1 - 1, t % self.Q1

    def call(self, vals, n_blocks, exact=False, ks=None, at=None):
        """vals: float32 VALUES [S, >= source_pairs(n_blocks), 2] -> float32 [S M, n_out, 2]; with exact, instead (float64
        evaluation of the definition [S M, n_out, 2], the bound's A [S, n_out]) and the state does not advance; with ks, only
        those sub-bands of every source: [S len(ks), n_out, 2]; with at (an index array of output instants of this call), only
        those instants are evaluated, [S M, len(at), 2], and the state advances as for the whole call"""
        n_call, M, Tb = n_blocks * 128 * self.D2, self.M, self.Tb
        pairs = self.source_pairs(n_blocks)
        assert vals.dtype == F32 and vals.shape[0] == self.S and vals.shape[1] >= pairs
        xh = np.concatenate([self.hist, vals[:, :pairs]], 1)
        ends = self._schedule([0, n_call - 1])[0]
        assert ends[0] >= 0 and ends[1] == pairs - 1
        inst = np.arange(n_call, dtype=np.int64) if at is None else np.asarray(at, np.int64)
        assert inst.ndim == 1 and (inst.size == 0 or (inst.min() >= 0 and inst.max() < n_call))
        n, r = self._schedule(inst)
        n_out = inst.size                                          # the instants evaluated
        N = self.T + n
        ar = np.arange(n_out)
        if exact:
            v = np.zeros((self.S, n_out, M), np.complex128)
            A = np.zeros((self.S, n_out))
            for j in range(Tb):
                h = self.hb[r, j].astype(np.float64)
                x = xh[:, Tb + n - j].astype(np.float64)
                v[:, ar, (N - j) % M] += h[None, :] * (x[..., 0] + 1j * x[..., 1])
                A += np.abs(h)[None, :] * (np.abs(x[..., 0]) + np.abs(x[..., 1]))
            k = np.arange(M) if ks is None else np.asarray(ks)
            w = np.exp(-2j * np.pi * ((k[:, None] * np.arange(M)[None, :]) % M) / M)                 # [k][q]
            y = np.einsum("kq,siq->ski", w, v).reshape(self.S * len(k), n_out)
            return np.stack([y.real, y.imag], -1), A
        vi = np.zeros((self.S, n_out, M), F32)
        vq = np.zeros((self.S, n_out, M), F32)
        for j in range(Tb):
            q = (N - j) % M
            h = self.hb[r, j][None, :]
            x = xh[:, Tb + n - j]
            vi[:, ar, q] = fma32(h, x[..., 0], vi[:, ar, q])
            vq[:, ar, q] = fma32(h, x[..., 1], vq[:, ar, q])
        k = np.arange(M) if ks is None else np.asarray(ks)
        re = np.zeros((self.S, len(k), n_out), F32)
        im = np.zeros((self.S, len(k), n_out), F32)
        for q in range(M):
            c, s = self.tw[(k * q) % M, 0][None, :, None], self.tw[(k * q) % M, 1][None, :, None]
            a, b = vi[:, None, :, q], vq[:, None, :, q]
            re = fma32(c, a, re)
            re = fma32(s, b, re)
            im = fma32(c, b, im)
            im = fma32(-s, a, im)
        self.hist = xh[:, pairs:pairs + Tb].copy()
        self.frac = (self.frac + n_call * self.P1) % self.Q1
        self.T += pairs
        return np.stack([re, im], -1).reshape(self.S * len(k), n_out, 2)

    def stream(self, fmt, raw, cuts):
        """raw rows [S, pairs, 2] of format fmt from a reset, in calls of `cuts` blocks -> the calls' rows, concatenated"""
        self.reset()
        vals, at, out = values(fmt, raw), 0, []
        for nb in cuts:
            pairs = self.source_pairs(nb)
            out.append(self.call(vals[:, at:at + pairs], nb))
            at += pairs
        return np.concatenate(out, 1)
