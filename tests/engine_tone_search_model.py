"""rdsp_engine_t's CTCSS tone search (include/rdsp.h, "tone search"; csrc/rdsp_tone_search.h) restated in numpy: the bank's
steps and its FNV-1a key, the 32-point decimation tree, the gain behind the boxcar and the de-emphasis, and a per-channel object
with the 200 state words that turns the demodulated rows of a call into the best / a2 / next records -- the phasor by
engine_sources_model.phasor, the fused operations through fma32.  engine_meter_model and engine_tone_model stay as they are."""
import math

import numpy as np

import engine_tone_model as T
from engine_sources_model import M32, fma32, phasor

F32 = np.float32
BLOCK, DEC, PER_BLOCK = 128, 32, 4
MAX_TONES = 64
WORDS = 200
K_, KEY, CNT, BEST1, A2, NEXT = range(6)
RE, IM, P = 8, 72, 136
NONE = 255
DEFAULT_MIN, DEFAULT_RATIO = 0.04, 4.0
STANDARD = (67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8, 123.0, 127.3,
            131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9, 183.5, 186.2, 189.9, 192.8,
            196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1)


def dphi_of(tone_hz):
    """(uint32) llround((double)(float) tone_hz 2^32 32 / 44100.0): half away from zero (the powers of two are exact)"""
    x = float(F32(tone_hz)) * 4294967296.0 * 32.0 / 44100.0
    r = math.floor(x)
    if x - r >= 0.5:
        r += 1
    return r & M32


def bank_key(dphi):
    """32-bit FNV-1a over the little-endian bytes of n_tones and every step; 0 is replaced by 1"""
    h = 2166136261
    for w in [len(dphi)] + [int(v) for v in dphi]:
        for k in range(4):
            h = ((h ^ ((w >> (8 * k)) & 0xff)) * 16777619) & M32
    return h or 1


def boxcar_gain(tone_hz):
    w = 3.141592653589793 * float(F32(tone_hz)) / 44100.0
    return abs(math.sin(32.0 * w) / (32.0 * math.sin(w)))


def gain(tone_hz, tau_us):
    """what the boxcar of 32 samples and the de-emphasis leave of a tone: float64, the operations of rdsp_engine_tone_search_gain"""
    return boxcar_gain(tone_hz) * T.gain(tone_hz, tau_us)


def tree32(q):
    """[..., 32] float32 -> [...]: adjacent pairs in index order, five levels"""
    q = np.asarray(q, F32)
    assert q.shape[-1] == DEC
    with np.errstate(all="ignore"):
        for _ in range(5):
            q = q[..., 0::2] + q[..., 1::2]
    return q[..., 0]


def _fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    return fma32(np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c))


class Search:
    """n channels; run(rows) takes the demodulated rows float32 [n, nb * 128] of a call and returns (best uint8, a2, next) [n, nb];
    the 200 words a channel carry on.  The bank is the engine's; K, min_amp and ratio are per channel here (the channel's
    group's).  A channel with K == 0 has zero words and the records 255 / 0 / 0."""

    def __init__(self, n, tab, bank=STANDARD, K=0, min_amp=DEFAULT_MIN, ratio=DEFAULT_RATIO):
        self.n, self.tab = n, np.asarray(tab, F32)
        self.w = np.zeros((n, WORDS), np.uint32)
        self.K, self.min2, self.ratio = np.zeros(n, np.uint32), np.zeros(n, F32), np.zeros(n, F32)
        self.set_bank(bank)
        self.set_search(K, min_amp, ratio)

    def set_bank(self, hz):
        hz = np.atleast_1d(np.asarray(hz, F32))
        assert 1 <= len(hz) <= MAX_TONES and np.all(np.diff(hz) > 0) and hz[0] >= 60 and hz[-1] <= 300
        self.n_tones = len(hz)
        self.dphi = np.zeros(MAX_TONES, np.uint32)
        self.dphi[:len(hz)] = [dphi_of(v) for v in hz]
        self.key = bank_key(self.dphi[:len(hz)])

    def set_search(self, K=128, min_amp=DEFAULT_MIN, ratio=DEFAULT_RATIO, channels=slice(None)):
        self.K[channels] = K
        self.min2[channels] = F32(min_amp) * F32(min_amp)
        self.ratio[channels] = F32(ratio)

    def reset(self, channels=slice(None)):
        self.w[channels] = 0

    def words(self):
        return self.w.copy()

    def spectrum(self):
        return self.w[:, P:P + self.n_tones].copy().view(F32)

    def run(self, rows, reset=None):
        """reset: channels whose group has an FM reset pending (a boolean mask or None)"""
        rows = np.asarray(rows, F32)
        n, nb, nt = rows.shape[0], rows.shape[1] // BLOCK, self.n_tones
        assert n == self.n
        d = tree32(rows.reshape(n, nb, PER_BLOCK, DEC))
        w = self.w
        fresh = (w[:, K_] != self.K) | (w[:, KEY] != np.uint32(self.key))
        if reset is not None:
            fresh |= np.asarray(reset, bool)
        w[fresh] = 0
        live = self.K != 0
        w[~live] = 0
        w[live, K_], w[live, KEY] = self.K[live], self.key
        best_rec, a2_rec, next_rec = np.full((n, nb), NONE, np.uint8), np.zeros((n, nb), F32), np.zeros((n, nb), F32)
        scale = np.array([T.scale_of(int(k)) if k else 0 for k in self.K], F32)
        re, im, pw = (w[:, o:o + nt].copy().view(F32) for o in (RE, IM, P))
        cnt, best1 = w[:, CNT].copy(), w[:, BEST1].copy()
        a2, nxt = w[:, A2].copy().view(F32), w[:, NEXT].copy().view(F32)
        step = self.dphi[None, :nt].astype(np.uint64)
        idx = np.arange(nt)[None]
        for b in range(nb):
            for q in range(PER_BLOCK):
                m = (np.uint64(PER_BLOCK) * cnt.astype(np.uint64) + np.uint64(q))[:, None]
                c, s = phasor(self.tab, ((m * step) & np.uint64(M32)).astype(np.uint32))
                with np.errstate(under="ignore"):
                    re, im = _fma(d[:, b, q, None], c, re), _fma(d[:, b, q, None], s, im)
            cnt = cnt + np.uint32(1)
            end = live & (cnt == self.K)
            if end.any():
                with np.errstate(under="ignore"):
                    v = (fma32(re, re, (im * im).astype(F32)) * scale[:, None]).astype(F32)
                    i = np.argmax(v, 1)                                              # the lowest index of the largest
                    pi = v[np.arange(n), i]
                    far = np.abs(idx - i[:, None]) > 1
                    nx = np.where(far, v, F32(0)).max(1).astype(F32)
                    found = (pi >= self.min2) & (pi >= (self.ratio * nx).astype(F32))
                pw = np.where(end[:, None], v, pw).astype(F32)
                best1 = np.where(end, np.where(found, i + 1, 0), best1).astype(np.uint32)
                a2, nxt = np.where(end, pi, a2).astype(F32), np.where(end, nx, nxt).astype(F32)
                re, im = np.where(end[:, None], F32(0), re).astype(F32), np.where(end[:, None], F32(0), im).astype(F32)
                cnt = np.where(end, np.uint32(0), cnt)
            best_rec[:, b] = np.where(live, (best1 - np.uint32(1)).astype(np.uint8), NONE)
            a2_rec[:, b], next_rec[:, b] = np.where(live, a2, F32(0)), np.where(live, nxt, F32(0))
        for o, v in ((RE, re), (IM, im), (P, pw)):
            w[live, o:o + nt] = np.ascontiguousarray(v).view(np.uint32)[live]
        for k, v in ((CNT, cnt), (BEST1, best1), (A2, a2.view(np.uint32)), (NEXT, nxt.view(np.uint32))):
            w[live, k] = v[live]
        return best_rec, a2_rec, next_rec
