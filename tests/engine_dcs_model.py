"""rdsp_engine_t's DCS code squelch (include/rdsp.h, "code squelch"; csrc/rdsp_dcs.h) restated in numpy: the code words, their
rotation classes and the standard list, the bit clock's step, and a per-channel object with the 232 state words that turns the
demodulated rows of a call into the dcs / hits / word records -- the decimation by engine_tone_search_model.tree32, every sum a
float32 add in the definition's order.  Also the test signals: NRZ of a code word under voice-band noise, clipped and
de-emphasised as engine_tone_model.demod_row builds its own, and a station that carries a code for the GPU tests."""
import math

import numpy as np

import engine_tone_model as T
from engine_tone_search_model import tree32

F32 = np.float32
U32 = np.uint32
M32 = 0xFFFFFFFF
BLOCK, DEC, PER_BLOCK = 128, 32, 4
HYP, BITS = 8, 23
MASK = 0x7FFFFF
GOLAY = 0xC75
KEY, K_, CNT, DCS, H_, WORD, MS = range(7)
HDR, HYP_WORDS = 8, 5 + BITS
ACC, POS, NB, HITS, LAST, RING = range(6)
WORDS = HDR + HYP * HYP_WORDS
ANY, INVERTED = 0xFFFF, 0x8000
KEY_SET, KEY_ANY, KEY_INV, ERR_SHIFT = 1 << 31, 1 << 30, 1 << 29, 24
DEFAULT_K, DEFAULT_ERR, DEFAULT_ON, DEFAULT_OFF = 64, 1, 16, 12
BIT_RATE = 134.4
STEP = int(math.floor(BIT_RATE * 32.0 * 4294967296.0 / 44100.0 + 0.5))
STANDARD = tuple(int(s, 8) for s in (
    "023 025 026 031 032 036 043 047 051 053 054 065 071 072 073 074 114 115 116 122 125 131 132 134 143 145 152 155 156 162 165 172 174 205 "
    "212 223 225 226 243 244 245 246 251 252 255 261 263 265 266 271 274 306 311 315 325 331 332 343 346 351 356 364 365 371 411 412 413 423 "
    "431 432 445 446 452 454 455 462 464 465 466 503 506 516 523 526 532 546 565 606 612 624 627 631 632 654 662 664 703 712 723 731 732 734 "
    "743 754").split())


def parity(d):
    """the remainder of d x^11 by g; d an int or a uint32 array of 12-bit values"""
    r = np.asarray(d, np.uint64) << np.uint64(11)
    for i in range(22, 10, -1):
        r = np.where((r >> np.uint64(i)) & np.uint64(1), r ^ (np.uint64(GOLAY) << np.uint64(i - 11)), r)
    r = (r & np.uint64(0x7FF)).astype(U32)
    return int(r) if r.ndim == 0 else r


def codeword(code):
    assert 0 <= code <= 511
    d = 0x800 | code
    return parity(d) << 12 | d


def rot(w, r):
    return ((w >> r) | (w << (BITS - r))) & MASK


def canon(w):
    return min(rot(w, r) for r in range(BITS))


def rotations(w):
    """uint32 [m] -> [m, 23]"""
    w = np.asarray(w, np.uint64)[:, None]
    r = np.arange(BITS, dtype=np.uint64)[None]
    return (((w >> r) | (w << (np.uint64(BITS) - r))) & np.uint64(MASK)).astype(U32)


def popcount(x):
    x = np.asarray(x, U32)
    return sum(((x >> U32(j)) & U32(1)) for j in range(BITS)).astype(U32)


def code_of_word(word):
    """(code, inverted) as rdsp_dcs_code_of_word, or None"""
    c = canon(word)
    for inv in (0, 1):
        for code in STANDARD:
            if canon(codeword(code) ^ (MASK if inv else 0)) == c:
                return code, bool(inv)
    return None


def max_hits(K):
    return K * 1024 // 2625


def sel_of(code):
    """a channel's setting as the kernel reads it: 0, or the key without max_err"""
    code = int(code)
    if code == 0:
        return 0
    if code == ANY:
        return KEY_SET | KEY_ANY
    w = codeword(code & 0x7FFF)
    return KEY_SET | KEY_INV | (w ^ MASK) if code & INVERTED else KEY_SET | w


class Dcs:
    """n channels; run(rows) takes the demodulated rows float32 [n, nb * 128] of a call and returns (dcs uint8, hits uint8, word
    uint32) [n, nb]; the 232 words a channel carry on.  The codes are per channel; K, max_err, on_hits and off_hits are per
    channel here (the channel's group's)."""

    def __init__(self, n, codes=0, K=DEFAULT_K, max_err=DEFAULT_ERR, on_hits=DEFAULT_ON, off_hits=DEFAULT_OFF):
        self.n = n
        self.w = np.zeros((n, WORDS), U32)
        self.sel = np.zeros(n, U32)
        self.K, self.err, self.on, self.off = (np.zeros(n, U32) for _ in range(4))
        self.set_codes(np.broadcast_to(np.asarray(codes, np.uint16), (n,)))
        self.set_squelch(K, max_err, on_hits, off_hits)

    def set_codes(self, codes, first=0):
        c = np.atleast_1d(np.asarray(codes, np.uint16))
        self.sel[first:first + len(c)] = [sel_of(v) for v in c]

    def set_squelch(self, K=DEFAULT_K, max_err=DEFAULT_ERR, on_hits=DEFAULT_ON, off_hits=DEFAULT_OFF, channels=slice(None)):
        assert 8 <= K <= 512 and 0 <= max_err <= 3 and 1 <= off_hits <= on_hits <= max_hits(K)
        self.K[channels], self.err[channels], self.on[channels], self.off[channels] = K, max_err, on_hits, off_hits

    def reset(self, channels=slice(None)):
        self.w[channels] = 0

    def words(self):
        return self.w.copy()

    def keys(self):
        return np.where(self.sel != 0, self.sel | (self.err << U32(ERR_SHIFT)), 0).astype(U32)

    def _tick(self, c, p, hyp, ring):
        """hypotheses p of channels c tick (index arrays)"""
        acc, pos, nb, hits, last = hyp
        ring[c, p, pos[c, p]] = acc[c, p]
        pos[c, p] = (pos[c, p] + U32(1)) % U32(BITS)
        acc[c, p] = 0
        nb[c, p] = np.minimum(nb[c, p] + U32(1), U32(BITS))
        rg = ring[c, p]
        s = rg[:, 0].copy()
        with np.errstate(all="ignore"):
            for i in range(1, BITS):
                s = (s + rg[:, i]).astype(F32)
            thr = (s * F32(1.0 / 23.0)).astype(F32)
        order = (pos[c, p][:, None].astype(np.int64) + np.arange(BITS)[None]) % BITS
        one = np.take_along_axis(rg, order, 1) > thr[:, None]
        w = (one.astype(np.uint64) << np.arange(BITS, dtype=np.uint64)[None]).sum(1).astype(U32)
        key = self.keys()[c]
        is_any = (key & U32(KEY_ANY)) != 0
        want = key & U32(MASK)
        rw = rotations(w)
        ok_any = (parity(w & U32(0xFFF)) == (w >> U32(12))) & (((rw >> U32(9)) & U32(7)) == 4).any(1)
        ok_code = (popcount(w[:, None] ^ rotations(want)).min(1) <= self.err[c])
        match = (nb[c, p] == BITS) & np.where(is_any, ok_any, ok_code)
        matched = np.where(is_any, rw.min(1), rotations(want).min(1)).astype(U32)
        cm, pm = c[match], p[match]
        hits[cm, pm] += U32(1)
        last[cm, pm] = matched[match]

    def run(self, rows, reset=None):
        """reset: channels whose group has an FM reset pending (a boolean mask or None)"""
        rows = np.asarray(rows, F32)
        n, nb_ = rows.shape[0], rows.shape[1] // BLOCK
        assert n == self.n
        d = tree32(rows.reshape(n, nb_, PER_BLOCK, DEC))
        w = self.w
        key = self.keys()
        fresh = (w[:, KEY] != key) | (w[:, K_] != self.K)
        if reset is not None:
            fresh |= np.asarray(reset, bool)
        w[fresh] = 0
        live = self.sel != 0
        w[~live] = 0
        w[live, KEY], w[live, K_] = key[live], self.K[live]
        hw = w[:, HDR:].reshape(n, HYP, HYP_WORDS)
        acc = hw[:, :, ACC].copy().view(F32)
        pos, nb, hits, last = (hw[:, :, k].copy() for k in (POS, NB, HITS, LAST))
        ring = hw[:, :, RING:].copy().view(F32)
        cnt, dcs, H, word, ms = (w[:, k].copy() for k in (CNT, DCS, H_, WORD, MS))
        dcs_rec, hits_rec, word_rec = np.zeros((n, nb_), np.uint8), np.zeros((n, nb_), np.uint8), np.zeros((n, nb_), U32)
        hyp = (acc, pos, nb, hits, last)
        for b in range(nb_):
            for q in range(PER_BLOCK):
                with np.errstate(all="ignore"):
                    acc[live] = (acc[live] + d[live, b, q, None]).astype(F32)
                ms = ((ms.astype(np.uint64) + np.uint64(STEP)) & np.uint64(M32)).astype(U32)
                tick = live & ((ms & U32(0x1FFFFFFF)) < U32(STEP))
                c = np.flatnonzero(tick)
                if len(c):
                    self._tick(c, ((U32(8) - (ms[c] >> U32(29))) & U32(7)).astype(np.int64), hyp, ring)
            cnt = cnt + U32(1)
            end = live & (cnt == self.K)
            if end.any():
                best = np.argmax(hits, 1)                                                     # the lowest p of the largest
                Hn = hits[np.arange(n), best]
                H = np.where(end, Hn, H).astype(U32)
                dcs = np.where(end, (Hn >= np.where(dcs != 0, self.off, self.on)).astype(U32), dcs)
                word = np.where(end, np.where(Hn != 0, last[np.arange(n), best], 0), word).astype(U32)
                hits[end], last[end] = 0, 0
                cnt = np.where(end, U32(0), cnt)
            dcs_rec[:, b], hits_rec[:, b], word_rec[:, b] = np.where(live, dcs, 0), np.where(live, H, 0), np.where(live, word, 0)
        hw[live, :, ACC] = acc.view(U32)[live]
        for k, v in ((POS, pos), (NB, nb), (HITS, hits), (LAST, last)):
            hw[live, :, k] = v[live]
        hw[live, :, RING:] = ring.view(U32)[live]
        w[:, HDR:] = hw.reshape(n, -1)
        for k, v in ((CNT, cnt), (DCS, dcs), (H_, H), (WORD, word), (MS, ms)):
            w[live, k] = v[live]
        return dcs_rec, hits_rec, word_rec

    def gate(self, before_open, dcs_rec):
        """the combined records: open & dcs for the channels with a code, the gates' in front for the others"""
        return np.where((self.sel != 0)[:, None], before_open & dcs_rec, before_open).astype(np.uint8)


def nrz(word, n, phase=0.0, rate=BIT_RATE, until=None, then=None):
    """the word repeated LSB first at `rate` bit/s as +-1 per sample, float64 [n]; `phase` bits into the word at sample 0; from
    sample `until` on nothing (0), or the word `then`"""
    bit = np.floor(phase + np.arange(n) * (rate / 44100.0)).astype(np.int64) % BITS
    x = 2.0 * ((word >> bit) & 1) - 1.0
    if until is not None:
        x[until:] = 0.0 if then is None else (2.0 * ((then >> bit[until:]) & 1) - 1.0)
    return x


def demod_row(seed, n_blocks, word, amp=0.15, dc=0.1, rms=0.25, tau_us=750.0, phase=0.0, rate=BIT_RATE, until=None, then=None):
    """a synthetic demodulated row: NRZ of `word` (None: no code) at amplitude amp, a DC offset, voice-band noise of the given
    rms, the sum clipped to +-1, then the de-emphasis: float32 [n_blocks * 128]"""
    n = n_blocks * BLOCK
    x = amp * nrz(word, n, phase, rate, until, then) if word is not None else np.zeros(n)
    u = np.clip(x + dc + (T.voice_noise(seed, n, rms) if rms else 0.0), -1.0, 1.0).astype(F32)
    return T.deemph(u, tau_us) if tau_us else u


def station(seed, n_blocks, word, amp=0.15, phase=0.0, carrier=8000.0, noise=3.0, rms=0.25, offset_hz=0.0, until=None, then=None):
    """int16 [n_blocks * 128, 2]: a carrier frequency-modulated (5000 Hz peak deviation) by NRZ of `word` (None: no code) at `amp`
    of the deviation and voice-band noise of the given rms, clipped to the deviation; `noise` counts of noise"""
    r = np.random.default_rng(seed)
    n = n_blocks * BLOCK
    x = amp * nrz(word, n, phase, BIT_RATE, until, then) if word is not None else np.zeros(n)
    mod = np.clip(x + (T.voice_noise(seed, n, rms) if rms else 0.0), -1.0, 1.0)
    ph = 2 * np.pi * 5000.0 / 44100.0 * np.cumsum(mod) + 2 * np.pi * offset_hz / 44100.0 * np.arange(n)
    z = carrier * np.exp(1j * ph) + noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return np.stack([np.clip(np.rint(z.real), -32768, 32767), np.clip(np.rint(z.imag), -32768, 32767)], 1).astype(np.int16)
