"""rdsp_engine_t's CTCSS tone squelch (include/rdsp.h, "tone squelch"; csrc/rdsp_tone.h) restated in numpy: the step, the scale,
the de-emphasis gain, and a per-channel object with the eight state words that turns the demodulated rows of a call into the
a2 and tone records -- the phasor by engine_sources_model.phasor, the block sums by engine_meter_model.tree_sum, the one fused
operation through fma32.  Also the test signal of the figures: a tone under band-limited noise, clipped and de-emphasised."""
import math

import numpy as np

from engine_fm_model import constants
from engine_meter_model import tree_sum
from engine_sources_model import M32, fma32, phasor

F32 = np.float32
BLOCK = 128
WORDS = 8
DPHI, K_, PH, RE, IM, CNT, TONE, A2 = range(8)
DEFAULT_K, DEFAULT_ON, DEFAULT_OFF = 128, 0.04, 0.025


def dphi_of(tone_hz):
    """(uint32) llround((double)(float) tone_hz 2^32 / 44100.0): half away from zero"""
    x = float(F32(tone_hz)) * 4294967296.0 / 44100.0
    r = math.floor(x)
    if x - r >= 0.5:
        r += 1
    return r & M32


def scale_of(K):
    return F32(4.0 / ((128.0 * K) * (128.0 * K)))


def gain(tone_hz, tau_us):
    """|H| of y <- fmaf(a, u - y, y) at tone_hz, a the float32 coefficient: float64"""
    if float(tau_us) == 0.0:
        return 1.0
    a = float(constants(5000.0, tau_us)[1])
    w, r = 6.283185307179586 * float(F32(tone_hz)) / 44100.0, 1.0 - a
    return a / math.sqrt(1.0 - 2.0 * r * math.cos(w) + r * r)


def block_sums(tab, ph, dphi, a):
    """ph, dphi uint32 [n]; a float32 [n, 128] -> (Sr, Si) float32 [n]"""
    t = np.arange(BLOCK, dtype=np.uint64)[None]
    p = ((ph.astype(np.uint64)[:, None] + t * dphi.astype(np.uint64)[:, None]) & np.uint64(M32)).astype(np.uint32)
    c, s = phasor(tab, p)
    with np.errstate(under="ignore"):
        return tree_sum((a * c).astype(F32)), tree_sum((a * s).astype(F32))


class Tone:
    """n channels; run(rows) takes the demodulated rows float32 [n, nb * 128] of a call and returns (a2, tone) [n, nb]; the eight
    words a channel carry on.  set_tones / set_squelch are settings (K, on, off per channel here: the channel's group's)."""

    def __init__(self, n, tab, tone_hz=0.0, K=DEFAULT_K, on_amp=DEFAULT_ON, off_amp=DEFAULT_OFF):
        self.n, self.tab = n, np.asarray(tab, F32)
        self.w = np.zeros((n, WORDS), np.uint32)
        self.set_tones(np.broadcast_to(np.asarray(tone_hz, F32), (n,)))
        self.set_squelch(K, on_amp, off_amp)

    def set_tones(self, tone_hz, first=0):
        t = np.atleast_1d(np.asarray(tone_hz, F32))
        if not hasattr(self, "dphi"):
            self.dphi = np.zeros(self.n, np.uint32)
        self.dphi[first:first + len(t)] = [dphi_of(v) for v in t]

    def set_squelch(self, K=DEFAULT_K, on_amp=DEFAULT_ON, off_amp=DEFAULT_OFF, channels=slice(None)):
        if not hasattr(self, "K"):
            self.K, self.on2, self.off2 = np.zeros(self.n, np.uint32), np.zeros(self.n, F32), np.zeros(self.n, F32)
        self.K[channels] = K
        self.on2[channels] = F32(on_amp) * F32(on_amp)
        self.off2[channels] = F32(off_amp) * F32(off_amp)

    def reset(self, channels=slice(None)):
        self.w[channels] = 0

    def words(self):
        return self.w.copy()

    def run(self, rows, reset=None):
        """reset: channels whose group has an FM reset pending (a boolean mask or None)"""
        rows = np.asarray(rows, F32)
        n, nb = rows.shape[0], rows.shape[1] // BLOCK
        assert n == self.n
        a = rows.reshape(n, nb, BLOCK)
        w = self.w
        fresh = (w[:, DPHI] != self.dphi) | (w[:, K_] != self.K)
        if reset is not None:
            fresh |= np.asarray(reset, bool)
        w[fresh] = 0
        w[:, DPHI], w[:, K_] = self.dphi, self.K
        live = self.dphi != 0
        w[~live] = 0
        a2_rec, tone_rec = np.zeros((n, nb), F32), np.zeros((n, nb), np.uint8)
        scale = np.array([scale_of(int(k)) if k else 0 for k in self.K], F32)
        re, im, a2 = (w[:, k].copy().view(F32) for k in (RE, IM, A2))
        ph, cnt, tone = w[:, PH].copy(), w[:, CNT].copy(), w[:, TONE].copy()
        for b in range(nb):
            Sr, Si = block_sums(self.tab, ph, self.dphi, a[:, b])
            with np.errstate(under="ignore"):
                re, im = (re + Sr).astype(F32), (im + Si).astype(F32)
                ph = ((ph.astype(np.uint64) + np.uint64(BLOCK) * self.dphi.astype(np.uint64)) & np.uint64(M32)).astype(np.uint32)
                cnt = cnt + np.uint32(1)
                end = live & (cnt == self.K)
                v = (fma32(re, re, (im * im).astype(F32)) * scale).astype(F32)
            a2 = np.where(end, v, a2).astype(F32)
            tone = np.where(end, (a2 >= np.where(tone != 0, self.off2, self.on2)).astype(np.uint32), tone)
            re, im, cnt = np.where(end, F32(0), re).astype(F32), np.where(end, F32(0), im).astype(F32), np.where(end, np.uint32(0), cnt)
            a2_rec[:, b], tone_rec[:, b] = np.where(live, a2, F32(0)), np.where(live, tone, 0)
        for k, v in ((PH, ph), (RE, re.view(np.uint32)), (IM, im.view(np.uint32)), (CNT, cnt), (TONE, tone), (A2, a2.view(np.uint32))):
            w[live, k] = v[live]
        return a2_rec, tone_rec

    def gate(self, carrier_open, tone_rec):
        """the combined records: open & tone for the channels with a tone, the carrier gate's for the others"""
        return np.where((self.dphi != 0)[:, None], carrier_open & tone_rec, carrier_open).astype(np.uint8)


def amplitude(a2):
    return np.sqrt(np.asarray(a2, np.float64))


def deemph(u, tau_us=750.0):
    """the NFM de-emphasis on a float32 row from y = 0, in float32 (a test signal: the product is exact in double and the sum
    rounded twice, which is the fused operation's answer but for rare last bits -- nothing here is compared with the engine's)"""
    a = float(constants(5000.0, tau_us)[1])
    y, y1 = np.zeros(len(u), F32), 0.0
    for j, v in enumerate(np.asarray(u, F32).tolist()):
        y1 = float(F32(a * float(F32(v - y1)) + y1))
        y[j] = y1
    return y


def voice_noise(seed, n, rms=0.25):
    """band-limited noise of 300 ... 3000 Hz standing in for voice: float64 [n]"""
    r = np.random.default_rng(seed)
    spec = np.fft.rfft(r.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / 44100.0)
    spec[(f < 300.0) | (f > 3000.0)] = 0.0
    v = np.fft.irfft(spec, n)
    return v * (rms / np.sqrt(np.mean(v * v)))


def demod_row(seed, n_blocks, tone_hz=100.0, tone_amp=0.12, rms=0.25, tau_us=750.0, tone_until=None):
    """a synthetic demodulated row: a tone (until sample tone_until, if given), voice-band noise, the sum clipped to +-1, then the
    de-emphasis: float32 [n_blocks * 128]"""
    n = n_blocks * BLOCK
    t = np.arange(n)
    tone = tone_amp * np.sin(2 * np.pi * tone_hz / 44100.0 * t + 0.7)
    if tone_until is not None:
        tone[tone_until:] = 0.0
    u = np.clip(tone + (voice_noise(seed, n, rms) if rms else 0.0), -1.0, 1.0).astype(F32)
    return deemph(u, tau_us) if tau_us else u
