"""rdsp_engine_t's narrow-band FM detector (include/rdsp.h, "narrow-band FM"; csrc/rdsp_fm.h) restated in numpy: the taps from
the prototype engine_sources_model already restates, fm_atan2, the constants, and a per-channel object with state that turns
the int16 IQ rows of a call into the demodulated rows and the level rows, every fused operation through fma32.  Also the same
definition evaluated in float64, for the distance between the two."""
import numpy as np

from engine_sources_model import fma32, taps_of

F32 = np.float32
BLOCK = 128
HIST = 47            # input pairs a channel keeps, whatever W
STATE_WORDS = 50
PI, PI_2 = F32(3.14159274101257324), F32(1.57079637050628662)
C = [F32(v) for v in (0.9999961256980896, -0.3331736922264099, 0.19807817041873932, -0.132333442568779,
                      0.07962367683649063, -0.0336042158305645, 0.006811788771301508)]


def taps(W):
    """h = ddc_taps(W, 1): float32 [16 W]"""
    assert W in (2, 3)
    return taps_of(W)


def constants(deviation_hz=5000.0, tau_us=750.0):
    """(k, a) as float32"""
    k = F32(44100.0 / (6.283185307179586 * float(F32(deviation_hz))))
    a = F32(1.0 / (1.0 + 44100.0 * float(F32(tau_us)) * 1e-6))
    return k, a


def atan2(y, x):
    """fm_atan2 on float32 arrays, the operations of csrc/rdsp_fm.h in their order"""
    y, x = np.asarray(y, F32), np.asarray(x, F32)
    ax, ay = np.abs(x), np.abs(y)
    mx, mn = np.where(ax > ay, ax, ay), np.where(ax > ay, ay, ax)
    zero = mx == 0
    with np.errstate(invalid="ignore", divide="ignore", under="ignore"):
        t = (mn / np.where(zero, F32(1.0), mx)).astype(F32)
        s = (t * t).astype(F32)
        p = np.full_like(t, C[6])
        for c in C[5::-1]:
            p = fma32(p, s, np.full_like(t, c))
        r = (t * p).astype(F32)
    r = np.where(ay > ax, PI_2 - r, r).astype(F32)
    r = np.where(x < 0, PI - r, r).astype(F32)
    return np.where(zero, F32(0.0), np.copysign(r, y)).astype(F32)


class Fm:
    """n channels: run(iq) takes the int16 rows [n, t, 2] of a call and returns (y, lvl), float32 [n, t] each; the state (the
    newest 47 pairs, z[n - 1], y[n - 1]) carries on"""

    def __init__(self, n, W=2, deviation_hz=5000.0, tau_us=750.0):
        self.n = n
        self.set(W, deviation_hz, tau_us)
        self.reset()

    def set(self, W=2, deviation_hz=5000.0, tau_us=750.0):
        self.W, self.h = W, taps(W)
        self.k, self.a = constants(deviation_hz, tau_us)
        self.deemph = float(tau_us) != 0.0

    def reset(self):
        self.hist = np.zeros((self.n, HIST, 2), np.int16)
        self.z1 = np.zeros((self.n, 2), F32)
        self.y1 = np.zeros(self.n, F32)

    def words(self):
        """the state as the engine's 50 words a channel, uint32 [n, 50]"""
        w = np.zeros((self.n, STATE_WORDS), np.uint32)
        w[:, :HIST] = self.hist[..., 0].astype(np.uint16).astype(np.uint32) | (self.hist[..., 1].astype(np.uint16).astype(np.uint32) << 16)
        w[:, HIST:HIST + 2] = self.z1.view(np.uint32)
        w[:, HIST + 2] = self.y1.view(np.uint32)
        return w

    def filtered(self, iq):
        """z of a call, (zI, zQ) float32 [n, t] each, and the history renewed"""
        iq = np.asarray(iq)
        assert iq.dtype == np.int16 and iq.shape[0] == self.n and iq.shape[2] == 2
        x = np.concatenate([self.hist, iq], 1).astype(F32)
        t = iq.shape[1]
        self.hist = np.concatenate([self.hist, iq], 1)[:, -HIST:].copy()
        m = HIST + np.arange(t)
        z = [np.zeros((self.n, t), F32), np.zeros((self.n, t), F32)]
        for k in range(len(self.h)):
            hk = np.full((self.n, t), self.h[k], F32)
            for c in range(2):
                z[c] = fma32(hk, x[:, m - k, c], z[c])
        return z[0], z[1]

    def run(self, iq):
        zi, zq = self.filtered(iq)
        t = zi.shape[1]
        with np.errstate(under="ignore"):
            lvl = (np.sqrt(fma32(zi, zi, (zq * zq).astype(F32))).astype(F32) * F32(2.0 ** -15)).astype(F32)
            pi = np.concatenate([self.z1[:, :1], zi[:, :-1]], 1)
            pq = np.concatenate([self.z1[:, 1:], zq[:, :-1]], 1)
            re = fma32(zi, pi, (zq * pq).astype(F32))
            im = fma32(zq, pi, -((zi * pq).astype(F32)))
            u = np.minimum(np.maximum((atan2(im, re) * self.k).astype(F32), F32(-1.0)), F32(1.0)).astype(F32)
            self.z1 = np.stack([zi[:, -1], zq[:, -1]], 1)
            if self.deemph:
                y = np.zeros_like(u)
                y1, a = self.y1, np.full(self.n, self.a, F32)
                for j in range(t):
                    y1 = fma32(a, (u[:, j] - y1).astype(F32), y1)
                    y[:, j] = y1
            else:
                y = u
            self.y1 = y[:, -1].copy()
        return y, lvl


def run64(iq, W=2, deviation_hz=5000.0, tau_us=0.0):
    """the same definition in float64 with the float32 taps and libm's atan2, one row int16 [t, 2] from a fresh state -> (y, lvl)"""
    h = taps(W).astype(np.float64)
    x = np.concatenate([np.zeros((HIST, 2)), np.asarray(iq, np.float64)])
    t = len(iq)
    m = HIST + np.arange(t)
    z = np.zeros(t, np.complex128)
    for k in range(len(h)):
        z += h[k] * (x[m - k, 0] + 1j * x[m - k, 1])
    p = np.concatenate([[0.0], z[:-1]])
    w = z * np.conj(p)
    d = np.arctan2(w.imag, w.real)
    u = np.clip(d * (44100.0 / (6.283185307179586 * deviation_hz)), -1.0, 1.0)
    if tau_us:
        a = 1.0 / (1.0 + 44100.0 * tau_us * 1e-6)
        y, y1 = np.zeros(t), 0.0
        for j in range(t):
            y1 = y1 + a * (u[j] - y1)
            y[j] = y1
    else:
        y = u
    return y, np.abs(z) / 32768.0


def station(seed, n_blocks, deviation_hz=5000.0, tone_hz=1000.0, carrier=8000.0, noise=3.0, offset_hz=0.0):
    """a complex carrier of `carrier` counts, frequency-modulated by a tone at the deviation, in noise of `noise` counts: int16 [t, 2]"""
    r = np.random.default_rng(seed)
    t = np.arange(n_blocks * BLOCK)
    phase = (deviation_hz / tone_hz) * np.sin(2 * np.pi * tone_hz / 44100.0 * t + r.uniform(0, 6)) + 2 * np.pi * offset_hz / 44100.0 * t + r.uniform(0, 6)
    z = carrier * np.exp(1j * phase) + noise * (r.standard_normal(len(t)) + 1j * r.standard_normal(len(t)))
    return np.stack([np.clip(np.rint(z.real), -32768, 32767), np.clip(np.rint(z.imag), -32768, 32767)], 1).astype(np.int16)
