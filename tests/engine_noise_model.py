"""rdsp_engine_t's noise squelch (include/rdsp.h, "noise squelch"; csrc/rdsp_noise.h) restated in numpy float32: the taps from
the sine and I0 series engine_sources_model already restates, the block reading (one fma32 chain per computed output, the
squares by engine_meter_model's pair tree), the level by engine_meter_model.level_step, the reversed gate, and a per-channel
object with the 68 state words that turns the demodulated rows of a call into the two records.  Also the reading in float64 on
the same taps, and the test stations of the figures: a carrier under voice-band noise modulation, in noise, off centre."""
import numpy as np

from engine_fm_model import constants
from engine_meter_model import level_step
from engine_sources_model import fma32, i0, sin_halfpi

F32 = np.float32
BLOCK, PROTO, TAPS, HIST, OUT = 128, 64, 65, 64, 32
WORDS = 68
KEY, N_, OPEN, HANG, HIST0 = 0, 1, 2, 3, 4
OFF, MEASURE, GATE = 0, 1, 2
BETA = 6.0
DEFAULTS = dict(open_n=0.01, close_n=0.025, hang_blocks=8, fall=0.75, rise=0.125)


def prototype():
    """hb, float64 [64]: the difference of the windowed sincs at 8000 and 4500 Hz, Kaiser beta 6"""
    q = np.abs(2 * np.arange(PROTO) - (PROTO - 1))
    u = (3.141592653589793 * q.astype(np.float64)) / 2.0
    rho = q.astype(np.float64) / float(PROTO - 1)
    s = sin_halfpi(160 * q, 441) - sin_halfpi(90 * q, 441)
    return (s / u) * (i0(BETA * np.sqrt(1.0 - rho * rho)) / i0(BETA))


def taps(tau_us=750.0):
    """g, float32 [65]: the prototype with the inverse of the de-emphasis of tau_us folded in"""
    hb = np.concatenate([[0.0], prototype(), [0.0]])
    if float(tau_us) == 0.0:
        return hb[1:].astype(F32)
    a = float(constants(5000.0, tau_us)[1])
    r = 1.0 - a
    return ((hb[1:] - r * hb[:-1]) / a).astype(F32)


def response_db(g, hz):
    """|G| in dB at the frequencies hz, of float taps"""
    k = np.arange(len(g))
    return 20.0 * np.log10(np.maximum(np.abs(np.exp(-2j * np.pi * np.outer(np.atleast_1d(hz), k) / 44100.0) @ np.asarray(g, np.float64)), 1e-30))


def key_of(mode, W, tau_us):
    return (1 << 31) | (int(mode) << 24) | (int(W) << 16) | (1 if float(tau_us) != 0.0 else 0)


def tree32(q):
    """[..., 32] float32 -> [...]: adjacent pairs in index order, five levels"""
    q = np.asarray(q, F32)
    assert q.shape[-1] == OUT
    with np.errstate(all="ignore"):
        for _ in range(5):
            q = q[..., 0::2] + q[..., 1::2]
    return q[..., 0]


def _windows(x, nb):
    """x [n, 64 + nb * 128] -> index array [nb, 32, 65] of a[n0 + 4 j + 3 - k] in x"""
    b, j, k = np.arange(nb)[:, None, None], np.arange(OUT)[None, :, None], np.arange(TAPS)[None, None, :]
    return HIST + b * BLOCK + 4 * j + 3 - k


def outputs(g, x, nb):
    """v, float32 [n, nb, 32]: g float32 [n, 65], x float32 [n, 64 + nb * 128] (the history in front)"""
    idx = _windows(x, nb)
    v = np.zeros((x.shape[0], nb, OUT), F32)
    for k in range(TAPS):
        v = fma32(np.broadcast_to(g[:, k, None, None], v.shape), x[:, idx[..., k]], v)
    return v


def outputs64(g, x, nb):
    """the same sums in float64, and their bound's sum_k |g_k| |a[.]|: ([n, nb, 32], [n, nb, 32])"""
    idx = _windows(x, nb)
    w = x.astype(np.float64)[:, idx]
    gd = g.astype(np.float64)[:, None, None, :]
    return (w * gd).sum(-1), (np.abs(w) * np.abs(gd)).sum(-1)


def readings(v):
    with np.errstate(all="ignore"):
        return (tree32((v * v).astype(F32)) * F32(0.03125)).astype(F32)


def gate_step(N, is_open, hang, open_n, close_n, hang_blocks):
    """one channel, python scalars: the four cases of the definition -> (open, hang)"""
    if N <= open_n:
        return 1, hang_blocks
    if is_open and N <= close_n:
        return 1, hang_blocks
    if is_open and hang > 0:
        return 1, hang - 1
    return 0, hang


class Noise:
    """n channels; run(rows) takes the demodulated rows float32 [n, nb * 128] of a call and returns (noise, nopen) [n, nb]; the 68
    words a channel carry on.  set(...) are settings (per channel here: the channel's group's, W and tau_us of its set_fm)."""

    def __init__(self, n, mode=GATE, W=2, tau_us=750.0, **kw):
        self.n = n
        self.w = np.zeros((n, WORDS), np.uint32)
        self.mode, self.W, self.tau = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, F32)
        self.open_n, self.close_n, self.fall, self.rise = (np.zeros(n, F32) for _ in range(4))
        self.hang_blocks = np.zeros(n, np.int64)
        self.g = np.zeros((n, TAPS), F32)
        self.set(mode, W, tau_us, **kw)

    def set(self, mode=GATE, W=2, tau_us=750.0, channels=slice(None), **kw):
        s = dict(DEFAULTS, **kw)
        self.mode[channels], self.W[channels], self.tau[channels] = mode, W, tau_us
        self.open_n[channels], self.close_n[channels] = F32(s["open_n"]), F32(s["close_n"])
        self.fall[channels], self.rise[channels], self.hang_blocks[channels] = F32(s["fall"]), F32(s["rise"]), s["hang_blocks"]
        self.g[channels] = taps(tau_us)

    def reset(self, channels=slice(None)):
        self.w[channels] = 0

    def words(self):
        return self.w.copy()

    def keys(self):
        return np.array([key_of(m, W, t) for m, W, t in zip(self.mode, self.W, self.tau)], np.uint32)

    def run(self, rows, reset=None, nfm=None):
        """reset: channels whose group has an FM reset pending; nfm: channels whose group is in NFM (others: untouched, zero
        records) -- boolean masks or None"""
        rows = np.asarray(rows, F32)
        n, nb = rows.shape[0], rows.shape[1] // BLOCK
        assert n == self.n
        run = np.ones(n, bool) if nfm is None else np.asarray(nfm, bool).copy()
        live = run & (self.mode != OFF)
        w = self.w
        w[run & ~live] = 0
        key = self.keys()
        fresh = w[:, KEY] != key
        if reset is not None:
            fresh |= np.asarray(reset, bool)
        fresh &= live
        w[fresh] = 0
        w[fresh, N_] = F32(1.0).view(np.uint32)
        w[live, KEY] = key[live]
        x = np.concatenate([w[:, HIST0:].view(F32), rows], 1)
        nz = readings(outputs(self.g, x, nb))
        N, is_open, hang = w[:, N_].copy().view(F32), w[:, OPEN].astype(np.int64), w[:, HANG].astype(np.int64)
        noise_rec, open_rec = np.zeros((n, nb), F32), np.zeros((n, nb), np.uint8)
        for b in range(nb):
            N = np.where(live, level_step(N, nz[:, b], self.rise, self.fall), N).astype(F32)
            for c in np.flatnonzero(live):
                is_open[c], hang[c] = gate_step(N[c], is_open[c], hang[c], self.open_n[c], self.close_n[c], self.hang_blocks[c])
            noise_rec[:, b], open_rec[:, b] = np.where(live, N, F32(0)), np.where(live, is_open, 0)
        w[live, N_] = N.view(np.uint32)[live]
        w[live, OPEN], w[live, HANG] = is_open[live].astype(np.uint32), hang[live].astype(np.uint32)
        w[live, HIST0:] = x[live, -HIST:].view(np.uint32)
        return noise_rec, open_rec

    def gate(self, before, nopen_rec, nfm=None):
        """the combined records: before & nopen for the channels of a group at mode 2 (in NFM), before's own for the others"""
        on = self.mode == GATE
        if nfm is not None:
            on &= np.asarray(nfm, bool)
        return np.where(on[:, None], before & nopen_rec, before).astype(np.uint8)


def level_step_rows(N, nz, rise, fall):
    """the level over a row of readings from N: float32 [len(nz)]"""
    out = np.zeros(len(nz), F32)
    for b, v in enumerate(nz):
        N = level_step(F32(N), F32(v), F32(rise), F32(fall))
        out[b] = N
    return out


def voice_noise(seed, n, rms):
    """band-limited noise of 300 ... 3000 Hz standing in for voice: float64 [n]"""
    r = np.random.default_rng(seed)
    spec = np.fft.rfft(r.standard_normal(n))
    f = np.fft.rfftfreq(n, 1.0 / 44100.0)
    spec[(f < 300.0) | (f > 3000.0)] = 0.0
    v = np.fft.irfft(spec, n)
    return v * (rms / np.sqrt(np.mean(v * v)))


def station(seed, n_blocks, carrier=8000.0, sigma=3.0, offset_hz=0.0, rms=0.35, deviation_hz=5000.0, until=None):
    """int16 [t, 2]: a carrier of `carrier` counts (until sample `until`, if given), frequency-modulated by voice-band noise at
    `rms` of the deviation (clipped to it), offset_hz off the centre, in noise of sigma counts per component; carrier 0: an empty
    channel"""
    r = np.random.default_rng(seed)
    n = n_blocks * BLOCK
    z = sigma * (r.standard_normal(n) + 1j * r.standard_normal(n))
    if carrier:
        mod = np.clip(voice_noise(seed + 1000, n, rms), -1.0, 1.0)
        c = carrier * np.exp(1j * (2 * np.pi * deviation_hz / 44100.0 * np.cumsum(mod) + 2 * np.pi * offset_hz / 44100.0 * np.arange(n) + r.uniform(0, 6)))
        if until is not None:
            c[until:] = 0.0
        z = z + c
    return np.stack([np.clip(np.rint(z.real), -32768, 32767), np.clip(np.rint(z.imag), -32768, 32767)], 1).astype(np.int16)
