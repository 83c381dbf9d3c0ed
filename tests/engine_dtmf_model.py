"""rdsp_engine_t's DTMF decoder (include/rdsp.h, "DTMF decoder"; csrc/rdsp_dtmf.h) restated in numpy: the eight tones' steps,
the decimation by 4, the gain behind the boxcar and the de-emphasis, and a per-channel object with the 168 state words that turns
the demodulated rows of a call into the key / new / lo / hi records -- the phasor by engine_sources_model.phasor, the fused
operations through fma32, the sums over the sub-chains by the tree.  Also the test signals: keyed tone pairs."""
import math

import numpy as np

import engine_tone_model as T
from engine_sources_model import M32, fma32, phasor

F32 = np.float32
BLOCK, DEC, PER_BLOCK = 128, 4, 32
TONES, SUBS, PER_SUB, RING = 8, 8, 4, 16
WORDS = 168
K_, CNT, LAST1, RUN, CUR1, MISS, NDIGITS, TBLOCKS, PL, PH = range(10)
RING_, RE, IM, E = 16, 32, 96, 160
NONE = 255
HZ = (697.0, 770.0, 852.0, 941.0, 1209.0, 1336.0, 1477.0, 1633.0)
KEYS = "123A456B789C*0#D"
DEFAULT_MIN, DEFAULT_RATIO, DEFAULT_TWIST, DEFAULT_SHARE, DEFAULT_ON, DEFAULT_OFF = 0.015, 4.0, 16.0, 0.5, 2, 2


def dphi_of(t):
    """(uint32) llround((double)(float) f_t 2^32 4 / 44100.0): half away from zero (the powers of two are exact)"""
    x = float(F32(HZ[t])) * 4294967296.0 * 4.0 / 44100.0
    r = math.floor(x)
    if x - r >= 0.5:
        r += 1
    return r & M32


def scale_of(K):
    return F32(1.0 / ((64.0 * K) * (64.0 * K)))


def escale_of(K):
    return F32(1.0 / (256.0 * K))


def boxcar_gain(hz):
    w = 3.141592653589793 * float(F32(hz)) / 44100.0
    return abs(math.sin(4.0 * w) / (4.0 * math.sin(w)))


def gain(hz, tau_us):
    """what the boxcar of 4 samples and the de-emphasis leave of a tone: float64, the operations of rdsp_engine_dtmf_gain"""
    return boxcar_gain(hz) * T.gain(hz, tau_us)


def symbol_of(key):
    return KEYS.index(key)


def tones_of(sym):
    """(low, high) in Hz"""
    return HZ[sym // 4], HZ[4 + sym % 4]


def quad(rows):
    """[..., 4 n] float32 -> [..., n]: (a0 + a1) + (a2 + a3)"""
    q = np.asarray(rows, F32).reshape(rows.shape[:-1] + (-1, 4))
    with np.errstate(all="ignore"):
        return ((q[..., 0] + q[..., 1]).astype(F32) + (q[..., 2] + q[..., 3]).astype(F32)).astype(F32)


def tree8(v):
    """[..., 8] float32 -> [...]: ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7))"""
    v = np.asarray(v, F32)
    for _ in range(3):
        v = (v[..., 0::2] + v[..., 1::2]).astype(F32)
    return v[..., 0]


def _fma(a, b, c):
    a, b, c = np.broadcast_arrays(np.asarray(a, F32), np.asarray(b, F32), np.asarray(c, F32))
    return fma32(np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c))


def keyed(keys, on, off, amp_lo=0.2, amp_hi=0.2, offset=0.0, lead=0, phase=0.3, total=None):
    """the modulating signal of a keypad: float64 [lead + len(keys) (on + off)] (or `total` samples), each key `on` samples of its
    tone pair (cut off at the end) (frequencies times 1 + offset) and `off` samples of nothing"""
    out = np.zeros(lead + len(keys) * (on + off) if total is None else total)
    t = np.arange(on)
    for k, key in enumerate(keys):
        lo, hi = tones_of(symbol_of(key))
        a = lead + k * (on + off)
        pair = (amp_lo * np.sin(2 * np.pi * lo * (1 + offset) / 44100.0 * t + phase + k) +
                amp_hi * np.sin(2 * np.pi * hi * (1 + offset) / 44100.0 * t + 2 * phase + 3 * k))
        out[a:a + on] = pair[:max(0, len(out) - a)]
    return out


def deemph_rows(u, tau_us=750.0):
    """engine_tone_model.deemph on every row of float32 [n, t] at once (a test signal, as there)"""
    u = np.asarray(u, F32)
    a = float(T.constants(5000.0, tau_us)[1])
    y, y1 = np.zeros(u.shape, F32), np.zeros(u.shape[0])
    for j in range(u.shape[1]):
        y1 = (a * (u[:, j] - y1).astype(F32).astype(np.float64) + y1).astype(F32).astype(np.float64)
        y[:, j] = y1
    return y


class Dtmf:
    """n channels; run(rows) takes the demodulated rows float32 [n, nb * 128] of a call and returns (key uint8, new uint8, lo, hi)
    [n, nb]; the 168 words a channel carry on.  The settings are per channel here (the channel's group's).  A channel with K == 0
    has zero words and the records 255 / 255 / 0 / 0."""

    def __init__(self, n, tab, K=0, min_amp=DEFAULT_MIN, ratio=DEFAULT_RATIO, twist=DEFAULT_TWIST, share=DEFAULT_SHARE, on_frames=DEFAULT_ON,
                 off_frames=DEFAULT_OFF):
        self.n, self.tab = n, np.asarray(tab, F32)
        self.w = np.zeros((n, WORDS), np.uint32)
        self.K, self.on, self.off = (np.zeros(n, np.uint32) for _ in range(3))
        self.min2, self.ratio, self.twist, self.share = (np.zeros(n, F32) for _ in range(4))
        self.dphi = np.array([dphi_of(t) for t in range(TONES)], np.uint64)
        self.set(K, min_amp, ratio, twist, share, on_frames, off_frames)

    def set(self, K=4, min_amp=DEFAULT_MIN, ratio=DEFAULT_RATIO, twist=DEFAULT_TWIST, share=DEFAULT_SHARE, on_frames=DEFAULT_ON,
            off_frames=DEFAULT_OFF, channels=slice(None)):
        self.K[channels], self.on[channels], self.off[channels] = K, on_frames, off_frames
        self.min2[channels] = F32(min_amp) * F32(min_amp)
        self.ratio[channels], self.twist[channels], self.share[channels] = F32(ratio), F32(twist), F32(share)

    def reset(self, channels=slice(None)):
        self.w[channels] = 0

    def words(self):
        return self.w.copy()

    def digits(self):
        """(n_digits uint32 [n], ring uint32 [n, 16])"""
        return self.w[:, NDIGITS].copy(), self.w[:, RING_:RING_ + RING].copy()

    def keys(self, c=0):
        """channel c's ring read as (key, t_blocks) pairs, oldest first: the last 16 at most"""
        n, ring = int(self.w[c, NDIGITS]), self.w[c, RING_:RING_ + RING]
        return [(KEYS[int(ring[k % RING]) & 0xFF], int(ring[k % RING]) >> 8) for k in range(max(0, n - RING), n)]

    def run(self, rows, reset=None, frames=None):
        """reset: channels whose group has an FM reset pending (a boolean mask or None); frames: a list that receives
        (P [n, 8], E [n], sym [n], end [n]) of every block at which a frame ended"""
        rows = np.asarray(rows, F32)
        n, nb = rows.shape[0], rows.shape[1] // BLOCK
        assert n == self.n
        d = quad(rows).reshape(n, nb, SUBS, PER_SUB)
        w = self.w
        fresh = w[:, K_] != self.K
        if reset is not None:
            fresh |= np.asarray(reset, bool)
        w[fresh] = 0
        live = self.K != 0
        w[~live] = 0
        w[live, K_] = self.K[live]
        key_rec, new_rec = np.full((n, nb), NONE, np.uint8), np.full((n, nb), NONE, np.uint8)
        lo_rec, hi_rec = np.zeros((n, nb), F32), np.zeros((n, nb), F32)
        scale = np.array([scale_of(int(k)) if k else 0 for k in self.K], F32)
        escale = np.array([escale_of(int(k)) if k else 0 for k in self.K], F32)
        re, im = (w[:, o:o + 64].copy().view(F32).reshape(n, TONES, SUBS) for o in (RE, IM))
        e = w[:, E:E + SUBS].copy().view(F32)
        cnt, run, miss, nd, tb = (w[:, k].copy() for k in (CNT, RUN, MISS, NDIGITS, TBLOCKS))
        last, cur = ((w[:, k] - np.uint32(1)) & np.uint32(0xFF) for k in (LAST1, CUR1))
        pl, ph = w[:, PL].copy().view(F32), w[:, PH].copy().view(F32)
        ring = w[:, RING_:RING_ + RING].copy()
        step = self.dphi[None, :, None]
        sub0 = (np.uint64(PER_SUB) * np.arange(SUBS, dtype=np.uint64))[None, None, :]
        rows_i = np.arange(n)
        for b in range(nb):
            for i in range(PER_SUB):
                m = np.uint64(PER_BLOCK) * cnt.astype(np.uint64)[:, None, None] + sub0 + np.uint64(i)
                c, s = phasor(self.tab, ((m * step) & np.uint64(M32)).astype(np.uint32))
                x = d[:, b, :, i]
                with np.errstate(under="ignore"):
                    re, im = _fma(x[:, None, :], c, re), _fma(x[:, None, :], s, im)
                    e = _fma(x, x, e)
            cnt = cnt + np.uint32(1)
            tb = tb + np.uint32(1)
            end = live & (cnt == self.K)
            out = np.full(n, NONE, np.uint32)
            if end.any():
                with np.errstate(under="ignore", over="ignore", invalid="ignore"):
                    R, I = tree8(re), tree8(im)
                    P = (fma32(R, R, (I * I).astype(F32)) * scale[:, None]).astype(F32)
                    En = (tree8(e) * escale).astype(F32)
                    iL, iH = np.argmax(P[:, :4], 1), 4 + np.argmax(P[:, 4:], 1)          # the lowest index of the largest
                    PLn, PHn = P[rows_i, iL], P[rows_i, iH]
                    others = np.ones((n, TONES), bool)
                    others[rows_i, iL] = False
                    others[rows_i, iH] = False
                    sec = np.where(others, P, F32(0))
                    secL, secH = sec[:, :4].max(1).astype(F32), sec[:, 4:].max(1).astype(F32)
                    ok = ((PLn >= self.min2) & (PHn >= self.min2) & (PLn >= (self.ratio * secL).astype(F32)) & (PHn >= (self.ratio * secH).astype(F32)) &
                          (PLn <= (self.twist * PHn).astype(F32)) & (PHn <= (self.twist * PLn).astype(F32)) &
                          ((PLn + PHn).astype(F32) >= (self.share * En).astype(F32)))
                sym = np.where(ok, 4 * iL + (iH - 4), NONE).astype(np.uint32)
                if frames is not None:
                    frames.append((P.copy(), En.copy(), sym.copy(), end.copy()))
                # the digit logic, on the channels whose frame ended
                s_ = sym
                run_n = np.where((s_ != NONE) & (s_ == last), run + np.uint32(1), (s_ != NONE).astype(np.uint32))
                held = cur != NONE
                match = held & (s_ == cur)
                miss_n = np.where(match, np.uint32(0), np.where(held, miss + np.uint32(1), miss))
                cur_n = np.where(held & ~match & (miss_n >= self.off), np.uint32(NONE), cur)
                emit = end & (cur_n == NONE) & (run_n >= self.on)
                cur_n = np.where(emit, s_, cur_n)
                miss_n = np.where(emit, np.uint32(0), miss_n)
                for c_ in np.flatnonzero(emit):
                    ring[c_, int(nd[c_]) % RING] = np.uint32(int(s_[c_]) | (int(tb[c_]) & 0xFFFFFF) << 8)
                nd = np.where(emit, nd + np.uint32(1), nd)
                out = np.where(emit, s_, np.uint32(NONE))
                run, last = np.where(end, run_n, run).astype(np.uint32), np.where(end, s_, last).astype(np.uint32)
                miss, cur = np.where(end, miss_n, miss).astype(np.uint32), np.where(end, cur_n, cur).astype(np.uint32)
                pl, ph = np.where(end, PLn, pl).astype(F32), np.where(end, PHn, ph).astype(F32)
                z = end[:, None, None]
                re, im = np.where(z, F32(0), re).astype(F32), np.where(z, F32(0), im).astype(F32)
                e = np.where(end[:, None], F32(0), e).astype(F32)
                cnt = np.where(end, np.uint32(0), cnt)
            key_rec[:, b] = np.where(live, cur, NONE).astype(np.uint8)
            new_rec[:, b] = np.where(live, out, NONE).astype(np.uint8)
            lo_rec[:, b], hi_rec[:, b] = np.where(live, pl, F32(0)), np.where(live, ph, F32(0))
        for o, v in ((RE, re.reshape(n, 64)), (IM, im.reshape(n, 64)), (E, e)):
            w[live, o:o + v.shape[1]] = np.ascontiguousarray(v).view(np.uint32)[live]
        w[live, RING_:RING_ + RING] = ring[live]
        for k, v in ((CNT, cnt), (LAST1, (last + np.uint32(1)) & np.uint32(0xFF)), (RUN, run), (CUR1, (cur + np.uint32(1)) & np.uint32(0xFF)), (MISS, miss),
                     (NDIGITS, nd), (TBLOCKS, tb), (PL, np.ascontiguousarray(pl).view(np.uint32)), (PH, np.ascontiguousarray(ph).view(np.uint32))):
            w[live, k] = v[live]
        return key_rec, new_rec, lo_rec, hi_rec
