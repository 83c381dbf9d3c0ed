"""rdsp_engine_t's AFSK 1200 packet decoder (include/rdsp.h, "AFSK 1200 packet decoder"; csrc/rdsp_afsk.h) restated in numpy:
the steps, the decimation by 4, the two correlators over their window of 12 (vectorised over the samples and the channels: the
phasor by engine_sources_model.phasor, the fused operations through fma32, the sums in the definition's order), and a per-channel
object with the 448 state words whose bit clock, HDLC machine and frame ring are plain Python integers walked sample by sample.
Also the test signals: HDLC bit streams (flags, stuffing, aborts, shared flags), NRZI and continuous-phase Bell 202 audio."""
import math

import numpy as np

import engine_dtmf_model as D
from engine_sources_model import M32, fma32, phasor

F32 = np.float32
BLOCK, DEC, PER_BLOCK, WINDOW, HIST = 128, 4, 32, 12, 11
WORDS, BUF_WORDS, RING, SLOT_WORDS = 448, 84, 4, 84
ON, PLL, PREV_RAW, PREV_SAMPLED, ONES, INFRAME, BYTE, NB, NBYTES, CRC, NFRAMES, NBAD, TBLOCKS = range(13)
HIST_, BUF, RING_ = 16, 28, 112
MAX_BYTES, MIN_BYTES = 330, 9
MARK, SPACE, BAUD = 1200.0, 2200.0, 1200.0
DEFAULT_GAIN, DEFAULT_PULL, DEFAULT_MIN_BYTES = 1.0, 2, 17
RESIDUE = 0xF0B8
FLAG = [0, 1, 1, 1, 1, 1, 1, 0]


def dphi_of(hz):
    """(uint32) llround((double)(float) hz 2^32 4 / 44100.0): half away from zero (the powers of two are exact)"""
    x = float(F32(hz)) * 4294967296.0 * 4.0 / 44100.0
    r = math.floor(x)
    if x - r >= 0.5:
        r += 1
    return r & M32


STEP, DPHI_MARK, DPHI_SPACE = dphi_of(BAUD), dphi_of(MARK), dphi_of(SPACE)
LSCALE = F32(1.0 / (32.0 * 24.0 * 24.0))


def space_gain(tau_us):
    """(dtmf_gain(1200) / dtmf_gain(2200))^2 in float64, the operations of rdsp_engine_afsk_space_gain"""
    r = D.gain(MARK, tau_us) / D.gain(SPACE, tau_us)
    return r * r


def crc_byte(crc, byte):
    crc ^= byte & 0xFF
    for _ in range(8):
        crc = (crc >> 1) ^ (0x8408 if crc & 1 else 0)
    return crc


def fcs(data):
    """CRC-16/X-25 of the bytes: what AX.25 appends, low byte first"""
    crc = 0xFFFF
    for b in bytes(data):
        crc = crc_byte(crc, b)
    return crc ^ 0xFFFF


def with_fcs(data):
    f = fcs(data)
    return bytes(data) + bytes([f & 0xFF, f >> 8])


# ---- test signals ----

def byte_bits(data):
    """the bytes' bits, least significant first, not stuffed"""
    return [(b >> k) & 1 for b in bytes(data) for k in range(8)]


def stuffed(data):
    """the bytes' bits, least significant first, a zero behind every five ones"""
    out, ones = [], 0
    for bit in byte_bits(data):
        out.append(bit)
        ones = ones + 1 if bit else 0
        if ones == 5:
            out.append(0)
            ones = 0
    return out


def frame_bits(payload, flags_before=2, flags_after=1):
    """flags, the payload with its FCS stuffed, flags: one frame as HDLC bits"""
    return FLAG * flags_before + stuffed(with_fcs(payload)) + FLAG * flags_after


def nrzi(bits, level=1):
    """a zero toggles the tone, a one keeps it: -> the tone of every bit (1: mark)"""
    out = []
    for b in bits:
        if not b:
            level ^= 1
        out.append(level)
    return out


def audio(levels, amp=0.3, ppm=0.0, tone_off=0.0, phase=0.0, lead=0, total=None, space_boost=1.0):
    """continuous-phase Bell 202 at the 44.1 kHz tap: float64, `lead` samples of nothing, then every level for 44100 / (1200 (1 +
    ppm 1e-6)) samples at 1200 or 2200 Hz (times 1 + tone_off), the space tone space_boost times the mark's amplitude (a sender
    that pre-emphasises), padded with nothing or cut to `total` samples"""
    per = 44100.0 / (BAUD * (1.0 + ppm * 1e-6))
    n = int(math.ceil(len(levels) * per))
    which = np.minimum((np.arange(n) / per).astype(np.int64), len(levels) - 1)
    mark = np.asarray(levels, np.int64)[which] == 1
    f = np.where(mark, MARK, SPACE) * (1.0 + tone_off)
    x = amp * np.where(mark, 1.0, space_boost) * np.sin(phase + 2.0 * np.pi * np.cumsum(f) / 44100.0)
    out = np.zeros(lead + n if total is None else total)
    k = min(n, len(out) - lead)
    out[lead:lead + k] = x[:k]
    return out


def packet_audio(payloads, gap_flags=8, **kw):
    """frames one after the other, each between flags of its own, through nrzi and audio"""
    bits = []
    for p in payloads:
        bits += frame_bits(p, flags_before=gap_flags, flags_after=2)
    return audio(nrzi(bits), **kw)


# ---- the definition ----

def _f(x):
    return np.asarray(x, F32)


def _quad(a, b, c, d):
    with np.errstate(all="ignore"):
        return _f(_f(a + b) + _f(c + d))


def _group(t):
    """up to four terms, oldest first, as dtmf_quad adds them (a missing term is left out, not added as a zero)"""
    with np.errstate(all="ignore"):
        if len(t) == 4:
            return _quad(*t)
        out = t[0]
        for v in t[1:]:
            out = _f(out + v)
        return out


def stage12(tab, rows, hist, t_blocks, g, window=WINDOW):
    """rows float32 [n, nb 128], hist float32 [n, 11], t_blocks uint32 [n], g float32 [n] -> (raw uint8 [n, nb 32], lvl float32
    [n, nb], the next hist [n, 11]).  window: the build's is 12; a shorter one, for the figures that the choice of 12 rests on,
    sums the newest `window` products in groups of four, oldest first, the groups from the left (12: (q0 + q1) + q2)"""
    assert 1 <= window <= WINDOW
    rows = _f(rows)
    n, N = rows.shape[0], rows.shape[1] // DEC
    d = D.quad(rows)
    ext = np.concatenate([_f(hist), d], 1)                                                   # d[m0 - 11 ... m0 + N - 1]
    m = (np.uint64(PER_BLOCK) * t_blocks.astype(np.uint64)[:, None] + np.arange(N + HIST, dtype=np.uint64)[None, :] + np.uint64((1 << 32) - HIST)) & np.uint64(M32)
    S = []
    with np.errstate(under="ignore"):
        for dphi in (DPHI_MARK, DPHI_SPACE):
            c, s = phasor(tab, ((m * np.uint64(dphi)) & np.uint64(M32)).astype(np.uint32))
            for comp in (c, s):
                p = _f(ext * comp)
                t = [p[:, k:k + N] for k in range(WINDOW - window, WINDOW)]
                S.append(_group([_group(t[i:i + 4]) for i in range(0, window, 4)]))
        Pm = fma32(np.ascontiguousarray(S[0]), np.ascontiguousarray(S[0]), _f(S[1] * S[1]))
        Ps = fma32(np.ascontiguousarray(S[2]), np.ascontiguousarray(S[2]), _f(S[3] * S[3]))
        gp = _f(_f(g)[:, None] * Ps)
        raw = (_f(Pm - gp) > 0).astype(np.uint8)
        v = _f(Pm + gp).reshape(n, -1, PER_BLOCK)
        for _ in range(5):
            v = _f(v[..., 0::2] + v[..., 1::2])
        lvl = _f(v[..., 0] * LSCALE)
    return raw, lvl, ext[:, N:].copy()


def machine(w, raw, pull, min_bytes, trace=None):
    """stages 3 to 5 of one channel: w its 448 words (changed in place), raw the call's decisions (a list of nb 32 integers) ->
    (sync, new, bad) lists of the call's blocks; trace receives (m, good) of every frame a flag closed, m the sample's index
    since the detector's start"""
    pll, prev_raw, prev_sampled, ones, inframe, byte, nb, nbytes, crc, n_frames, n_bad, t_blocks = (int(v) for v in w[PLL:TBLOCKS + 1])
    buf = bytearray(w[BUF:BUF + BUF_WORDS].astype("<u4").tobytes())
    sync, new, bad = [], [], []
    for b in range(len(raw) // PER_BLOCK):
        fresh = wrong = 0
        for at, r in enumerate(raw[b * PER_BLOCK:(b + 1) * PER_BLOCK]):
            if r != prev_raw:
                sp = pll - (1 << 32) if pll & 0x80000000 else pll
                pll = (sp - (sp >> pull)) & M32
                prev_raw = r
            old = pll
            pll = (pll + STEP) & M32
            if not (old < 0x80000000 <= pll):
                continue
            bit = r == prev_sampled
            prev_sampled = r
            if bit:
                ones = min(ones + 1, 7)
                if ones >= 7:
                    inframe = 0
                elif inframe:
                    byte |= 1 << nb
                    nb += 1
            else:
                if ones == 6:
                    if inframe and nb == 7 and nbytes >= min_bytes:
                        if trace is not None:
                            trace.append((PER_BLOCK * t_blocks + at, crc == RESIDUE))
                        if crc == RESIDUE:
                            assert fcs(buf[:nbytes - 2]) == buf[nbytes - 2] | buf[nbytes - 1] << 8   # the two statements of "FCS good"
                            length = nbytes - 2
                            slot = np.zeros(SLOT_WORDS, np.uint32)
                            slot[0], slot[1] = length, t_blocks + 1
                            slot[2:] = np.frombuffer(bytes(buf[:length]) + bytes(4 * (SLOT_WORDS - 2) - length), "<u4")
                            w[RING_ + (n_frames % RING) * SLOT_WORDS:RING_ + (n_frames % RING + 1) * SLOT_WORDS] = slot
                            n_frames = (n_frames + 1) & M32
                            fresh += 1
                        else:
                            n_bad = (n_bad + 1) & M32
                            wrong += 1
                    inframe, nbytes, byte, nb, crc = 1, 0, 0, 0, 0xFFFF
                elif ones != 5 and inframe:
                    nb += 1
                ones = 0
            if inframe and nb == 8:
                buf[nbytes] = byte
                nbytes += 1
                crc = crc_byte(crc, byte)
                byte = nb = 0
                if nbytes > MAX_BYTES:
                    inframe = 0
        t_blocks = (t_blocks + 1) & M32
        sync.append(inframe)
        new.append(fresh)
        bad.append(wrong)
    w[PLL:TBLOCKS + 1] = [pll, prev_raw, prev_sampled, ones, inframe, byte, nb, nbytes, crc, n_frames, n_bad, t_blocks]
    w[BUF:BUF + BUF_WORDS] = np.frombuffer(bytes(buf), "<u4")
    return sync, new, bad


class Afsk:
    """n channels; run(rows) takes the demodulated rows float32 [n, nb * 128] of a call and returns (sync uint8, new uint8, bad
    uint8, lvl float32) [n, nb]; the 448 words a channel carry on.  The settings are per channel here (the channel's group's).
    A channel with on == 0 has zero words and zero records."""

    def __init__(self, n, tab, on=0, space_gain=DEFAULT_GAIN, pull=DEFAULT_PULL, min_bytes=DEFAULT_MIN_BYTES, window=WINDOW):
        self.n, self.tab, self.window = n, np.asarray(tab, F32), window                     # window: stage12's, 12 in the build
        self.w = np.zeros((n, WORDS), np.uint32)
        self.on, self.pull, self.min_bytes = (np.zeros(n, np.uint32) for _ in range(3))
        self.g = np.zeros(n, F32)
        self.set(on, space_gain, pull, min_bytes)

    def set(self, on=1, space_gain=DEFAULT_GAIN, pull=DEFAULT_PULL, min_bytes=DEFAULT_MIN_BYTES, channels=slice(None)):
        self.on[channels], self.pull[channels], self.min_bytes[channels], self.g[channels] = on, pull, min_bytes, F32(space_gain)

    def reset(self, channels=slice(None)):
        self.w[channels] = 0

    def words(self):
        return self.w.copy()

    def ring(self):
        """(n_frames uint32 [n], ring uint32 [n, 4, 84])"""
        return self.w[:, NFRAMES].copy(), self.w[:, RING_:].reshape(self.n, RING, SLOT_WORDS).copy()

    def frames(self, c=0):
        """channel c's ring read as (t_blocks, bytes) pairs, oldest first: the last four at most"""
        n, ring = int(self.w[c, NFRAMES]), self.w[c, RING_:].reshape(RING, SLOT_WORDS)
        return [(int(ring[k % RING, 1]), ring[k % RING, 2:].astype("<u4").tobytes()[:int(ring[k % RING, 0])]) for k in range(max(0, n - RING), n)]

    def run(self, rows, reset=None, raws=None, trace=None):
        """reset: channels whose group has an FM reset pending (a boolean mask or None); raws: a list that receives raw [n, nb 32];
        trace: a list that receives channel 0's (m, good) of machine()"""
        rows = np.asarray(rows, F32)
        n, nb = rows.shape[0], rows.shape[1] // BLOCK
        assert n == self.n
        w = self.w
        fresh = w[:, ON] != self.on
        if reset is not None:
            fresh |= np.asarray(reset, bool)
        w[fresh] = 0
        live = self.on != 0
        w[~live] = 0
        w[live, ON] = 1
        raw, lvl, hist = stage12(self.tab, rows, w[:, HIST_:HIST_ + HIST].copy().view(F32), w[:, TBLOCKS], self.g, self.window)
        if raws is not None:
            raws.append(raw)
        sync, new, bad = (np.zeros((n, nb), np.uint8) for _ in range(3))
        for c in np.flatnonzero(live):
            s, f, b = machine(w[c], raw[c].tolist(), int(self.pull[c]), int(self.min_bytes[c]), trace if c == 0 else None)
            sync[c], new[c], bad[c] = s, np.array(f) & 0xFF, np.array(b) & 0xFF
        w[live, HIST_:HIST_ + HIST] = np.ascontiguousarray(hist).view(np.uint32)[live]
        return sync, new, bad, np.where(live[:, None], lvl, F32(0)).astype(F32)
