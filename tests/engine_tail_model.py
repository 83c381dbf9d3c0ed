"""The tail of rdsp_engine_t restated in numpy from the "demod" tap on (what rdsp_engine_read_demod returns): the four-section
DF1 audio cascade with every product rounded (0xd944), the hang AGC with its 129-entry gain curve (0xdb58, 0xdc10), the 55-tap
ALS line enhancer (0xda24) and the truncating, wrapping int16 store (0xebfa) -- the operations of oracle/rdsp_engine_oracle.c
and csrc/rdsp_engine_laws.h in their order, float32 throughout.  Vectorised over channels; samples in order.
tests/test_engine_fm.py holds it bit for bit to the stage taps and the audio of tests/golden/engine_kat.npz; an NFM group's
int16 audio is then this model on the FM model's rows."""
import os

import numpy as np

from engine_sources_model import fma32

F32 = np.float32
BLOCK = 128
ALS_TAPS, ALS_DELAY = 55, 3
SET_OF_AUDIO_ID = (7, 8, 9, 0, 1, 2, 3, 4, 5, 6)
_AGC_BITS = {1: (0x3f79673b, 0x3cd318a0, 0x3f7fddca, 0x3a08d800, 4410), 2: (0x3f7d5732, 0x3c2a3380, 0x3f7ff250, 0x395b0000, 22050),
             3: (0x3f7eaab6, 0x3baaa500, 0x3f7ff928, 0x38db0000, 88200)}


def _f(bits):
    return np.array([bits], np.uint32).view(F32)[0]


def tables():
    """(the fifteen biquad sets float32 [15, 4, 5], the AGC's gain curve float32 [130]) from the fixtures"""
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    sets = np.load(os.path.join(here, "firmware_tables.npz"))["biquad_sets"].astype(F32).reshape(15, 4, 5)
    curve = np.zeros(130, F32)
    c = np.load(os.path.join(here, "engine_kat.npz"))["agc_curve"]
    curve[:len(c)] = c
    return sets, curve


def trunc_s32(x):
    """VCVT.S32.F64: toward zero, saturating"""
    return np.clip(np.trunc(np.asarray(x, np.float64)), -2147483648.0, 2147483647.0).astype(np.int64)


class Tail:
    """n channels with the sketch's set-up (INO:120-139: audio filter 6 on, AGC medium, ALS off, output gain 0.5); the setters
    carry the engine's names and act on every channel; run(demod) takes float32 [n, t], t a multiple of 128, and returns the
    int16 audio [n, t]; the taps of the last run stay in self.filt, self.agc, self.als"""

    def __init__(self, n, sets=None, curve=None):
        if sets is None or curve is None:
            sets, curve = tables()
        self.n, self.sets, self.curve = n, sets, curve
        self.audio_on, self.agc_on, self.als_on, self.als_notch, self.als_adaptive, self.mute = 1, 1, 0, 1, 1, 0
        self.output_gain = F32(0.5)
        self.makeup = F32(10.0)
        self.setAGCmode(2)
        self.reset()
        self.setAudioFilter(6)

    def reset(self):
        n = self.n
        self.bq = np.zeros((n, 4, 4), F32)               # per section x1, x2, y1, y2
        self.env, self.gain, self.hang = np.zeros(n, F32), np.zeros(n, F32), np.zeros(n, np.int64)
        self.line, self.w = np.zeros((n, 2 * BLOCK), F32), np.zeros((n, ALS_TAPS), F32)

    # ---- the engine's setters ----
    def setAudioFilter(self, ident):
        if ident == 10:
            self.audio_on = 0
        elif 0 <= ident < 10:
            self.coef = self.sets[SET_OF_AUDIO_ID[ident]]
            self.bq[:] = 0
        return self

    def enableAudioFilter(self):
        self.audio_on = 1
        return self

    def setAGCmode(self, mode):
        if mode == 0:
            self.agc_on = 0
        elif mode in _AGC_BITS:
            b = _AGC_BITS[mode]
            self.attack_a, self.attack_b, self.decay_a, self.decay_b, self.hang_time = _f(b[0]), _f(b[1]), _f(b[2]), _f(b[3]), b[4]
            self.agc_on = 1
        return self

    def enableAGC(self):
        self.agc_on = 1
        return self

    def enableALSfilter(self):
        self.als_on = 1
        self.line[:] = 0
        self.w[:] = 0
        return self

    def disableALSfilter(self):
        self.als_on = 0
        return self

    def setALSfilterNotch(self):
        self.als_notch = 1
        return self

    def setALSfilterPeak(self):
        self.als_notch = 0
        return self

    def setALSfilterAdaptive(self):
        self.als_adaptive = 1
        return self

    def setOutputGain(self, g):
        self.output_gain = F32(g)
        return self

    def setMute(self, on):
        self.mute = 1 if on else 0
        return self

    # ---- the stages ----
    def _cascade(self, a):
        out = np.empty_like(a)
        c, st = self.coef, self.bq
        for i in range(a.shape[1]):
            v = a[:, i]
            for s in range(4):
                y = (c[s, 0] * v) + (c[s, 1] * st[:, s, 0]) + (c[s, 2] * st[:, s, 1]) + (c[s, 3] * st[:, s, 2]) + (c[s, 4] * st[:, s, 3])
                st[:, s, 1] = st[:, s, 0]; st[:, s, 0] = v
                st[:, s, 3] = st[:, s, 2]; st[:, s, 2] = y
                v = y
            out[:, i] = v
        return out

    def _lookup(self, env):
        idx = trunc_s32(env.astype(np.float64) * 32767.0)
        hi = (idx >> 8) & 0xff
        hi1 = np.where(hi > 127, 128, hi + 1)
        hi = np.minimum(hi, 127)
        frac = (idx & 0xff).astype(F32) * F32(0.00390625)
        t0 = self.curve[hi]
        return fma32(frac, self.curve[hi1] - t0, t0)

    def _agc(self, a):
        out = np.empty_like(a)
        for i in range(a.shape[1]):
            x = a[:, i]
            inp = np.minimum(np.abs(x), F32(1.0))
            attack = self.env < inp
            decay = ~attack & (self.hang == 0)
            ea = fma32(self.env, np.full(self.n, self.attack_a, F32), inp * self.attack_b)
            ed = fma32(self.env, np.full(self.n, self.decay_a, F32), inp * self.decay_b)
            self.env = np.where(attack, ea, np.where(decay, ed, self.env)).astype(F32)
            self.hang = np.where(attack, self.hang_time, np.where(decay, 0, self.hang - 1))
            self.gain = np.where(attack | decay, self._lookup(self.env), self.gain).astype(F32)
            out[:, i] = np.clip((self.gain * self.makeup) * x, F32(-1.0), F32(1.0))
        return out

    def _als(self, a):
        out = np.empty_like(a)
        for b in range(a.shape[1] // BLOCK):
            self.line[:, :BLOCK] = self.line[:, BLOCK:]
            self.line[:, BLOCK:] = a[:, b * BLOCK:(b + 1) * BLOCK]
            blk = out[:, b * BLOCK:(b + 1) * BLOCK]
            # the taps move behind the first of every four samples (0, 4, ... 124), which still sees the taps in front of the move:
            # spans of samples that share their taps -- {0}, {1 .. 4}, ... {121 .. 124}, {125 .. 127} -- one 55-step chain each
            spans = [(0, 1)] + [(j, min(j + 4, BLOCK)) for j in range(1, BLOCK, 4)] if self.als_adaptive else [(0, BLOCK)]
            for lo, hi in spans:
                m = BLOCK + np.arange(lo, hi)
                y = np.zeros((self.n, hi - lo), F32)
                for k in range(ALS_TAPS):
                    y = fma32(np.repeat(self.w[:, k:k + 1], hi - lo, 1), self.line[:, m - ALS_DELAY - k], y)
                err = self.line[:, m] - y
                blk[:, lo:hi] = err if self.als_notch else y
                if self.als_adaptive and (hi - 1) % 4 == 0:                      # the span ends on the sample that moves the taps
                    x = self.line[:, BLOCK + hi - 1 - ALS_DELAY - np.arange(ALS_TAPS)]
                    self.w = fma32(err[:, -1:] * x, np.full_like(x, 0.5), self.w)
        return out

    def run(self, demod):
        a = np.ascontiguousarray(demod, F32)
        assert a.shape[0] == self.n and a.shape[1] % BLOCK == 0
        with np.errstate(all="ignore"):
            if self.audio_on:
                a = self._cascade(a)
            self.filt = a
            if self.agc_on:
                a = self._agc(a)
            self.agc = a
            if self.als_on:
                a = self._als(a)
            self.als = a
            v = trunc_s32((a * self.output_gain).astype(np.float64) * 32767.0) & 0xffff
        v = np.where(v >= 32768, v - 65536, v).astype(np.int16)
        return np.zeros_like(v) if self.mute else v
