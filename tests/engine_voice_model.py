"""rdsp_engine_t's voice-rate audio (include/rdsp.h, "voice-rate audio") restated in numpy: the taps from the prototype
engine_sources_model already restates, a per-channel object with history that turns the left words a call returned into the
voice rows, in int64, and the pack of those rows."""
import numpy as np

import engine_pack_model
from engine_sources_model import taps_of

BLOCK = 128
HIST = 60            # left words a channel keeps, whatever R
SHIFT = 18


def taps(R):
    """q_k = rint(h_k 2^18), h the float32 prototype of a source at R x 44 100 Hz: int32 [16 R]"""
    assert R in (2, 4)
    return np.rint(taps_of(R).astype(np.float64) * 262144.0).astype(np.int32)


def round_sat(acc):
    """(acc + 2^17) >> 18 with an arithmetic shift -- floor, ties upwards -- clamped to int16"""
    acc = np.asarray(acc, np.int64)
    return np.clip((acc + (1 << (SHIFT - 1))) >> SHIFT, -32768, 32767).astype(np.int16)


def accumulate(x, R):
    """x int64 [n, HIST + t]: the history and a call's left words -> acc int64 [n, t / R], exact"""
    q = taps(R).astype(np.int64)
    t = x.shape[1] - HIST
    assert t % R == 0
    m = np.arange(t // R)
    acc = np.zeros((x.shape[0], t // R), np.int64)
    for k in range(16 * R):
        acc += q[k] * x[:, HIST + R * m + R - 1 - k]
    return acc


class Voice:
    """n channels at rate R: run(left) takes the left words int16 [n, t] a call returned (t a multiple of 128) and returns
    the call's voice rows int16 [n, t / R]; the history (int32 [n, 60], oldest first) carries on"""

    def __init__(self, n, R):
        self.R, self.hist = R, np.zeros((n, HIST), np.int64)

    def run(self, left):
        left = np.asarray(left)
        assert left.dtype == np.int16 and left.shape[0] == len(self.hist) and left.shape[1] % BLOCK == 0
        x = np.concatenate([self.hist, left.astype(np.int64)], 1)
        self.hist = x[:, -HIST:].copy()
        return round_sat(accumulate(x, self.R))

    def reset(self):
        self.hist[:] = 0


def pack(voice_rows, gate, R, capacity=None):
    """voice rows int16 [n, nb * 128 / R], gate [n, nb] -> (blocks int16 [written, 128 / R], records int32 [written, 2],
    needed): engine_pack_model.pack over blocks of 128 / R words"""
    voice_rows, gate = np.asarray(voice_rows), np.asarray(gate)
    n, nb = gate.shape
    w = BLOCK // R
    assert voice_rows.shape == (n, nb * w)
    wide = np.zeros((n, nb, BLOCK), np.int16)
    wide[:, :, :w] = voice_rows.reshape(n, nb, w)
    blocks, records, needed = engine_pack_model.pack(wide.reshape(n, nb * BLOCK), gate, capacity)
    return np.ascontiguousarray(blocks[:, :w]), records, needed
