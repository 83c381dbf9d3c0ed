"""The signal meter and squelch of rdsp_engine_t (include/rdsp.h, csrc/rdsp_meter.h) restated in numpy, operation for
operation in float32: per block of 128 demodulated samples the mean square by the balanced pair tree, the peak, the level
recursion L <- fmaf(d > 0 ? attack : decay, d, L) with d = ms - L, and the gate.  Vectorised over channels; blocks in order."""
import numpy as np

from engine_sources_model import fmaf

F32 = np.float32
BLOCK = 128
ATTACK, DECAY = F32(0.5), F32(0.0625)


def tree_sum(q):
    """[..., 128] float32 -> [...]: adjacent pairs in index order, seven levels"""
    q = np.asarray(q, F32)
    assert q.shape[-1] == BLOCK
    with np.errstate(all="ignore"):
        for _ in range(7):
            q = q[..., 0::2] + q[..., 1::2]
    return q[..., 0]


def left_to_right_sum(q):
    """the sum a plain loop would form (NOT the definition: the tests show that it differs)"""
    q = np.asarray(q, F32)
    s = np.zeros(q.shape[:-1], F32)
    with np.errstate(all="ignore"):
        for t in range(q.shape[-1]):
            s = s + q[..., t]
    return s


def measure(a):
    """a: float32 [..., n_blocks * 128] -> (ms, pk) float32 [..., n_blocks]"""
    a = np.asarray(a, F32)
    a = a.reshape(a.shape[:-1] + (-1, BLOCK))
    with np.errstate(all="ignore"):
        ms = tree_sum(a * a) * F32(0.0078125)
    pk = np.fmax.reduce(np.abs(a), axis=-1, initial=F32(0.0))
    return ms, pk


def level_step(level, ms, attack=ATTACK, decay=DECAY):
    with np.errstate(all="ignore"):
        d = np.asarray(ms, F32) - np.asarray(level, F32)
        return fmaf(np.where(d > 0, F32(attack), F32(decay)), d, level).astype(F32)


class Squelch:
    """a group's settings; squelch None: off"""

    def __init__(self, open_ms=None, close_ms=0.0, hang_blocks=0, attack=ATTACK, decay=DECAY):
        self.on = open_ms is not None
        self.open_ms, self.close_ms = F32(open_ms if self.on else 0.0), F32(close_ms)
        self.hang_blocks, self.attack, self.decay = int(hang_blocks), F32(attack), F32(decay)


def gate_step(level, is_open, hang, s):
    """one channel, python scalars: the four cases of the definition -> (open, hang)"""
    if not s.on or level >= s.open_ms:
        return 1, s.hang_blocks
    if is_open and level >= s.close_ms:
        return 1, s.hang_blocks
    if is_open and hang > 0:
        return 1, hang - 1
    return 0, hang


def gate_case(level, is_open, hang, s):
    """which case of the squelch-on gate a block takes: 1 ... 4"""
    if level >= s.open_ms:
        return 1
    if is_open and level >= s.close_ms:
        return 2
    if is_open and hang > 0:
        return 3
    return 4


class Meter:
    """the meter state of n channels; settings[c]: the Squelch in force for channel c (may change between runs)"""

    def __init__(self, n):
        self.level = np.zeros(n, F32)
        self.open = np.zeros(n, np.int32)
        self.hang = np.zeros(n, np.int32)
        self.ms = np.zeros(n, F32)
        self.pk = np.zeros(n, F32)

    def run(self, rows, settings):
        """rows: float32 [n, n_blocks * 128] demodulated audio -> (level, peak, open) [n, n_blocks]"""
        ms, pk = measure(rows)
        n, nb = ms.shape
        if not isinstance(settings, (list, tuple)):
            settings = [settings] * n
        att = np.array([s.attack for s in settings], F32)
        dec = np.array([s.decay for s in settings], F32)
        level, gate = np.zeros((n, nb), F32), np.zeros((n, nb), np.uint8)
        self.cases, self.hangs = np.zeros((n, nb), np.int32), np.zeros((n, nb), np.int32)   # per block: the gate's case (0: squelch off), hang after it
        for b in range(nb):
            with np.errstate(all="ignore"):
                d = ms[:, b] - self.level
                self.level = fmaf(np.where(d > 0, att, dec), d, self.level).astype(F32)
            for c in range(n):
                self.cases[c, b] = gate_case(self.level[c], self.open[c], self.hang[c], settings[c]) if settings[c].on else 0
                self.open[c], self.hang[c] = gate_step(self.level[c], self.open[c], self.hang[c], settings[c])
                self.hangs[c, b] = self.hang[c]
            level[:, b], gate[:, b] = self.level, self.open
        if nb:
            self.ms, self.pk = ms[:, -1].copy(), pk[:, -1].copy()
        return level, pk, gate

    def scalars(self):
        """what rdsp_engine_get_meter returns: [n, 4]"""
        return np.stack([self.level, self.ms, self.pk, self.open.astype(F32)], 1)


def transitions(gate, cases, hangs):
    """what a squelch test must have seen, over [n, n_blocks] arrays of a run from the closed state: the gate opening, the
    gate closing, a hang that ran out (case 3 down to 0, then case 4), a hang re-armed while it ran (case 3, then 1 or 2)"""
    g = np.concatenate([np.zeros((gate.shape[0], 1), gate.dtype), gate], 1)
    return dict(opened=bool(np.any((g[:, :-1] == 0) & (g[:, 1:] == 1))), closed=bool(np.any((g[:, :-1] == 1) & (g[:, 1:] == 0))),
                ran_out=bool(np.any((cases[:, :-1] == 3) & (hangs[:, :-1] == 0) & (cases[:, 1:] == 4))),
                rearmed=bool(np.any((cases[:, :-1] == 3) & ((cases[:, 1:] == 1) | (cases[:, 1:] == 2)))))


def gated(audio, gate):
    """int16 [n, n_blocks * 128(, 2)] with the closed blocks zeroed"""
    y = audio.copy()
    v = y.reshape((y.shape[0], gate.shape[1], BLOCK) + y.shape[2:])
    v[gate == 0] = 0
    return y
