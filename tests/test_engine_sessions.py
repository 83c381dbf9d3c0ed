"""Drawn sessions of rdsp_engine_t across sources, meter, pack, groups and state (include/rdsp.h), bit for bit.

A session is a script: a list of ops drawn from a seed (draw_session) for two engines that hear the same source rows in the
same calls -- A: 13 ... 37 receivers, ring 2048; B: 5 ... 11 receivers, ring 4096, where the blobs go.  The stream is cut into
eras of another rate (integer and rational) and sample format (int16, uint8, int8, float32 with NaN, +-inf and wild values);
between the calls the script makes the sketch's setters on one group or all, sets meters and squelches (thresholds from the
model's own levels), retunes, regroups (splits, merges between groups whose side-band lines sit at other positions, a merge
that is refused, a boundary moved between groups of other tuning offsets), moves receivers by blob from A to B and back to a
third index, loads a blob saved before the meter existed, resets both engines, sends a rate setter that is refused, and
makes plain update() calls on per-channel IQ.  After every call a pack is made: a sizing call, an exact or a short capacity,
with sentinels behind `written`; the output rows alternate between contiguous and strided, unaligned ones.

tests/engine_session_model.py is the whole object on the CPU, call by call, made of the restatements the suite has.
`-m "not gpu"`: the model against the whole-stream restatements (engine_sources_model.Rx's, Meter.run); what the drawn
sessions contain.  `-m gpu`: both engines against their models after every call; and the same script with its calls cut
in other ways, engine against engine."""
import functools
import json
import time

import numpy as np
import pytest

import engine_meter_model as M
import engine_pack_model as PK
import engine_session_model as E
import engine_sources_model as S
from engine_session_model import Refused, SessionModel

F32 = np.float32
SEEDS = [1, 2, 3, 4, 5, 6, 7, 8]
CUT_SEEDS = [1, 2, 3]
RATES = [(1, 1), (2, 1), (5, 1), (3, 2), (160, 147), (2500, 441)]
# the menu of test_engine_kat.py's _drawn_session
MENU = [["setDemodMode", int(m)] for m in range(7)] + [["setAudioFilter", int(f)] for f in range(11)] + [["setAGCmode", int(a)] for a in range(4)]
MENU += [["enableAGC"], ["enableALSfilter"], ["disableALSfilter"], ["setALSfilterNotch"], ["setALSfilterPeak"], ["setALSfilterAdaptive"],
         ["enableNoiseBlanker"], ["disableNoiseBlanker"], ["setMute", 1], ["setMute", 0], ["enableAudioFilter"]]
MENU += [["setInputGain", g] for g in (0.25, 1.0, 3.0)] + [["setOutputGain", g] for g in (0.2, 0.5, 0.9)] + [["setIQgainBalance", g] for g in (0.95, 1.0, 1.02)]
CLEARING = ("setDemodMode", "setAudioFilter", "enableALSfilter", "disableALSfilter")   # what changes mode, audio set or ALS on / off
OP_KINDS = {"groups", "setter", "set_meter", "squelch", "no_squelch", "tune", "save", "load", "reset", "enable_meter", "rate", "format", "call"}


def _band(rate):
    return 22050.0 * rate[0] / rate[1]


def same_bits(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


# ---- the signals ----------------------------------------------------------------------------------------------------------
def era_rows(seed, era, n_sources, rate, fmt, n_blocks, grid):
    """the source rows of an era in its format: at every station of `grid` a carrier with a 1 kHz tone on both sides (something to
    hear in every mode), keyed in drawn bursts of whole output blocks, over weak noise; float rows carry a few NaN, +-inf and
    values far outside +-1"""
    P, Q = rate
    r = np.random.default_rng([seed, 100 + era])
    fs = S._fs(P, Q)
    n = S._pairs(P, Q, n_blocks) + 8
    t = np.arange(n)
    blk = np.minimum((t * Q) // (P * 128), n_blocks)
    out = np.zeros((n_sources, n, 2), np.int16)
    for s in range(n_sources):
        z = 0.0003 * (r.standard_normal(n) + 1j * r.standard_normal(n))
        for f in grid[s]:
            amp = np.full(n_blocks + 1, 0.0004)
            b = int(r.integers(0, 4))
            while b < n_blocks:
                loud = int(r.integers(2, 5))
                amp[b:b + loud] = r.uniform(0.03, 0.09)
                b += loud + int(r.choice([4, 9, 10, 12, 14]))
            z = z + amp[blk] * (1 + 0.6 * np.cos(2 * np.pi * 1000.0 / fs * t + r.uniform(0, 6))) * np.exp(2j * np.pi * f / fs * t + 1j * r.uniform(0, 6))
        out[s] = S._int16(z * 32767)
    raw = S._raw_of(fmt, out, seed=1 + era)
    if fmt == S.FL:
        raw = raw.copy()
        flat = raw.reshape(-1)
        at = r.integers(0, flat.size, 12)
        flat[at] = [np.nan, np.inf, -np.inf, 300.0, -1e30, 7.5, np.nan, 1e-40, -256.0, 256.5, np.inf, -3.0]
    return raw


def iq_rows(seed, which, n, n_blocks):
    """per-channel IQ at the engine's IF for the plain update() calls: keyed tones inside the passband over weak noise"""
    r = np.random.default_rng([seed, 900 + which])
    t = np.arange(n_blocks * 128)
    x = np.zeros((n, len(t), 2), np.int16)
    for c in range(n):
        amp = np.repeat(r.choice([0.0005, 0.2, 0.3], n_blocks), 128)
        z = amp * np.exp(2j * np.pi * r.uniform(6200, 7800) / 44100.0 * t + 1j * r.uniform(0, 6)) + 0.0003 * (r.standard_normal(len(t)) + 1j * r.standard_normal(len(t)))
        x[c] = S._int16(z * 32767)
    return x


# ---- the script -----------------------------------------------------------------------------------------------------------
def _models(cfg, tab):
    return {e: SessionModel(cfg[e]["n"], cfg[e]["max_blocks"], cfg[e]["source_of"], tab, cfg["n_sources"]) for e in "AB"}


def _engines_of(e):
    return "AB" if e == "AB" else e


def apply_op(ms, op, slots, events=None):
    """an op that is no call, on the models ms = {"A": ..., "B": ...}; a predicted refusal is asserted to be one.  events: a list
    that receives what the op turned out to be"""
    kind, ev = op[0], (events if events is not None else [])
    if kind == "groups":
        _, e, firsts, refused = op
        m = ms[e]
        before = len(m.groups)
        try:
            what = m.set_groups(firsts)
            assert not refused, op
            if len(firsts) < before and what["pos"]:
                ev.append("merge_with_other_pos")
            ev.append("merge" if len(firsts) < before else "split" if len(firsts) > before else "moved_boundary")
            if what["offset"]:
                ev.append("offset_changed_by_regrouping")
        except Refused as x:
            assert refused and x.code == -5, op
            ev.append("refused_merge")
    elif kind == "setter":
        ms[op[1]].call(op[2], op[3], *op[4:])
    elif kind == "set_meter":
        ms[op[1]].set_meter(op[2], op[3], op[4])
    elif kind == "squelch":
        _, e, g, hang, open_ms, close_ms = op
        if open_ms is None:
            open_ms, close_ms = ms[e].thresholds(g)
            op[4], op[5] = float(open_ms), float(close_ms)
        ms[e].set_squelch(g, open_ms, close_ms, hang)
    elif kind == "no_squelch":
        ms[op[1]].disable_squelch(op[2])
    elif kind == "tune":
        ms[op[1]].tune(op[2], op[3])
    elif kind == "save":
        slots[op[4]] = ms[op[1]].save(op[2], op[3])
    elif kind == "load":
        m, tok = ms[op[1]], slots[op[3]]
        for k, p in enumerate(tok["pos"]):
            g = m.groups[m.group_of(op[2] + k)]
            if g.pos != p:
                ev.append("blob_into_other_pos")
            if g.st["mode"] in E.LINE_MODES and (g.pos != m.groups[0].pos or p != tok["pos0"]):
                ev.append("blob_where_the_first_group_sits_elsewhere")
        if tok["meter"] is None and m.meter is not None and m.meter.level[op[2]:op[2] + tok["n"]].any():
            ev.append("blob_without_meter_words")
        m.load(op[2], tok)
    elif kind == "reset":
        for m in ms.values():
            if m.cases is not None and np.any((m.cases[:, -1] == 3) & (m.meter.hang > 0)):
                ev.append("reset_in_a_hang")
            m.reset()
            m.watch()
    elif kind == "enable_meter":
        for m in ms.values():
            m.enable_meter()
    elif kind == "rate":
        _, e, P, Q, gain, refused = op
        for m in (ms[k] for k in _engines_of(e)):
            was = (m.P, m.Q)
            try:
                m.set_source_rate(P, Q, gain)
                assert not refused, op
                if was[1] > 1 and m.Q == 1:
                    ev.append("rational_to_integer")
                m.watch()
            except Refused as x:
                assert refused and x.code == -1 and (m.P, m.Q) == was, op
                ev.append("refused_rate")
    elif kind == "format":
        for m in ms.values():
            if m.fmt != op[1]:
                ev.append("format_change_with_history" if S.keep(m.P, m.Q) else "format_change")
            m.set_source_format(op[1])
            m.watch()
    else:
        raise KeyError(kind)


class _Draw:
    """draws a script: the ops are applied to two models as they are drawn (settings only: skip() stands for a call), so
    that every op is drawn against the settings it will meet"""

    def __init__(self, seed, tab):
        self.r = r = np.random.default_rng(seed)
        n_src = int(r.integers(2, 4))
        nA, nB = int(r.choice([n for n in range(13, 38) if n % 4])), int(r.choice([n for n in range(5, 12) if n % 4]))
        self.cfg = dict(seed=int(seed), n_sources=n_src,
                        A=dict(n=nA, max_blocks=int(r.integers(6, 13)), source_of=[int(s) for s in r.integers(0, n_src, nA)]),
                        B=dict(n=nB, max_blocks=int(r.integers(16, 29)), source_of=[int(s) for s in r.integers(0, n_src, nB)]))
        self.total = int(r.integers(60, 91))
        n_eras = int(r.integers(2, 5))
        while True:
            rates, fmts = [RATES[int(r.integers(0, 6))]], [int(r.integers(0, 4))]
            for _ in range(n_eras - 1):
                if r.random() < 0.35 and rates[-1] != (1, 1):
                    rates.append(rates[-1]); fmts.append(int(r.choice([f for f in range(4) if f != fmts[-1]])))
                else:
                    rates.append(RATES[int(r.choice([k for k in range(6) if RATES[k] != rates[-1]]))])
                    fmts.append(int(r.integers(0, 4)))
            if any(q > 1 for _, q in rates) and any(f != S.S16 for f in fmts):
                break
        cuts = sorted(int(c) for c in r.choice(np.arange(1, self.total // 8), n_eras - 1, replace=False) * 8)
        self.eras = [dict(start=a, blocks=b - a, rate=list(rt), fmt=f) for a, b, rt, f in zip([0] + cuts, cuts + [self.total], rates, fmts)]
        self.cfg["eras"] = self.eras
        self.grid = [[-15000.0 + 6000.0 * k + float(r.uniform(-500, 500)) for k in range(6)] for _ in range(n_src)]
        self.cfg["grid"] = self.grid
        self.ms, self.slots, self.ops, self.events = _models(self.cfg, tab), {}, [], []
        self.maxc = min(self.cfg["A"]["max_blocks"], self.cfg["B"]["max_blocks"])
        self.busy = False

    # -- helpers
    def emit(self, *op):
        op = json.loads(json.dumps(list(op)))                      # what the file will hold
        apply_op(self.ms, list(op), self.slots, self.events)       # (a copy: thresholds are filled in when the signal is there)
        self.ops.append(op)

    def station(self, e, c):
        return float(self.grid[self.cfg[e]["source_of"][c]][int(self.r.integers(0, 6))] + self.r.uniform(-20, 20))

    def align(self, e, g, want):
        """the setters that give group g of engine e the mode, audio set and ALS on / off `want` -> whether any was needed"""
        st, n = self.ms[e].groups[g].st, len(self.ops)
        if st["mode"] != want[0]:
            self.emit("setter", e, g, "setDemodMode", want[0])
        if st["audio_id"] != want[1]:
            self.emit("setter", e, g, "setAudioFilter", want[1])
        if st["als_on"] != want[2]:
            self.emit("setter", e, g, "enableALSfilter" if want[2] else "disableALSfilter")
        return len(self.ops) > n

    def aligned(self, e, g, want):
        grp = self.ms[e].groups[g]
        return not grp.pending and E.hard(grp.st) == tuple(want)

    def split(self, e):
        m = self.ms[e]
        wide = [k for k in range(len(m.groups)) if len(m.channels(k)) >= 2]
        if wide and len(m.groups) < 6:
            k = int(self.r.choice(wide))
            ch = m.channels(k)
            self.emit("groups", e, sorted(m.firsts() + [int(self.r.integers(ch[0] + 1, ch[-1] + 1))]), False)

    def pair_with_other_offsets(self):
        """two neighbouring groups of A with other tuning offsets and the same resets pending (made so, if there is none)"""
        m = self.ms["A"]
        if len(m.groups) < 2:
            self.split("A")
        off = lambda g: S.TUNING_OFFSET[g.st["mode"]]
        ks = [k for k in range(len(m.groups) - 1) if off(m.groups[k]) != off(m.groups[k + 1]) and m.groups[k].pending == m.groups[k + 1].pending]
        return int(self.r.choice(ks)) if ks else None

    def move_boundary(self, k):
        m = self.ms["A"]
        lo, hi = m.groups[k].first + 1, (m.groups[k + 2].first if k + 2 < len(m.groups) else m.n) - 1
        cand = [f for f in range(lo, hi + 1) if f != m.groups[k + 1].first]
        if not cand:
            return None
        f = m.firsts()
        f[k + 1] = int(self.r.choice(cand))
        return f

    # -- the plans: generators that emit ops and yield where a call has to pass
    def plan_merge_other_pos(self):
        m = self.ms["A"]
        if len(m.groups) < 2:
            self.split("A")
        if len(m.groups) < 2:
            return
        k = int(self.r.integers(0, len(m.groups) - 1))
        a, b = m.groups[k], m.groups[k + 1]
        if (a.st["mode"] in E.LINE_MODES) == (b.st["mode"] in E.LINE_MODES):
            self.emit("setter", "A", k + 1, "setDemodMode", 4 if b.st["mode"] in E.LINE_MODES else 0)
        yield
        for _ in range(4):
            k = min(k, len(m.groups) - 2)
            want = E.hard(m.groups[k].st)
            if not self.align("A", k + 1, want) and self.aligned("A", k, want) and self.aligned("A", k + 1, want):
                f = m.firsts()
                del f[k + 1]
                self.emit("groups", "A", f, False)
                return
            yield

    def plan_refused_merge(self):
        m = self.ms["A"]
        if len(m.groups) < 2:
            self.split("A")
        if len(m.groups) < 2:
            return
        k = int(self.r.integers(0, len(m.groups) - 1))
        for name, arg in (("setAudioFilter", int(self.r.integers(0, 10))), ("setDemodMode", m.groups[k].st["mode"])):
            if m.groups[k].pending == m.groups[k + 1].pending:
                self.emit("setter", "A", k, name, arg)
        if m.groups[k].pending != m.groups[k + 1].pending:
            f = m.firsts()
            del f[k + 1]
            self.emit("groups", "A", f, True)
        yield

    def plan_moved_boundary_then_mode(self):
        k = self.pair_with_other_offsets()
        f = None if k is None else self.move_boundary(k)
        if f is None:
            return
        m = self.ms["A"]
        grew = k if f[k + 1] > m.groups[k + 1].first else k + 1      # the group that takes receivers over
        self.emit("groups", "A", f, False)
        st = m.groups[grew].st
        self.emit("setter", "A", grew, "setDemodMode", st["mode"])
        self.emit("setter", "A", grew, "setAudioFilter", st["audio_id"])
        if st["als_on"]:
            self.emit("setter", "A", grew, "enableALSfilter")
        yield

    def plan_reset(self):
        m = self.ms["A"]
        k = self.pair_with_other_offsets()
        if k is None and len(m.groups) >= 2:
            k = int(self.r.integers(0, len(m.groups) - 1))
            other = [md for md in range(6) if S.TUNING_OFFSET[md] != S.TUNING_OFFSET[m.groups[k].st["mode"]]]
            self.emit("setter", "A", k + 1, "setDemodMode", int(self.r.choice(other)))
        self.emit("reset")
        f = None if k is None else self.move_boundary(k)
        if f is not None:
            self.emit("groups", "A", f, False)                     # every receiver is in the constructor's state: any group may be joined
        self.refresh = self.t + 5
        yield

    def _place(self, e, n, avoid=()):
        """a group of engine e that is not its first (if it has another) and a first channel for n receivers in it"""
        m = self.ms[e]
        ks = [k for k in range(len(m.groups)) if len(m.channels(k)) >= n and (k > 0 or len(m.groups) == 1)] or [k for k in range(len(m.groups)) if len(m.channels(k)) >= n]
        for _ in range(8 if ks else 0):
            k = int(self.r.choice(ks))
            ch = m.channels(k)
            first = int(self.r.integers(ch[0], ch[-1] + 2 - n))
            if first not in avoid:
                return k, first
        return None

    def _carry(self, src, first, n, dst, slot, saved=None, avoid=()):
        """receivers first ... of engine src into a place of engine dst whose group is given their mode, audio set and ALS on / off"""
        ms = self.ms
        want = saved if saved is not None else E.hard(ms[src].groups[ms[src].group_of(first)].st)
        place = self._place(dst, n, avoid=avoid)
        if place is None:
            return
        k, at = place
        for _ in range(4):
            k = ms[dst].group_of(at)
            gs = ms[src].groups[ms[src].group_of(first)]
            ok = saved is not None or (not gs.pending and E.hard(gs.st) == tuple(want) and ms[src].group_of(first) == ms[src].group_of(first + n - 1))
            if not self.align(dst, k, want) and self.aligned(dst, k, want) and ok and ms[dst].group_of(at) == ms[dst].group_of(at + n - 1):
                if saved is None:
                    self.emit("tune", dst, at, [float(v) for v in ms[src].station[first:first + n]])
                    self.emit("save", src, first, n, slot)
                self.emit("load", dst, at, slot)
                self.moved = (dst, at, n)
                return
            yield
            if saved is None:
                want = E.hard(ms[src].groups[ms[src].group_of(first)].st)

    def plan_move(self):
        """A -> B, some calls, B -> A at a third index"""
        mA = self.ms["A"]
        ks = [k for k in range(len(mA.groups)) if mA.groups[k].st["mode"] in E.LINE_MODES and not mA.groups[k].pending and (k > 0 or len(mA.groups) == 1)]
        if not ks:
            return
        k = int(self.r.choice(ks))
        ch = mA.channels(k)
        n = int(self.r.integers(1, min(3, len(ch)) + 1))
        first = int(self.r.integers(ch[0], ch[-1] + 2 - n))
        self.moved = None
        yield from self._carry("A", first, n, "B", "move")
        if self.moved is None:
            return
        _, at, n = self.moved
        yield
        yield
        self.moved = None
        yield from self._carry("B", at, n, "A", "back", avoid=range(first - n + 1, first + n))

    def plan_old_blob(self):
        """the blob saved before the meter existed, into B"""
        tok = self.slots["old"]
        yield from self._carry("A", 0, tok["n"], "B", "old", saved=tok["hard"][0])

    def plan_probe(self):
        """a rate the header refuses: a receiver of A is tuned outside 22 050 Hz, then a source rate of 44 100 Hz is asked for"""
        m = self.ms["A"]
        if m.band() <= 22050.0 + 200:
            return
        c = int(self.r.integers(0, m.n))
        old = float(m.station[c])
        self.emit("tune", "A", c, [float(self.r.uniform(22050.0 + 50, m.band() - 50))])
        self.emit("rate", "A", 1, 1, 1.0, True)
        self.probed = True
        self.emit("tune", "A", c, [old])
        yield

    def plan_iq(self):
        self.iq_next = True
        yield

    # -- what is drawn between the calls when no plan has the word
    def random_ops(self):
        r = self.r
        for _ in range(int(r.integers(0, 3))):
            e = "A" if r.random() < 0.6 else "B"
            m = self.ms[e]
            g = int(r.integers(-1, len(m.groups)))
            k = r.random()
            if k < 0.45:
                item = MENU[int(r.integers(0, len(MENU)))]
                if self.busy and item[0] in CLEARING:
                    continue
                self.emit("setter", e, g, *item)
            elif k < 0.55 and m.meter is not None:
                self.emit("set_meter", e, g, float(r.choice([0.5, 1.0, 0.25])), float(r.choice([0.5, 1.0, 0.75])))
            elif k < 0.7 and self.squelched:
                for q in (range(len(m.groups)) if g < 0 else [g]):
                    self.emit("squelch", e, q, int(r.integers(1, 4)), None, None)
            elif k < 0.74 and self.squelched:
                self.emit("no_squelch", e, max(g, 0))
            elif k < 0.9:
                first = int(r.integers(0, m.n))
                n = int(r.integers(1, min(6, m.n - first) + 1))
                self.emit("tune", e, first, [self.station(e, first + j) for j in range(n)])
            elif not self.busy:
                self.split(e)

    def squelch_all(self):
        for e in "AB":
            for g in range(len(self.ms[e].groups)):
                self.emit("squelch", e, g, int(self.r.integers(1, 4)), None, None)
        self.squelched = True

    def era_change(self, was, now):
        if _band(now["rate"]) < _band(was["rate"]) and not self.probed:   # the setter in front of the retune: refused
            m = self.ms["A"]
            c = int(self.r.integers(0, m.n))
            old = float(m.station[c])
            self.emit("tune", "A", c, [float(self.r.uniform(_band(now["rate"]) + 20, _band(was["rate"]) - 20))])
            self.emit("rate", "A", now["rate"][0], now["rate"][1], 2.0, True)
            self.emit("tune", "A", c, [old])
            self.probed = True
        for e in "AB":
            first = int(self.r.integers(0, self.ms[e].n - 2))
            n = int(self.r.integers(1, self.ms[e].n - first + 1))
            self.emit("tune", e, first, [self.station(e, first + j) for j in range(n)])
        if now["rate"] != was["rate"]:
            self.emit("rate", "AB", now["rate"][0], now["rate"][1], 2.0, False)
        if now["fmt"] != was["fmt"]:
            self.emit("format", now["fmt"])
        self.refresh = self.t + 5

    def draw(self):
        r, cfg = self.r, self.cfg
        self.t, self.probed, self.squelched, self.iq_next, self.refresh, self.moved = 0, False, False, False, None, None
        # the set-up: groups in modes of their own (the first group of each engine in AM or SAM: its lines stay behind the others'),
        # stations, the first era's rate and format
        for e, n_groups in (("A", int(r.integers(3, 5))), ("B", 2)):
            n = cfg[e]["n"]
            self.emit("groups", e, [0] + sorted(int(f) for f in r.choice(np.arange(2, n - 1), n_groups - 1, replace=False)), False)
            modes = [int(r.choice([4, 5]))] + [int(v) for v in r.permutation([0, 1, 2, 3])[:n_groups - 1]]
            for g, md in enumerate(modes):
                self.emit("setter", e, g, "setDemodMode", md)
            self.emit("tune", e, 0, [self.station(e, c) for c in range(n)])
        era0 = self.eras[0]
        self.emit("rate", "AB", era0["rate"][0], era0["rate"][1], 2.0, False)
        self.emit("format", era0["fmt"])
        t_meter, t_squelch = int(r.integers(3, 7)), None
        todo = ["merge_other_pos", "refused_merge", "moved_boundary_then_mode", "reset", "move", "old_blob", "iq", "probe"]
        todo = [todo[k] for k in r.permutation(len(todo))]
        plan, era, n_iq = None, 0, 0
        while self.t < self.total:
            if era + 1 < len(self.eras) and self.t >= self.eras[era + 1]["start"]:
                era += 1
                self.era_change(self.eras[era - 1], self.eras[era])
            if t_meter is not None and self.t >= t_meter:
                self.emit("save", "A", int(self.ms["A"].groups[1].first), min(2, len(self.ms["A"].channels(1))), "old")
                self.emit("enable_meter")
                for e in "AB":
                    self.emit("set_meter", e, -1, 0.5, 0.5)
                t_meter, t_squelch = None, self.t + 6
            elif t_squelch is not None and self.t >= t_squelch:
                self.squelch_all()
                t_squelch = None
            elif self.squelched:
                if self.refresh is not None and self.t >= self.refresh:
                    self.squelch_all()
                    self.refresh = None
                if plan is None and todo and r.random() < 0.8:
                    if "probe" in todo and self.probed:
                        todo.remove("probe")
                    ready = [n for n in todo if n != "probe" or self.ms["A"].band() > 22050.0 + 200]
                    if ready:
                        name = "probe" if "probe" in ready else ready[-1]      # the refusal every session has: as soon as it can be made
                        todo.remove(name)
                        plan = getattr(self, "plan_" + name)()
                self.busy = plan is not None
                if plan is not None:
                    try:
                        next(plan)
                    except StopIteration:
                        plan = None
                self.random_ops()
            end = self.eras[era]["start"] + self.eras[era]["blocks"]
            top = min(self.maxc, end - self.t)
            nb = int(r.integers(1, top + 1)) if r.random() < 0.35 else int(r.integers(1, min(3, top) + 1))
            kind = "src"
            if self.iq_next:
                kind, self.iq_next, n_iq = "iq", False, n_iq + nb
            pack_nb = int(r.integers(1, nb + 1)) if r.random() < 0.3 else nb
            cap = ["size", "exact", float(r.uniform(0.2, 0.9))][int(r.integers(0, 3))]
            self.emit_call(kind, nb, pack_nb, cap)
            if kind == "src":
                self.t += nb
        cfg["iq_blocks"] = n_iq
        return dict(cfg=cfg, ops=self.ops)

    def emit_call(self, kind, nb, pack_nb, cap):
        self.ops.append(["call", kind, nb, pack_nb, cap])
        for m in self.ms.values():
            m.skip(nb, kind == "src")


@functools.lru_cache(maxsize=None)
def _tab():
    import radiodsp_sdr_rx_amd as R
    return S.table(R)


def draw_session(seed):
    """-> {"cfg": the two engines, the eras, the stations' grid; "ops": the list of ops}, the same for the same seed"""
    return _Draw(seed, _tab()).draw()


# ---- a script through the models ------------------------------------------------------------------------------------------
class _Feed:
    """the rows of the calls of a script: the era's source rows from where the last call stopped, the IQ rows of the plain calls"""

    def __init__(self, cfg):
        self.cfg, self.era, self.at, self.iq_at = cfg, -1, 0, 0
        self.t = 0
        self.iq = {e: iq_rows(cfg["seed"], k, cfg[e]["n"], max(cfg["iq_blocks"], 1)) for k, e in enumerate("AB")}

    def sources(self, nb, pairs):
        eras = self.cfg["eras"]
        while self.era + 1 < len(eras) and self.t >= eras[self.era + 1]["start"]:
            self.era += 1
            e = eras[self.era]
            self.rows, self.at = era_rows(self.cfg["seed"], self.era, self.cfg["n_sources"], tuple(e["rate"]), e["fmt"], e["blocks"], self.cfg["grid"]), 0
        rows = self.rows[:, self.at:self.at + pairs]
        assert rows.shape[1] == pairs
        self.at += pairs
        self.t += nb
        return rows

    def plain(self, e, nb):
        return self.iq[e][:, self.iq_at * 128:(self.iq_at + nb) * 128]

    def plain_done(self, nb):
        self.iq_at += nb


def _transitions(gate, cases, hangs):
    """engine_meter_model.transitions on a stretch of blocks that does not start from the closed state"""
    return dict(opened=bool(np.any((gate[:, :-1] == 0) & (gate[:, 1:] == 1))), closed=bool(np.any((gate[:, :-1] == 1) & (gate[:, 1:] == 0))),
                ran_out=bool(np.any((cases[:, :-1] == 3) & (hangs[:, :-1] == 0) & (cases[:, 1:] == 4))),
                rearmed=bool(np.any((cases[:, :-1] == 3) & ((cases[:, 1:] == 1) | (cases[:, 1:] == 2)))))


@functools.lru_cache(maxsize=None)
def model_run(seed):
    """the script of a seed through the two models -> (script with the thresholds filled in, per op what the engines must show,
    what the session contained)"""
    script = draw_session(seed)
    cfg, ops = script["cfg"], json.loads(json.dumps(script["ops"]))
    ms, slots, feed = _models(cfg, _tab()), {}, _Feed(cfg)
    trace, events, modes, gates = [], [], set(), []
    stretch = {e: [] for e in "AB"}                          # per engine: (gate, cases, hangs) of the calls since the last break
    seen = dict(opened=False, closed=False, ran_out=False, rearmed=False)

    def close_stretch():
        for e in "AB":
            if stretch[e]:
                for k, v in _transitions(*(np.concatenate([s[i] for s in stretch[e]], 1) for i in range(3))).items():
                    seen[k] |= v
            stretch[e] = []
    for op in ops:
        if op[0] != "call":
            ev = []
            apply_op(ms, op, slots, ev)
            events += ev + [op[0]]
            if op[0] in ("reset", "load", "groups", "squelch", "no_squelch", "set_meter"):
                close_stretch()                              # the next block's case is no longer the last one's successor
            trace.append(None)
            continue
        _, kind, nb, pack_nb, cap = op
        events.append("call_" + kind)
        want = {}
        rows = feed.sources(nb, ms["A"].source_pairs(nb)) if kind == "src" else None
        for e, m in ms.items():
            modes |= {g.st["mode"] for g in m.groups}
            out = m.update_sources(list(rows), nb) if kind == "src" else m.update(feed.plain(e, nb))
            out["scalars"] = m.scalars()
            if m.meter is not None:
                blocks, rec, needed = m.pack(pack_nb)
                capacity = 0 if cap == "size" else needed if cap == "exact" else int(needed * cap)
                out["pack"] = dict(blocks=blocks[:capacity], rec=rec[:capacity], needed=needed, capacity=capacity)
                if pack_nb < nb:
                    events.append("pack_of_fewer_blocks")
                if 0 < capacity < needed and rec[capacity - 1, 0] == rec[capacity, 0]:
                    events.append("capacity_ends_inside_a_channel")
                if any(g.squelch for g in m.groups):
                    gates.append(out["gate"].reshape(-1))
                stretch[e].append((out["gate"], out["cases"], out["hangs"]))
            want[e] = out
        if kind == "iq":
            feed.plain_done(nb)
        trace.append(want)
    close_stretch()
    what = dict(events=events, modes=modes, transitions=seen, gate_mean=float(np.concatenate(gates).mean()) if gates else 0.0)
    return dict(cfg=cfg, ops=ops), trace, what


# ---- CPU ------------------------------------------------------------------------------------------------------------------
class _AsEngine:
    """what engine_sources_model.Rx asks of an engine, answered by a SessionModel"""

    def __init__(self, m):
        self.m, self.sel, self.n_channels = m, -1, m.n

    def set_groups(self, firsts):
        self.m.set_groups(firsts)
        self.sel = -1

    def select_group(self, g):
        self.sel = g

    def tune(self, first, stations):
        self.m.tune(first, stations)

    def __getattr__(self, name):
        return lambda *a: self.m.call(self.sel, name, *a)


class _ModelRx(S.Rx):
    """engine_sources_model.Rx with a SessionModel where the engine is: the same book of steps and calls, the calls made on
    the model"""

    def __init__(self, m, src, firsts, stations, P, Q, gain):
        self.eng, self.src, self.n, self.P, self.Q, self.gain = _AsEngine(m), src, m.n, P, Q, gain
        self.source_of = m.source_of
        m.set_source_rate(P, Q, gain)
        self.firsts, self.modes = [0], [0]
        self.set_groups(firsts)
        self.station = np.zeros(self.n)
        self.tune(0, stations)
        self.calls, self.steps = [[] for _ in range(self.n)], [[] for _ in range(self.n)]
        self.nb = (src.shape[1] * Q + Q - 1) // (128 * P)
        self.outs, self.demod, self.level, self.gate = [], [], [], []
        self.tab, self.h, self.rows = m.tab, S.lib_taps(P, Q, gain), {}

    def run(self, a, b, split):
        a, b = min(a, self.nb), min(b, self.nb)
        for u in range(a, b, split):
            v = min(b, u + split)
            for c in range(self.n):
                self.steps[c] += [S.dphi_of(S.TUNING_OFFSET[self.modes[self.group_of(c)]], self.station[c], self.P, self.Q)] * (v - u)
            at, m = S._pairs(self.P, self.Q, u), self.eng.m
            pairs = m.source_pairs(v - u)
            assert pairs == S._pairs(self.P, self.Q, v) - at
            out = m.update_sources(list(self.src[:, at:at + pairs]), v - u)
            self.outs.append(out["audio"]); self.demod.append(out["demod"]); self.level.append(out["level"]); self.gate.append(out["gate"])


@pytest.mark.parametrize("P,Q", [(2, 1), (160, 147)])
def test_session_model_is_the_existing_restatements(rdsp, oracle, P, Q):
    """engine_sources_model._script_97 (five groups in modes of their own, a retune, a regrouping into six with every mode set
    again, mode and filter changes) on 3 sources x 97 receivers, 40 blocks: the call-by-call model's audio of every receiver
    equals Rx's restatement of the whole stream (stream(), then OracleEngine.run on the receiver's own calls), its levels and
    gates equal Meter.run on the concatenated demod taps, and calls of 7 blocks and of 3 give the bits of calls of 13"""
    nch, nb, gain = 97, 40, 2.5
    r = np.random.default_rng(20 + P)
    src = S.wide(40 + P, 3, nb, P, Q)
    source_of = r.integers(0, 3, nch)
    lim = (22050.0 * P) / Q
    stations = r.uniform(-lim + 1, lim - 1, nch)
    runs = {}
    for split in (13, 7, 3):
        m = SessionModel(nch, 16, source_of, S.table(rdsp), 3)
        m.enable_meter()
        m.set_meter(-1, 0.5, 0.25)
        R = _ModelRx(m, src, [0, 19, 40, 58, 77], stations, P, Q, gain)
        S._script_97(R, split, nb)
        runs[split] = (R, np.concatenate(R.outs, 1), np.concatenate(R.demod, 1), np.concatenate(R.level, 1), np.concatenate(R.gate, 1))
    R, audio, demod, level, gate = runs[13]
    assert audio.shape == (nch, nb * 128) and gate.all()
    for c in range(nch):
        want = R.want(c)
        assert np.array_equal(audio[c], want), (c, int(np.argmax(audio[c] != want)))
    want_level, _, want_gate = M.Meter(nch).run(demod, M.Squelch(attack=0.5, decay=0.25))
    assert same_bits(level, want_level) and np.array_equal(gate, want_gate)
    # with a squelch between the levels: the model's gates and gated audio are Meter.run's on the same taps
    open_ms, close_ms = F32(0.2 * np.median(level.max(1))), F32(0.02 * np.median(level.max(1)))
    for split in (7, 3):
        R2, a2, d2, l2, _ = runs[split]
        assert R2.steps == R.steps and R2.calls == R.calls
        assert np.array_equal(a2, audio) and same_bits(d2, demod) and same_bits(l2, level), split
    m = SessionModel(nch, 16, source_of, S.table(rdsp), 3)
    m.enable_meter()
    m.set_meter(-1, 0.5, 0.25)
    m.set_squelch(-1, open_ms, close_ms, 2)
    R3 = _ModelRx(m, src, [0, 19, 40, 58, 77], stations, P, Q, gain)
    S._script_97(R3, 5, nb)
    mm = M.Meter(nch)
    sq_level, _, sq_gate = mm.run(demod, M.Squelch(open_ms, close_ms, 2, attack=0.5, decay=0.25))
    assert np.array_equal(np.concatenate(R3.gate, 1), sq_gate) and same_bits(np.concatenate(R3.level, 1), sq_level)
    assert 0 < sq_gate.mean() < 1 and np.array_equal(np.concatenate(R3.outs, 1), M.gated(audio, sq_gate))


def test_drawn_sessions_contain_what_they_are_for(rdsp, oracle):
    """the seeds of the GPU tests, on the models alone: the sizes are the ones asked for; every kind of op occurs; over the
    seeds there is a merge between groups whose lines sit at other positions, a refused merge, a refused rate, a blob loaded into
    a group with another position, a blob without meter words onto receivers whose levels are not zero, a boundary moved
    between groups of other tuning offsets, a change from a rational to an integer rate, a change of format (also at a rate
    with a history), a reset while a hang is running, a short capacity that ends inside a channel and a pack of fewer blocks than
    the call had; in EVERY seed the gate opens, closes, has a hang run out and a hang re-armed, and its mean lies in
    (0.15, 0.9); every mode 0 ... 5 runs in some group"""
    events, modes = set(), set()
    for seed in SEEDS:
        script, trace, what = model_run(seed)
        cfg = script["cfg"]
        again = draw_session(seed)
        assert again["cfg"] == cfg and len(again["ops"]) == len(script["ops"]) == len(trace)
        assert all(a == b or (a[0] == "squelch" and a[:4] == b[:4] and a[4] is None) for a, b in zip(again["ops"], script["ops"]))
        assert 2 <= cfg["n_sources"] <= 3 and 13 <= cfg["A"]["n"] <= 37 and cfg["A"]["n"] % 4 and 6 <= cfg["A"]["max_blocks"] <= 12
        assert 5 <= cfg["B"]["n"] <= 11 and cfg["B"]["n"] % 4 and 16 <= cfg["B"]["max_blocks"] <= 28
        rings = {e: SessionModel(1, cfg[e]["max_blocks"], [0], _tab()).ring for e in "AB"}
        assert rings == dict(A=2048, B=4096)
        assert 2 <= len(cfg["eras"]) <= 4 and 60 <= sum(e["blocks"] for e in cfg["eras"]) <= 90
        assert any(e["rate"][1] > 1 for e in cfg["eras"]) and any(e["fmt"] != S.S16 for e in cfg["eras"])
        assert max(-(-e["rate"][0] // e["rate"][1]) for e in cfg["eras"]) <= 6
        assert sum(op[2] for op in script["ops"] if op[0] == "call" and op[1] == "src") == sum(e["blocks"] for e in cfg["eras"])
        assert all(what["transitions"].values()), (seed, what["transitions"])
        assert 0.15 < what["gate_mean"] < 0.9, (seed, what["gate_mean"])
        assert "refused_rate" in what["events"], seed                                   # once per session
        events |= set(what["events"])
        modes |= what["modes"]
    assert events >= OP_KINDS - {"call"} | {"call_src", "call_iq"}, OP_KINDS - events
    for e in ("merge_with_other_pos", "refused_merge", "refused_rate", "blob_into_other_pos", "blob_where_the_first_group_sits_elsewhere", "blob_without_meter_words", "offset_changed_by_regrouping",
              "rational_to_integer", "format_change", "format_change_with_history", "reset_in_a_hang", "capacity_ends_inside_a_channel",
              "pack_of_fewer_blocks", "split", "merge", "moved_boundary"):
        assert e in events, e
    assert modes >= set(range(6))


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _torch_rows(rows):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rows)).cuda()


class _Gpu:
    """the two engines of a script, and the ops on them"""

    def __init__(self, cfg):
        from radiodsp_sdr_rx_amd.engine import Engine
        import oracle_lib
        self.cfg, self.blobs, self.calls = cfg, {}, 0
        self.eng = {}
        for e in "AB":
            g = Engine(cfg[e]["n"], max_blocks_per_call=cfg[e]["max_blocks"], tables=oracle_lib.engine_tables())
            g.sketch_setup()
            g.set_sources(cfg["n_sources"], cfg[e]["source_of"])
            self.eng[e] = g

    def close(self):
        for g in self.eng.values():
            g.close()

    def on_group(self, e, g, f):
        eng = self.eng[e]
        eng.select_group(g)
        try:
            f(eng)
        finally:
            eng.select_group(-1)

    def op(self, op):
        from radiodsp_sdr_rx_amd._lib import RdspError
        kind = op[0]
        if kind == "groups":
            if op[3]:
                with pytest.raises(RdspError) as ex:
                    self.eng[op[1]].set_groups(op[2])
                assert ex.value.code == -5
            else:
                self.eng[op[1]].set_groups(op[2])
        elif kind == "setter":
            self.on_group(op[1], op[2], lambda eng: getattr(eng, op[3])(*op[4:]))
        elif kind == "set_meter":
            self.on_group(op[1], op[2], lambda eng: eng.set_meter(op[3], op[4]))
        elif kind == "squelch":
            self.on_group(op[1], op[2], lambda eng: eng.set_squelch(op[4], op[5], op[3]))
        elif kind == "no_squelch":
            self.on_group(op[1], op[2], lambda eng: eng.disable_squelch())
        elif kind == "tune":
            self.eng[op[1]].tune(op[2], op[3])
        elif kind == "save":
            self.blobs[op[4]] = self.eng[op[1]].save_state(op[2], op[3])
        elif kind == "load":
            self.eng[op[1]].load_state(op[2], self.blobs[op[3]])
        elif kind == "reset":
            for eng in self.eng.values():
                eng.reset()
        elif kind == "enable_meter":
            for eng in self.eng.values():
                eng.enable_meter()
        elif kind == "rate":
            for e in _engines_of(op[1]):
                if op[5]:
                    was = self.eng[e].source_rate()
                    with pytest.raises(RdspError) as ex:
                        self.eng[e].set_source_rate(op[2], op[3], op[4])
                    assert ex.value.code == -1 and self.eng[e].source_rate() == was
                else:
                    self.eng[e].set_source_rate(op[2], op[3], op[4])
        elif kind == "format":
            for eng in self.eng.values():
                eng.set_source_format(op[1])
        else:
            raise KeyError(kind)

    def call(self, e, kind, rows, nb, odd):
        """one call through the C entry point, into contiguous rows or (odd) into rows nb x 128 + 2 pairs apart that start at an
        odd word -> (the rows as a tensor view, pointer, stride in pairs)"""
        import ctypes as C
        import torch
        eng = self.eng[e]
        n, d = eng.n_channels, _torch_rows(rows)
        if odd:
            stride = nb * 128 + 2
            buf = torch.full((n * stride + 1, 2), 7, dtype=torch.int16, device="cuda")
            ptr, view = buf.data_ptr() + 4, buf.as_strided((n, nb * 128, 2), (2 * stride, 2, 1), 2)
        else:
            stride = nb * 128
            buf = view = torch.full((n, stride, 2), 7, dtype=torch.int16, device="cuda")
            ptr = buf.data_ptr()
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        if kind == "src":
            assert d.shape[1] == eng.source_pairs(nb)
            rc = eng.lib.rdsp_engine_update_source_samples(eng.h, d.data_ptr(), d.shape[1], nb, ptr, stride, s)
        else:
            rc = eng.lib.rdsp_engine_update(eng.h, d.data_ptr(), nb * 128, nb, ptr, stride, s)
        assert rc == 0, eng.lib.rdsp_last_error()
        if odd:
            torch.cuda.synchronize()
            pad = buf[1:].reshape(n, stride, 2)[:, nb * 128:]
            assert bool((pad == 7).all()) and int(buf[0, 0]) == 7 and int(buf[0, 1]) == 7     # nothing between or in front of the rows
        return view, ptr, stride


def _first_difference(got, want):
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f"shapes {got.shape} and {want.shape}"
    a, b = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == F32 else (got, want)
    bad = np.argwhere(a != b)
    return f"first difference at {tuple(int(v) for v in bad[0])} (channel first): {got[tuple(bad[0])]!r} for {want[tuple(bad[0])]!r}; {len(bad)} differ"


def _check(ctx, name, got, want, bits=False):
    ok = same_bits(got, want) if bits else np.array_equal(got, want)
    assert ok, f"{ctx}: {name}: {_first_difference(got, want)}"


def _check_call(gpu, e, op, want, view, ptr, stride, first_block, ctx):
    """everything an engine shows after a call against the model's `want`"""
    import torch
    from radiodsp_sdr_rx_amd.engine import pack_runs
    _, kind, nb, pack_nb, cap = op
    eng = gpu.eng[e]
    y = view.cpu().numpy()
    _check(ctx, "audio L against R", y[..., 0], y[..., 1])
    _check(ctx, "audio", y[..., 0], want["audio"])
    _check(ctx, "read_demod", eng.read_demod(nb).cpu().numpy(), want["demod"], bits=True)
    _check(ctx, "scalars", eng.scalars(), want["scalars"], bits=True)
    if want["gate"] is None:
        assert not eng.meter_enabled(), ctx
        return
    level, peak, gate = (v.cpu().numpy() for v in eng.read_meter(nb))
    _check(ctx, "gate", gate, want["gate"])
    _check(ctx, "level", level, want["level"], bits=True)
    _check(ctx, "peak", peak, want["peak"], bits=True)
    lst, cnt = eng.active()
    assert cnt == len(lst), ctx
    _check(ctx, "active", lst.cpu().numpy(), want["active"])
    _check(ctx, "meter", eng.meter(), want["meter"], bits=True)
    p = want["pack"]
    room = p["needed"] + 4
    a = torch.full((room, 128), -21846, dtype=torch.int16, device="cuda")
    r = torch.full((room, 2), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    sizing = cap == "size"
    rc = eng.lib.rdsp_engine_pack_active(eng.h, ptr, stride, pack_nb, None if sizing else a.data_ptr(), None if sizing else r.data_ptr(),
                                         p["capacity"], cnt.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, (ctx, eng.lib.rdsp_last_error())
    w = min(p["needed"], p["capacity"])
    assert cnt.tolist() == [p["needed"], w], (ctx, "pack counts", cnt.tolist(), [p["needed"], w])
    a, r = a.cpu().numpy(), r.cpu().numpy()
    _check(ctx, "pack records", r[:w], p["rec"])
    _check(ctx, "pack blocks", a[:w], p["blocks"])
    assert np.all(a[w:] == -21846) and np.all(r[w:] == -7), (ctx, "written behind `written`")
    _check(ctx, "pack_runs", pack_runs(r[:w], first_block), PK.runs(p["rec"], first_block))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_engine_drawn_sessions(rdsp, tmp_path, seed):
    """the drawn session of `seed` on both engines: after every call audio (L == R, gated), read_demod, read_meter's level, peak
    and gate, active(), meter(), scalars(), the pack (counts, blocks, records, the sentinels behind `written`) and pack_runs
    equal the model's, bit for bit; every predicted refusal raises, and the call behind it still matches"""
    t0 = time.time()
    script, trace, what = model_run(seed)
    t1 = time.time()
    (tmp_path / f"session_{seed}.json").write_text(json.dumps(script))
    cfg, ops = script["cfg"], script["ops"]
    gpu, feed, n_call, block = _Gpu(cfg), _Feed(cfg), 0, 0
    for k, op in enumerate(ops):
        if op[0] != "call":
            gpu.op(op)
            continue
        _, kind, nb, pack_nb, cap = op
        rows = feed.sources(nb, gpu.eng["A"].source_pairs(nb)) if kind == "src" else None
        for e in "AB":
            ctx = f"seed {seed}, op {k} {op}, call {n_call}, engine {e}"
            view, ptr, stride = gpu.call(e, kind, rows if kind == "src" else feed.plain(e, nb), nb, odd=n_call % 2 == 1)
            _check_call(gpu, e, op, trace[k][e], view, ptr, stride, block, ctx)
        if kind == "iq":
            feed.plain_done(nb)
        n_call, block = n_call + 1, block + nb
    gpu.close()
    print(f"seed {seed}: {n_call} calls, {len(ops)} ops, model {t1 - t0:.1f} s, engines and comparisons {time.time() - t1:.1f} s")


def _recut(ops, way):
    """every run of calls of one kind cut anew: way 1 into calls of one block, way 2 into calls of 2, 1, 2, 1 ... blocks"""
    out, k = [], 0
    while k < len(ops):
        if ops[k][0] != "call":
            out.append(ops[k])
            k += 1
            continue
        kind, total = ops[k][1], 0
        while k < len(ops) and ops[k][0] == "call" and ops[k][1] == kind:
            total += ops[k][2]
            k += 1
        sizes, n = [], 0
        while sum(sizes) < total:
            sizes.append(min(total - sum(sizes), 1 if way == 1 else 2 - n % 2))
            n += 1
        out += [["call", kind, nb, nb, "exact"] for nb in sizes]
    return out


def _play(cfg, ops):
    """a script on the engines alone -> per engine audio, level, gate over the stream, the union of the active lists of every run
    of calls, and the packed (channel, absolute block, 128 words) in order"""
    gpu, feed = _Gpu(cfg), _Feed(cfg)
    got = {e: dict(audio=[], level=[], gate=[], active=[], packed=[]) for e in "AB"}
    block, run_open, n_call = 0, False, 0
    for op in ops:
        if op[0] != "call":
            gpu.op(op)
            run_open = False
            continue
        _, kind, nb = op[:3]
        rows = feed.sources(nb, gpu.eng["A"].source_pairs(nb)) if kind == "src" else None
        for e in "AB":
            eng, g = gpu.eng[e], got[e]
            view, _, _ = gpu.call(e, kind, rows if kind == "src" else feed.plain(e, nb), nb, odd=n_call % 2 == 1)
            g["audio"].append(view.cpu().numpy()[..., 0])
            if eng.meter_enabled():
                level, _, gate = (v.cpu().numpy() for v in eng.read_meter(nb))
                g["level"].append(level); g["gate"].append(gate)
                lst = set(eng.active()[0].cpu().numpy().tolist())
                if run_open:
                    g["active"][-1] |= lst
                else:
                    g["active"].append(lst)
                a, r, _ = eng.pack_active(view)
                a, r = a.cpu().numpy(), r.cpu().numpy()
                g["packed"] += [(int(c), block + int(b), w.tobytes()) for (c, b), w in zip(r, a)]
        if kind == "iq":
            feed.plain_done(nb)
        run_open, block, n_call = True, block + nb, n_call + 1
    gpu.close()
    for g in got.values():
        g["packed"].sort(key=lambda v: v[:2])                # by receiver, then block: the cut decides only where a call's records end
        for k in ("audio", "level", "gate"):
            g[k] = np.concatenate(g[k], 1)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("seed", CUT_SEEDS)
def test_gpu_engine_drawn_sessions_do_not_depend_on_the_call_cut(rdsp, seed):
    """the drawn session of `seed` as drawn, with every run of calls cut into calls of one block, and into calls of 2, 1, 2, 1 ...
    blocks, the ops at the same blocks: audio, levels, gates, the union of the active lists of every run and the packed
    (receiver, absolute block, 128 words) are identical.  Engine against engine: no model takes part (the thresholds of the
    squelches are numbers in the script)"""
    script, _, _ = model_run(seed)
    cfg, ops = script["cfg"], script["ops"]
    as_drawn = _play(cfg, ops)
    assert sum(len(g["packed"]) for g in as_drawn.values()) > 50
    for way in (1, 2):
        other = _play(cfg, _recut(ops, way))
        for e in "AB":
            ctx = f"seed {seed}, cut {way}, engine {e}"
            _check(ctx, "audio", other[e]["audio"], as_drawn[e]["audio"])
            _check(ctx, "gate", other[e]["gate"], as_drawn[e]["gate"])
            _check(ctx, "level", other[e]["level"], as_drawn[e]["level"], bits=True)
            assert other[e]["active"] == as_drawn[e]["active"], ctx
            assert other[e]["packed"] == as_drawn[e]["packed"], ctx
