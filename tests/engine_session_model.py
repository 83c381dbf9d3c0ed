"""One rdsp_engine_t object on the CPU, call by call: SessionModel, for tests/test_engine_sessions.py.

It is composed of the restatements the suite already has and adds no arithmetic of its own: a call's tuned rows are
engine_sources_model.call_rows on the explicit phase, frac and source history; every receiver is an
oracle_lib.OracleEngine(taps=True) (audio, the "demod" tap, final()); the meter is engine_meter_model.Meter, the pack
engine_pack_model.  The state is carried from call to call -- nothing is recomputed from block 0 -- and the methods mirror
radiodsp_sdr_rx_amd.engine.Engine's.  A call the header (include/rdsp.h) refuses raises Refused with the header's code
and leaves the model as it was.

Settings are not signal state, and the three setters that clear a filter (setDemodMode, setAudioFilter, enableALSfilter)
clear it in the restatement when they are called, in the product at the next update.  So a receiver may change its group
(set_groups) or its object (load) only between groups that agree in mode, audio set and ALS on / off and have no reset
pending -- or, in a regrouping, when the joined group makes the clearing call itself before the next update; the model
asserts it (Unmodelled: the script is wrong, not the product) -- and the joined group's other
settings are applied again to the receiver's restatement: gains, IQ balance, mute, AGC on / off and mode, blanker, ALS
notch / peak, audio filter on / off; each of these setters stores a value and touches no state (oracle/rdsp_engine_oracle.c).
A receiver that has heard nothing since a reset has the constructor's state whatever its settings: it is built anew from
the joined group's settings, and may join any group."""
import copy
import math

import numpy as np

import engine_meter_model as M
import engine_pack_model as PK
import engine_sources_model as S
import oracle_lib

F32 = np.float32
M32 = S.M32
LINE_MODES = (0, 1, 2, 3, 6)                                # the side-band lines (and a group's pos) move in these
SKETCH = dict(mode=0, audio_id=6, audio_on=1, agc_mode=2, agc_on=1, als_on=0, als_notch=1, nb_on=0, input_gain=1.0,
              iq_balance=1.02, output_gain=0.5, mute=0)     # Engine.sketch_setup()
HARD = ("mode", "audio_id", "als_on")


class Refused(Exception):
    def __init__(self, code, why):
        super().__init__(f"{code}: {why}")
        self.code = code


class Unmodelled(AssertionError):
    """the script asks for something the restatement cannot follow (see the module's text)"""


def apply_setting(st, name, *args):
    """one of the sketch's setters on a group's settings -> the resets it leaves pending"""
    a = args[0] if args else None
    if name == "setDemodMode":
        if int(a) in S.TUNING_OFFSET:
            st["mode"] = int(a)
            return {"pre"}
    elif name == "setAudioFilter":
        if int(a) == 10:
            st["audio_on"] = 0
        elif 0 <= int(a) < 10:
            st["audio_id"] = int(a)
            return {"audio"}
    elif name == "enableAudioFilter":
        st["audio_on"] = 1
    elif name == "setAGCmode":
        if int(a) == 0:
            st["agc_on"] = 0
        elif 1 <= int(a) <= 3:
            st["agc_mode"], st["agc_on"] = int(a), 1
    elif name == "enableAGC":
        st["agc_on"] = 1
    elif name == "enableALSfilter":
        st["als_on"] = 1
        return {"als"}
    elif name == "disableALSfilter":
        st["als_on"] = 0
    elif name == "setALSfilterNotch":
        st["als_notch"] = 1
    elif name == "setALSfilterPeak":
        st["als_notch"] = 0
    elif name == "setALSfilterAdaptive":
        pass                                                # the flag is 1 from the constructor on
    elif name == "enableNoiseBlanker":
        st["nb_on"] = 1
    elif name == "disableNoiseBlanker":
        st["nb_on"] = 0
    elif name == "setMute":
        st["mute"] = 1 if a else 0
    elif name == "setInputGain":
        st["input_gain"] = min(max(float(a), 0.0), 10.0)
    elif name == "setOutputGain":
        st["output_gain"] = float(a)
    elif name == "setIQgainBalance":
        st["iq_balance"] = float(a)
    else:
        raise KeyError(name)
    return set()


def soft_calls(st):
    """the setters that store a value and touch no state, with a group's values"""
    return [("setInputGain", st["input_gain"]), ("setIQgainBalance", st["iq_balance"]), ("setOutputGain", st["output_gain"]),
            ("setMute", st["mute"]), ("setAGCmode", st["agc_mode"]), ("setAGCmode", 0) if not st["agc_on"] else ("enableAGC",),
            ("enableNoiseBlanker",) if st["nb_on"] else ("disableNoiseBlanker",),
            ("setALSfilterNotch",) if st["als_notch"] else ("setALSfilterPeak",),
            ("enableAudioFilter",) if st["audio_on"] else ("setAudioFilter", 10)]


def all_calls(st):
    """every setting of a group, for a receiver in the constructor's state"""
    return [("setDemodMode", st["mode"]), ("setAudioFilter", st["audio_id"]),
            ("enableALSfilter",) if st["als_on"] else ("disableALSfilter",)] + soft_calls(st)


def hard(st):
    return tuple(st[k] for k in HARD)


class Group:
    def __init__(self, first):
        self.first, self.st, self.pending, self.pos = first, dict(SKETCH), set(), 0
        self.attack, self.decay, self.squelch, self.open_ms, self.close_ms, self.hang = M.ATTACK, M.DECAY, False, F32(0), F32(0), 0

    def meter_set(self):
        return M.Squelch(self.open_ms if self.squelch else None, self.close_ms, self.hang, self.attack, self.decay)

    def copy(self, first):
        g = copy.copy(self)
        g.first, g.st, g.pending = first, dict(self.st), set(self.pending)
        return g


class SessionModel:
    def __init__(self, n_channels, max_blocks, source_of, tab, n_sources=None):
        self.n, self.max_blocks, self.tab = n_channels, max_blocks, tab
        self.ring = 512
        while self.ring < max_blocks * 128 + 256:
            self.ring <<= 1
        self.source_of = [int(s) for s in source_of]
        self.n_sources = max(self.source_of) + 1 if n_sources is None else int(n_sources)
        self.o = [oracle_lib.OracleEngine(taps=True) for _ in range(self.n)]
        self.fresh = np.ones(self.n, bool)                  # the constructor's signal state
        self.unsettled = [set() for _ in range(self.n)]     # settings a regrouping left different in the restatement
        self.station = np.zeros(self.n)
        self.phase = np.zeros(self.n, np.uint64)
        self.groups = [Group(0)]
        self.P, self.Q, self.gain, self.fmt, self.frac = 1, 1, 1.0, S.S16, 0
        self._restart()
        self.meter = None
        self.seen = np.zeros(self.n, F32)                   # the highest level since watch()
        self.audio = self.gate = self.cases = None          # the last call's
        self.blocks = 0                                     # blocks heard since the constructor

    # ---- groups ----
    def firsts(self):
        return [g.first for g in self.groups]

    def group_of(self, c, groups=None):
        groups = self.groups if groups is None else groups
        return max(k for k, g in enumerate(groups) if g.first <= c)

    def channels(self, k, groups=None):
        groups = self.groups if groups is None else groups
        return range(groups[k].first, groups[k + 1].first if k + 1 < len(groups) else self.n)

    def _selected(self, group):
        return self.groups if group < 0 else [self.groups[group]]

    def _rebuild(self, c, st):
        self.o[c] = oracle_lib.OracleEngine(taps=True)
        for call in all_calls(st):
            self.o[c].call(*call)

    def _join(self, c, st):
        """receiver c continues under the settings st of the group it joined"""
        if self.fresh[c]:
            self._rebuild(c, st)
        else:
            for call in soft_calls(st) + ([] if st["als_on"] else [("disableALSfilter",)]):
                self.o[c].call(*call)

    def set_groups(self, firsts):
        """-> what the regrouping was: {"pos": some receiver's lines were rotated, "offset": some receiver's tuning offset changed}"""
        firsts = [int(f) for f in firsts]
        if not firsts or firsts[0] != 0 or any(b <= a for a, b in zip(firsts, firsts[1:])) or firsts[-1] >= self.n:
            raise Refused(-1, "first channels")
        new = [self.groups[self.group_of(f)].copy(f) for f in firsts]
        moves = [(c, self.groups[self.group_of(c)], new[self.group_of(c, new)]) for c in range(self.n)]
        if any(was.pending != now.pending for _, was, now in moves):
            raise Refused(-5, "other resets pending")
        what = dict(pos=any(was.pos != now.pos for _, was, now in moves),
                    offset=any(S.TUNING_OFFSET[was.st["mode"]] != S.TUNING_OFFSET[now.st["mode"]] for _, was, now in moves))
        for c, was, now in moves:
            if was.st != now.st:
                self._join(c, now.st)
                if not self.fresh[c]:                       # until the joined group makes the call that clears the filter on both sides
                    self.unsettled[c] |= {k for k in ("mode", "audio_id") if was.st[k] != now.st[k]} | ({"als_on"} if now.st["als_on"] > was.st["als_on"] else set())
        self.groups = new
        return what

    def settled(self):
        for c, u in enumerate(self.unsettled):
            if u:
                raise Unmodelled(f"receiver {c} changed {sorted(u)} in a regrouping with its filters running and no setter cleared them since")

    def call(self, group, name, *args):
        for g in self._selected(group):
            cleared = apply_setting(g.st, name, *args)      # the call clears these on both sides
            g.pending |= cleared
            for c in self.channels(self.groups.index(g)):
                self.o[c].call(name, *args)
                self.unsettled[c] -= {dict(pre="mode", audio="audio_id", als="als_on")[k] for k in cleared}

    def set_meter(self, group, attack, decay):
        for g in self._selected(group):
            g.attack, g.decay = F32(attack), F32(decay)

    def set_squelch(self, group, open_ms, close_ms, hang):
        for g in self._selected(group):
            g.squelch, g.open_ms, g.close_ms, g.hang = True, F32(open_ms), F32(close_ms), int(hang)

    def disable_squelch(self, group):
        for g in self._selected(group):
            g.squelch = False

    def enable_meter(self):
        if self.meter is None:
            self.meter = M.Meter(self.n)

    def thresholds(self, group):
        """open and close thresholds between the loud and the quiet levels the group's receivers have shown since watch()"""
        top = float(np.median(self.seen[list(self.channels(group))]))
        return (F32(0.2 * top), F32(0.02 * top)) if top > 0 else (F32(1e-4), F32(1e-5))

    def watch(self):
        self.seen[:] = 0

    # ---- sources ----
    def band(self, P=None, Q=None):
        return (22050.0 * (self.P if P is None else P)) / (self.Q if Q is None else Q)

    def _restart(self):
        self.frac = 0
        self.hist = [np.zeros((S.keep(self.P, self.Q), 2), F32) for _ in range(self.n_sources)]

    def tune(self, first, stations):
        stations = np.atleast_1d(np.asarray(stations, np.float64))
        if first < 0 or len(stations) < 1 or first + len(stations) > self.n or not np.all(np.abs(stations) < self.band()):
            raise Refused(-1, "station")
        self.station[first:first + len(stations)] = stations

    def set_source_rate(self, P, Q, gain=1.0):
        g = math.gcd(int(P), int(Q))
        P, Q = int(P) // g, int(Q) // g
        if not (1 <= Q <= 441 and Q <= P <= 64 * Q and gain > 0 and math.isfinite(gain)):
            raise Refused(-1, "rate")
        if not np.all(np.abs(self.station) < self.band(P, Q)):
            raise Refused(-1, "a station outside the new band")
        restart = (P, Q) != (self.P, self.Q)
        self.P, self.Q, self.gain = P, Q, float(gain)
        if restart:
            self._restart()

    def set_source_decimation(self, D, gain=1.0):
        self.set_source_rate(D, 1, gain)

    def set_source_format(self, fmt):
        if fmt not in (S.S16, S.U8, S.S8, S.FL):
            raise Refused(-1, "format")
        if fmt != self.fmt:
            self.fmt = fmt
            self._restart()

    def source_pairs(self, n_blocks):
        return (self.frac + n_blocks * 128 * self.P) // self.Q

    def dphi(self, c):
        return S.dphi_of(S.TUNING_OFFSET[self.groups[self.group_of(c)].st["mode"]], self.station[c], self.P, self.Q)

    def update_sources(self, raw_rows, n_blocks):
        """raw_rows: per source source_pairs(n_blocks) pairs [pairs, 2] in the format's type"""
        P, Q, n_out = self.P, self.Q, n_blocks * 128
        pairs = self.source_pairs(n_blocks)
        assert 0 < n_blocks <= self.max_blocks and len(raw_rows) == self.n_sources
        h = S.lib_taps(P, Q, self.gain)
        tuned = np.zeros((self.n, n_out, 2), np.int16)
        for s in range(self.n_sources):
            assert raw_rows[s].shape == (pairs, 2)
            xh = np.concatenate([self.hist[s], S.values(self.fmt, raw_rows[s])])
            self.hist[s] = xh[len(xh) - S.keep(P, Q):].copy()
            cs = [c for c in range(self.n) if self.source_of[c] == s]
            if not cs:
                continue
            step = np.array([self.dphi(c) for c in cs], np.uint64)
            tuned[cs] = S.call_rows(xh, P, Q, self.frac, h, step, self.phase[cs], self.tab, n_out)
            self.phase[cs] = (self.phase[cs] + np.uint64(pairs) * step) & np.uint64(M32)
        self.frac = (self.frac + n_out * P) % Q
        return self.update(tuned)

    def skip(self, n_blocks, sources=True):
        """what a call leaves in the settings, without the signal (for whoever draws a script)"""
        if sources:
            self.frac = (self.frac + n_blocks * 128 * self.P) % self.Q
        self._after(n_blocks)

    def _after(self, n_blocks):
        for g in self.groups:
            g.pending = set()
            if g.st["mode"] in LINE_MODES:
                g.pos = (g.pos + n_blocks * 128) % self.ring
        self.fresh[:] = False
        self.blocks += n_blocks

    def update(self, iq):
        """iq int16 [n, n_blocks * 128, 2], every row at the engine's IF -> what the call returns and leaves to be read"""
        n_blocks = iq.shape[1] // 128
        assert iq.shape == (self.n, n_blocks * 128, 2) and 0 < n_blocks <= self.max_blocks
        self.settled()
        audio, demod = np.zeros((self.n, n_blocks * 128), np.int16), np.zeros((self.n, n_blocks * 128), F32)
        for c, o in enumerate(self.o):
            for b in range(n_blocks):
                v = slice(b * 128, (b + 1) * 128)
                audio[c, v] = o.update(iq[c, v, 0], iq[c, v, 1])
                demod[c, v] = o.tapbuf[5, 0]
            for t in o.taps.values():
                t.clear()
        out = dict(demod=demod, level=None, peak=None, gate=None, active=None, meter=None, cases=None, hangs=None)
        if self.meter is not None:
            sets = [None] * self.n
            for k, g in enumerate(self.groups):
                for c in self.channels(k):
                    sets[c] = g.meter_set()
            out["level"], out["peak"], out["gate"] = self.meter.run(demod, sets)
            out["cases"], out["hangs"] = self.meter.cases, self.meter.hangs
            audio = M.gated(audio, out["gate"])
            out["active"], out["meter"] = np.flatnonzero(out["gate"].any(1)), self.meter.scalars()
            self.seen = np.maximum(self.seen, out["level"].max(1))
        out["audio"] = audio
        self.audio, self.gate, self.cases = audio, out["gate"], out["cases"]
        self._after(n_blocks)
        return out

    def pack(self, n_blocks, capacity=None):
        return PK.pack(self.audio[:, :n_blocks * 128], self.gate[:, :n_blocks], capacity)

    def scalars(self):
        return np.stack([o.final() for o in self.o])

    # ---- reset, state as data ----
    def reset(self):
        for k, g in enumerate(self.groups):
            g.pending, g.pos = set(), 0
            for c in self.channels(k):
                self._rebuild(c, g.st)
        self.fresh[:] = True
        self.unsettled = [set() for _ in range(self.n)]
        self.phase[:] = 0
        self._restart()
        if self.meter is not None:
            self.meter = M.Meter(self.n)

    def save(self, first, n):
        assert 0 <= first and n >= 1 and first + n <= self.n
        ch = range(first, first + n)
        groups = [self.groups[self.group_of(c)] for c in ch]
        if any(g.pending for g in groups):
            raise Unmodelled("a blob of receivers with a reset pending")
        m = self.meter
        return dict(n=n, pos0=self.groups[0].pos, o=[oracle_lib.OracleEngine(like=self.o[c]) for c in ch], hard=[hard(g.st) for g in groups],
                    fresh=self.fresh[first:first + n].copy(), phase=self.phase[first:first + n].copy(), pos=[g.pos for g in groups],
                    meter=None if m is None else (m.level[first:first + n].copy(), m.open[first:first + n].copy(), m.hang[first:first + n].copy()))

    def load(self, first, token):
        n = token["n"]
        if first < 0 or first + n > self.n:
            raise Refused(-1, "no such channels")
        if token["meter"] is not None and self.meter is None:
            raise Refused(-4, "meter words, no meter")
        for k in range(n):
            g = self.groups[self.group_of(first + k)]
            if g.pending or (hard(g.st) != token["hard"][k] and not token["fresh"][k]):
                raise Unmodelled(f"receiver {first + k} would change mode, audio set or ALS on / off with its filters running")
        for k in range(n):
            c = first + k
            self.o[c] = oracle_lib.OracleEngine(taps=True, like=token["o"][k])
            self.fresh[c], self.unsettled[c] = token["fresh"][k], set()
            self._join(c, self.groups[self.group_of(c)].st)
            self.phase[c] = token["phase"][k]
            if self.meter is not None:
                lv, op, hg = (v[k] for v in token["meter"]) if token["meter"] is not None else (F32(0), 0, 0)
                self.meter.level[c], self.meter.open[c], self.meter.hang[c] = lv, op, hg
                self.meter.ms[c] = self.meter.pk[c] = 0          # the last call's are no state
