"""Drawn sessions across narrow-band FM, its squelches, decoders and events (docs/engine.md, "Where the features meet: drawn
sessions").  Three engines run a script drawn from a seed on plain update() calls: A with every feature, B with every feature,
fewer receivers and another max_blocks, C with FM and the meter only.  tests/engine_nfm_session_model.py follows them call by
call on the CPU, and after every call everything an engine shows is compared with it bit for bit.  The script is drawn against
the models (draw_session applies every op to them as it draws, so only scripts the models can follow and predicted refusals
come out); the same script with its calls cut in other ways is compared engine against engine.

The rows come from the feature files' builders: page / packet / keypad / station / placed of test_engine_events_gpu.py, and
the stations of engine_dcs_model, engine_noise_model, engine_tone_model and engine_fm_model.  A receiver's row follows it when
it moves by blob."""
import functools
import json
import time

import numpy as np
import pytest

import engine_afsk_model as AF
import engine_dcs_model as DC
import engine_dtmf_model as DT
import engine_events_model as EV
import engine_fm_model as FM
import engine_nfm_session_model as N
import engine_noise_model as NZ
import engine_pack_model as PK
import engine_pocsag_model as PO
import engine_sources_model as S
import engine_tone_model as TN
import test_engine_events_gpu as E
from engine_session_model import Refused
from test_engine_sessions import _check, _first_difference, _recut, same_bits

F32, U32 = np.float32, np.uint32
SEEDS = [1, 2, 3, 4, 5, 6]
CUT_SEEDS = [1, 2]
T = 96                                                      # blocks of stream in a session
NFM, LSB, USB, AM = 7, 0, 1, 4
ALL = dict(meter=1, voice=2, fm=1, tone=1, search=1, dcs=1, noise=1, dtmf=1, afsk=1, pocsag=1)
PLAIN = dict(meter=1, voice=0, fm=1)
LOOSE = (4, 0.05, 2.0, 8.0, 0.3, 1, 1)                      # DTMF frames of 4 blocks that emit a key after one frame
SENTINEL = 0x5EA15EA1
OP_KINDS = {"groups", "mode", "tail", "set", "meter", "squelch", "no_squelch", "tones", "codes", "bank", "save", "load", "reset", "zero", "call"}
SET_KINDS = ("fm", "tone", "search", "dcs", "noise", "dtmf", "afsk", "pocsag")
BAD = [["set", "fm", [4, 5000.0, 750.0]], ["set", "fm", [2, 500.0, 750.0]], ["set", "fm", [2, 5000.0, 10.0]], ["set", "tone", [2, 0.04, 0.025]],
       ["set", "tone", [8, 0.02, 0.03]], ["set", "search", [3, 0.04, 4.0]], ["set", "search", [8, 0.04, 0.5]], ["set", "dcs", [4, 1, 1, 1]],
       ["set", "dcs", [16, 4, 2, 1]], ["set", "dcs", [16, 1, 7, 1]], ["set", "noise", [3, 0.01, 0.025, 8, 0.75, 0.125]],
       ["set", "noise", [2, 0.03, 0.025, 8, 0.75, 0.125]], ["set", "noise", [2, 0.01, 0.025, 8, 0.0, 0.125]], ["set", "dtmf", [3, 0.015, 4.0, 16.0, 0.5, 2, 2]],
       ["set", "dtmf", [4, 0.015, 4.0, 16.0, 0.5, 17, 2]], ["set", "afsk", [2, 1.0, 2, 17]], ["set", "afsk", [1, 1.0, 5, 17]], ["set", "afsk", [1, 1.0, 2, 8]],
       ["set", "pocsag", [600, 2, 3, 2, 1, 2]], ["set", "pocsag", [1200, 3, 3, 2, 1, 2]], ["set", "pocsag", [0, 2, 3, 4, 1, 2]],
       ["tones", [59.0]], ["tones", [100.0] * 99], ["codes", [600]], ["bank", [100.0, 90.0]], ["groups", [0, 0]], ["groups", [1, 2]],
       ["squelch", [1e-3, 2e-3, 1]], ["squelch", [1e-3, 5e-4, 70000]], ["squelch", [1e-3, -1.0, 1]], ["tones_at", [100.0]], ["codes_at", [0o023]],
       ["set", "fm", [2, float("nan"), 750.0]], ["set", "tone", [8, float("nan"), 0.025]], ["set", "dtmf", [4, float("nan"), 4.0, 16.0, 0.5, 2, 2]],
       ["meter", [0.0, 0.0625]]]


# ---- rows ------------------------------------------------------------------------------------------------------------------
def _row(seed, spec):
    """one receiver's int16 [T * 128, 2] from its description"""
    kind, t = spec[0], T * 128
    r = np.random.default_rng(seed)
    draw = lambda k: [int(v) for v in r.integers(0, 1 << 20, k)]
    payload = lambda k: bytes(r.integers(0, 256, k, dtype=np.uint8))
    if kind == "page":                                      # a page of three words at 2400 baud from block spec[1] on, a numeric one behind it
        first = E.page([(800 + 64 * (seed % 16), 3, draw(3))], whole=False)
        mod = E.placed(t, (first, spec[1] * 128 + 20), (E.page([(16, 1, [])], whole=False), spec[1] * 128 + 20 + len(first) + 300))
    elif kind == "packet":
        mod = E.packet(payload(15), lead=spec[1] * 128 + 50, total=t)
    elif kind == "keypad":                                  # a key every nine blocks from block 4 on
        mod = E.keypad("159D*0#A26", 6, 3, lead=4 * 128, total=t)
    elif kind == "six":                                     # six tone-only pages in one batch: more than a ring holds
        mod = E.page([(8 * k + k, k % 4, []) for k in range(6)], lead=spec[1] * 128 + 30, total=t)
    elif kind == "both":                                    # a packet, then a tone-only page: two kinds of item on one channel
        frame = E.packet(payload(15))
        mod = E.placed(t, (frame, spec[1] * 128), (E.page([(8, 2, [])], whole=False), spec[1] * 128 + len(frame) + 200))
    elif kind == "pages_x":                                 # a tone-only page at 2400 baud at once, one at 1200 baud from block spec[1] on
        mod = E.placed(t, (E.page([(24, 1, [])], whole=False), 10), (E.page([(32, 2, [])], 1200, whole=False), spec[1] * 128 + 10))
    elif kind == "page512":                                 # a tone-only page at 512 baud behind a preamble of 16 bits: read near block 75
        P = E._P()
        words = P.batches([(40, 1, [])])
        last = max(k for k, w in enumerate(words) if w != P.IDLE and w != P.SYNC)
        mod = P.transmit(P.bits(words[:last + 2], 16), 512, 0.6, lead=10, total=t)
    elif kind == "tone":                                    # a CTCSS tone under voice noise until block spec[1]
        mod = TN.demod_row(seed, T, 100.0, 0.12, tone_until=spec[1] * 128).astype(np.float64)
    elif kind == "dcs":
        return DC.station(seed, T, DC.codeword(0o023))
    elif kind == "burst":                                   # a carrier under voice noise until block spec[1]
        return NZ.station(seed, T, until=spec[1] * 128)
    elif kind == "fm":
        return FM.station(seed, T, 5000.0, 700.0 + 100.0 * (seed % 7), 6000.0)
    elif kind == "idle":
        return np.rint(300.0 * r.standard_normal((t, 2))).astype(np.int16)
    elif kind == "zeros":
        return np.zeros((t, 2), np.int16)
    elif kind == "rails":
        return r.choice(np.array([32767, -32768], np.int16), (t, 2))
    else:
        raise KeyError(kind)
    return E.station(seed, mod, float(r.uniform(3000, 16000)))


@functools.lru_cache(maxsize=None)
def session_rows(seed, specs):
    return np.stack([_row(1000 * seed + k, spec) for k, spec in enumerate(specs)])


# ---- ops on a model --------------------------------------------------------------------------------------------------------
def apply_op(ms, op, slots):
    """one op that is not a call on the models -> the refusal's code (0: none).  ["load"] takes its rows along"""
    kind, e = op[0], op[1]
    m = ms[e]
    try:
        if kind == "groups":
            m.set_groups(op[2])
        elif kind == "mode":
            m.call(op[2], "setDemodMode", op[3])
        elif kind == "tail":
            m.call(op[2], op[3], *op[4])
        elif kind == "set":
            m.set(op[2], op[3], *op[4])
        elif kind == "meter":
            m.set_meter(op[2], op[3], op[4])
        elif kind == "squelch":
            m.set_squelch(op[2], op[3], op[4], op[5])
        elif kind == "no_squelch":
            m.disable_squelch(op[2])
        elif kind == "tones":
            m.set_tones(op[2], op[3])
        elif kind == "codes":
            m.set_dcs_codes(op[2], op[3])
        elif kind == "bank":
            m.set_tone_bank(op[2])
        elif kind == "save":
            slots[op[4]] = m.save(op[2], op[3])
        elif kind == "load":
            m.load(op[2], slots[op[3]])
        elif kind == "reset":
            m.reset()
        elif kind == "zero":
            m.update(np.zeros((m.n, 0, 2), np.int16))
        else:
            raise KeyError(kind)
    except Refused as r:
        return r.code
    return 0


class _Feed:
    """which row every receiver hears: a blob takes its receivers' rows along"""

    def __init__(self, cfg):
        self.rows = session_rows(cfg["seed"], tuple(tuple(s) for s in cfg["specs"]))
        self.of = {e: list(cfg[e]["rows"]) for e in "ABC"}
        self.saved, self.at = {}, 0

    def op(self, op, code):
        if op[0] == "save":
            self.saved[op[4]] = self.of[op[1]][op[2]:op[2] + op[3]]
        elif op[0] == "load" and code == 0:
            got = self.saved[op[3]]
            self.of[op[1]][op[2]:op[2] + len(got)] = got

    def call(self, e, nb):
        return np.ascontiguousarray(self.rows[self.of[e], self.at * 128:(self.at + nb) * 128])

    def done(self, nb):
        self.at += nb


# ---- the draw --------------------------------------------------------------------------------------------------------------
def _fine(op):
    """the forms of an accepted op the issue asks for one by one"""
    kind = op[0]
    if kind == "tail":
        return [f"tail:{op[3]}" + (f":{op[4][0]}" if op[3] in ("setAGCmode", "setMute") else ":off" if op[3] == "setAudioFilter" and op[4][0] == 10 else "")]
    if kind == "mode":
        return [f"mode:{op[3]}"]
    if kind == "codes":
        return ["codes:" + ("none" if v == 0 else "any" if v == 0xFFFF else "inverted" if v & 0x8000 else "plain") for v in op[3]]
    if kind == "tones":
        return ["tones:" + ("none" if v == 0 else "tone") for v in op[3]]
    if kind == "set":
        a = op[4]
        return {"fm": [f"fm:W{a[0]}", "fm:tau0" if a[2] == 0 else "fm:tau"], "search": ["search:K0" if a[0] == 0 else "search:K"], "dtmf": ["dtmf:K0" if a[0] == 0 else "dtmf:K"],
                "noise": [f"noise:{a[0]}"], "afsk": [f"afsk:{a[0]}"], "pocsag": [f"pocsag:{a[0]}"], "tone": ["tone:K"], "dcs": ["dcs:K"]}[op[3]]
    return []


FINE = {"tail:setAudioFilter", "tail:setAudioFilter:off", "tail:enableAudioFilter", "tail:setAGCmode:0", "tail:setAGCmode:1", "tail:setAGCmode:2", "tail:setAGCmode:3",
        "tail:enableALSfilter", "tail:disableALSfilter", "tail:setALSfilterNotch", "tail:setALSfilterPeak", "tail:setOutputGain", "tail:setMute:0", "tail:setMute:1",
        "mode:0", "mode:1", "mode:4", "mode:7", "codes:none", "codes:any", "codes:inverted", "codes:plain", "tones:none", "tones:tone", "fm:W2", "fm:W3", "fm:tau0", "fm:tau",
        "search:K0", "search:K", "dtmf:K0", "dtmf:K", "noise:0", "noise:1", "noise:2", "afsk:0", "afsk:1", "pocsag:0", "pocsag:512", "pocsag:1200", "pocsag:2400", "tone:K",
        "dcs:K"}


# every form of FINE and every kind of op once over the seeds, whatever the draw picks: on A's side-band group and its first receiver
SWEEP = [["tail", "setAudioFilter", [3]], ["tail", "setAudioFilter", [10]], ["tail", "enableAudioFilter", []], ["tail", "setAGCmode", [1]], ["tail", "setAGCmode", [3]],
         ["tail", "setAGCmode", [0]], ["tail", "setAGCmode", [2]], ["tail", "enableALSfilter", []], ["tail", "setALSfilterPeak", []], ["tail", "setALSfilterNotch", []],
         ["tail", "disableALSfilter", []], ["tail", "setOutputGain", [0.25]], ["tail", "setMute", [1]], ["tail", "setMute", [0]], ["mode", USB], ["mode", AM], ["mode", LSB],
         ["codes", [0o023]], ["codes", [0o047 | 0x8000]], ["codes", [0xFFFF]], ["codes", [0]], ["tones", [123.0]], ["tones", [0.0]], ["set", "fm", [3, 2500.0, 0.0]],
         ["set", "fm", [2, 5000.0, 75.0]], ["set", "search", [4, 0.1, 2.0]], ["set", "search", [0, 0.04, 4.0]], ["set", "dtmf", [8] + list(LOOSE[1:])],
         ["set", "dtmf", [0] + list(LOOSE[1:])], ["set", "noise", [1, 0.01, 0.05, 3, 0.75, 0.125]], ["set", "noise", [2, 0.01, 0.025, 1, 0.75, 0.125]],
         ["set", "noise", [0, 0.01, 0.025, 8, 0.75, 0.125]], ["set", "afsk", [1, 1.25, 3, 17]], ["set", "afsk", [0, 1.0, 2, 17]], ["set", "pocsag", [512, 2, 3, 2, 1, 2]],
         ["set", "pocsag", [1200, 1, 2, 1, 2, 2]], ["set", "pocsag", [2400, 0, 3, 2, 1, 1]], ["set", "pocsag", [0, 2, 3, 2, 1, 2]], ["set", "tone", [12, 0.05, 0.03]],
         ["set", "dcs", [32, 2, 3, 2]], ["bank", [67.0, 100.0, 123.0, 254.1]], ["meter", [0.25, 0.125]], ["squelch", [1e-4, 1e-5, 1]], ["no_squelch", []], ["zero"]]


class _Draw:
    def __init__(self, seed, tab):
        self.seed, self.tab, self.r = seed, tab, np.random.default_rng(4200 + seed)
        self.ops, self.trace, self.events, self.slots = [], [], [], {}

    def pick(self, seq):
        return seq[int(self.r.integers(len(seq)))]

    def op(self, *op, expect=0):
        op = json.loads(json.dumps(list(op)))
        code = apply_op(self.ms, op, self.slots)
        assert code == expect, (op, code, expect)
        self.feed.op(op, code)
        self.ops.append(op + [code])
        self.trace.append(None)
        self.events.append(op[0] if code == 0 else f"refused_{op[0]}")
        if code == 0:
            self.events += _fine(op)
        return code

    def call(self, nb):
        r = self.r
        pack_nb = nb if r.random() < 0.7 else int(r.integers(1, nb + 1))
        cap = self.pick(["exact", "exact", "size", 0.5])
        ev_cap = self.pick(["exact", "exact", "size", "events", "words"])
        want = {}
        for e, m in self.ms.items():
            out = m.update(self.feed.call(e, nb))
            blocks, rec, needed = m.pack(pack_nb)
            capacity = 0 if cap == "size" else needed if cap == "exact" else int(needed * cap)
            out["pack"] = dict(blocks=blocks[:capacity], rec=rec[:capacity], needed=needed, capacity=capacity)
            if m.voice is not None:
                blocks, rec, needed = m.pack_voice(pack_nb)
                capacity = 0 if cap == "size" else needed if cap == "exact" else int(needed * cap)
                out["pack_voice"] = dict(blocks=blocks[:capacity], rec=rec[:capacity], needed=needed, capacity=capacity)
            out["parts"] = {p: m.part_words(p) for p in m.parts()}
            want[e] = out
        self.feed.done(nb)
        self.ops.append(["call", nb, pack_nb, cap, ev_cap])
        self.trace.append(want)
        self.events.append("call")
        self.at += nb
        self.watch(want)

    def watch(self, want):
        """what the session contained, from the models' own records"""
        w = self.what
        for e, out in want.items():
            m = self.ms[e]
            nfm = out["nfm"]
            keys = {(g.det["pocsag"][0], g.det["dtmf"][0], g.det["tone"][0], g.det["fm"]) for g in m.groups if g.nfm}
            if len(keys) >= 2 and any(not g.nfm for g in m.groups):
                w["two_keys_beside_side_band"] = True
            w["nfm_between_two_others"] |= any(g.nfm and 0 < k < len(m.groups) - 1 for k, g in enumerate(m.groups))
            sq = np.array([m.groups[m.group_of(c)].squelch for c in range(m.n)])
            w["carrier"] |= set(np.unique(out["carrier"][sq]).tolist())
            if "noise" in m.det:
                on = nfm & (m.det["noise"].mode == NZ.GATE)
                w["noise"] |= set(np.unique(out["noise"][1][on]).tolist())
                w["tone"] |= set(np.unique(out["tone"][1][nfm & (m.det["tone"].dphi != 0)]).tolist())
                w["dcs"] |= set(np.unique(out["dcs"][0][nfm & (m.det["dcs"].sel != 0)]).tolist())
                new = (out["dtmf"][1] != 255).sum(1), out["afsk"][1].astype(int).sum(1), out["pocsag"][1].astype(int).sum(1)
                for k in range(3):
                    w["items"][k] += int(new[k].sum())
                w["afsk_and_pocsag_on_one_channel"] |= bool(np.any((new[1] > 0) & (new[2] > 0)))
                w["messages_at_512"] += int(new[2][nfm & (m.det["pocsag"].baud == 512)].sum())
                w["lost"] += out["events"][1]
                w["gathered"] += len(out["events"][0])

    def fill(self, until):
        """calls and drawn ops up to block `until`; a call never crosses a protected span's inside"""
        r = self.r
        while self.at < until:
            nb = min(int(self.pick([1, 1, 2, 3, 5, 8, 13, self.maxb])), until - self.at, self.maxb)
            for a, b in self.spans:                         # one call from a to b
                if self.at == a:
                    nb = b - a
                elif self.at < a < self.at + nb:
                    nb = a - self.at
            self.call(nb)
            if self.n_bad < 8 or sum(op[0] == "call" for op in self.ops) % 2 == 0:   # a seed's share of BAD, then one behind every other call
                self.bad_op()
            if self.n_sweep < 8:
                self.sweep_op()
            for _ in range(int(r.integers(0, 3)) if self.at < until else 0):   # what is planned at `until` follows a call: no reset is pending there
                self.drawn_op()

    def groups_by_role(self, e):
        return {role: k for k, role in enumerate(self.roles[e])}

    def drawn_op(self):
        r, e = self.r, self.pick(["A", "A", "B", "C"])
        m = self.ms[e]
        g = int(r.integers(-1, len(m.groups))) if r.random() < 0.85 else -1
        role = self.roles[e][g] if g >= 0 else None
        kind = self.pick(["tail", "tail", "tail", "set", "set", "meter", "squelch", "no_squelch", "tones", "codes", "bank", "mode", "zero"])
        if kind == "tail":
            name, args = self.pick([("setAudioFilter", [int(r.integers(0, 11))]), ("enableAudioFilter", []), ("setAGCmode", [int(self.pick([0, 0, 0, 0, 0, 1, 2, 3]))]),
                                    ("enableALSfilter", []), ("disableALSfilter", []), ("disableALSfilter", []), ("disableALSfilter", []), ("setALSfilterNotch", []), ("setALSfilterPeak", []),
                                    ("setOutputGain", [float(self.pick([0.25, 0.5, 1.0, 3.0]))]), ("setMute", [int(r.integers(0, 2))])])
            self.op("tail", e, g, name, args)
        elif kind == "set":
            k = self.pick(SET_KINDS)
            if e == "C" and k != "fm":
                k = "fm"
            if k == "fm":                                   # the stations of V and P are read at their own settings
                if role in ("X", "S", "C"):
                    self.op("set", e, g, "fm", [int(self.pick([2, 3])), float(self.pick([2500.0, 5000.0, 7500.0])), float(self.pick([0.0, 75.0, 750.0]))])
            elif k == "tone" and role != "V" and g >= 0:
                self.op("set", e, g, "tone", [int(self.pick([4, 8, 12])), 0.05, 0.03])
            elif k == "search" and g >= 0:
                self.op("set", e, g, "search", [int(self.pick([0, 4, 8])), float(self.pick([0.04, 0.1])), float(self.pick([2.0, 4.0]))])
            elif k == "dcs" and role == "V":                # thresholds only: the code's window runs on
                self.op("set", e, g, "dcs", [16, 1, int(self.pick([2, 3])), int(self.pick([1, 2]))])
            elif k == "noise" and role != "V" and g >= 0:
                self.op("set", e, g, "noise", [int(r.integers(0, 3)), 0.01, float(self.pick([0.025, 0.05])), int(r.integers(0, 4)), 0.75, 0.125])
            elif k == "dtmf" and role in ("X", "S"):
                self.op("set", e, g, "dtmf", [int(self.pick([0, 4, 8]))] + list(LOOSE[1:]))
            elif k == "dtmf" and role == "P":               # thresholds only
                self.op("set", e, g, "dtmf", [4, float(self.pick([0.04, 0.05])), 2.0, float(self.pick([8.0, 10.0])), 0.3, 1, 1])
            elif k == "afsk" and role == "P":
                self.op("set", e, g, "afsk", [1, float(self.pick([1.0, 1.25])), int(self.pick([2, 3])), 17])
            elif k == "afsk" and role in ("X", "S"):
                self.op("set", e, g, "afsk", [int(r.integers(0, 2)), 1.0, 2, 17])
            elif k == "pocsag" and role == "P":
                self.op("set", e, g, "pocsag", [2400, int(self.pick([0, 2])), int(self.pick([2, 3])), int(self.pick([1, 2])), 1, 2])
            elif k == "pocsag" and role == "S":
                self.op("set", e, g, "pocsag", [int(self.pick([0, 512, 1200, 2400])), 2, 3, 2, 1, 2])
        elif kind == "meter":
            self.op("meter", e, g, float(self.pick([0.5, 0.25, 1.0])), float(self.pick([0.0625, 0.125])))
        elif kind == "squelch" and g >= 0:                  # thresholds between the levels the group's receivers show
            top = float(np.median(m.meter.level[list(m.channels(g))]))
            self.op("squelch", e, g, float(F32(0.2 * top)) if top > 0 else 1e-4, float(F32(0.02 * top)) if top > 0 else 1e-5, int(r.integers(0, 4)))
        elif kind == "no_squelch" and g >= 0 and role != "V":
            self.op("no_squelch", e, g)
        elif kind == "tones" and e != "C":
            c = int(r.integers(m.n))
            if c not in self.keep[e]:
                self.op("tones", e, c, [float(self.pick([0.0, 88.5, 100.0, 123.0]))])
        elif kind == "codes" and e != "C":
            c = int(r.integers(m.n))
            if c not in self.keep[e]:
                self.op("codes", e, c, [int(self.pick([0, 0o023, 0o047 | 0x8000, 0xFFFF]))])
        elif kind == "bank" and e != "C":
            self.op("bank", e, [float(v) for v in (TS_STANDARD[::2] if r.random() < 0.5 else TS_STANDARD)])
        elif kind == "mode" and role == "S":
            self.op("mode", e, g, int(self.pick([LSB, USB, AM])))
        elif kind == "zero":
            self.op("zero", e)

    def bad_op(self):
        """one refused setter per kind of argument check, in turn"""
        e = self.pick(["A", "A", "B"])
        g = int(self.r.integers(-1, len(self.ms[e].groups)))
        b = BAD[self.bad_at % len(BAD)]
        self.events.append(f"bad:{self.bad_at % len(BAD)}")
        self.bad_at += 1
        self.n_bad += 1
        if b[0] == "set":
            self.op("set", e, g, b[1], b[2], expect=-1)
        elif b[0] == "groups":
            self.op("groups", e, b[1], expect=-1)
        elif b[0] == "bank":
            self.op("bank", e, b[1], expect=-1)
        elif b[0] == "squelch":
            self.op("squelch", e, g, *b[1], expect=-1)
        elif b[0] == "meter":
            self.op("meter", e, g, *b[1], expect=-1)
        elif b[0] in ("tones_at", "codes_at"):              # a range outside the object
            self.op(b[0][:5], e, self.ms[e].n, b[1], expect=-1)
        else:
            self.op(b[0], e, 0, b[1], expect=-1)

    def sweep_op(self):
        b = SWEEP[self.sweep_at % len(SWEEP)]
        self.sweep_at += 1
        self.n_sweep += 1
        if b[0] in ("tail", "set"):
            self.op(b[0], "A", 0, b[1], b[2])
        elif b[0] == "mode":
            self.op("mode", "A", 0, b[1])
        elif b[0] in ("codes", "tones"):
            self.op(b[0], "A", 0, b[1])
        elif b[0] == "bank":
            self.op("bank", "A", b[1])
        elif b[0] == "zero":
            self.op("zero", "A")
        else:
            self.op(b[0], "A", 0, *b[1])

    def draw(self):
        seed, r = self.seed, self.r
        # over the seeds: a receiver moved by blob in mid-item, a call with two kinds of item on one channel, a call that loses items
        plan = ("move", "both", "six")[seed % 3]
        tm1 = int(self.pick([36, 37, 44, 45] if plan == "move" else [36, 37]))   # the blob leaves A here, inside a message, a frame and a key
        tm2 = tm1 + (16 if plan == "move" else 8)
        at = dict(move=dict(tx1=26, tx2=46, late=tm2 + 12, span=None), both=dict(tx1=26, tx2=40, late=80, span=(46, 78)),
                  six=dict(tx1=16, tx2=62, late=70, span=(22, 62)))[plan]
        self.spans = [at["span"]] if at["span"] else []
        self.maxb = max([b - a for a, b in self.spans] + [int(self.pick([24, 32, 40]))])
        sizes = dict(S=int(r.integers(1, 3)), V=int(r.integers(3, 5)), P=4 if plan != "move" else int(r.integers(3, 6)), X=int(r.integers(1, 3)))
        nA = sum(sizes.values())
        assert 8 <= nA <= 13
        v0, p0, x0 = sizes["S"], sizes["S"] + sizes["V"], sizes["S"] + sizes["V"] + sizes["P"]
        specs, rows = [], {}

        def row(*spec):
            specs.append(list(spec))
            return len(specs) - 1
        rows["A"] = [row(self.pick(["fm", "idle"])) for _ in range(sizes["S"])]
        rows["A"] += [row("dcs"), row("tone", 50), row("burst", 52)] + [row(self.pick(["idle", "burst"]), 30) for _ in range(sizes["V"] - 3)]
        rows["A"] += [row("page", tm1 - 24), row("packet", tm1 - 25), row("keypad")]
        if plan != "move":
            rows["A"].append(row(plan, 0))
        rows["A"] += [row(self.pick(["zeros", "rails", "idle"])) for _ in range(x0 - len(rows["A"]))]
        rows["A"] += [row("pages_x", at["tx2"] + 1)] + [row(self.pick(["rails", "zeros"])) for _ in range(sizes["X"] - 1)]
        nB = 3 + seed % 3
        rows["B"] = [row(self.pick(["idle", "zeros", "fm"])) for _ in range(nB - (nB > 3))] + ([row("page512")] if nB > 3 else [])
        rows["C"] = [row("burst", 40), row("idle"), row("fm")]
        cfg = dict(seed=seed, specs=specs, A=dict(n=nA, max_blocks=self.maxb + 8, rows=rows["A"], features=ALL, R=int(self.pick([2, 4]))),
                   B=dict(n=nB, max_blocks=self.maxb, rows=rows["B"], features=ALL, R=int(self.pick([2, 4]))),
                   C=dict(n=3, max_blocks=self.maxb + 4, rows=rows["C"], features=PLAIN, R=0))
        self.cfg = cfg
        self.ms = _models(cfg, self.tab)
        self.feed, self.at, self.bad_at, self.n_bad = _Feed(cfg), 0, 6 * (seed - 1), 0
        self.sweep_at, self.n_sweep = 8 * (seed - 1), 0
        self.what = dict(two_keys_beside_side_band=False, nfm_between_two_others=False, carrier=set(), noise=set(), tone=set(), dcs=set(), items=[0, 0, 0],
                         afsk_and_pocsag_on_one_channel=False, lost=0, gathered=0, messages_at_512=0, stale_page=False, restarted_by_key_alone=False, kept_by_threshold=False, left_and_returned=False,
                         moved={}, finished={})
        self.roles = dict(A=["S", "V", "P", "X"], B=[["P"], ["P", "Q"], ["P", "S", "Q"]][nB - 3], C=["C", "S"])
        self.keep = dict(A={v0, v0 + 1, v0 + 2}, B=set(), C=set())     # the receivers whose tone and code the gates' conditions rest on
        W = int(self.pick([2, 3]))
        op, what = self.op, self.what
        words = lambda e, name, c, k: int(self.ms[e].det[name].w[c, k])
        mB = self.ms["B"]
        b0 = 0
        q = p0 + 2
        mem = {}
        # ---- set-up
        op("groups", "A", [0, v0, p0, x0])
        op("mode", "A", 0, int(self.pick([LSB, USB, AM])))
        for g in (1, 2, 3):
            op("mode", "A", g, NFM)
            op("tail", "A", g, "setAGCmode", [0])
        op("set", "A", 1, "fm", [W, 5000.0, 750.0])
        op("set", "A", 1, "tone", [8, 0.04, 0.025])
        op("set", "A", 1, "search", [8, 0.04, 4.0])
        op("set", "A", 1, "dcs", [16, 1, 2, 1])
        op("set", "A", 1, "noise", [2, 0.01, 0.025, 2, 0.75, 0.125])
        op("squelch", "A", 1, 1e-3, 5e-4, 2)
        op("tones", "A", v0, [0.0, 100.0, 88.5])
        op("codes", "A", v0, [0o023, 0, 0])
        for g in (2, 3):
            op("set", "A", g, "fm", [2, 7500.0, 0.0])
            op("set", "A", g, "dtmf", list(LOOSE))
            op("set", "A", g, "afsk", [1, 1.0, 2, 17])
            op("set", "A", g, "pocsag", [2400, 2, 3, 2, 1, 2])
            op("set", "A", g, "noise", [1, 0.01, 0.025, 8, 0.75, 0.125])
        op("set", "A", 3, "search", [8, 0.04, 4.0])
        if nB > 3:                                          # Q: a paging group at 512 baud behind P (and, with five receivers, a side-band one)
            op("groups", "B", [0, 3] if nB == 4 else [0, 3, 4])
            op("mode", "B", nB - 3, NFM)
            op("tail", "B", nB - 3, "setAGCmode", [0])
            op("set", "B", nB - 3, "fm", [2, 7500.0, 0.0])
            op("set", "B", nB - 3, "pocsag", [512, 2, 3, 2, 1, 2])
            if nB == 5:
                op("mode", "B", 1, int(self.pick([USB, AM])))
        op("mode", "B", 0, NFM)
        op("tail", "B", 0, "setAGCmode", [0])
        op("set", "B", 0, "fm", [2, 7500.0, 0.0])
        op("set", "B", 0, "dtmf", list(LOOSE))
        op("set", "B", 0, "afsk", [1, 1.0, 2, 17])
        op("set", "B", 0, "pocsag", [2400, 2, 3, 2, 1, 2])
        op("groups", "C", [0, 2])
        op("mode", "C", 0, NFM)
        op("squelch", "C", 0, 1e-3, 5e-4, 1)

        # ---- the stream: what happens at which block
        def thresholds():
            mem["tb"] = words("A", "pocsag", p0, PO.TBLOCKS)
            op("set", "A", 2, "pocsag", [2400, 0, 2, 1, 1, 2])   # thresholds: nothing restarts
            op("set", "A", 2, "afsk", [1, 1.0, 3, 17])

        def thresholds_kept():
            what["kept_by_threshold"] = words("A", "pocsag", p0, PO.TBLOCKS) == mem["tb"] + 4 and words("A", "afsk", p0 + 1, AF.TBLOCKS) == 16

        def before_x_leaves():
            self.call(4)                                    # X's page closes in this call (not where X leaves at block 16)
            what["stale_page"] = bool(self.trace[-1]["A"]["pocsag"][1][x0].any())

        def x_leaves():
            op("mode", "A", 3, AM)                          # X leaves NFM; V and P sit between two side-band groups
            self.call(4)                                    # its record buffers still hold the page that closed in the call before

        def x_off():
            op("set", "A", 3, "dtmf", [0] + list(LOOSE[1:]))   # K = 0 outside NFM: the words are zeroed all the same
            op("set", "A", 3, "search", [0, 0.04, 4.0])

        def x_returns():
            op("mode", "A", 3, NFM)                         # X comes back, with another baud
            op("set", "A", 3, "pocsag", [1200, 2, 3, 2, 1, 2])
            op("set", "A", 3, "dtmf", list(LOOSE))

        def x_restarted():
            what["left_and_returned"] = words("A", "pocsag", x0, PO.TBLOCKS) == 4 and words("A", "pocsag", x0, PO.BAUD) == 1200

        def leave_a():
            what["moved"] = dict(message=words("A", "pocsag", p0, PO.INSYNC) == 1 and words("A", "pocsag", p0, PO.OPEN) == 1,
                                 frame=words("A", "afsk", p0 + 1, AF.INFRAME) == 1, key=words("A", "dtmf", p0 + 2, DT.CUR1) != 0, other_index=b0 != p0)
            op("save", "A", p0, 3, "m1")
            if plan != "six":
                op("load", "B", b0, "m1")
            op("load", "C", 0, "m1", expect=-4)             # C lacks ten of the blob's parts
            mem["counts"] = [int(mB.det[k].w[b0 + i, j]) for i, (k, j) in enumerate((("pocsag", PO.NMSGS), ("afsk", AF.NFRAMES), ("dtmf", DT.NDIGITS)))]

        def back_to_a():
            what["finished"] = dict(message=int(mB.det["pocsag"].w[b0, PO.NMSGS]) > mem["counts"][0], key=int(mB.det["dtmf"].w[b0 + 2, DT.NDIGITS]) > mem["counts"][2])
            mem["frames"] = words("B", "afsk", b0 + 1, AF.NFRAMES)
            what["moved"]["frame"] &= words("B", "afsk", b0 + 1, AF.INFRAME) == 1
            op("save", "B", b0 + 1, 1, "m2")
            op("load", "A", q, "m2")                        # back in A at a third index
            what["moved"]["third_index"] = q not in (p0 + 1, b0 + 1)

        def boundary():
            if plan != "six":
                what["finished"]["frame"] = words("A", "afsk", q, AF.NFRAMES) > mem["frames"]
            op("groups", "A", [0, v0, p0 + 1, x0])          # P's first receiver joins V: every detector key of its differs

        def split():
            op("groups", "A", [0, v0, p0 + 1, p0 + 2, x0])  # a split of P: the new group copies P's settings, not group 0's
            self.roles["A"] = ["S", "V", "P", "P", "X"]
            op("tail", "A", 3, "setAudioFilter", [int(r.integers(0, 10))])
            op("groups", "A", [0, v0, p0 + 1, x0], expect=-5)   # a merge of groups with other resets pending

        def from_c():
            op("save", "C", 0, 1, "c1")
            op("load", "A", v0 + 2, "c1")                   # a blob without ten of the parts: they are zeros where it lands
            op("set", "A", 3, "pocsag", [1200, 2, 3, 2, 1, 2])   # the halves of P now differ in a key

        def merge():
            # half of P changed its baud with no FM reset pending: its detectors started anew four blocks ago
            what["restarted_by_key_alone"] = words("A", "pocsag", p0 + 2, PO.TBLOCKS) == 4 and words("A", "pocsag", p0 + 2, PO.BAUD) == 1200 and \
                words("A", "afsk", p0 + 2, AF.TBLOCKS) > 4
            op("groups", "A", [0, v0, p0 + 1, x0])
            self.roles["A"] = ["S", "V", "P", "X"]

        late = at["late"]
        todo = [(12, thresholds), (16, thresholds_kept), (at["tx1"] - 4, before_x_leaves), (at["tx1"], x_leaves), (at["tx1"] + 4, x_off), (at["tx2"], x_returns), (at["tx2"] + 4, x_restarted),
                (22 if plan == "six" else tm1, leave_a), (late, boundary), (late + 2, split), (late + 4, from_c), (late + 8, merge), (89, lambda: op("reset", "B")), (93, lambda: op("reset", "A"))]
        if plan != "six":
            todo.append((tm2, back_to_a))
        for when, what_to_do in sorted(todo, key=lambda v: v[0]):
            assert not any(a < when < b for a, b in self.spans) and when >= self.at, (plan, when)
            self.fill(when)
            what_to_do()
        self.fill(T)
        return dict(cfg=cfg, ops=self.ops), self.trace, dict(self.what, events=self.events, plan=plan)


TS_STANDARD = [float(v) for v in N.TS.STANDARD]


def _models(cfg, tab):
    return {e: N.NfmSessionModel(cfg[e]["n"], cfg[e]["max_blocks"], tab, dict(cfg[e]["features"], voice=cfg[e]["R"])) for e in "ABC"}


@functools.lru_cache(maxsize=None)
def _tab():
    import radiodsp_sdr_rx_amd as R
    return S.table(R)


@functools.lru_cache(maxsize=None)
def model_run(seed):
    """draw_session(seed): (the script, per op what the engines must show, what the session contained), once per process"""
    return _Draw(seed, _tab()).draw()


def draw_session(seed):
    """-> {"cfg": the three engines and the rows' descriptions; "ops": the list of ops}, the same for the same seed"""
    return model_run(seed)[0]


# ---- CPU -------------------------------------------------------------------------------------------------------------------
def test_nfm_session_model_is_the_existing_restatements(rdsp, oracle):
    """one fixed script with every detector on and no regrouping or blob -- seven receivers in three groups, a side-band one,
    a voice channel (tone, code, noise squelch, tone search) and a paging channel (DTMF, AFSK, POCSAG), 56 blocks as [7, 1, 12, 20, 16]:
    the NfmSessionModel call by call equals each feature model run over the whole stream in one piece, for records, words and
    audio, bit for bit"""
    tab = _tab()
    specs = (("fm",), ("dcs",), ("tone", 30), ("burst", 20), ("page", 0), ("packet", 0), ("keypad",))
    x = session_rows(77, specs)[:, :56 * 128]
    m = N.NfmSessionModel(7, 20, tab, dict(ALL, voice=2))
    m.set_groups([0, 1, 4])
    m.call(0, "setDemodMode", USB)
    for g in (1, 2):
        m.call(g, "setDemodMode", NFM)
        m.call(g, "setAGCmode", 0)
    m.set(1, "tone", 8, 0.04, 0.025); m.set(1, "search", 8, 0.04, 4.0); m.set(1, "dcs", 16, 1, 2, 1); m.set(1, "noise", 2, 0.01, 0.025, 2, 0.75, 0.125)
    m.set_squelch(1, 1e-3, 5e-4, 2)
    m.set_tones(1, [0.0, 100.0, 88.5]); m.set_dcs_codes(1, [0o023, 0, 0])
    m.set(2, "fm", 2, 7500.0, 0.0); m.set(2, "dtmf", *LOOSE); m.set(2, "afsk", 1, 1.0, 2, 17); m.set(2, "pocsag", 2400, 2, 3, 2, 1, 2)
    outs, a = [], 0
    for k in (7, 1, 12, 20, 16):
        outs.append(m.update(x[:, a * 128:(a + k) * 128]))
        a += k
    cat = lambda f: np.concatenate([f(o) for o in outs], 1)
    # the whole stream in one piece, feature by feature
    o = oracle.OracleEngine(taps=True)
    o.call("setDemodMode", USB)
    o.run(x[0])
    demod = [np.concatenate([t[0] for t in o.taps["demod"]])[None]]
    yv, lv = FM.Fm(3, 2, 5000.0, 750.0).run(x[1:4])
    yp, lp = FM.Fm(3, 2, 7500.0, 0.0).run(x[4:7])
    demod = np.concatenate(demod + [yv, yp])
    assert same_bits(cat(lambda o: o["demod"]), demod) and same_bits(cat(lambda o: o["fm_level"])[1:], np.concatenate([lv, lp]))
    tails = [N.TM.Tail(1), N.TM.Tail(6).setAGCmode(0)]
    audio = np.concatenate([tails[0].run(demod[:1]), tails[1].run(demod[1:])])
    sq = [N.M.Squelch()] + [N.M.Squelch(F32(1e-3), F32(5e-4), 2)] * 3 + [N.M.Squelch()] * 3
    level, peak, carrier = N.M.Meter(7).run(np.concatenate([demod[:1], lv, lp]), sq)
    assert same_bits(cat(lambda o: o["level"]), level) and same_bits(cat(lambda o: o["peak"]), peak) and np.array_equal(cat(lambda o: o["carrier"]), carrier)
    nz = NZ.Noise(3, NZ.GATE, 2, 750.0, hang_blocks=2)
    tn = TN.Tone(3, tab, [0.0, 100.0, 88.5], 8)
    ts = N.TS.Search(3, tab, K=8)
    dc = DC.Dcs(3, [0o023, 0, 0], 16, 1, 2, 1)
    rec = dict(noise=nz.run(yv), tone=tn.run(yv), search=ts.run(yv), dcs=dc.run(yv))
    gate = carrier.copy()
    gate[1:4] = dc.gate(tn.gate(nz.gate(carrier[1:4], rec["noise"][1]), rec["tone"][1]), rec["dcs"][0])
    dt, af, po = DT.Dtmf(3, tab, *LOOSE), AF.Afsk(3, tab, 1), PO.Pocsag(3, 2400)
    rec.update(dtmf=dt.run(yp), afsk=af.run(yp), pocsag=po.run(yp))
    assert np.array_equal(cat(lambda o: o["gate"]), gate) and gate[1:4].min() == 0 and gate[1:4].max() == 1
    audio = N.M.gated(audio, gate)
    assert np.array_equal(cat(lambda o: o["audio"]), audio) and audio[0].any() and audio[4:].any()
    assert np.array_equal(cat(lambda o: o["voice"]), N.V.Voice(7, 2).run(audio))
    for name, sel, d in (("noise", slice(1, 4), nz), ("tone", slice(1, 4), tn), ("search", slice(1, 4), ts), ("dcs", slice(1, 4), dc), ("dtmf", slice(4, 7), dt),
                         ("afsk", slice(4, 7), af), ("pocsag", slice(4, 7), po)):
        for k, want in enumerate(rec[name]):
            got = cat(lambda o: o[name][k])
            assert same_bits(got[sel], want), (name, k, _first_difference(got[sel], want))
            rest = np.delete(got, np.r_[sel], 0)
            assert (rest == N.IDLE[name][k]).all(), (name, k)
        assert np.array_equal(m.det[name].w[sel], d.w), name
        assert not np.delete(m.det[name].w, np.r_[sel], 0).any(), name
    assert rec["dtmf"][1].min() < 255 and rec["afsk"][1].any() and rec["pocsag"][1].any() and rec["tone"][1].any() and rec["noise"][1].any()
    # the events of the last call are the events model on the whole-stream models' own words and the call's records
    new = [np.full((7, 16), 255, np.uint8), np.zeros((7, 16), np.uint8), np.zeros((7, 16), np.uint8)]
    for k, name in enumerate(("dtmf", "afsk", "pocsag")):
        new[k][4:7] = rec[name][1][:, 40:]
    count = [np.concatenate([np.zeros(4, U32), v]) for v in (dt.digits()[0], af.ring()[0], po.ring()[0])]
    ring = [np.concatenate([np.zeros((4,) + v.shape[1:], U32), v]) for v in (dt.digits()[1], af.ring()[1], po.ring()[1])]
    want, lost = EV.sequence(new, count, ring)
    got, lost_m = outs[-1]["events"]
    assert lost == lost_m and [(c, k, s, p.tolist()) for c, k, s, p in got] == [(c, k, s, p.tolist()) for c, k, s, p in want]


def test_nfm_drawn_sessions_contain_what_they_are_for(rdsp, oracle):
    """the conditions of docs/engine.md on the six drawn sessions: no script raises Unmodelled (model_run would) and the draw
    is the same twice; over the seeds every kind of op and every kind of refusal; in every seed a call in which two NFM groups
    with different detector keys run beside a side-band group, every squelch gate open and closed, an item of every decoder;
    over the seeds a call that loses items, a call with an AFSK and a POCSAG item on one channel, a detector restarted by a
    changed key and one kept through changed thresholds, a group that leaves NFM and returns, a receiver that moves by blob
    inside a message, a frame and a key to another index and finishes there, a refused merge and a refused blob"""
    whats = {}
    for seed in SEEDS:
        script, trace, what = model_run(seed)
        whats[seed] = what
        cfg = script["cfg"]
        assert 8 <= cfg["A"]["n"] <= 13 and 3 <= cfg["B"]["n"] <= 5 and cfg["A"]["max_blocks"] != cfg["B"]["max_blocks"], seed
        assert sum(op[1] for op in script["ops"] if op[0] == "call") == T and len(trace) == len(script["ops"])
        assert all(1 <= op[1] <= cfg["B"]["max_blocks"] for op in script["ops"] if op[0] == "call")
        assert what["two_keys_beside_side_band"] and what["nfm_between_two_others"], seed
        for gate in ("carrier", "noise", "tone", "dcs"):
            assert what[gate] == {0, 1}, (seed, gate, what[gate])
        assert all(what["items"]), (seed, what["items"])
        assert what["gathered"] >= 6, (seed, what["gathered"])
    assert json.dumps(_Draw(SEEDS[0], _tab()).draw()[0]) == json.dumps(model_run(SEEDS[0])[0])
    events = set().union(*(set(w["events"]) for w in whats.values()))
    assert OP_KINDS <= events, OP_KINDS - events
    assert {"refused_groups", "refused_load", "refused_set", "refused_tones", "refused_codes", "refused_bank", "refused_squelch", "refused_meter"} <= events, events
    refused = {(op[3], tuple(op[4])) for s in SEEDS for op in model_run(s)[0]["ops"] if op[0] == "set" and op[-1] == -1}
    assert {k for k, _ in refused} == set(SET_KINDS), refused
    assert {f"bad:{k}" for k in range(len(BAD))} <= events, sorted(k for k in range(len(BAD)) if f"bad:{k}" not in events)
    assert FINE <= events, sorted(FINE - events)
    assert any(w["messages_at_512"] for w in whats.values()) and any(w["stale_page"] for w in whats.values())
    assert any(w["lost"] > 0 for w in whats.values()) and any(w["afsk_and_pocsag_on_one_channel"] for w in whats.values())
    assert any(w["restarted_by_key_alone"] for w in whats.values()) and any(w["kept_by_threshold"] for w in whats.values())
    assert any(w["left_and_returned"] for w in whats.values())
    assert any(all(w["moved"].values()) and all(w["finished"].values()) for w in whats.values()), [(w["moved"], w["finished"]) for w in whats.values()]
    codes = {op[-1] for s in SEEDS for op in model_run(s)[0]["ops"] if op[0] in ("groups", "load")}
    assert {-5, -4} <= codes


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _host(v):
    return v.cpu().numpy()


class _Gpu:
    """the three engines of a script"""

    def __init__(self, cfg):
        import oracle_lib
        from radiodsp_sdr_rx_amd.engine import Engine
        self.eng, self.blobs = {}, {}
        for e in "ABC":
            c = cfg[e]
            eng = Engine(c["n"], max_blocks_per_call=c["max_blocks"], tables=oracle_lib.engine_tables())
            eng.sketch_setup()
            eng.enable_meter()
            eng.enable_fm()
            if c["R"]:
                eng.enable_voice(c["R"])
            for k in ("tone", "tone_search", "dcs", "noise", "dtmf", "afsk", "pocsag"):
                if c["features"].get("search" if k == "tone_search" else k):
                    getattr(eng, "enable_" + k)()
            self.eng[e] = eng

    def close(self):
        for e in self.eng.values():
            e.close()

    def _do(self, op):
        kind, eng = op[0], self.eng[op[1]]
        if kind == "groups":
            return eng.set_groups(op[2])
        if kind == "save":
            self.blobs[op[4]] = eng.save_state(op[2], op[3])
            return
        if kind == "load":
            return eng.load_state(op[2], self.blobs[op[3]])
        if kind == "reset":
            return eng.reset()
        if kind == "tones":
            return eng.set_tones(op[2], op[3])
        if kind == "codes":
            return eng.set_dcs_codes(op[2], op[3])
        if kind == "bank":
            return eng.set_tone_bank(op[2])
        if kind == "zero":
            import torch
            x = torch.zeros((eng.n_channels, 128, 2), dtype=torch.int16, device="cuda")
            rc = eng.lib.rdsp_engine_update(eng.h, x.data_ptr(), 128, 0, x.data_ptr(), 128, None)
            assert rc == 0
            return
        eng.select_group(op[2])
        try:
            if kind == "mode":
                eng.setDemodMode(op[3])
            elif kind == "tail":
                getattr(eng, op[3])(*op[4])
            elif kind == "set":
                name = dict(fm="set_fm", tone="set_tone_squelch", search="set_tone_search", dcs="set_dcs_squelch", noise="set_noise_squelch", dtmf="set_dtmf",
                            afsk="set_afsk", pocsag="set_pocsag")[op[3]]
                getattr(eng, name)(*op[4])
            elif kind == "meter":
                eng.set_meter(op[3], op[4])
            elif kind == "squelch":
                eng.set_squelch(op[3], op[4], op[5])
            elif kind == "no_squelch":
                eng.disable_squelch()
            else:
                raise KeyError(kind)
        finally:
            eng.select_group(-1)

    def op(self, op, ctx, rdsp):
        """an op that is not a call; a predicted refusal raises with the header's code and leaves the blob as it was"""
        code = op[-1]
        if code == 0:
            self._do(op[:-1])
            return
        eng = self.eng[op[1]]
        before = eng.save_state(0, eng.n_channels)
        with pytest.raises(rdsp.RdspError) as ex:
            self._do(op[:-1])
        assert ex.value.code == code, (ctx, ex.value.code, code)
        assert np.array_equal(eng.save_state(0, eng.n_channels), before), (ctx, "a refused call changed the state")


def _blob_parts(blob, n, flags):
    """the optional parts of a blob by name, uint32 [n, words]"""
    w = blob[16:].view(U32)
    at, out = n * N.CORE_WORDS, {}
    for name, flag in N.FLAGS.items():
        if flags & flag:
            k = N.PART_WORDS[name]
            out[name] = w[at:at + n * k].reshape(n, k)
            at += n * k
    assert at == len(w)
    return out


def _packed(ctx, name, call, p, width):
    """a pack entry point into sentinel-filled buffers: counts, records, blocks and the sentinels behind `written`"""
    import torch
    room = p["needed"] + 4
    a = torch.full((room, width), -21846, dtype=torch.int16, device="cuda")
    r = torch.full((room, 2), -7, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    sizing = p["capacity"] == 0
    rc = call(None if sizing else a.data_ptr(), None if sizing else r.data_ptr(), p["capacity"], cnt.data_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (ctx, name)
    w = min(p["needed"], p["capacity"])
    assert cnt.tolist() == [p["needed"], w], (ctx, name, "counts", cnt.tolist(), [p["needed"], w])
    a, r = _host(a), _host(r)
    _check(ctx, name + " records", r[:w], p["rec"])
    _check(ctx, name + " blocks", a[:w], p["blocks"])
    assert np.all(a[w:] == -21846) and np.all(r[w:] == -7), (ctx, name, "written behind `written`")


def _check_events(ctx, eng, want, ev_cap):
    events, lost = want
    full = EV.cut(events, lost)
    got = E.gather(eng)                                     # a sizing call, then exactly what is needed
    assert got[2] == full[2], (ctx, "gather counts", got[2], full[2])
    _check(ctx, "gather records", got[0], full[0])
    _check(ctx, "gather words", got[1], full[1])
    ne, nw = full[2][0], full[2][2]
    ce, cw = dict(exact=(ne, nw), size=(0, 0), events=(ne // 2, nw), words=(ne, max(nw - 1, 0)))[ev_cap]
    cut = EV.cut(events, lost, ce, cw)
    raw = E.raw_gather(eng, ce, cw)                         # the entry point into sentinel-filled buffers
    assert raw[2] == cut[2], (ctx, "gather counts under capacities", (ce, cw), raw[2], cut[2])
    _check(ctx, "gather records under capacities", raw[0], cut[0])
    _check(ctx, "gather words under capacities", raw[1], cut[1])


def _check_call(eng, op, want, y, ptr, stride, ctx):
    """everything an engine shows after a call against the model's `want`"""
    _, nb, pack_nb, cap, ev_cap = op
    _check(ctx, "audio L against R", y[..., 0], y[..., 1])
    _check(ctx, "audio", y[..., 0], want["audio"])
    _check(ctx, "read_demod", _host(eng.read_demod(nb)), want["demod"], bits=True)
    _check(ctx, "read_fm_level", _host(eng.read_fm_level(nb)), want["fm_level"], bits=True)
    level, peak, gate = (_host(v) for v in eng.read_meter(nb))
    _check(ctx, "gate", gate, want["gate"])
    _check(ctx, "level", level, want["level"], bits=True)
    _check(ctx, "peak", peak, want["peak"], bits=True)
    lst, cnt = eng.active()
    assert cnt == len(lst), ctx
    _check(ctx, "active", _host(lst), want["active"])
    _check(ctx, "meter", eng.meter(), want["meter"], bits=True)
    reads = dict(noise="read_noise", tone="read_tone", search="read_tone_search", dcs="read_dcs", dtmf="read_dtmf", afsk="read_afsk", pocsag="read_pocsag")
    for name, read in reads.items():
        if name in want:
            for k, (g, w) in enumerate(zip(getattr(eng, read)(nb), want[name])):
                g = _host(g)
                _check(ctx, f"{read}[{k}]", g.view(U32) if g.dtype == np.int32 else g, w, bits=w.dtype == F32)
    if "spectrum" in want:
        _check(ctx, "read_tone_spectrum", _host(eng.read_tone_spectrum()), want["spectrum"], bits=True)
    for k, read in enumerate(("read_dtmf_digits", "read_afsk_ring", "read_pocsag_ring")):
        if want["rings"][k] is not None:
            count, ring = (_host(v).view(U32) for v in getattr(eng, read)())
            _check(ctx, read + " count", count, want["rings"][k][0])
            _check(ctx, read + " ring", ring, want["rings"][k][1])
    lib, h = eng.lib, eng.h
    _packed(ctx, "pack_active", lambda a, r, c, n: lib.rdsp_engine_pack_active(h, ptr, stride, pack_nb, a, r, c, n, None), want["pack"], 128)
    if "voice" in want:
        R = eng.voice_rate
        _check(ctx, "read_voice", _host(eng.read_voice(nb)), want["voice"])
        _packed(ctx, "pack_voice", lambda a, r, c, n: lib.rdsp_engine_pack_voice(h, pack_nb, a, r, c, n, None), want["pack_voice"], 128 // R)
    if "dtmf" in want:
        _check_events(ctx, eng, want["events"], ev_cap)
    n = eng.n_channels
    blob = eng.save_state(0, n)
    flags = int(blob.view(U32)[3])
    assert flags == sum(N.FLAGS[p] for p in want["parts"]), (ctx, "blob flags", flags)
    for name, got in _blob_parts(blob, n, flags).items():
        _check(ctx, f"blob part {name}", got, want["parts"][name])


def _call(eng, x, nb, odd):
    """update() into a buffer of its own with, on odd calls, a row stride above the call's and sentinels around -> (view, ptr, stride)"""
    import torch
    n = eng.n_channels
    stride = nb * 128 + (64 if odd else 0)
    buf = torch.full((n * stride + 1, 2), 7, dtype=torch.int16, device="cuda")
    view = buf[1:].reshape(n, stride, 2)[:, :nb * 128]
    d = torch.from_numpy(x).cuda()
    ptr = buf[1:].data_ptr()
    rc = eng.lib.rdsp_engine_update(eng.h, d.data_ptr(), nb * 128, nb, ptr, stride, None)
    assert rc == 0, eng.lib.rdsp_last_error()
    torch.cuda.synchronize()
    if odd:
        assert bool((buf[1:].reshape(n, stride, 2)[:, nb * 128:] == 7).all()) and int(buf[0, 0]) == 7
    return view, ptr, stride


@pytest.mark.gpu
@pytest.mark.parametrize("seed", SEEDS)
def test_gpu_engine_nfm_drawn_sessions(rdsp, seed):
    """the drawn session of `seed` on the three engines: after every call the int16 audio (L == R, gated), read_demod,
    read_fm_level, read_meter, active(), meter(), every detector's records, the tone spectrum, the decoders' counts and rings,
    pack_active and pack_voice (a sizing call or a capacity, the sentinels behind `written`), read_voice, gather_events (a sizing
    call, then exact or short capacities through the raw entry point) and every optional part of save_state(0, n) equal the
    model's, bit for bit; every predicted refusal raises with its code and leaves the blob as it was"""
    t0 = time.time()
    script, trace, _ = model_run(seed)
    t1 = time.time()
    cfg, ops = script["cfg"], script["ops"]
    gpu, feed, n_call = _Gpu(cfg), _Feed(cfg), 0
    for k, op in enumerate(ops):
        if op[0] != "call":
            gpu.op(op, f"seed {seed}, op {k} {op}", rdsp)
            feed.op(op, op[-1])
            if op[0] in ("zero", "reset", "load") and op[-1] == 0 and op[1] != "C":
                assert E.gather(gpu.eng[op[1]])[2] == (0, 0, 0, 0, 0), (seed, k, op, "gathered counts behind it")
            continue
        nb = op[1]
        for e in "ABC":
            ctx = f"seed {seed}, op {k} {op}, call {n_call}, engine {e}"
            view, ptr, stride = _call(gpu.eng[e], feed.call(e, nb), nb, odd=n_call % 2 == 1)
            _check_call(gpu.eng[e], op, trace[k][e], _host(view), ptr, stride, ctx)
        feed.done(nb)
        n_call += 1
    gpu.close()
    print(f"seed {seed}: {n_call} calls, {len(ops)} ops, model {t1 - t0:.1f} s, engines and comparisons {time.time() - t1:.1f} s")


RECORDS = dict(read_meter=None, read_noise="noise_enabled", read_tone="tone_enabled", read_tone_search="tone_search_enabled", read_dcs="dcs_enabled",
               read_dtmf="dtmf_enabled", read_afsk="afsk_enabled", read_pocsag="pocsag_enabled")


def _play(cfg, ops, rdsp):
    """a script on the engines alone -> per engine the audio and every record row over the stream, the final blob, the decoders'
    counts and rings at the end and the gathered items of every call with what was lost.  An item's key is (the last op in front
    of its call that was no call, channel, kind, seq): a detector restarts, and its seq with it, only behind such an op, and the
    ops lie at the same blocks however the calls between them are cut"""
    gpu, feed, last_op = _Gpu(cfg), _Feed(cfg), -1
    got = {e: dict(audio=[], rec={}, gathered={}, lost=0, twice=0) for e in "ABC"}
    for k, op in enumerate(ops):
        if op[0] != "call":
            gpu.op(op, f"op {k} {op}", rdsp)
            feed.op(op, op[-1])
            last_op = sum(1 for o in ops[:k + 1] if o[0] != "call")
            continue
        nb = op[1]
        for e in "ABC":
            eng, g = gpu.eng[e], got[e]
            view, _, _ = _call(eng, feed.call(e, nb), nb, odd=False)
            g["audio"].append(_host(view)[..., 0])
            for read, enabled in RECORDS.items():
                if enabled is None or getattr(eng, enabled):
                    for j, v in enumerate(getattr(eng, read)(nb)):
                        g["rec"].setdefault((read, j), []).append(_host(v))
            if eng.dtmf_enabled:
                records, words, counts = E.gather(eng)
                g["lost"] += counts[4]
                for ch, kw, seq, off in records.tolist():
                    key = (last_op, ch, kw & 0xFF, seq)
                    g["twice"] += key in g["gathered"]
                    g["gathered"][key] = words[off:off + (kw >> 8)].tobytes()
        feed.done(nb)
    for e, g in got.items():
        eng = gpu.eng[e]
        g["audio"] = np.concatenate(g["audio"], 1)
        g["rec"] = {k: np.concatenate(v, 1) for k, v in g["rec"].items()}
        g["blob"] = eng.save_state(0, eng.n_channels)
        if eng.dtmf_enabled:
            g["rings"] = [_host(v).view(U32) for read in (eng.read_dtmf_digits, eng.read_afsk_ring, eng.read_pocsag_ring) for v in read()]
    gpu.close()
    return got


def _recut_nfm(ops, way):
    """test_engine_sessions._recut on this file's calls: every run of calls cut into calls of one block, or of 2, 1, 2, 1 ..."""
    marked = [["call", "iq", op[1]] if op[0] == "call" else op for op in ops]
    return [["call", op[2], op[2], "exact", "exact"] if op[0] == "call" else op for op in _recut(marked, way)]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", CUT_SEEDS)
def test_gpu_engine_nfm_sessions_do_not_depend_on_the_call_cut(rdsp, seed):
    """the drawn session of `seed` as drawn, with every run of calls cut into calls of one block, and into calls of 2, 1, 2, 1 ...
    blocks, the ops at the same blocks.  Engine against engine the audio over the stream, every record row over the stream, the
    final blob and the decoders' counts and rings at the end are the same bytes; every (channel, kind, seq) is gathered exactly
    once over a way's calls, and a way that lost nothing gathered every item another way gathered, with the same payload words"""
    script, _, _ = model_run(seed)
    cfg, ops = script["cfg"], script["ops"]
    as_drawn = _play(cfg, ops, rdsp)
    assert sum(len(g["gathered"]) for g in as_drawn.values()) >= 6
    for way in (1, 2):
        other = _play(cfg, _recut_nfm(ops, way), rdsp)
        for e in "ABC":
            ctx = f"seed {seed}, cut {way}, engine {e}"
            a, b = as_drawn[e], other[e]
            _check(ctx, "audio", b["audio"], a["audio"])
            assert a["rec"].keys() == b["rec"].keys(), ctx
            for key in a["rec"]:
                _check(ctx, f"{key[0]}[{key[1]}]", b["rec"][key], a["rec"][key], bits=a["rec"][key].dtype == F32)
            _check(ctx, "final blob", b["blob"], a["blob"])
            for k, (ra, rb) in enumerate(zip(a.get("rings", []), b.get("rings", []))):
                _check(ctx, f"counts and rings {k}", rb, ra)
            assert a["twice"] == 0 and b["twice"] == 0, (ctx, "an item gathered twice")
            assert b["lost"] == 0, (ctx, "calls of one or two blocks lose nothing")
            for key, payload in a["gathered"].items():
                assert b["gathered"].get(key) == payload, (ctx, "gathered item", key)
            if a["lost"] == 0:
                assert a["gathered"].keys() == b["gathered"].keys(), (ctx, set(a["gathered"]) ^ set(b["gathered"]))
