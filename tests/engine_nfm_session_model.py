"""One rdsp_engine_t object with narrow-band FM, its squelches, decoders and events on the CPU, call by call: NfmSessionModel,
for tests/test_engine_nfm_sessions.py.

It adds no arithmetic.  It is composed of the restatements the suite already has: engine_fm_model.Fm gives y and the level rows
of a group in NFM; a receiver outside NFM is an oracle_lib.OracleEngine(taps=True) up to its "demod" tap; from that tap on
engine_tail_model.Tail gives the audio of both (tests/test_engine_fm.py holds that split bit for bit), so the tail's state is
continuous when a group enters or leaves NFM; engine_meter_model.Meter runs on the level rows in NFM and on the tap otherwise;
the detectors are engine_noise_model.Noise, engine_tone_model.Tone, engine_tone_search_model.Search, engine_dcs_model.Dcs,
engine_dtmf_model.Dtmf, engine_afsk_model.Afsk and engine_pocsag_model.Pocsag; engine_voice_model, engine_pack_model and
engine_events_model give the voice rows, the packs and the gathered events.  Fm and Tail carry one setting for all their
channels, so a call builds one of each per set of settings in force, hands it the state of the channels that run under them
and takes the state back; the detectors carry per-channel settings and are handed their groups' before every call.  State is
carried from call to call; nothing is recomputed from block 0.

What the model owns are the rules of include/rdsp.h between the features: which settings a new group copies; the per-channel
tables, which no regrouping moves; the pending resets and the refused merge; what each detector does in a call of a group that
is not in NFM (nothing -- but the tone search and the DTMF decoder zero the words of a group whose K is 0 whatever its mode);
what restarts a detector (the models compare their stored keys themselves) and what "off" clears; what reset zeroes; the eleven
optional parts of a blob; when the gathered counts are zeros.  A refused call raises engine_session_model.Refused with the
header's code and leaves the model as it was.

setDemodMode clears the IF filter of an OracleEngine when it is called and of the product at the next update, and a side-band
receiver's restatement holds its mode itself.  So a receiver may join a side-band group (by set_groups or by blob) only in the
mode its restatement is in, or before its front has run since a reset, and no blob is taken of a group with that reset
pending: Unmodelled (the script is wrong, not the product).  The audio filter's, the ALS filter's and the FM reset are the
model's own pending resets and follow the product's timing."""
import copy

import numpy as np

import engine_afsk_model as AF
import engine_dcs_model as DC
import engine_dtmf_model as DT
import engine_events_model as EV
import engine_fm_model as FM
import engine_meter_model as M
import engine_noise_model as NZ
import engine_pack_model as PK
import engine_pocsag_model as PO
import engine_tail_model as TM
import engine_tone_model as TN
import engine_tone_search_model as TS
import engine_voice_model as V
import oracle_lib
from engine_session_model import SKETCH, Refused, Unmodelled, apply_setting

F32 = np.float32
U32 = np.uint32
NFM = 7
SIDE_MODES = (0, 1, 2, 3, 4, 5, 6)
DETECTORS = ("tone", "search", "dcs", "noise", "dtmf", "afsk", "pocsag")
FLAGS = dict(meter=2, voice=4, fm=8, tone=16, search=32, dcs=64, noise=128, dtmf=256, afsk=512, pocsag=1024)   # the blob's header flags
PART_WORDS = dict(meter=3, voice=V.HIST, fm=FM.STATE_WORDS, tone=TN.WORDS, search=TS.WORDS, dcs=DC.WORDS, noise=NZ.WORDS, dtmf=DT.WORDS,
                  afsk=AF.WORDS, pocsag=PO.WORDS)
CORE_WORDS = 96 + 2 * 512 + 3 * 384 + 320                  # a channel's words in front of the optional parts
TAIL_KEYS = ("audio_id", "audio_on", "agc_mode", "agc_on", "als_on", "als_notch", "output_gain", "mute")
DEFAULTS = dict(fm=(2, 5000.0, 750.0), tone=(128, 0.04, 0.025), search=(0, 0.04, 4.0), dcs=(64, 1, 16, 12), noise=(0, 0.01, 0.025, 8, 0.75, 0.125),
                dtmf=(0, 0.015, 4.0, 16.0, 0.5, 2, 2), afsk=(0, 1.0, 2, 17), pocsag=(0, 2, 3, 2, 1, 2))
# what a receiver the detector did not run on reads, by record
IDLE = dict(tone=(0, 0), search=(255, 0, 0), dcs=(0, 0, 0), noise=(0, 0), dtmf=(255, 255, 0, 0), afsk=(0, 0, 0, 0), pocsag=(0, 0, 0, 0, 0))


def _finite(*v):
    return all(np.isfinite(float(x)) for x in v)


def check_setting(kind, a):
    """the argument checks of include/rdsp.h for a group's settings -> Refused(-1)"""
    ok = False
    if kind == "fm":
        W, dev, tau = a
        ok = W in (2, 3) and _finite(dev, tau) and 1000.0 <= dev <= 7500.0 and (tau == 0 or 25.0 <= tau <= 1000.0)
    elif kind == "tone":
        K, on, off = a
        ok = 4 <= K <= 512 and _finite(on, off) and 0 < off <= on <= 1
    elif kind == "search":
        K, mn, ratio = a
        ok = (K == 0 or 4 <= K <= 512) and _finite(mn, ratio) and 0 < mn <= 1 and 1 <= ratio <= 1e6
    elif kind == "dcs":
        K, err, on, off = a
        ok = 8 <= K <= 512 and 0 <= err <= 3 and 1 <= off <= on <= DC.max_hits(K)
    elif kind == "noise":
        mode, op, cl, hang, fall, rise = a
        ok = mode in (0, 1, 2) and _finite(op, cl, fall, rise) and 0 < op <= cl and 0 <= hang <= 65535 and 0 < fall <= 1 and 0 < rise <= 1
    elif kind == "dtmf":
        K, mn, ratio, twist, share, on, off = a
        ok = (K == 0 or 4 <= K <= 32) and _finite(mn, ratio, twist, share) and 0 < mn <= 1 and 1 <= ratio <= 1e6 and 1 <= twist <= 1e6 and \
            0 < share <= 1 and 1 <= on <= 16 and 1 <= off <= 16
    elif kind == "afsk":
        on, g, pull, mb = a
        ok = on in (0, 1) and _finite(g) and 1.0 / 16 <= g <= 16 and 1 <= pull <= 4 and 9 <= mb <= 330
    elif kind == "pocsag":
        baud, inv, pull, se, fa, fd = a
        ok = baud in (0, 512, 1200, 2400) and inv in (0, 1, 2) and 1 <= pull <= 4 and 0 <= se <= 3 and fa in (0, 1, 2) and fd in (0, 1, 2)
    if not ok:
        raise Refused(-1, f"{kind} {a}")


class Group:
    def __init__(self, first):
        self.first, self.st, self.pending, self.nfm = first, dict(SKETCH), set(), False
        self.attack, self.decay, self.squelch, self.open_ms, self.close_ms, self.hang = M.ATTACK, M.DECAY, False, F32(0), F32(0), 0
        self.det = dict(DEFAULTS)

    def meter_set(self):
        return M.Squelch(self.open_ms if self.squelch else None, self.close_ms, self.hang, self.attack, self.decay)

    def copy(self, first):
        g = copy.copy(self)
        g.first, g.st, g.pending, g.det = first, dict(self.st), set(self.pending), dict(self.det)
        return g

    def tail_key(self):
        return tuple(self.st[k] for k in TAIL_KEYS)


class NfmSessionModel:
    """features: the enabled parts, a dict of meter, fm, tone, search, dcs, noise, dtmf, afsk, pocsag (truth values) and voice (R
    or 0); the engine has had sketch_setup()"""

    def __init__(self, n_channels, max_blocks, tab, features):
        self.n, self.max_blocks, self.tab = n_channels, max_blocks, np.asarray(tab, F32)
        self.f = dict(features)
        assert self.f.get("meter") and self.f.get("fm"), "the sessions' engines all have the meter and FM"
        self.sets, self.curve = TM.tables()
        self.groups = [Group(0)]
        self.tones, self.codes, self.bank = np.zeros(self.n, F32), np.zeros(self.n, np.uint16), np.array(TS.STANDARD, F32)
        n = self.n
        self.det = dict(tone=TN.Tone(n, tab), search=TS.Search(n, tab), dcs=DC.Dcs(n), noise=NZ.Noise(n, NZ.OFF), dtmf=DT.Dtmf(n, tab),
                        afsk=AF.Afsk(n, tab), pocsag=PO.Pocsag(n))
        self.det = {k: v for k, v in self.det.items() if self.f.get(k)}
        self.voice = V.Voice(n, self.f["voice"]) if self.f.get("voice") else None
        self.blocks = 0
        self._zero_state()

    # ---- state ----
    def _zero_state(self):
        n = self.n
        self.o = [oracle_lib.OracleEngine(taps=True) for _ in range(n)]
        self.omode, self.front_fresh = np.zeros(n, np.int64), np.ones(n, bool)
        t, f = TM.Tail(n, self.sets, self.curve), FM.Fm(n)
        self.tail = dict(bq=t.bq, env=t.env, gain=t.gain, hang=t.hang, line=t.line, w=t.w)
        self.fm = dict(hist=f.hist, z1=f.z1, y1=f.y1)
        for d in self.det.values():
            d.reset()
        self.meter = M.Meter(n)
        if self.voice is not None:
            self.voice.reset()
        self.events_valid = False
        self.last = None                                    # the last call's records

    def parts(self):
        return [k for k in FLAGS if self.f.get(k)]

    def flags(self):
        return sum(FLAGS[k] for k in self.parts())

    def part_words(self, name):
        """a part of the blob as uint32 [n, words]"""
        if name == "meter":
            return np.stack([self.meter.level.view(U32), self.meter.open.astype(U32), self.meter.hang.astype(U32)], 1)
        if name == "voice":
            return self.voice.hist.astype(np.int32).view(U32)
        if name == "fm":
            f = FM.Fm(self.n)
            f.hist, f.z1, f.y1 = self.fm["hist"], self.fm["z1"], self.fm["y1"]
            return f.words()
        return self.det[name].words()

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
        if not -1 <= group < len(self.groups):
            raise Refused(-1, "no such group")
        return self.groups if group < 0 else [self.groups[group]]

    def nfm_mask(self):
        m = np.zeros(self.n, bool)
        for k, g in enumerate(self.groups):
            m[list(self.channels(k))] = g.nfm
        return m

    def set_groups(self, firsts):
        firsts = [int(f) for f in firsts]
        if not firsts or firsts[0] != 0 or any(b <= a for a, b in zip(firsts, firsts[1:])) or firsts[-1] >= self.n:
            raise Refused(-1, "first channels")
        new = [self.groups[self.group_of(f)].copy(f) for f in firsts]
        for c in range(self.n):
            if self.groups[self.group_of(c)].pending != new[self.group_of(c, new)].pending:
                raise Refused(-5, "other resets pending")
        self.groups = new

    # ---- setters ----
    def call(self, group, name, *args):
        """one of the sketch's setters"""
        for g in self._selected(group):
            if name == "setDemodMode":
                mode = int(args[0]) & 0xffff
                if mode == NFM:
                    g.st["mode"], g.nfm = NFM, True
                    g.pending.add("fm")
                    continue
                g.nfm = False
                if mode not in SIDE_MODES:
                    g.st["mode"] = mode
                    continue
            g.pending |= apply_setting(g.st, name, *args)
            if name == "setDemodMode":
                for c in self.channels(self.groups.index(g)):
                    self.o[c].call(name, *args)
                    self.omode[c] = g.st["mode"]

    def set(self, group, kind, *args):
        """set_fm, set_tone_squelch, set_tone_search, set_dcs_squelch, set_noise_squelch, set_dtmf, set_afsk, set_pocsag by kind"""
        sel = self._selected(group)
        check_setting(kind, args)
        for g in sel:
            g.det[kind] = tuple(args)

    def set_meter(self, group, attack, decay):
        if not (_finite(attack, decay) and 0 < attack <= 1 and 0 < decay <= 1):
            raise Refused(-1, "meter")
        for g in self._selected(group):
            g.attack, g.decay = F32(attack), F32(decay)

    def set_squelch(self, group, open_ms, close_ms, hang):
        if not (_finite(open_ms, close_ms) and 0 <= close_ms <= open_ms and 0 <= hang <= 65535):
            raise Refused(-1, "squelch")
        for g in self._selected(group):
            g.squelch, g.open_ms, g.close_ms, g.hang = True, F32(open_ms), F32(close_ms), int(hang)

    def disable_squelch(self, group):
        for g in self._selected(group):
            g.squelch = False

    def set_tones(self, first, hz):
        hz = np.atleast_1d(np.asarray(hz, F32))
        if first < 0 or len(hz) < 1 or first + len(hz) > self.n or not all(_finite(v) and (v == 0 or 60 <= v <= 300) for v in hz):
            raise Refused(-1, "tones")
        self.tones[first:first + len(hz)] = hz

    def set_dcs_codes(self, first, codes):
        codes = [int(v) for v in codes]
        if first < 0 or len(codes) < 1 or first + len(codes) > self.n or not all(v == 0 or v == DC.ANY or 1 <= (v & 0x7FFF) <= 511 for v in codes):
            raise Refused(-1, "codes")
        self.codes[first:first + len(codes)] = codes

    def set_tone_bank(self, hz):
        hz = np.atleast_1d(np.asarray(hz, F32))
        if not (1 <= len(hz) <= 64 and all(_finite(v) and 60 <= v <= 300 for v in hz) and np.all(np.diff(hz) > 0)):
            raise Refused(-1, "bank")
        self.bank = hz.copy()

    # ---- a call ----
    def _push_settings(self):
        """the detectors' per-channel settings are their groups'; the per-channel tables and the bank are the engine's"""
        d = self.det
        if "tone" in d:
            d["tone"].set_tones(self.tones)
        if "dcs" in d:
            d["dcs"].set_codes(self.codes)
        if "search" in d:
            d["search"].set_bank(self.bank)
        for k, g in enumerate(self.groups):
            ch = slice(g.first, g.first + len(self.channels(k)))
            s = g.det
            if "tone" in d:
                d["tone"].set_squelch(*s["tone"], channels=ch)
            if "search" in d:
                d["search"].set_search(*s["search"], channels=ch)
            if "dcs" in d:
                d["dcs"].set_squelch(*s["dcs"], channels=ch)
            if "noise" in d:
                mode, op, cl, hang, fall, rise = s["noise"]
                d["noise"].set(mode, s["fm"][0], s["fm"][2], channels=ch, open_n=op, close_n=cl, hang_blocks=hang, fall=fall, rise=rise)
            if "dtmf" in d:
                d["dtmf"].set(*s["dtmf"], channels=ch)
            if "afsk" in d:
                d["afsk"].set(*s["afsk"], channels=ch)
            if "pocsag" in d:
                d["pocsag"].set(*s["pocsag"], channels=ch)

    def _front(self, iq, nb):
        """the "demod" tap and the FM level rows of a call"""
        demod, level = np.zeros((self.n, nb * 128), F32), np.zeros((self.n, nb * 128), F32)
        by = {}
        for k, g in enumerate(self.groups):
            ch = list(self.channels(k))
            if g.nfm:
                by.setdefault(g.det["fm"], []).extend(ch)
                continue
            if g.st["mode"] not in SIDE_MODES:
                raise Unmodelled(f"group {k} in mode {g.st['mode']}")
            for c in ch:
                if self.omode[c] != g.st["mode"]:
                    if not self.front_fresh[c]:
                        raise Unmodelled(f"receiver {c} joined a group in mode {g.st['mode']} with its IF filter running in mode {self.omode[c]}")
                    self.o[c].call("setDemodMode", g.st["mode"])
                    self.omode[c] = g.st["mode"]
                o = self.o[c]
                for b in range(nb):
                    v = slice(b * 128, (b + 1) * 128)
                    o.update(iq[c, v, 0], iq[c, v, 1])
                    demod[c, v] = o.tapbuf[5, 0]
                for t in o.taps.values():
                    t.clear()
                self.front_fresh[c] = False
        reset = np.zeros(self.n, bool)
        for k, g in enumerate(self.groups):
            reset[list(self.channels(k))] = "fm" in g.pending
        for (W, dev, tau), ch in by.items():
            f = FM.Fm(len(ch), W, dev, tau)
            f.hist, f.z1, f.y1 = (np.where(reset[ch].reshape((-1,) + (1,) * (self.fm[k].ndim - 1)), 0, self.fm[k][ch]).astype(self.fm[k].dtype)
                                  for k in ("hist", "z1", "y1"))
            demod[ch], level[ch] = f.run(iq[ch])
            self.fm["hist"][ch], self.fm["z1"][ch], self.fm["y1"][ch] = f.hist, f.z1, f.y1
        return demod, level, reset

    def _tail(self, demod):
        audio = np.zeros(demod.shape, np.int16)
        by = {}
        for k, g in enumerate(self.groups):
            by.setdefault((g.tail_key(), "audio" in g.pending, "als" in g.pending), []).extend(self.channels(k))
        for (key, clear_audio, clear_als), ch in by.items():
            st = dict(zip(TAIL_KEYS, key))
            t = TM.Tail(len(ch), self.sets, self.curve)
            t.setAudioFilter(st["audio_id"])
            if not st["audio_on"]:
                t.setAudioFilter(10)
            t.setAGCmode(st["agc_mode"])
            if not st["agc_on"]:
                t.setAGCmode(0)
            t.als_on = st["als_on"]
            t.setALSfilterNotch() if st["als_notch"] else t.setALSfilterPeak()
            t.setOutputGain(st["output_gain"])
            t.setMute(st["mute"])
            for name in self.tail:
                setattr(t, name, self.tail[name][ch].copy())
            if clear_audio:
                t.bq[:] = 0
            if clear_als:
                t.line[:] = 0
                t.w[:] = 0
            audio[ch] = t.run(demod[ch])
            for name in self.tail:
                self.tail[name][ch] = getattr(t, name)
        return audio

    def _detect(self, name, demod, nfm, reset, nb):
        """a detector's records of a call: its model on the receivers of the NFM groups, the words of the others left alone"""
        d = self.det[name]
        before = d.w.copy()
        rows = np.where(nfm[:, None], demod, F32(0))
        rec = d.run(rows, reset=reset, nfm=nfm) if name == "noise" else d.run(rows, reset=reset)
        out = []
        for r, idle in zip(rec, IDLE[name]):
            r = np.array(r)
            r[~nfm] = idle
            out.append(r)
        d.w[~nfm] = before[~nfm]
        if name in ("search", "dtmf"):                     # a group without a window keeps zero words, whatever its mode
            d.w[~nfm & (d.K == 0)] = 0
        return tuple(out)

    def update(self, iq):
        """iq int16 [n, n_blocks * 128, 2] -> what the call returns and leaves to be read"""
        nb = iq.shape[1] // 128
        assert iq.shape == (self.n, nb * 128, 2) and 0 <= nb <= self.max_blocks
        self.events_valid = False
        if nb == 0:
            return None
        self._push_settings()
        demod, fm_level, reset = self._front(iq, nb)
        audio = self._tail(demod)
        nfm = self.nfm_mask()
        out = dict(demod=demod, fm_level=fm_level, nfm=nfm.copy(), nb=nb)
        sets = [None] * self.n
        for k, g in enumerate(self.groups):
            for c in self.channels(k):
                sets[c] = g.meter_set()
        out["level"], out["peak"], carrier = self.meter.run(np.where(nfm[:, None], fm_level, demod), sets)
        out["carrier"] = carrier.copy()
        gate = carrier
        for name in DETECTORS:
            if name not in self.det:
                continue
            rec = out[name] = self._detect(name, demod, nfm, reset, nb)
            d = self.det[name]
            if name == "noise":
                gate = d.gate(gate, rec[1], nfm)
            elif name == "tone":
                gate = np.where(nfm[:, None], d.gate(gate, rec[1]), gate).astype(np.uint8)
            elif name == "dcs":
                gate = np.where(nfm[:, None], d.gate(gate, rec[0]), gate).astype(np.uint8)
        out["gate"] = gate
        out["audio"] = audio = M.gated(audio, gate)
        out["active"], out["meter"] = np.flatnonzero(gate.any(1)), self.meter.scalars()
        if self.voice is not None:
            out["voice"] = self.voice.run(audio)
        if "search" in self.det:
            out["spectrum"] = self.det["search"].spectrum()
        out["rings"] = self.rings()
        for g in self.groups:
            g.pending = set()
        self.blocks += nb
        self.events_valid = True
        self.last = out
        out["events"] = self.events()
        return out

    def rings(self):
        """(count, ring) by kind, None for a decoder the engine lacks"""
        d = self.det
        return (d["dtmf"].digits() if "dtmf" in d else None, d["afsk"].ring() if "afsk" in d else None, d["pocsag"].ring() if "pocsag" in d else None)

    def events(self):
        """(events, lost) of rdsp_engine_gather_events behind the last call: engine_events_model on the model's own records"""
        if not self.events_valid:
            return [], 0
        new = [self.last[k][1] if k in self.det else None for k in ("dtmf", "afsk", "pocsag")]
        rings = self.rings()
        return EV.sequence(new, [r[0] if r else None for r in rings], [r[1] if r else None for r in rings])

    def pack(self, n_blocks, capacity=None):
        return PK.pack(self.last["audio"][:, :n_blocks * 128], self.last["gate"][:, :n_blocks], capacity)

    def pack_voice(self, n_blocks, capacity=None):
        R = self.voice.R
        return V.pack(self.last["voice"][:, :n_blocks * 128 // R], self.last["gate"][:, :n_blocks], R, capacity)

    # ---- reset, state as data ----
    def reset(self):
        for g in self.groups:
            g.pending = set()
        self._zero_state()

    def save(self, first, n):
        if first < 0 or n < 1 or first + n > self.n:
            raise Refused(-1, "no such channels")
        ch = list(range(first, first + n))
        for c in ch:
            g = self.groups[self.group_of(c)]
            if "pre" in g.pending:
                raise Unmodelled("a blob of receivers whose IF filter has a reset pending")
        tok = dict(n=n, parts=self.parts(), o=[oracle_lib.OracleEngine(like=self.o[c]) for c in ch], omode=self.omode[ch].copy(),
                   front_fresh=self.front_fresh[ch].copy(), tail={k: v[ch].copy() for k, v in self.tail.items()},
                   fm={k: v[ch].copy() for k, v in self.fm.items()}, det={k: d.w[ch].copy() for k, d in self.det.items()},
                   meter=(self.meter.level[ch].copy(), self.meter.open[ch].copy(), self.meter.hang[ch].copy()),
                   voice=self.voice.hist[ch].copy() if self.voice is not None else None)
        return tok

    def load(self, first, tok):
        n = tok["n"]
        if first < 0 or first + n > self.n:
            raise Refused(-1, "no such channels")
        for p in tok["parts"]:
            if not self.f.get(p):
                raise Refused(-4, f"the blob carries the {p} part")
        ch = list(range(first, first + n))
        for k, c in enumerate(ch):
            self.o[c] = oracle_lib.OracleEngine(taps=True, like=tok["o"][k])
        self.omode[ch], self.front_fresh[ch] = tok["omode"], tok["front_fresh"]
        for k, v in self.tail.items():
            v[ch] = tok["tail"][k]
        for k, v in self.fm.items():
            v[ch] = tok["fm"][k] if "fm" in tok["parts"] else 0
        for k, d in self.det.items():
            d.w[ch] = tok["det"][k] if k in tok["parts"] else 0
        self.meter.level[ch], self.meter.open[ch], self.meter.hang[ch] = tok["meter"] if "meter" in tok["parts"] else (0, 0, 0)
        self.meter.ms[ch] = self.meter.pk[ch] = 0           # the last call's are no state
        if self.voice is not None:
            self.voice.hist[ch] = tok["voice"] if "voice" in tok["parts"] else 0
        self.events_valid = False
