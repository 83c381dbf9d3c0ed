"""The AFSK 1200 packet decoder of rdsp_engine_t on the GPU (include/rdsp.h "AFSK 1200 packet decoder"; csrc/rdsp_engine_afsk.hip,
csrc/rdsp_engine_afsk_host.hip) against tests/engine_afsk_model.py.  Every comparison with the model is exact: floats as uint32,
audio as int16.  The four records, n_frames with the ring and all 448 state words (through a blob) for 1, 5, 97 and 300 receivers
on the demodulated rows of tests/engine_fm_model.py, four settings and four call splits; a station's five frames read back once
each with the model's stamps and the sent bytes; a frame whose closing flag ends with a call's first sampled bit while a
transition falls on a trip's first sample; a shared flag, an abort and an oversize frame; a full ring; the decoder beside the
other detectors, none of which it changes; an engine that enabled the decoder but has it on nowhere against one that never did;
the state through blobs, regroupings, mode changes, resets and `on` toggled; the refusals.  The long streams feed the model with
the rows the engine's own detector wrote (rdsp_engine_read_demod; tests/test_engine_fm.py holds those to the FM model), without
a de-emphasis.  tests/test_engine_afsk.py has what needs no GPU."""
import functools

import numpy as np
import pytest

import engine_afsk_model as A
import engine_fm_model as FM
import engine_tone_model as T
from engine_sources_model import table

F32 = np.float32
NFM = 7
CH_WORDS = 96 + 2 * 512 + 3 * 384 + 320      # a channel's words in a blob, in front of the optional parts
G750 = A.space_gain(750.0)
SETTINGS = (dict(space_gain=1.0, pull=2), dict(space_gain=G750, pull=2), dict(space_gain=1.0, pull=1), dict(space_gain=G750, pull=1, min_bytes=9))
PATTERNS = ([57], [7, 8, 9, 33], [9, 48], [1] * 57)
DISTINCT = 8
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _engine(n, max_blocks, meter=False, afsk=True, nfm=True, others=False, tau_us=750.0):
    """sketch set-up, NFM at its defaults (W = 2, 5000 Hz) with the given de-emphasis, the tail's AGC and ALS off"""
    from radiodsp_sdr_rx_amd.engine import Engine
    import oracle_lib
    e = Engine(n, max_blocks_per_call=max_blocks, tables=oracle_lib.engine_tables())
    e.sketch_setup()
    e.setAGCmode(0)
    if meter:
        e.enable_meter()
    e.enable_fm()
    if others:
        e.enable_tone()
        e.enable_dcs()
        e.enable_noise()
        e.enable_dtmf()
    if afsk:
        e.enable_afsk()
    if nfm:
        assert e.setDemodMode(NFM) == 0.0
        e.set_fm(2, 5000.0, tau_us)
    return e


def _station(seed, mod, carrier=8000.0, noise=3.0):
    """int16 [t, 2]: a carrier frequency-modulated (5000 Hz peak deviation) by mod (+-1.0: the deviation), `noise` counts of noise"""
    r = np.random.default_rng(seed)
    n = len(mod)
    z = carrier * np.exp(1j * (2 * np.pi * 5000.0 / 44100.0 * np.cumsum(np.clip(mod, -1.0, 1.0)) + r.uniform(0, 6))) + \
        noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16)


def _payload(r, k):
    return bytes(r.integers(0, 256, k, dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def _distinct(nb=57):
    """eight distinct receivers, nb blocks: (iq int16 [8, t, 2], y float32 [8, t] by the FM model, the payloads of rows 0 ... 4).
    Rows 0 ... 3: a keyed station sends one frame of 15 bytes (17 with the FCS: a minimum frame) behind 3 flags and a
    drawn lead, flat, at 0.3 to 0.5 of the deviation; row 4 the same from a sender that pre-emphasises (the space tone 2.2 times
    the mark's amplitude); row 5 all zeros; row 6 on the rails; row 7 an idle discriminator (noise and no carrier)"""
    r = np.random.default_rng(808)
    t = nb * 128
    x, sent = [], []
    for c in range(5):
        p = _payload(r, 15)
        levels = A.nrzi(A.frame_bits(p, 3, 2))
        mod = A.audio(levels, r.uniform(0.3, 0.5), ppm=r.uniform(-300, 300), phase=r.uniform(0, 6), lead=int(r.integers(0, 300)), total=t)
        if c == 4:
            mod = A.audio(levels, 0.2, lead=40, total=t, space_boost=2.2)
        x.append(_station(900 + c, mod, r.uniform(2000, 20000)))
        sent.append(p)
    x.append(np.zeros((t, 2), np.int16))
    x.append(r.choice(np.array([32767, -32768], np.int16), (t, 2)))
    x.append(np.rint(300.0 * r.standard_normal((t, 2))).astype(np.int16))
    x = np.stack(x)
    return x, FM.Fm(DISTINCT).run(x)[0], sent


@functools.lru_cache(maxsize=None)
def _model_runs(rdsp_key, s, p):
    """the model on the eight distinct rows under setting s and call pattern p, computed once for every receiver count: per
    call (records, n_frames, ring, words)"""
    x, y, sent = _distinct()
    m = A.Afsk(DISTINCT, _TAB[0], 1, **SETTINGS[s])
    out, a = [], 0
    for k in PATTERNS[p]:
        rec = m.run(y[:, a * 128:(a + k) * 128])
        out.append((rec,) + m.ring() + (m.words(),))
        a += k
    return out


_TAB = []


def _afsk_words(blob, n):
    """the AFSK words of a blob of n channels: its last part"""
    return blob[-n * A.WORDS * 4:].view(np.uint32).reshape(n, A.WORDS)


def _update(e, x):
    return e.update(_cuda(x)).cpu().numpy()


def _records(e, k):
    return tuple(v.cpu().numpy() for v in e.read_afsk(k))


def _ring(e):
    return tuple(v.cpu().numpy().view(np.uint32) for v in e.read_afsk_ring())


def _same(got, want, where):
    """the four records of a call against the model's"""
    for k in (0, 1, 2):
        assert np.array_equal(got[k], want[k]), (where, k, np.argwhere(got[k] != want[k])[:3])
    assert np.array_equal(bits(got[3]), bits(want[3])), (where, 3, np.argwhere(bits(got[3]) != bits(want[3]))[:3])


def _same_ring(e, m, where):
    (gc, gr), (wc, wr) = _ring(e), m.ring()
    assert np.array_equal(gc, wc) and np.array_equal(gr, wr), where


@pytest.mark.parametrize("n", [1, 5, 97, 300])
def test_gpu_afsk_rows_are_the_model(rdsp, n):
    """1, 5, 97 and 300 receivers (a ragged last workgroup, more than one workgroup) that cycle the eight rows of _distinct (keyed
    stations through the FM model, a pre-emphasised one, silence, the rails, an idle discriminator), pull 1 and 2 with space_gain 1
    and the de-emphasis value, 57 blocks as [57], [7, 8, 9, 33], [9, 48] and 57 calls of one -- a whole trip, ragged trips, a trip
    boundary inside a frame -- each from a reset: after every call rdsp_engine_read_afsk's four records,
    rdsp_engine_read_afsk_frames' counts and rings and all 448 state words (through a blob) equal the model's.  These clean
    stations' frames are read under every one of the settings"""
    nb = 57
    x, y, sent = _distinct()
    if not _TAB:
        _TAB.append(table(rdsp))
    idx = np.arange(n) % DISTINCT
    xs = np.ascontiguousarray(x[idx])
    e = _engine(n, nb)
    for s, setting in enumerate(SETTINGS):
        e.set_afsk(1, **setting)
        for p, pattern in enumerate(PATTERNS):
            e.reset()
            a = 0
            for k, (rec, count, ring, words) in zip(pattern, _model_runs(0, s, p)):
                e.update(_cuda(xs[:, a * 128:(a + k) * 128]))
                _same(_records(e, k), tuple(v[idx] for v in rec), (setting, pattern, a))
                gc, gr = _ring(e)
                assert np.array_equal(gc, count[idx]) and np.array_equal(gr, ring[idx]), (setting, pattern, a)
                assert np.array_equal(_afsk_words(e.save_state(0, n), n), words[idx]), (setting, pattern, a)
                a += k
            assert (words[:, A.TBLOCKS] == nb).all() and words[5, A.ONES] == 7 and not words[5, A.NFRAMES] and rec[3][6].all()
            got = [[f for _, f in _frames_of(count, ring, c)] for c in range(5)]
            assert got == [[f] for f in sent], setting
    e.close()


def _frames_of(count, ring, c):
    n = int(count[c])
    return [(int(ring[c, k % 4, 1]), ring[c, k % 4, 2:].astype("<u4").tobytes()[:int(ring[c, k % 4, 0])]) for k in range(max(0, n - 4), n)]


_LONG = {}


def _long_case(rdsp):
    """three receivers, no de-emphasis, the defaults, 1056 blocks in calls of 32, computed once; the model runs on the rows
    rdsp_engine_read_demod returns.  Receiver 0: a station sends five frames of 17 to 120 bytes under voice-band noise of rms
    0.03.  Receiver 1: a frame aborted by seven ones, two frames that share one flag, a frame of 331 bytes with its FCS (one
    too many) and a short one behind it.  Receiver 2: six frames of 17 to 22 bytes.
    -> the engine's and the model's records of every call, the model, the engine's final ring and words, what was sent"""
    if _LONG:
        return _LONG
    nb, call = 1056, 32
    x, five, shared, after, six = _long_signals(nb)
    e = _engine(3, call, tau_us=0.0)
    e.set_afsk(1)
    m = A.Afsk(3, table(rdsp), 1)
    got, want, trace, raws = [], [], [], []
    for a in range(0, nb, call):
        e.update(_cuda(x[:, a * 128:(a + call) * 128]))
        got.append(_records(e, call))
        want.append(m.run(e.read_demod(call).cpu().numpy(), trace=trace, raws=raws))
    _LONG.update(five=five, shared=shared, after=after, six=six, model=m, x=x, trace=trace, raw=np.concatenate(raws, 1),
                 got=[np.concatenate([g[k] for g in got], 1) for k in range(4)], want=[np.concatenate([w[k] for w in want], 1) for k in range(4)],
                 ring=_ring(e), words=_afsk_words(e.save_state(0, 3), 3), frames=e.read_afsk_frames())
    e.close()
    return _LONG


def _long_signals(nb):
    """_long_case's three stations -> (iq int16 [3, nb 128, 2], the five frames, the two that share a flag, the one behind the
    oversize frame, the six)"""
    t = nb * 128
    r = np.random.default_rng(606)
    five = [_payload(r, k) for k in (17, 30, 50, 80, 120)]
    bits5 = []
    for p in five:
        bits5 += A.frame_bits(p, 6, 2)
    station = A.audio(A.nrzi(bits5), 0.3, ppm=200.0, tone_off=0.004, lead=333, total=t) + T.voice_noise(77, t, 0.03)
    ab, s1, s2, big, after = _payload(r, 24), _payload(r, 18), _payload(r, 31), _payload(r, 329), _payload(r, 19)
    odd = (A.FLAG * 6 + A.stuffed(ab)[:100] + [1] * 7 + A.FLAG * 3 + A.stuffed(A.with_fcs(s1)) + A.FLAG + A.stuffed(A.with_fcs(s2)) + A.FLAG * 3 +
           A.stuffed(A.with_fcs(big)) + A.FLAG * 3 + A.stuffed(A.with_fcs(after)) + A.FLAG * 2)
    assert len(odd) * 36.75 + 200 < t
    six = [_payload(r, 17 + k) for k in range(6)]
    bits6 = []
    for p in six:
        bits6 += A.frame_bits(p, 4, 1)
    x = np.stack([_station(60, station), _station(61, A.audio(A.nrzi(odd), 0.3, lead=200, total=t)), _station(62, A.audio(A.nrzi(bits6), 0.25, lead=64, total=t))])
    return x, five, [s1, s2], after, six


def test_gpu_afsk_reads_a_stations_frames(rdsp):
    """a station sends five frames of 17 to 120 bytes under noise, the baud rate 200 ppm and the tones 0.4 % off: the engine's
    records, counts, rings and words equal the model's, and on them every frame is read back exactly once, in order, with the
    model's block stamps -- new_rec counts one in the stamp's block -- and the sent bytes; none has a bad FCS; the ring holds the
    last four, Engine.read_afsk_frames returns them oldest first"""
    c = _long_case(rdsp)
    _same(c["got"], c["want"], "long")
    m = c["model"]
    assert np.array_equal(c["ring"][0], m.ring()[0]) and np.array_equal(c["ring"][1], m.ring()[1]) and np.array_equal(c["words"], m.words())
    new, bad = c["got"][1], c["got"][2]
    assert c["ring"][0][0] == 5 and new[0].sum() == 5 and new[0].max() == 1 and not bad[0].any()
    stamps = [int(b) + 1 for b in np.flatnonzero(new[0])]
    frames = [f for f in c["frames"] if f[0] == 0]
    print("read back:", [(t, len(f)) for _, t, f in frames])
    assert [(t, f) for _, t, f in frames] == list(zip(stamps[1:], c["five"][1:])) == m.frames(0)
    assert [m0 // 32 + 1 for m0, good in c["trace"]] == stamps and all(good for _, good in c["trace"])
    sync = c["got"][0][0]
    assert sync[stamps[0] - 30:stamps[0] - 1].all() and not sync[:2].any()          # inside the frame the decoder is in sync


def test_gpu_afsk_shared_flag_abort_and_oversize(rdsp):
    """a frame aborted by seven ones is no frame and no bad FCS; two frames that share one flag are both read; a frame of 331
    bytes is dropped without a trace and the frame behind it is read"""
    c = _long_case(rdsp)
    count, ring = c["ring"]
    assert count[1] == 3 and c["words"][1, A.NBAD] == 0 and not c["got"][2][1].any()
    assert [f for _, f in _frames_of(count, ring, 1)] == c["shared"] + [c["after"]]
    stamps = [t for t, _ in _frames_of(count, ring, 1)]
    assert stamps[2] - stamps[1] > 331 * 8 * 36.75 / 128                               # the long frame lies between them


def test_gpu_afsk_full_ring(rdsp):
    """six frames through the ring of four: n_frames is 6, frame k lies in slot k mod 4, so the ring holds frames 4, 5, 2, 3, each
    slot whole (the bytes behind a shorter frame are zeros), with ascending stamps in the order 2, 3, 4, 5"""
    c = _long_case(rdsp)
    count, ring = c["ring"]
    assert count[2] == 6
    for slot, k in enumerate((4, 5, 2, 3)):
        p = c["six"][k]
        assert ring[2, slot, 0] == len(p) and ring[2, slot, 2:].astype("<u4").tobytes() == p + bytes(328 - len(p)), slot
    stamps = [int(ring[2, k % 4, 1]) for k in (2, 3, 4, 5)]
    assert stamps == sorted(stamps) and [f for _, f in _frames_of(count, ring, 2)] == c["six"][2:]
    assert [(ch, f) for ch, _, f in c["frames"] if ch == 2] == [(2, p) for p in c["six"][2:]]


def test_gpu_afsk_frame_across_calls_and_trips(rdsp):
    """the station's first frame again, cut so that the flag that closes it ends with the FIRST bit a call samples (the frame's
    bytes, the shift register and the clock all come from the words) and so that a transition falls on the first sample of a
    call's second trip (prev_raw and the clock cross the trip): records, ring and words equal the model's at every call, the
    frame is read in that call's first block"""
    c = _long_case(rdsp)
    raw, trace = c["raw"][0], c["trace"]
    m_end = trace[0][0]
    E = m_end // 32
    first = raw[32 * np.arange(1, E)] != raw[32 * np.arange(1, E) - 1]
    J = [int(j) for j in np.flatnonzero(first) + 1 if 8 <= j and j + 24 <= E]
    assert J, "no transition on a block's first sample"
    j = J[len(J) // 2]
    # the bit before the closing one was sampled in an earlier block: the closing bit is the first the call samples
    assert m_end % 32 < 9, m_end % 32
    pattern, a = [], 0
    for stop in (j - 8, E, E + 5):
        while a < stop:
            k = min(32, stop - a)
            pattern.append(k)
            a += k
    assert j - 8 in np.cumsum([0] + pattern) and E in np.cumsum([0] + pattern)
    e = _engine(1, 32, tau_us=0.0)
    e.set_afsk(1)
    m = A.Afsk(1, table(rdsp), 1)
    a = 0
    for k in pattern:
        e.update(_cuda(c["x"][:1, a * 128:(a + k) * 128]))
        want = m.run(e.read_demod(k).cpu().numpy())
        got = _records(e, k)
        _same(got, want, a)
        _same_ring(e, m, a)
        assert np.array_equal(_afsk_words(e.save_state(0, 1), 1), m.words()), a
        if a == E:
            assert got[1][0, 0] == 1 and m.frames(0)[0][1] == c["five"][0] and m.frames(0)[0][0] == E + 1
        else:
            assert not got[1].any()
        a += k
    e.close()


def test_gpu_afsk_beside_the_other_detectors(rdsp):
    """meter with its squelch, tone squelch, code squelch, noise squelch, DTMF decoder, voice stage (R = 2) and the decoder
    together against the same engine without the decoder, 97 receivers, 57 blocks as [9, 48]: the int16 audio, the other
    detectors' records, the active list, the voice rows and every blob part with a flag below 512 are the same bytes, and the
    decoder's records, ring and words equal the model's"""
    n, nb = 97, 57
    x, y, sent = _distinct()
    if not _TAB:
        _TAB.append(table(rdsp))
    idx = np.arange(n) % DISTINCT
    xs = np.ascontiguousarray(x[idx])
    engines = []
    for with_afsk in (True, False):
        e = _engine(n, 48, meter=True, afsk=with_afsk, others=True)
        e.set_squelch(2e-3, 1e-3, 1)
        e.set_tones(0, np.where(np.arange(n) % 3 == 0, F32(100.0), F32(0.0)).astype(F32))
        e.set_tone_squelch(4, 0.06, 0.045)
        e.set_dcs_codes(0, [0o023 if c % 5 == 0 else 0 for c in range(n)])
        e.set_noise_squelch()
        e.set_dtmf(4)
        e.enable_voice(2)
        engines.append(e)
    a, b = engines
    a.set_afsk(1, **SETTINGS[1])
    same = lambda va, vb: np.array_equal(va.cpu().numpy().view(np.uint8), vb.cpu().numpy().view(np.uint8))
    at = 0
    for k, (rec, count, ring, words) in zip(PATTERNS[2], _model_runs(0, 1, 2)):
        d = _cuda(xs[:, at * 128:(at + k) * 128])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        assert np.array_equal(ya, yb)
        for read in ("read_meter", "read_tone", "read_dcs", "read_noise", "read_dtmf"):
            for va, vb in zip(getattr(a, read)(k), getattr(b, read)(k)):
                assert same(va, vb), read
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        assert same(a.read_voice(k), b.read_voice(k))
        _same(_records(a, k), tuple(v[idx] for v in rec), at)
        gc, gr = _ring(a)
        assert np.array_equal(gc, count[idx]) and np.array_equal(gr, ring[idx])
        at += k
    assert count[:4].all()
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert blob_b.view(np.uint32)[3] == 2 | 4 | 8 | 16 | 64 | 128 | 256 and blob_a.view(np.uint32)[3] == 2 | 4 | 8 | 16 | 64 | 128 | 256 | 512
    assert len(blob_a) == len(blob_b) + n * A.WORDS * 4 and np.array_equal(blob_a[16:len(blob_b)], blob_b[16:])
    assert np.array_equal(_afsk_words(blob_a, n), words[idx])
    for e in engines:
        e.close()


def test_gpu_afsk_off_changes_nothing(rdsp):
    """NFM, LSB and AM groups (5 + 3 + 4 receivers), meter and squelch on: an engine that enabled the decoder with on = 0
    everywhere gives the audio, the meter records and the active list of one that never enabled it, and reads zero records and no
    frames; the blob of the engine that never enabled it has the size and the flags it always had (meter 2, FM 8) and is, byte for
    byte, the other's without its header flag 512 and its tenth part, which is zeros"""
    from test_engine_meter import _bursts
    n, nb, first = 12, 6, [0, 5, 8]
    x = _bursts(83, n, nb)
    x[:5] = FM.station(90, nb, 4000.0, 1000.0, 9000.0, 3.0)[None]
    engines = []
    for with_afsk in (True, False):
        e = _engine(n, 4, meter=True, afsk=with_afsk, nfm=False)
        e.set_squelch(2e-3, 1e-3, 1)
        e.set_groups(first)
        e.select_group(0); assert e.setDemodMode(NFM) == 0.0
        e.select_group(2); e.setDemodMode(4); e.setAudioFilter(0)
        e.select_group(-1)
        engines.append(e)
    a, b = engines
    assert a.afsk_enabled and not b.afsk_enabled
    for k0, k in ((0, 4), (4, 2)):
        d = _cuda(x[:, k0 * 128:(k0 + k) * 128])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        assert np.array_equal(ya, yb) and ya[:5].any() and ya[5:].any()
        for va, vb in zip(a.read_meter(k), b.read_meter(k)):
            assert np.array_equal(bits(va.cpu().numpy().astype(F32)), bits(vb.cpu().numpy().astype(F32)))
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        assert not any(v.any() for v in _records(a, k))
        count, ring = _ring(a)
        assert not count.any() and not ring.any() and a.read_afsk_frames() == []
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert len(blob_b) == 16 + n * (CH_WORDS + 3 + 50) * 4 == b.lib.rdsp_engine_state_bytes(b.h, n) and blob_b.view(np.uint32)[3] == 2 | 8
    assert len(blob_a) == len(blob_b) + n * A.WORDS * 4 == a.lib.rdsp_engine_state_bytes(a.h, n) and blob_a.view(np.uint32)[3] == 2 | 8 | 512
    assert np.array_equal(blob_a[16:len(blob_b)], blob_b[16:]) and not blob_a[len(blob_b):].any()
    assert np.array_equal(blob_a[:12], blob_b[:12])
    with pytest.raises(rdsp.RdspError) as ex:
        b.read_afsk(0)
    assert ex.value.code == -4
    for e in engines:
        e.close()


def test_gpu_afsk_state(rdsp):
    """the decoder's words are signal state.  A receiver in the middle of a frame (in sync, bytes in buf) moves by blob to an
    engine with another channel count, another index and another max_blocks, and continues bit for bit to the frame's end.  An
    engine without the decoder refuses the part with nothing changed; a blob without the part zeroes the words.  A regrouping
    keeps the detector; changed space_gain, pull and min_bytes do not restart it; on = 0 zeroes a group's words and on = 1
    restarts them; outside NFM the words are left alone and coming back restarts them; rdsp_engine_reset zeroes them and keeps
    the settings"""
    nb, cut = 57, 30
    x, y, sent = _distinct()
    x, y = x[:5], y[:5]
    tab = table(rdsp)
    S1 = SETTINGS[1]
    a = _engine(5, 16)
    a.enable_afsk()                                                                           # again: a no-op
    a.set_afsk(1, **S1)
    m = A.Afsk(5, tab, 1, **S1)
    for k0 in (0, 16):
        k = min(16, cut - k0)
        a.update(_cuda(x[:, k0 * 128:(k0 + k) * 128]))
        _same(_records(a, k), m.run(y[:, k0 * 128:(k0 + k) * 128]), k0)
    blob = a.save_state(0, 1)
    w0 = m.words()[0]
    assert w0[A.INFRAME] == 1 and w0[A.NBYTES] > 3 and w0[A.TBLOCKS] == cut and w0[A.HIST_:A.HIST_ + 11].all() and w0[A.BUF:A.BUF + 1].any() and w0[A.PLL]
    assert np.array_equal(_afsk_words(blob, 1)[0], w0) and blob.view(np.uint32)[3] == 8 | 512
    plain = _engine(3, 8, afsk=False)
    assert len(blob) == a.lib.rdsp_engine_state_bytes(a.h, 1) == plain.lib.rdsp_engine_state_bytes(plain.h, 1) + A.WORDS * 4
    before = plain.save_state(0, 3)
    with pytest.raises(rdsp.RdspError) as ex:                                                 # an engine without the decoder refuses the part
        plain.load_state(0, blob)
    assert ex.value.code == -4 and np.array_equal(plain.save_state(0, 3), before)
    # the receiver continues in another engine: 7 channels, index 4, 32 blocks a call, a past of its own
    b = _engine(7, 32)
    b.set_afsk(1, **S1)
    b.update(_cuda(np.broadcast_to(x[1:2, :128], (7, 128, 2)).copy()))
    b.load_state(4, blob)
    assert np.array_equal(_afsk_words(b.save_state(4, 1), 1)[0], w0)
    rest = np.zeros((7, (nb - cut) * 128, 2), np.int16)
    rest[4] = x[0, cut * 128:]
    b.update(_cuda(rest))
    want = m.run(y[:, cut * 128:])
    got = _records(b, nb - cut)
    _same(tuple(v[4:5] for v in got), tuple(v[:1] for v in want), "moved")
    assert np.array_equal(_afsk_words(b.save_state(4, 1), 1)[0], m.words()[0]) and m.frames(0)[0][1] == sent[0]
    assert [f for f in b.read_afsk_frames() if f[0] == 4] == [(4,) + m.frames(0)[0]]
    b.load_state(4, plain.save_state(0, 1))                                                   # a blob without the part zeroes the words
    assert not _afsk_words(b.save_state(4, 1), 1).any()
    # a's own stream goes on from block `cut`.  A regrouping keeps the detector
    a.set_groups([0, 2])
    m2 = A.Afsk(5, tab, 1, **S1)
    m2.run(y[:, :cut * 128])
    at = cut

    def step(k):
        nonlocal at
        a.update(_cuda(x[:, at * 128:(at + k) * 128]))
        _same(_records(a, k), m2.run(y[:, at * 128:(at + k) * 128]), at)
        assert np.array_equal(_afsk_words(a.save_state(0, 5), 5), m2.words()), at
        _same_ring(a, m2, at)
        at += k
        return m2.words()
    w = step(3)
    assert (w[:, A.TBLOCKS] == cut + 3).all()
    # changed settings restart nothing
    S2 = dict(space_gain=2.5, pull=3, min_bytes=12)
    a.select_group(1); a.set_afsk(1, **S2); a.select_group(-1)
    m2.set(1, channels=slice(2, None), **S2)
    w = step(4)
    assert (w[:, A.TBLOCKS] == cut + 7).all()
    # group 0 (channels 0, 1) switches the decoder off: its words are zeros, its records too; group 1 goes on
    a.select_group(0); a.set_afsk(0); a.select_group(-1)
    m2.set(0, channels=slice(0, 2))
    w = step(3)
    assert not w[:2].any() and (w[2:, A.TBLOCKS] == cut + 10).all()
    # and on again: a fresh detector
    a.select_group(0); a.set_afsk(1, **S1); a.select_group(-1)
    m2.set(1, channels=slice(0, 2), **S1)
    w = step(5)
    assert (w[:2, A.TBLOCKS] == 5).all() and (w[2:, A.TBLOCKS] == cut + 15).all()
    # a regrouping into a group with other settings keeps the words: channel 2 joins group 0
    a.set_groups([0, 3])
    m2.set(1, channels=slice(2, 3), **S1)
    w = step(nb - at)
    assert w[2, A.TBLOCKS] == nb and at == nb
    # leaving NFM and coming back: the words are not maintained outside the mode and start from zeros at the next NFM update
    a.set_groups([0])
    a.set_afsk(1, **S1)
    a.setDemodMode(4)
    a.update(_cuda(x[:, :128]))
    assert np.array_equal(_afsk_words(a.save_state(0, 5), 5), w) and not any(v.any() for v in _records(a, 1))
    a.setDemodMode(NFM)
    a.update(_cuda(x[:, :9 * 128]))
    ya = FM.Fm(5).run(x[:, :9 * 128])[0]
    m3 = A.Afsk(5, tab, 1, **S1)
    _same(_records(a, 9), m3.run(ya), "back in NFM")
    assert np.array_equal(_afsk_words(a.save_state(0, 5), 5), m3.words()) and (m3.words()[:, A.TBLOCKS] == 9).all()
    # rdsp_engine_reset zeroes the words and keeps the settings
    a.reset()
    assert not _afsk_words(a.save_state(0, 5), 5).any()
    a.update(_cuda(x[:, :9 * 128]))
    m3.reset()
    _same(_records(a, 9), m3.run(ya), "after the reset")
    assert np.array_equal(_afsk_words(a.save_state(0, 5), 5), m3.words())
    for e in (a, b, plain):
        e.close()


def test_gpu_afsk_refusals(rdsp):
    """every refusal that needs an engine, each with the object unchanged: rdsp_engine_enable_afsk before rdsp_engine_enable_fm; the
    reads before rdsp_engine_enable_afsk; the records before a call; on outside 0 and 1; space_gain below 1/16, above 16 or NaN;
    pull outside 1 ... 4; min_bytes outside 9 ... 330; n_blocks above the last call's; short strides; a frame range outside the
    object"""
    import torch
    from test_engine_meter import _engine as plain_engine
    p = plain_engine(2, 4, meter=False)
    assert p.lib.rdsp_engine_enable_afsk(p.h) == -4 and b"rdsp_engine_enable_fm" in p.lib.rdsp_last_error() and not p.afsk_enabled
    p.set_afsk(1, 2.0, 3, 20)                                                                 # a setting: it may precede the decoder
    p.enable_fm()
    for f in (lambda: p.read_afsk(0), p.read_afsk_ring, p.read_afsk_frames):
        with pytest.raises(rdsp.RdspError) as ex:
            f()
        assert ex.value.code == -4
    p.enable_afsk()                                                                           # without the meter and the other detectors
    assert p.afsk_enabled and not p.dtmf_enabled
    with pytest.raises(rdsp.RdspError) as ex:                                                 # no call yet: there are no records
        p.read_afsk(1)
    assert ex.value.code == -1
    count, ring = _ring(p)                                                                    # the words exist: no frames
    assert not count.any() and not ring.any()
    p.close()
    x, y, sent = _distinct()
    x, y = x[:5], y[:5]
    e = _engine(5, 8)
    e.set_afsk(1, **SETTINGS[1])
    m = A.Afsk(5, table(rdsp), 1, **SETTINGS[1])
    e.update(_cuda(x[:, :3 * 128]))
    m.run(y[:, :3 * 128])
    nan, inf = float("nan"), float("inf")
    ok = (1, 1.0, 2, 17)
    bad_values = {0: (2, -1), 1: (0.0, 0.06, 16.01, -1.0, nan, inf), 2: (0, 5, -1), 3: (8, 331, 0, -1)}
    for k, values in bad_values.items():
        for v in values:
            bad = ok[:k] + (v,) + ok[k + 1:]
            with pytest.raises(rdsp.RdspError) as ex:
                e.set_afsk(*bad)
            assert ex.value.code == -1 and b"rdsp_engine_set_afsk" in e.lib.rdsp_last_error(), bad
    with pytest.raises(rdsp.RdspError):
        e.set_afsk(0, 0.0)                                                                    # on = 0 does not excuse the rest
    sync = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    new = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    bad = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    lvl = torch.full((5, 4), 7.0, dtype=torch.float32, device="cuda")
    for nblk, s0, s1, s2, s3 in ((4, 4, 4, 4, 4), (-1, 4, 4, 4, 4), (3, 2, 4, 4, 4), (3, 4, 2, 4, 4), (3, 4, 4, 2, 4), (3, 4, 4, 4, 2)):
        assert e.lib.rdsp_engine_read_afsk(e.h, nblk, sync.data_ptr(), s0, new.data_ptr(), s1, bad.data_ptr(), s2, lvl.data_ptr(), s3, None) == -1, (nblk, s0, s1, s2, s3)
        assert b"rdsp_engine_read_afsk" in e.lib.rdsp_last_error()
    count = torch.full((5,), 7, dtype=torch.int32, device="cuda")
    ring = torch.full((5, 4, 84), 7, dtype=torch.int32, device="cuda")
    for c0, cn in ((-1, 1), (0, 6), (5, 1), (0, 0), (3, 3)):
        assert e.lib.rdsp_engine_read_afsk_frames(e.h, c0, cn, count.data_ptr(), ring.data_ptr(), None) == -1, (c0, cn)
        assert b"rdsp_engine_read_afsk_frames" in e.lib.rdsp_last_error()
    torch.cuda.synchronize()
    assert (sync == 7).all() and (new == 7).all() and (bad == 7).all() and (lvl == 7.0).all() and (count == 7).all() and (ring == 7).all()
    assert e.lib.rdsp_engine_read_afsk(e.h, 3, None, 0, None, 0, None, 0, lvl.data_ptr(), 4, None) == 0   # any pointer may be NULL
    assert e.lib.rdsp_engine_read_afsk(e.h, 3, sync.data_ptr(), 4, new.data_ptr(), 4, bad.data_ptr(), 4, None, 0, None) == 0
    assert e.lib.rdsp_engine_read_afsk_frames(e.h, 1, 3, count.data_ptr(), None, None) == 0
    assert e.lib.rdsp_engine_read_afsk_frames(e.h, 1, 3, None, ring.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(count[:3].cpu().numpy().view(np.uint32), m.ring()[0][1:4]) and (count[3:] == 7).all()
    assert np.array_equal(ring[:3].cpu().numpy().view(np.uint32), m.ring()[1][1:4]) and (ring[3:] == 7).all() and (lvl[:, 3] == 7.0).all()
    # nothing of all that changed the object: the stream goes on as the model's
    e.update(_cuda(x[:, 3 * 128:8 * 128]))
    _same(_records(e, 5), m.run(y[:, 3 * 128:8 * 128]), "goes on")
    assert np.array_equal(_afsk_words(e.save_state(0, 5), 5), m.words())
    e.close()
