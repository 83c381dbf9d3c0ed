"""The CTCSS tone search of rdsp_engine_t on the GPU (include/rdsp.h "tone search"; csrc/rdsp_engine_tone_search.hip,
csrc/rdsp_engine_tone_search_host.hip) against tests/engine_tone_search_model.py on the demodulated rows of
tests/engine_fm_model.py.  Every comparison with the model is exact: floats as uint32, audio as int16.  The three records, the
spectrum rows and all 200 state words (through a blob) for 1, 5, 97 and 300 receivers, K = 4 and 8, four call splits and banks
of 50, 64, 3 and 1 tones; a station's tone found among seven; the search beside the meter, the tone squelch and the voice stage,
none of which it changes; an engine that enabled the search with K = 0 everywhere against one that never did; the state through
blobs, regroupings, mode changes, resets, a changed K and a changed bank; the refusals.  tests/test_engine_tone_search.py has
what needs no GPU."""
import functools

import numpy as np
import pytest

import engine_fm_model as FM
import engine_tail_model as TM
import engine_tone_model as T
import engine_tone_search_model as TS
from engine_meter_model import Meter, Squelch, gated
from engine_sources_model import table

F32 = np.float32
NFM = 7
CH_WORDS = 96 + 2 * 512 + 3 * 384 + 320      # a channel's words in a blob, in front of the optional parts
BANK64 = tuple(np.round(np.linspace(60.0, 300.0, 64), 1))
BANK7 = (67.0, 88.5, 100.0, 103.5, 151.4, 203.5, 254.1)
BANKS = (TS.STANDARD, BANK64, (88.5, 100.0, 254.1), (151.4,))
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _engine(n, max_blocks, meter=False, search=True, tone=False, nfm=True):
    """sketch set-up, NFM at its defaults (W = 2, 5000 Hz, 750 us), the tail's AGC and ALS off, audio filter 2700"""
    from radiodsp_sdr_rx_amd.engine import Engine
    import oracle_lib
    e = Engine(n, max_blocks_per_call=max_blocks, tables=oracle_lib.engine_tables())
    e.sketch_setup()
    e.setAGCmode(0)
    if meter:
        e.enable_meter()
    e.enable_fm()
    if tone:
        e.enable_tone()
    if search:
        e.enable_tone_search()
    if nfm:
        assert e.setDemodMode(NFM) == 0.0
    return e


@functools.lru_cache(maxsize=None)
def _drawn(n, nb=17):
    """n receivers, nb blocks: (iq int16 [n, t, 2], tones float32 [n], y, lvl float32 [n, t], tail int16 [n, t]).  Every third
    receiver's station carries a standard tone at 15 % of the deviation, the others a drawn audio tone at a drawn deviation;
    with three or more, channel 1 is on the rails and channel 2 all zeros"""
    r = np.random.default_rng(700 + n)
    tones = r.choice(np.array(TS.STANDARD, F32), n)
    x = np.stack([FM.station(900 + c, nb, 750.0, float(tones[c]), r.uniform(500, 20000), 3.0) if c % 3 == 0 else
                  FM.station(900 + c, nb, r.uniform(1500, 5000), r.uniform(300, 3000), r.uniform(200, 20000), r.uniform(1, 30)) for c in range(n)])
    if n >= 3:
        x[1] = r.choice(np.array([32767, -32768], np.int16), (nb * 128, 2))
        x[2] = 0
    y, lvl = FM.Fm(n).run(x)
    return x, tones, y, lvl, TM.Tail(n).setAGCmode(0).run(y)


def _search_words(blob, n):
    """the search words of a blob of n channels: its last part"""
    return blob[-n * TS.WORDS * 4:].view(np.uint32).reshape(n, TS.WORDS)


def _update(e, x):
    return e.update(_cuda(x)).cpu().numpy()


def _records(e, k):
    return tuple(v.cpu().numpy() for v in e.read_tone_search(k))


def _same(got, want, where):
    """the three records of a call against the model's"""
    assert np.array_equal(got[0], want[0]), (where, np.argwhere(got[0] != want[0])[:3])
    assert np.array_equal(bits(got[1]), bits(want[1])), (where, np.argwhere(bits(got[1]) != bits(want[1]))[:3])
    assert np.array_equal(bits(got[2]), bits(want[2])), (where, np.argwhere(bits(got[2]) != bits(want[2]))[:3])


@pytest.mark.parametrize("n", [1, 5, 97, 300])
def test_gpu_search_rows_are_the_model(rdsp, n):
    """1, 5, 97 and 300 receivers (a ragged last workgroup, more than one workgroup; channel 1 on the rails, channel 2 all zeros),
    K = 4 and 8, banks of 50, 64, 3 and 1 tones, 17 blocks as [17], [7, 8, 2], seventeen calls of 1 and [9, 8] -- windows end in
    mid-call, at a call boundary and inside the eight-block trip -- each from a reset: after every call
    rdsp_engine_read_tone_search's three records, rdsp_engine_read_tone_spectrum's rows and all 200 state words (through a blob)
    equal the model's, and the int16 audio is that of an engine that never enabled the search"""
    nb = 17
    x, tones, y, lvl, tail = _drawn(n)
    tab = table(rdsp)
    plain = _engine(n, nb, search=False)
    audio_ref = _update(plain, x)
    plain.close()
    assert np.array_equal(audio_ref[..., 0], tail)
    e = _engine(n, nb)
    found = set()
    for bank in BANKS:
        e.set_tone_bank(bank)
        assert np.array_equal(e.tone_bank(), np.array(bank, F32))
        for K, lo, ratio in ((4, 0.06, 2.0), (8, 0.02, 1.25)):
            e.set_tone_search(K, lo, ratio)
            for pattern in ([17], [7, 8, 2], [1] * 17, [9, 8]):
                e.reset()
                m = TS.Search(n, tab, bank, K, lo, ratio)
                a = 0
                for k in pattern:
                    s = slice(a * 128, (a + k) * 128)
                    audio = _update(e, x[:, s])
                    want = m.run(y[:, s])
                    _same(_records(e, k), want, (len(bank), K, pattern, a))
                    assert np.array_equal(bits(e.read_tone_spectrum().cpu().numpy()), bits(m.spectrum())), (len(bank), K, pattern, a)
                    assert np.array_equal(_search_words(e.save_state(0, n), n), m.words()), (len(bank), K, pattern, a)
                    assert np.array_equal(audio, audio_ref[:, s]), (len(bank), K, pattern, a)
                    found |= set(want[0].ravel().tolist())
                    a += k
                w = m.words()
                assert (want[0][:, :K - 1 if pattern == [17] else 0] == 255).all() and w[:, TS.CNT].max() == 17 % K
                if n >= 3:
                    assert w[1, TS.A2] and not w[2, TS.A2] and (want[0][2] == 255).all()      # the rails read something, silence nothing
    assert 255 in found and (len(found) > 1 or n < 97)                                        # decisions of both kinds occurred
    e.close()


def _voice_station(seed, nb, tone_hz=100.0, tone_amp=0.12, carrier=8000.0):
    """int16 [nb * 128, 2]: a carrier frequency-modulated (5000 Hz peak deviation) by a tone of tone_amp of the deviation and
    voice-band noise of rms 0.25, clipped to the deviation; 3 counts of noise.  carrier 0: an idle channel"""
    r = np.random.default_rng(seed)
    n = nb * 128
    t = np.arange(n)
    mod = np.clip(tone_amp * np.sin(2 * np.pi * tone_hz / 44100.0 * t + 0.7) + T.voice_noise(seed, n), -1.0, 1.0)
    z = carrier * np.exp(1j * 2 * np.pi * 5000.0 / 44100.0 * np.cumsum(mod)) + 3.0 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _station_case():
    nb = 128
    x = np.stack([_voice_station(7, nb), _voice_station(8, nb, tone_amp=0.0), _voice_station(9, nb, carrier=0.0)])
    return x, FM.Fm(3).run(x)[0]


def test_gpu_search_finds_the_stations_tone(rdsp):
    """a station with a 100 Hz tone at 0.12 of the deviation under voice-band noise, one without a tone and one idle channel; a
    bank of the seven tones 67.0, 88.5, 100.0, 103.5, 151.4, 203.5, 254.1, K = 32, the default thresholds, 128 blocks in four
    calls.  The records equal the model's; on the model's output the first receiver reads index 2 from block 31 on, the other two
    read 255 throughout, and sqrt(a2) of the first lies within 3.6 % of 0.12 x rdsp_engine_tone_search_gain(100, 750) after the
    first window (the float32 model alone reads +1.0, -1.4, +1.8 and -2.4 % in the four windows: at K = 32 the voice-band noise
    under the tone moves the reading by that much, so the 2 % first asked for is widened to the model's 2.4 % plus half again)"""
    from radiodsp_sdr_rx_amd.engine import tone_search_gain
    nb, call = 128, 32
    x, y = _station_case()
    e = _engine(3, call)
    e.set_tone_bank(BANK7)
    e.set_tone_search(32)
    m = TS.Search(3, table(rdsp), BANK7, 32)
    recs = []
    for a in range(0, nb, call):
        sl = slice(a * 128, (a + call) * 128)
        e.update(_cuda(x[:, sl]))
        want = m.run(y[:, sl])
        _same(_records(e, call), want, a)
        assert np.array_equal(bits(e.read_tone_spectrum().cpu().numpy()), bits(m.spectrum()))
        recs.append(want)
    best, a2, nxt = (np.concatenate([r[k] for r in recs], 1) for k in range(3))
    amp = np.sqrt(a2[:, 31::32].astype(np.float64))
    want_amp = 0.12 * tone_search_gain(100.0, 750.0)
    print("sqrt(a2) at the ends of the four windows, per receiver:", np.round(amp, 4).tolist(), "0.12 x gain =", round(want_amp, 4))
    assert (best[0, :31] == 255).all() and (best[0, 31:] == 2).all() and (best[1:] == 255).all()
    assert np.abs(amp[0, 1:] / want_amp - 1.0).max() < 0.036
    e.close()


SQUELCH = Squelch(F32(2e-3), F32(1e-3), 1)     # a carrier of 2000 counts reads 3.7e-3: some of the drawn stations open it, some do not


def test_gpu_search_beside_the_squelch(rdsp):
    """meter, tone squelch, voice stage (R = 2) and search together against the same engine without the search, 97 receivers, 17
    blocks as [9, 8], K = 4: the int16 audio, rdsp_engine_read_meter's records (the combined gate among them), the active list,
    rdsp_engine_read_tone's records, the voice rows and every blob part with a flag below 32 are the same bytes, the gate is the
    models' (so it is not trivially shut or open), and the search's records and words equal the model's"""
    n, nb = 97, 17
    x, tones, y, lvl, tail = _drawn(n)
    engines = []
    for with_search in (True, False):
        e = _engine(n, nb, meter=True, search=with_search, tone=True)
        e.set_squelch(float(SQUELCH.open_ms), float(SQUELCH.close_ms), SQUELCH.hang_blocks)
        e.set_tones(0, tones)
        e.set_tone_squelch(4, 0.06, 0.045)
        e.enable_voice(2)
        engines.append(e)
    a, b = engines
    a.set_tone_search(4, 0.06, 2.0)
    tab = table(rdsp)
    m, mt, mm = TS.Search(n, tab, TS.STANDARD, 4, 0.06, 2.0), T.Tone(n, tab, tones, 4, 0.06, 0.045), Meter(n)
    at, seen = 0, set()
    for k in (9, 8):
        s = slice(at * 128, (at + k) * 128)
        d = _cuda(x[:, s])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        wa, wt = mt.run(y[:, s])
        both = mt.gate(mm.run(lvl[:, s], SQUELCH)[2], wt)
        assert np.array_equal(ya, yb) and np.array_equal(ya[..., 0], gated(tail[:, s], both))
        for va, vb in zip(a.read_meter(k), b.read_meter(k)):
            assert np.array_equal(bits(va.cpu().numpy().astype(F32)), bits(vb.cpu().numpy().astype(F32)))
        assert np.array_equal(a.read_meter(k)[2].cpu().numpy(), both)
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        for va, vb in zip(a.read_tone(k), b.read_tone(k)):
            assert np.array_equal(bits(va.cpu().numpy().astype(F32)), bits(vb.cpu().numpy().astype(F32)))
        assert np.array_equal(a.read_voice(k).cpu().numpy(), b.read_voice(k).cpu().numpy())
        _same(_records(a, k), m.run(y[:, s]), at)
        seen |= set(both.ravel().tolist())
        at += k
    assert seen == {0, 1}
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert blob_b.view(np.uint32)[3] == 2 | 4 | 8 | 16 and blob_a.view(np.uint32)[3] == 2 | 4 | 8 | 16 | 32
    assert len(blob_a) == len(blob_b) + n * TS.WORDS * 4 and np.array_equal(blob_a[16:len(blob_b)], blob_b[16:])
    assert np.array_equal(_search_words(blob_a, n), m.words())
    for e in engines:
        e.close()


def test_gpu_search_off_changes_nothing(rdsp):
    """NFM, LSB and AM groups (5 + 3 + 4 receivers), meter and squelch on: an engine that enabled the search with K = 0 everywhere
    gives the audio, the meter records and the active list of one that never enabled it, and reads 255 / 0 / 0; the blob of the
    engine that never enabled it has the size and the flags it always had (meter 2, FM 8) and is, byte for byte, the other's
    without its header flag 32 and its sixth part, which is zeros"""
    from test_engine_meter import _bursts
    n, nb, first = 12, 6, [0, 5, 8]
    x = _bursts(83, n, nb)
    x[:5] = FM.station(90, nb, 4000.0, 1000.0, 9000.0, 3.0)[None]
    engines = []
    for with_search in (True, False):
        e = _engine(n, 4, meter=True, search=with_search, nfm=False)
        e.set_squelch(2e-3, 1e-3, 1)
        e.set_groups(first)
        e.select_group(0); assert e.setDemodMode(NFM) == 0.0
        e.select_group(2); e.setDemodMode(4); e.setAudioFilter(0)
        e.select_group(-1)
        engines.append(e)
    a, b = engines
    assert a.tone_search_enabled and not b.tone_search_enabled
    for k0, k in ((0, 4), (4, 2)):
        d = _cuda(x[:, k0 * 128:(k0 + k) * 128])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        assert np.array_equal(ya, yb) and ya[:5].any() and ya[5:].any()
        for va, vb in zip(a.read_meter(k), b.read_meter(k)):
            assert np.array_equal(bits(va.cpu().numpy().astype(F32)), bits(vb.cpu().numpy().astype(F32)))
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        best, a2, nxt = _records(a, k)
        assert (best == 255).all() and not a2.any() and not nxt.any() and not a.read_tone_spectrum().cpu().numpy().any()
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert len(blob_b) == 16 + n * (CH_WORDS + 3 + 50) * 4 == b.lib.rdsp_engine_state_bytes(b.h, n) and blob_b.view(np.uint32)[3] == 2 | 8
    assert len(blob_a) == len(blob_b) + n * TS.WORDS * 4 == a.lib.rdsp_engine_state_bytes(a.h, n) and blob_a.view(np.uint32)[3] == 2 | 8 | 32
    assert np.array_equal(blob_a[16:len(blob_b)], blob_b[16:]) and not blob_a[len(blob_b):].any()
    assert np.array_equal(blob_a[:12], blob_b[:12])
    with pytest.raises(rdsp.RdspError) as ex:
        b.read_tone_search(0)
    assert ex.value.code == -4
    for e in engines:
        e.close()


def test_gpu_search_state(rdsp):
    """the search's words are signal state.  A receiver whose re, im, cnt and P are nonzero moves by blob to an engine with another
    channel count, another index and another max_blocks and the same bank and K, and continues bit for bit; moved onto an engine
    with another bank it restarts from zeros, as the model does.  An engine without the search refuses the part with nothing
    changed; a blob without the part zeroes the words.  A regrouping with the same K keeps the detector; a changed K, a
    regrouping into a group with another K and a changed bank restart it as the model says; outside NFM the words are left alone
    and coming back restarts them; K = 0 zeroes them; rdsp_engine_reset zeroes them and keeps the bank and the settings"""
    nb, cut, K = 17, 6, 4
    x, tones, y, lvl, tail = _drawn(5)
    tab = table(rdsp)
    a = _engine(5, 8)
    a.enable_tone_search()                                                                    # again: a no-op
    a.set_tone_search(K, 0.06, 2.0)
    m = TS.Search(5, tab, TS.STANDARD, K, 0.06, 2.0)
    a.update(_cuda(x[:, :cut * 128]))
    _same(_records(a, cut), m.run(y[:, :cut * 128]), "cut")
    blob = a.save_state(0, 1)
    w0 = m.words()[0]
    assert w0[TS.CNT] == cut % K and w0[TS.RE:TS.RE + 50].all() and w0[TS.IM + 1:TS.IM + 50].all() and w0[TS.P:TS.P + 50].all() and w0[TS.A2]
    assert np.array_equal(_search_words(blob, 1)[0], w0) and blob.view(np.uint32)[3] == 8 | 32
    plain = _engine(3, 8, search=False)
    assert len(blob) == a.lib.rdsp_engine_state_bytes(a.h, 1) == plain.lib.rdsp_engine_state_bytes(plain.h, 1) + TS.WORDS * 4
    before = plain.save_state(0, 3)
    with pytest.raises(rdsp.RdspError) as ex:                                                 # an engine without the search refuses the part
        plain.load_state(0, blob)
    assert ex.value.code == -4 and np.array_equal(plain.save_state(0, 3), before)
    # the receiver continues in another engine: 7 channels, index 4, 16 blocks a call, a past of its own
    b = _engine(7, 16)
    b.set_tone_search(K, 0.06, 2.0)
    b.update(_cuda(np.broadcast_to(x[1:2, :128], (7, 128, 2)).copy()))
    b.load_state(4, blob)
    assert np.array_equal(_search_words(b.save_state(4, 1), 1)[0], w0)
    rest = np.zeros((7, (nb - cut) * 128, 2), np.int16)
    rest[4] = x[0, cut * 128:]
    b.update(_cuda(rest))
    want = m.run(y[:, cut * 128:])
    got = _records(b, nb - cut)
    _same(tuple(v[4:5] for v in got), tuple(v[:1] for v in want), "moved")
    assert np.array_equal(_search_words(b.save_state(4, 1), 1)[0], m.words()[0])
    # onto another bank: the key does not match, zeros
    c = _engine(2, 16)
    c.set_tone_bank(BANK7)
    c.set_tone_search(K, 0.06, 2.0)
    c.update(_cuda(x[1:3, :128]))                                                             # the mode change's FM reset is spent
    c.load_state(1, blob)
    rest2 = np.zeros((2, (nb - cut) * 128, 2), np.int16)
    rest2[1] = x[0, cut * 128:]
    c.update(_cuda(rest2))
    other = TS.Search(1, tab, BANK7, K, 0.06, 2.0)
    other.w[0] = w0
    fresh = TS.Search(1, tab, BANK7, K, 0.06, 2.0).run(y[:1, cut * 128:])
    _same(tuple(v[1:2] for v in _records(c, nb - cut)), other.run(y[:1, cut * 128:]), "another bank")
    _same(tuple(v[1:2] for v in _records(c, nb - cut)), fresh, "another bank, fresh")
    assert np.array_equal(_search_words(c.save_state(1, 1), 1)[0], other.words()[0])
    b.load_state(4, plain.save_state(0, 1))                                                   # a blob without the part zeroes the words
    assert not _search_words(b.save_state(4, 1), 1).any()
    # a's own stream goes on.  A regrouping with the same K keeps the detector
    a.set_groups([0, 2])
    m2 = TS.Search(5, tab, TS.STANDARD, K, 0.06, 2.0)
    m2.run(y[:, :cut * 128])
    at = cut

    def step(k):
        nonlocal at
        a.update(_cuda(x[:, at * 128:(at + k) * 128]))
        _same(_records(a, k), m2.run(y[:, at * 128:(at + k) * 128]), at)
        assert np.array_equal(_search_words(a.save_state(0, 5), 5), m2.words()), at
        assert np.array_equal(bits(a.read_tone_spectrum().cpu().numpy()), bits(m2.spectrum())), at
        at += k
        return m2.words()
    w = step(3)
    assert w[2, TS.CNT] == (cut + 3) % K
    # group 1 (channels 2, 3, 4) gets K = 8: a changed K restarts its receivers
    a.select_group(1); a.set_tone_search(8, 0.06, 2.0); a.select_group(-1)
    m2.set_search(8, 0.06, 2.0, slice(2, None))
    w = step(4)
    assert w[2, TS.CNT] == 4 and w[2, TS.K_] == 8 and w[0, TS.CNT] == (cut + 7) % K
    # a regrouping into a group with another K: channel 2 joins group 0 (K = 4) and restarts, channels 3 and 4 go on
    a.set_groups([0, 3])
    m2.set_search(K, 0.06, 2.0, slice(2, 3))
    w = step(2)
    assert w[2, TS.CNT] == 2 and w[2, TS.K_] == K and w[4, TS.CNT] == 6 and w[0, TS.CNT] == (cut + 9) % K
    # a changed bank restarts every receiver
    a.set_tone_bank(BANK7)
    m2.set_bank(BANK7)
    w = step(2)
    assert (w[:, TS.CNT] == 2).all() and (w[:, TS.KEY] == m2.key).all() and not w[:, TS.RE + 7:TS.IM].any() and at == nb
    # leaving NFM and coming back: the words are not maintained outside the mode and start from zeros at the next NFM update
    a.set_groups([0])
    a.set_tone_search(K, 0.06, 2.0)
    a.setDemodMode(4)
    a.update(_cuda(x[:, :128]))
    best, a2, nxt = _records(a, 1)
    assert np.array_equal(_search_words(a.save_state(0, 5), 5), w) and (best == 255).all() and not a2.any() and not nxt.any()
    a.setDemodMode(NFM)
    a.update(_cuda(x[:, :5 * 128]))
    ya = FM.Fm(5).run(x[:, :5 * 128])[0]
    m3 = TS.Search(5, tab, BANK7, K, 0.06, 2.0)
    _same(_records(a, 5), m3.run(ya), "back in NFM")
    assert np.array_equal(_search_words(a.save_state(0, 5), 5), m3.words()) and m3.words()[:, TS.P:TS.P + 7].any()
    # K = 0: the words are zeros and the records 255 / 0 / 0
    a.set_tone_search(0)
    a.update(_cuda(x[:, :128]))
    best, a2, nxt = _records(a, 1)
    assert not _search_words(a.save_state(0, 5), 5).any() and (best == 255).all() and not a2.any() and not nxt.any()
    # rdsp_engine_reset zeroes the words and keeps the bank and the settings
    a.set_tone_search(K, 0.06, 2.0)
    a.update(_cuda(x[:, :3 * 128]))
    assert _search_words(a.save_state(0, 5), 5).any()
    a.reset()
    assert not _search_words(a.save_state(0, 5), 5).any() and np.array_equal(a.tone_bank(), np.array(BANK7, F32))
    a.update(_cuda(x[:, :5 * 128]))
    m3.reset()
    _same(_records(a, 5), m3.run(ya), "after the reset")
    for e in (a, b, c, plain):
        e.close()


def test_gpu_search_refusals(rdsp):
    """every refusal that needs an engine, each with the object unchanged: rdsp_engine_enable_tone_search before
    rdsp_engine_enable_fm; the reads before rdsp_engine_enable_tone_search; K outside {0} and 4 ... 512; min_amp zero, negative,
    above 1 or NaN; ratio below 1, above 1e6, NaN or infinite; a bank with a NaN, a value outside [60, 300], not strictly
    ascending, of 0 or 65 tones or NULL; n_blocks above the last call's; short strides; a spectrum range outside the object"""
    import torch
    from test_engine_meter import _engine as plain_engine
    p = plain_engine(2, 4, meter=False)
    assert p.lib.rdsp_engine_enable_tone_search(p.h) == -4 and b"rdsp_engine_enable_fm" in p.lib.rdsp_last_error() and not p.tone_search_enabled
    p.set_tone_bank([100.0, 103.5])                                                           # a setting: it may precede the search
    p.set_tone_search(8)
    p.enable_fm()
    for f in (lambda: p.read_tone_search(0), p.read_tone_spectrum):
        with pytest.raises(rdsp.RdspError) as ex:
            f()
        assert ex.value.code == -4
    p.enable_tone_search()                                                                    # without the tone squelch and the meter
    assert p.tone_search_enabled and not p.tone_enabled and np.array_equal(p.tone_bank(), np.array([100.0, 103.5], F32))
    p.close()
    x, tones, y, lvl, tail = _drawn(5)
    e = _engine(5, 8)
    e.set_tone_search(4, 0.06, 2.0)
    m = TS.Search(5, table(rdsp), TS.STANDARD, 4, 0.06, 2.0)
    e.update(_cuda(x[:, :3 * 128]))
    m.run(y[:, :3 * 128])
    nan, inf = float("nan"), float("inf")
    for bad in ((3, 0.04, 4.0), (1, 0.04, 4.0), (513, 0.04, 4.0), (-1, 0.04, 4.0), (128, 0.0, 4.0), (128, -0.01, 4.0), (128, 1.01, 4.0), (128, nan, 4.0),
                (128, 0.04, 0.99), (128, 0.04, 1.01e6), (128, 0.04, nan), (128, 0.04, inf), (0, 0.0, 4.0)):
        with pytest.raises(rdsp.RdspError) as ex:
            e.set_tone_search(*bad)
        assert ex.value.code == -1, bad
    for bad in ([100.0, nan], [59.9, 100.0], [100.0, 300.1], [100.0, 100.0], [103.5, 100.0], [inf], list(np.linspace(60.0, 300.0, 65)), []):
        with pytest.raises(rdsp.RdspError) as ex:
            e.set_tone_bank(np.array(bad, F32))
        assert ex.value.code == -1, bad
    assert e.lib.rdsp_engine_set_tone_bank(e.h, None, 2) == -1 and e.lib.rdsp_engine_tone_bank(e.h, None) == -1
    assert np.array_equal(e.tone_bank(), np.array(TS.STANDARD, F32))
    best = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    a2 = torch.full((5, 4), 7.0, dtype=torch.float32, device="cuda")
    nxt = torch.full((5, 4), 7.0, dtype=torch.float32, device="cuda")
    for nblk, sb, sa, sn in ((4, 4, 4, 4), (-1, 4, 4, 4), (3, 2, 4, 4), (3, 4, 2, 4), (3, 4, 4, 2)):
        assert e.lib.rdsp_engine_read_tone_search(e.h, nblk, best.data_ptr(), sb, a2.data_ptr(), sa, nxt.data_ptr(), sn, None) == -1, (nblk, sb, sa, sn)
        assert b"rdsp_engine_read_tone_search" in e.lib.rdsp_last_error()
    spec = torch.full((5, 64), 7.0, dtype=torch.float32, device="cuda")
    for c0, cn, ptr, stride in ((0, 5, None, 64), (-1, 1, spec.data_ptr(), 64), (0, 6, spec.data_ptr(), 64), (5, 1, spec.data_ptr(), 64), (0, 0, spec.data_ptr(), 64),
                                (0, 5, spec.data_ptr(), 49)):
        assert e.lib.rdsp_engine_read_tone_spectrum(e.h, c0, cn, ptr, stride, None) == -1, (c0, cn, stride)
        assert b"rdsp_engine_read_tone_spectrum" in e.lib.rdsp_last_error()
    torch.cuda.synchronize()
    assert (best == 7).all() and (a2 == 7.0).all() and (nxt == 7.0).all() and (spec == 7.0).all()
    assert e.lib.rdsp_engine_read_tone_search(e.h, 3, None, 0, a2.data_ptr(), 4, None, 0, None) == 0   # any pointer may be NULL
    assert e.lib.rdsp_engine_read_tone_search(e.h, 3, best.data_ptr(), 4, None, 0, nxt.data_ptr(), 4, None) == 0
    assert e.lib.rdsp_engine_read_tone_spectrum(e.h, 1, 3, spec.data_ptr(), 64, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(spec[:3, :50].cpu().numpy()), bits(m.spectrum()[1:4])) and (spec[:, 50:] == 7.0).all() and (spec[3:] == 7.0).all()
    # nothing of all that changed the object: the stream goes on as the model's
    e.update(_cuda(x[:, 3 * 128:8 * 128]))
    _same(_records(e, 5), m.run(y[:, 3 * 128:8 * 128]), "goes on")
    assert np.array_equal(_search_words(e.save_state(0, 5), 5), m.words())
    e.close()
