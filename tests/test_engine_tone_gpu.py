"""The CTCSS tone squelch of rdsp_engine_t on the GPU (include/rdsp.h "tone squelch"; csrc/rdsp_engine_tone.hip,
csrc/rdsp_engine_tone_host.hip) against tests/engine_tone_model.py on the demodulated rows of tests/engine_fm_model.py.  Every
comparison with the model is exact: floats as uint32, audio as int16.  The rows, the records, all eight state words (through a
blob) and the combined gate for 1, 5, 97 and 300 receivers, K = 4 and 8, four call splits, with and without the meter, aligned
and unaligned output rows; the gate on a station that carries a tone, with the active list and both packs; an engine that
enabled the detector with all tones 0 against one that never did; the state through blobs, regroupings, mode changes, resets
and a changed tone; the refusals.  tests/test_engine_tone.py has what needs no GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import engine_fm_model as FM
import engine_pack_model as P
import engine_tail_model as TM
import engine_tone_model as T
import engine_voice_model as V
from engine_meter_model import Meter, Squelch, gated
from engine_sources_model import table

F32 = np.float32
NFM = 7
CH_WORDS = 96 + 2 * 512 + 3 * 384 + 320      # a channel's words in a blob, in front of the optional parts
TONES = (0.0, 67.0, 88.5, 100.0, 103.5, 151.4, 203.5, 254.1)
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _engine(n, max_blocks, meter=False, tone=True, nfm=True):
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
    if nfm:
        assert e.setDemodMode(NFM) == 0.0
    return e


def _tail(n):
    return TM.Tail(n).setAGCmode(0)


@functools.lru_cache(maxsize=None)
def _drawn(n, nb=17):
    """n receivers, nb blocks: (iq int16 [n, t, 2], tones float32 [n], y, lvl float32 [n, t], tail int16 [n, t]).  Channel c's tone
    is drawn from TONES (0 among them); every third receiver's station carries its tone at 15 % of the deviation, the others a
    drawn audio tone at a drawn deviation; with three or more, channel 1 is on the rails and channel 2 all zeros"""
    r = np.random.default_rng(400 + n)
    tones = r.choice(np.array(TONES, F32), n)
    if n >= 5:
        tones[:5] = (100.0, 151.4, 67.0, 0.0, 254.1)
    x = np.stack([FM.station(500 + c, nb, 750.0, float(tones[c]), r.uniform(500, 20000), 3.0) if c % 3 == 0 and tones[c] else
                  FM.station(500 + c, nb, r.uniform(1500, 5000), r.uniform(300, 3000), r.uniform(200, 20000), r.uniform(1, 30)) for c in range(n)])
    if n >= 3:
        x[1] = r.choice(np.array([32767, -32768], np.int16), (nb * 128, 2))
        x[2] = 0
    y, lvl = FM.Fm(n).run(x)
    return x, tones, y, lvl, _tail(n).run(y)


def _tone_words(blob, n):
    """the detector words of a blob of n channels: its last part"""
    return blob[-n * 8 * 4:].view(np.uint32).reshape(n, 8)


SQUELCH = Squelch(F32(2e-3), F32(1e-3), 1)     # a carrier of 2000 counts reads 3.7e-3: some of the drawn stations open it, some do not


def _update(e, x, out=None):
    """one call; out: a (tensor, stride in pairs) pair for rows that are not 16-byte aligned -> the int16 rows [n, t, 2] on the host"""
    if out is None:
        return e.update(_cuda(x)).cpu().numpy()
    rows, stride = out
    d = _cuda(x)
    assert e.lib.rdsp_engine_update(e.h, d.data_ptr(), x.shape[1], x.shape[1] // 128, rows.data_ptr(), stride, None) == 0, e.lib.rdsp_last_error()
    return rows[:, :x.shape[1]].cpu().numpy()


@pytest.mark.parametrize("meter", [False, True])
@pytest.mark.parametrize("n", [1, 5, 97, 300])
def test_gpu_tone_rows_are_the_model(rdsp, n, meter):
    """1, 5, 97 and 300 receivers (a ragged last workgroup, more than one workgroup) with drawn tones, some of them 0, K = 4 and 8,
    17 blocks as [17], [7, 8, 2], seventeen calls of 1 and [9, 8] -- windows end in mid-call, at a call boundary and inside the
    eight-block trip -- each from a reset: rdsp_engine_read_tone's a2 and tone rows, all eight state words (through a blob) and,
    with the meter, rdsp_engine_read_meter's open records (the carrier gate of engine_meter_model on the model's level rows, and
    the tone records) and the int16 audio (engine_tail_model, gated) equal the models.  Without the meter nothing is gated: the
    audio is the tail's.  [9, 8] runs once more into output rows that are not 16-byte aligned"""
    import torch
    nb = 17
    x, tones, y, lvl, tail = _drawn(n)
    tab = table(rdsp)
    e = _engine(n, nb, meter)
    e.set_tones(0, tones)
    if meter:
        e.set_squelch(float(SQUELCH.open_ms), float(SQUELCH.close_ms), SQUELCH.hang_blocks)
    stride = nb * 128 + 3
    buf = torch.zeros(n * stride * 2 + 8, dtype=torch.int16, device="cuda")
    odd = buf[2:2 + n * stride * 2].view(n, stride, 2)
    assert odd.data_ptr() % 16 == 4
    seen = set()
    for K in (4, 8):
        e.set_tone_squelch(K, 0.06, 0.045)
        for pattern, out in (([17], None), ([7, 8, 2], None), ([1] * 17, None), ([9, 8], None), ([9, 8], (odd, stride))):
            e.reset()
            m, mm = T.Tone(n, tab, tones, K, 0.06, 0.045), Meter(n)
            a = 0
            for k in pattern:
                s = slice(a * 128, (a + k) * 128)
                audio = _update(e, x[:, s], out)
                a2, tone = (v.cpu().numpy() for v in e.read_tone(k))
                wa, wt = m.run(y[:, s])
                assert np.array_equal(bits(a2), bits(wa)), (K, pattern, a, np.argwhere(bits(a2) != bits(wa))[:3])
                assert np.array_equal(tone, wt), (K, pattern, a)
                assert np.array_equal(_tone_words(e.save_state(0, n), n), m.words()), (K, pattern, a)
                want = tail[:, s]
                if meter:
                    carrier = mm.run(lvl[:, s], SQUELCH)[2]
                    both = m.gate(carrier, wt)
                    assert np.array_equal(e.read_meter(k)[2].cpu().numpy(), both), (K, pattern, a)
                    assert np.array_equal(e.active()[0].cpu().numpy(), np.flatnonzero(both.any(1)))
                    assert np.array_equal(e.meter()[:, 3], mm.open.astype(F32))               # the carrier gate's state is the meter's own
                    want = gated(want, both)
                    seen |= {(int(c), int(t)) for c, t in zip(carrier[tones != 0].ravel(), wt[tones != 0].ravel())}
                assert np.array_equal(audio[..., 0], want) and np.array_equal(audio[..., 1], want), (K, pattern, a)
                a += k
            if n >= 5:
                w = m.words()
                assert wt[0].any() and not w[3].any() and not wa[3].any() and w[0, [T.PH, T.RE, T.IM, T.CNT, T.A2]].all()
    if meter and n >= 97:
        assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}                                       # every combination of the two gates occurred
    e.close()


def _voice_station(seed, nb, tone_hz=100.0, tone_until=None, carrier=8000.0):
    """int16 [nb * 128, 2]: a carrier frequency-modulated (5000 Hz peak deviation) by a tone of 0.12 of the deviation (until sample
    tone_until, if given) and voice-band noise of rms 0.25, clipped to the deviation; 3 counts of noise"""
    r = np.random.default_rng(seed)
    n = nb * 128
    t = np.arange(n)
    tone = 0.12 * np.sin(2 * np.pi * tone_hz / 44100.0 * t + 0.7)
    if tone_until is not None:
        tone[tone_until:] = 0.0
    mod = np.clip(tone + T.voice_noise(seed, n), -1.0, 1.0)
    z = carrier * np.exp(1j * 2 * np.pi * 5000.0 / 44100.0 * np.cumsum(mod)) + 3.0 * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _gate_case(stops):
    nb = 128
    x = np.broadcast_to(_voice_station(7, nb, tone_until=64 * 128 if stops else None), (3, nb * 128, 2)).copy()
    y, lvl = FM.Fm(3).run(x)
    return x, y, lvl, _tail(3).run(y)


@pytest.mark.parametrize("stops", [False, True])
def test_gpu_tone_gate(rdsp, stops):
    """three receivers on one synthetic station that carries a 100.0 Hz tone at 0.12 of the deviation under voice-band noise, set
    to 100.0 Hz, to 151.4 Hz and to no tone; K = 32, on_amp 0.06, off_amp 0.045 (idle noise reads up to 0.037 at K = 32: the
    defaults are for K = 128); 128 blocks in four calls.  The first receiver opens after the first full window (block 31), the
    second never opens, the third follows the carrier gate alone.  The int16 audio is the model's gated audio; the open records,
    the active list, rdsp_engine_pack_active and rdsp_engine_pack_voice (R = 2) are their models' on the combined gate, while
    rdsp_engine_get_meter still reports the carrier gate.  stops: the tone is switched off half-way through (block 64) -- the gate
    closes one window later, after block 95, while the carrier gate stays open"""
    from radiodsp_sdr_rx_amd.engine import ms_of_db
    nb, call = 128, 32
    x, y, lvl, tail = _gate_case(stops)
    s = Squelch(F32(ms_of_db(-30.0)), F32(ms_of_db(-36.0)), 2)                              # the carrier of 8000 counts is -9 dB
    e = _engine(3, call, meter=True)
    e.set_squelch(float(s.open_ms), float(s.close_ms), s.hang_blocks)
    e.set_tones(0, [100.0, 151.4, 0.0])
    e.set_tone_squelch(32, 0.06, 0.045)
    e.enable_voice(2)
    m, mm, voice = T.Tone(3, table(rdsp), [100.0, 151.4, 0.0], 32, 0.06, 0.045), Meter(3), V.Voice(3, 2)
    gates, carriers, amps = [], [], []
    for a in range(0, nb, call):
        sl = slice(a * 128, (a + call) * 128)
        yd = e.update(_cuda(x[:, sl]))
        audio = yd.cpu().numpy()
        wa, wt = m.run(y[:, sl])
        carrier = mm.run(lvl[:, sl], s)[2]
        both = m.gate(carrier, wt)
        a2, tone = (v.cpu().numpy() for v in e.read_tone(call))
        assert np.array_equal(bits(a2), bits(wa)) and np.array_equal(tone, wt)
        assert np.array_equal(e.read_meter(call)[2].cpu().numpy(), both) and np.array_equal(e.meter()[:, 3], mm.open.astype(F32))
        want = gated(tail[:, sl], both)
        assert np.array_equal(audio[..., 0], want) and np.array_equal(audio[..., 1], want)
        assert np.array_equal(e.active()[0].cpu().numpy(), np.flatnonzero(both.any(1)))
        pa, pr, needed = e.pack_active(yd)
        wpa, wpr, wn = P.pack(want, both)
        assert needed == wn and np.array_equal(pa.cpu().numpy(), wpa) and np.array_equal(pr.cpu().numpy(), wpr)
        vrows = voice.run(want)
        assert np.array_equal(e.read_voice(call).cpu().numpy(), vrows)
        va, vr, vneeded = e.pack_voice(call)
        wva, wvr, wvn = V.pack(vrows, both, 2)
        assert vneeded == wvn and np.array_equal(va.cpu().numpy(), wva) and np.array_equal(vr.cpu().numpy(), wvr)
        gates.append(both); carriers.append(carrier); amps.append(np.sqrt(wa[:, -1].astype(np.float64)))
    gate, carrier = np.concatenate(gates, 1), np.concatenate(carriers, 1)
    print("tone amplitudes at the ends of the four windows, per receiver:", np.round(np.stack(amps, 1), 4).tolist())
    assert carrier[:, 2:].all() and np.array_equal(gate[2], carrier[2]) and not gate[1].any()
    last = 95 if stops else nb
    assert not gate[0, :31].any() and gate[0, 31:last].all() and not gate[0, last:].any()
    e.close()


def test_gpu_tone_off_changes_nothing(rdsp):
    """NFM, LSB and AM groups (5 + 3 + 4 receivers), meter and squelch on: an engine that enabled the detector with every tone 0
    gives the audio, the meter records and the active list of one that never enabled it, and reads zero tone records; the blob of
    the engine that never enabled it has the size and the flags it always had (sources none, meter 2, FM 8) and is, byte for byte,
    the other's without its fifth part"""
    from test_engine_meter import _bursts
    n, nb, first = 12, 6, [0, 5, 8]
    x = _bursts(83, n, nb)
    x[:5] = FM.station(90, nb, 4000.0, 1000.0, 9000.0, 3.0)[None]
    x[1] = _bursts(84, 1, nb)[0]                                                              # an NFM receiver whose carrier is keyed
    engines = []
    for with_tone in (True, False):
        e = _engine(n, 4, meter=True, tone=with_tone, nfm=False)
        e.set_squelch(2e-3, 1e-3, 1)
        e.set_groups(first)
        e.select_group(0); assert e.setDemodMode(NFM) == 0.0
        e.select_group(2); e.setDemodMode(4); e.setAudioFilter(0)
        e.select_group(-1)
        engines.append(e)
    a, b = engines
    assert a.tone_enabled and not b.tone_enabled
    gates = []
    for k0, k in ((0, 4), (4, 2)):
        d = _cuda(x[:, k0 * 128:(k0 + k) * 128])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        assert np.array_equal(ya, yb) and ya[:5].any() and ya[5:].any()
        for va, vb in zip(a.read_meter(k), b.read_meter(k)):
            assert np.array_equal(bits(va.cpu().numpy().astype(F32)), bits(vb.cpu().numpy().astype(F32)))
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        a2, tone = a.read_tone(k)
        assert not a2.any() and not tone.any()
        gates.append(b.read_meter(k)[2].cpu().numpy())
    gate = np.concatenate(gates, 1)
    assert np.array_equal(gate[1], [0, 0, 1, 1, 1, 1]) and gate[0].all()                      # the keyed NFM receiver: closed blocks, then open ones
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert len(blob_b) == 16 + n * (CH_WORDS + 3 + 50) * 4 == b.lib.rdsp_engine_state_bytes(b.h, n) and blob_b.view(np.uint32)[3] == 2 | 8
    assert len(blob_a) == len(blob_b) + n * 8 * 4 == a.lib.rdsp_engine_state_bytes(a.h, n) and blob_a.view(np.uint32)[3] == 2 | 8 | 16
    assert np.array_equal(blob_a[16:len(blob_b)], blob_b[16:]) and not blob_a[len(blob_b):].any()
    with pytest.raises(rdsp.RdspError) as ex:
        b.read_tone(0)
    assert ex.value.code == -4
    for e in engines:
        e.close()


def test_gpu_tone_state(rdsp):
    """the detector's words are signal state.  A toned receiver whose ph, re, im, cnt and a2 are all nonzero moves by blob to an
    engine with another channel count, another index and another max_blocks, set to the same tone and K, and continues bit for
    bit; moved onto a channel with another tone it restarts from zeros, as the model does.  An engine without the detector refuses
    the part with nothing changed; a blob without the part zeroes the words.  A regrouping into a group with another K, leaving
    NFM and coming back, rdsp_engine_reset and a changed tone in mid-stream each restart the detector as the model says; a
    regrouping with the same K keeps it"""
    nb, cut, K = 17, 6, 4
    x, tones, y, lvl, tail = _drawn(5)                                                        # tones 100, 151.4, 67, 0, 254.1
    tab = table(rdsp)
    a = _engine(5, 8)
    a.enable_tone()                                                                           # again: a no-op
    a.set_tones(0, tones)
    a.set_tone_squelch(K, 0.06, 0.045)
    m = T.Tone(5, tab, tones, K, 0.06, 0.045)
    a.update(_cuda(x[:, :cut * 128]))
    wa, wt = m.run(y[:, :cut * 128])
    assert np.array_equal(bits(a.read_tone(cut)[0].cpu().numpy()), bits(wa))
    blob = a.save_state(0, 1)
    w0 = m.words()[0]
    assert w0[[T.PH, T.RE, T.IM, T.CNT, T.A2]].all() and np.array_equal(_tone_words(blob, 1)[0], w0) and blob.view(np.uint32)[3] == 8 | 16
    plain = _engine(3, 8, tone=False)
    assert len(blob) == a.lib.rdsp_engine_state_bytes(a.h, 1) == plain.lib.rdsp_engine_state_bytes(plain.h, 1) + 8 * 4
    before = plain.save_state(0, 3)
    with pytest.raises(rdsp.RdspError) as ex:                                                 # an engine without the detector refuses the part
        plain.load_state(0, blob)
    assert ex.value.code == -4 and np.array_equal(plain.save_state(0, 3), before)
    # the receiver continues in another engine: 7 channels, index 4, 16 blocks a call, a past of its own; index 5 has another tone
    b = _engine(7, 16)
    b.set_tone_squelch(K, 0.06, 0.045)
    b.set_tones(4, [100.0, 103.5])
    b.update(_cuda(np.broadcast_to(x[1:2, :128], (7, 128, 2)).copy()))
    b.load_state(4, blob)
    b.load_state(5, blob)
    assert np.array_equal(_tone_words(b.save_state(4, 2), 2), np.stack([w0, w0]))
    rest = np.zeros((7, (nb - cut) * 128, 2), np.int16)
    rest[4] = rest[5] = x[0, cut * 128:]
    b.update(_cuda(rest))
    a2, tone = (v.cpu().numpy() for v in b.read_tone(nb - cut))
    ca, ct = m.run(y[:, cut * 128:])
    assert np.array_equal(bits(a2[4]), bits(ca[0])) and np.array_equal(tone[4], ct[0])        # the same tone and K: bit for bit
    other = T.Tone(1, tab, [103.5], K, 0.06, 0.045)
    other.w[0] = w0                                                                           # another tone: the words do not match, zeros
    oa, ot = other.run(y[:1, cut * 128:])
    fresh = T.Tone(1, tab, [103.5], K, 0.06, 0.045).run(y[:1, cut * 128:])
    assert np.array_equal(bits(a2[5]), bits(oa[0])) and np.array_equal(tone[5], ot[0]) and np.array_equal(bits(oa), bits(fresh[0]))
    assert np.array_equal(_tone_words(b.save_state(4, 2), 2), np.stack([m.words()[0], other.words()[0]]))
    b.load_state(4, plain.save_state(0, 1))                                                   # a blob without the part zeroes the words
    assert not _tone_words(b.save_state(4, 1), 1).any()
    # a's own stream goes on.  A regrouping with the same K keeps the detector
    a.set_groups([0, 2])
    m2 = T.Tone(5, tab, tones, K, 0.06, 0.045)
    m2.run(y[:, :cut * 128])
    at = cut

    def step(k):
        nonlocal at
        a.update(_cuda(x[:, at * 128:(at + k) * 128]))
        ka, kt = m2.run(y[:, at * 128:(at + k) * 128])
        got = a.read_tone(k)
        assert np.array_equal(bits(got[0].cpu().numpy()), bits(ka)) and np.array_equal(got[1].cpu().numpy(), kt), at
        assert np.array_equal(_tone_words(a.save_state(0, 5), 5), m2.words()), at
        at += k
        return m2.words()
    w = step(3)
    assert w[2, T.CNT] == (cut + 3) % K
    # group 1 (channels 2, 3, 4) gets K = 8: a changed K restarts its receivers
    a.select_group(1); a.set_tone_squelch(8, 0.06, 0.045); a.select_group(-1)
    m2.set_squelch(8, 0.06, 0.045, slice(2, None))
    w = step(4)
    assert w[2, T.CNT] == 4 and w[2, T.K_] == 8 and w[0, T.CNT] == (cut + 7) % K
    # a regrouping into a group with another K: channel 2 joins group 0 (K = 4) and restarts, channel 4 goes on (3 has no tone)
    a.set_groups([0, 3])
    m2.set_squelch(K, 0.06, 0.045, slice(2, 3))
    w = step(2)
    assert w[2, T.CNT] == 2 and w[2, T.K_] == K and w[4, T.CNT] == 6 and not w[3].any() and w[0, T.CNT] == (cut + 9) % K
    # a changed tone in mid-stream restarts that receiver only
    tones2 = tones.copy()
    tones2[0] = 103.5
    a.set_tones(0, [103.5])
    m2.set_tones([103.5])
    w = step(2)
    assert w[0, T.CNT] == 2 and w[0, T.DPHI] == T.dphi_of(103.5) and w[4, T.CNT] == 0 and w[1, T.CNT] == (cut + 11) % K and at == nb
    # leaving NFM and coming back: the words are not maintained outside the mode and start from zeros at the next NFM update
    a.set_groups([0])
    a.set_tone_squelch(K, 0.06, 0.045)
    m3 = T.Tone(5, tab, tones2, K, 0.06, 0.045)
    a.setDemodMode(4)
    a.update(_cuda(x[:, :128]))
    assert np.array_equal(_tone_words(a.save_state(0, 5), 5), w) and not a.read_tone(1)[0].any()   # untouched, and no records
    a.setDemodMode(NFM)
    a.update(_cuda(x[:, :5 * 128]))
    ya = FM.Fm(5).run(x[:, :5 * 128])[0]
    ra, rt = m3.run(ya)
    assert np.array_equal(bits(a.read_tone(5)[0].cpu().numpy()), bits(ra)) and np.array_equal(_tone_words(a.save_state(0, 5), 5), m3.words())
    # rdsp_engine_reset zeroes the words and keeps the tones and the thresholds
    a.reset()
    assert not _tone_words(a.save_state(0, 5), 5).any()
    a.update(_cuda(x[:, :5 * 128]))
    m3.reset()
    ra, rt = m3.run(ya)
    assert np.array_equal(bits(a.read_tone(5)[0].cpu().numpy()), bits(ra)) and np.array_equal(a.read_tone(5)[1].cpu().numpy(), rt)
    for e in (a, b, plain):
        e.close()


def test_gpu_tone_refusals(rdsp):
    """every refusal that needs an engine, each with the object unchanged: rdsp_engine_enable_tone before rdsp_engine_enable_fm;
    rdsp_engine_read_tone before rdsp_engine_enable_tone; K outside 4 ... 512; thresholds that are zero, negative, above 1, crossed
    or NaN; tones outside {0} and [60, 300] or NaN anywhere in the array, a range outside the object; n_blocks above the last
    call's; a short stride"""
    import torch
    from test_engine_meter import _engine as plain_engine
    p = plain_engine(2, 4, meter=False)
    assert p.lib.rdsp_engine_enable_tone(p.h) == -4 and b"rdsp_engine_enable_fm" in p.lib.rdsp_last_error() and not p.tone_enabled
    p.set_tones(0, [100.0, 0.0])                                                              # a setting: it may precede the detector
    p.enable_fm()
    with pytest.raises(rdsp.RdspError) as ex:
        p.read_tone(0)
    assert ex.value.code == -4
    p.close()
    x, tones, y, lvl, tail = _drawn(5)
    e = _engine(5, 8)
    e.set_tones(0, tones)
    e.set_tone_squelch(4, 0.06, 0.045)
    m = T.Tone(5, table(rdsp), tones, 4, 0.06, 0.045)
    e.update(_cuda(x[:, :3 * 128]))
    m.run(y[:, :3 * 128])
    nan, inf = float("nan"), float("inf")
    for bad in ((3, 0.04, 0.025), (513, 0.04, 0.025), (-1, 0.04, 0.025), (128, 0.04, 0.0), (128, 0.04, -0.01), (128, 1.01, 0.025), (128, 0.02, 0.025),
                (128, nan, 0.025), (128, 0.04, nan), (128, inf, 0.025)):
        with pytest.raises(rdsp.RdspError) as ex:
            e.set_tone_squelch(*bad)
        assert ex.value.code == -1, bad
    for first, bad in ((0, [100.0, 59.9]), (0, [300.1]), (2, [nan]), (0, [100.0, 100.0, -67.0]), (0, [inf]), (4, [100.0, 100.0]), (-1, [100.0]), (5, [100.0])):
        with pytest.raises(rdsp.RdspError) as ex:
            e.set_tones(first, bad)
        assert ex.value.code == -1, (first, bad)
    assert e.lib.rdsp_engine_set_tones(e.h, 0, 1, None) == -1 and e.lib.rdsp_engine_set_tones(e.h, 0, 0, (C.c_float * 1)(100.0)) == -1
    a2 = torch.full((5, 4), 7.0, dtype=torch.float32, device="cuda")
    tone = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    for nblk, s_a2, s_tone in ((4, 4, 4), (-1, 4, 4), (3, 2, 4), (3, 4, 2)):
        assert e.lib.rdsp_engine_read_tone(e.h, nblk, a2.data_ptr(), s_a2, tone.data_ptr(), s_tone, None) == -1, (nblk, s_a2, s_tone)
        assert b"rdsp_engine_read_tone" in e.lib.rdsp_last_error()
    torch.cuda.synchronize()
    assert (a2 == 7.0).all() and (tone == 7).all()
    assert e.lib.rdsp_engine_read_tone(e.h, 3, None, 0, tone.data_ptr(), 4, None) == 0         # either pointer may be NULL
    assert e.lib.rdsp_engine_read_tone(e.h, 3, a2.data_ptr(), 4, None, 0, None) == 0
    # nothing of all that changed the object: the stream goes on as the model's
    e.update(_cuda(x[:, 3 * 128:8 * 128]))
    wa, wt = m.run(y[:, 3 * 128:8 * 128])
    got = e.read_tone(5)
    assert np.array_equal(bits(got[0].cpu().numpy()), bits(wa)) and np.array_equal(got[1].cpu().numpy(), wt)
    assert np.array_equal(_tone_words(e.save_state(0, 5), 5), m.words())
    e.close()
