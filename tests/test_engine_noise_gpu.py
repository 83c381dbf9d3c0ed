"""The noise squelch of rdsp_engine_t on the GPU (include/rdsp.h "noise squelch"; csrc/rdsp_engine_noise.hip,
csrc/rdsp_engine_noise_host.hip) against tests/engine_noise_model.py on the demodulated rows of tests/engine_fm_model.py.  Every
comparison with the model is exact: floats as uint32, audio as int16.  The records, all 68 state words (through a blob), the
combined gate, the active list and the gated audio for 1, 5, 97 and 300 receivers in groups of both W, both time constants and
all three modes, six call splits, with and without the meter, aligned and unaligned output rows; the gate on a station that
stops, an empty channel, an off-centre station and a station 40 dB down, with both packs; an engine whose groups are all at mode
0 against one that never enabled the detector; the detector beside the tone and the code squelch; the state through blobs,
regroupings, changed settings, mode changes and resets; the refusals.  tests/test_engine_noise.py has what needs no GPU."""
import functools

import numpy as np
import pytest

import engine_dcs_model as D
import engine_fm_model as FM
import engine_noise_model as NZ
import engine_pack_model as P
import engine_tail_model as TM
import engine_tone_model as T
import engine_voice_model as V
from engine_meter_model import Meter, Squelch, gated
from engine_sources_model import table

F32 = np.float32
NFM = 7
CH_WORDS = 96 + 2 * 512 + 3 * 384 + 320      # a channel's words in a blob, in front of the optional parts
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _engine(n, max_blocks, meter=False, noise=True, nfm=True, tone=False, dcs=False):
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
    if dcs:
        e.enable_dcs()
    if noise:
        e.enable_noise()
    if nfm:
        assert e.setDemodMode(NFM) == 0.0
    return e


def _tail(n):
    return TM.Tail(n).setAGCmode(0)


def _noise_words(blob, n):
    """the detector words of a blob of n channels: its last part"""
    return blob[-n * NZ.WORDS * 4:].view(np.uint32).reshape(n, NZ.WORDS)


def _update(e, x, out=None):
    """one call; out: a (tensor, stride in pairs) pair for rows that are not 16-byte aligned -> the int16 rows [n, t, 2] on the host"""
    if out is None:
        return e.update(_cuda(x)).cpu().numpy()
    rows, stride = out
    d = _cuda(x)
    assert e.lib.rdsp_engine_update(e.h, d.data_ptr(), x.shape[1], x.shape[1] // 128, rows.data_ptr(), stride, None) == 0, e.lib.rdsp_last_error()
    return rows[:, :x.shape[1]].cpu().numpy()


def _records(e, k):
    N, nopen = (v.cpu().numpy() for v in e.read_noise(k))
    return N, nopen


SQUELCH = Squelch(F32(2e-3), F32(1e-3), 1)     # a carrier of 2000 counts reads 3.7e-3: some of the drawn rows open it, some do not
ROWS_SET = dict(open_n=0.01, close_n=0.025, hang_blocks=2, fall=0.75, rise=0.125)            # a short hang: gates close inside 20 blocks
NB = 20


def _groups(n):
    """(first channels, (W, tau_us, mode) per group): one group for one receiver, three for five, six for more -- both W, both
    time constants, all three modes"""
    if n == 1:
        return [0], [(2, 750.0, NZ.GATE)]
    if n == 5:
        return [0, 2, 4], [(2, 750.0, NZ.GATE), (3, 0.0, NZ.MEASURE), (2, 0.0, NZ.OFF)]
    r = np.random.default_rng(60 + n)
    first = [0] + sorted(int(v) for v in r.choice(np.arange(4, n - 1), 5, replace=False))
    return first, [(2, 750.0, NZ.GATE), (3, 0.0, NZ.GATE), (3, 750.0, NZ.MEASURE), (2, 0.0, NZ.OFF), (2, 0.0, NZ.GATE), (3, 750.0, NZ.GATE)]


@functools.lru_cache(maxsize=None)
def _drawn(n):
    """n receivers, NB blocks: (iq int16 [n, t, 2], y, lvl float32 [n, t], tail int16 [n, t]), the FM rows by group.  A receiver's
    row is drawn from: a station at a drawn carrier level (60 ... 20000 counts) and offset (within +-1500 Hz) over drawn noise, an
    empty channel at a drawn level (some open the carrier squelch), a station that stops after a drawn block; with three or more,
    channel 1 is on the rails and channel 2 all zeros"""
    r = np.random.default_rng(700 + n)
    rows = []
    for c in range(n):
        kind = r.integers(0, 4) if c else 0
        if kind == 0:
            rows.append(NZ.station(800 + c, NB, r.uniform(60, 20000), r.uniform(0.3, 30), r.uniform(-1500, 1500)))
        elif kind == 1:
            rows.append(NZ.station(800 + c, NB, 0, 10.0 ** r.uniform(0, 3.6)))
        elif kind == 2:
            rows.append(NZ.station(800 + c, NB, r.uniform(2000, 20000), 3.0, r.uniform(-1500, 1500), until=int(r.integers(3, 9)) * 128))
        else:
            rows.append(NZ.station(800 + c, NB, r.uniform(300, 1500), 212.0, r.uniform(-1500, 1500)))
    x = np.stack(rows)
    if n >= 3:
        x[1] = r.choice(np.array([32767, -32768], np.int16), (NB * 128, 2))
        x[2] = 0
    first, sets = _groups(n)
    y, lvl = np.zeros((n, NB * 128), F32), np.zeros((n, NB * 128), F32)
    for g, (W, tau, _) in enumerate(sets):
        s = slice(first[g], first[g + 1] if g + 1 < len(first) else n)
        y[s], lvl[s] = FM.Fm(s.stop - s.start, W, 5000.0, tau).run(x[s])
    return x, y, lvl, _tail(n).run(y)


def _model(n):
    first, sets = _groups(n)
    m = NZ.Noise(n)
    for g, (W, tau, mode) in enumerate(sets):
        m.set(mode, W, tau, channels=slice(first[g], first[g + 1] if g + 1 < len(first) else n), **ROWS_SET)
    return m


@pytest.mark.parametrize("meter", [False, True])
@pytest.mark.parametrize("n", [1, 5, 97, 300])
def test_gpu_noise_rows_are_the_model(rdsp, n, meter):
    """1, 5, 97 and 300 receivers (a ragged last workgroup, more than one workgroup) on drawn rows -- stations at drawn levels and
    offsets, empty channels, stations that stop, one row on the rails, one all zeros -- in groups of both W, tau_us 0 and 750 and
    modes 0, 1 and 2; 3 blocks as [3], [1, 2], [1, 1, 1] and 20 blocks as [20], [7, 9, 4] and twenty calls of one -- they cross
    the eight-block trip inside a call and between calls -- each from a reset: rdsp_engine_read_noise's two records, all 68 state
    words (through a blob) and, with the meter, rdsp_engine_read_meter's open records (the carrier gate of engine_meter_model on
    the model's level rows, and the noise gate of the groups at mode 2), the active list and the int16 audio (engine_tail_model,
    gated) equal the models.  Without the meter nothing is gated: the audio is the tail's.  [7, 9, 4] runs once more into output
    rows that are not 16-byte aligned.  At 97 and 300 receivers every combination of the two gates occurs"""
    import torch
    x, y, lvl, tail = _drawn(n)
    first, sets = _groups(n)
    e = _engine(n, NB, meter)
    e.set_groups(first)
    for g, (W, tau, mode) in enumerate(sets):
        e.select_group(g)
        e.set_fm(W, 5000.0, tau)
        e.set_noise_squelch(mode, **ROWS_SET)
    e.select_group(-1)
    if meter:
        e.set_squelch(float(SQUELCH.open_ms), float(SQUELCH.close_ms), SQUELCH.hang_blocks)
    stride = NB * 128 + 3
    buf = torch.zeros(n * stride * 2 + 8, dtype=torch.int16, device="cuda")
    odd = buf[2:2 + n * stride * 2].view(n, stride, 2)
    assert odd.data_ptr() % 16 == 4
    gating = _model(n).mode == NZ.GATE
    seen = set()
    for pattern, out in (([3], None), ([1, 2], None), ([1, 1, 1], None), ([20], None), ([7, 9, 4], None), ([1] * 20, None), ([7, 9, 4], (odd, stride))):
        e.reset()
        m, mm = _model(n), Meter(n)
        a = 0
        for k in pattern:
            s = slice(a * 128, (a + k) * 128)
            audio = _update(e, x[:, s], out)
            N, nopen = _records(e, k)
            wN, wo = m.run(y[:, s])
            assert np.array_equal(bits(N), bits(wN)), (pattern, a, np.argwhere(bits(N) != bits(wN))[:3])
            assert np.array_equal(nopen, wo), (pattern, a)
            assert np.array_equal(_noise_words(e.save_state(0, n), n), m.words()), (pattern, a)
            want = tail[:, s]
            if meter:
                carrier = mm.run(lvl[:, s], SQUELCH)[2]
                both = m.gate(carrier, wo)
                assert np.array_equal(e.read_meter(k)[2].cpu().numpy(), both), (pattern, a)
                assert np.array_equal(e.active()[0].cpu().numpy(), np.flatnonzero(both.any(1)))
                assert np.array_equal(e.meter()[:, 3], mm.open.astype(F32))                   # the carrier gate's state is the meter's own
                want = gated(want, both)
                seen |= {(int(c), int(t)) for c, t in zip(carrier[gating].ravel(), wo[gating].ravel())}
            assert np.array_equal(audio[..., 0], want) and np.array_equal(audio[..., 1], want), (pattern, a)
            a += k
        if n == 5 and pattern == [NB]:
            w = m.words()
            assert not wo[1].any()                                                            # the rails (mode 2): shut
            assert not wo[2, :3].any() and wo[2, 3:].all() and not w[2, NZ.HIST0:].any()      # silence (mode 1) opens: N decays from 1.0
            assert w[2, NZ.KEY] == NZ.key_of(NZ.MEASURE, 3, 0.0) and w[0, NZ.HIST0:].all()
            assert not w[4].any() and not wN[4].any() and not wo[4].any()                     # mode 0: zero words, zero records
    if meter and n >= 97:
        assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}
    e.close()


@functools.lru_cache(maxsize=None)
def _gate_case():
    """four receivers of one band, 48 blocks: a station that stops after block 24, an empty channel, a station 1500 Hz off centre,
    a strong station whose input is 40 dB down (80 counts over the rounding to int16)"""
    nb = 48
    x = np.stack([NZ.station(21, nb, 8000.0, 3.0, until=24 * 128), NZ.station(22, nb, 0, 212.0), NZ.station(23, nb, 8000.0, 3.0, 1500.0),
                  NZ.station(24, nb, 80.0, 0.03)])
    y, lvl = FM.Fm(4).run(x)
    return x, y, lvl, _tail(4).run(y)


@pytest.mark.parametrize("carrier_squelch", [False, True])
def test_gpu_noise_gate(rdsp, carrier_squelch):
    """four receivers on one band, the defaults at mode 2, the meter's squelch off: the noise gate works alone.  The station that
    stops after block 24 of 48 is open from its fourth block on and closes hang_blocks blocks after N crosses close_n; the empty
    channel never opens; the station 1500 Hz off centre and the strong station whose input is 40 dB down are open from their
    fourth block on -- one pair of thresholds for both levels.  48 blocks in three calls: the records, the open records, the
    int16 audio, the active list, rdsp_engine_pack_active and rdsp_engine_pack_voice (R = 2) are their models' on the combined
    gate, while rdsp_engine_get_meter reports the carrier gate.  carrier_squelch: once more with the carrier squelch on at
    thresholds the station 40 dB down does not reach -- it stays shut, the others are as before: the AND"""
    from radiodsp_sdr_rx_amd.engine import ms_of_db
    nb, call = 48, 16
    x, y, lvl, tail = _gate_case()
    s = Squelch(F32(ms_of_db(-30.0)), F32(ms_of_db(-36.0)), 2) if carrier_squelch else Squelch()
    e = _engine(4, call, meter=True)
    if carrier_squelch:
        e.set_squelch(float(s.open_ms), float(s.close_ms), s.hang_blocks)
    e.set_noise_squelch()
    e.enable_voice(2)
    m, mm, voice = NZ.Noise(4), Meter(4), V.Voice(4, 2)
    gates, carriers, levels = [], [], []
    for a in range(0, nb, call):
        sl = slice(a * 128, (a + call) * 128)
        yd = e.update(_cuda(x[:, sl]))
        audio = yd.cpu().numpy()
        wN, wo = m.run(y[:, sl])
        carrier = mm.run(lvl[:, sl], s)[2]
        both = m.gate(carrier, wo)
        N, nopen = _records(e, call)
        assert np.array_equal(bits(N), bits(wN)) and np.array_equal(nopen, wo)
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
        gates.append(both); carriers.append(carrier); levels.append(wN)
    gate, carrier, N = np.concatenate(gates, 1), np.concatenate(carriers, 1), np.concatenate(levels, 1)
    cross = 24 + int(np.argmax(N[0, 24:] > F32(0.025)))
    print(f"N crosses close_n at block {cross}; the gate closes at block {cross + 8}; N of the four receivers at the end: {np.round(N[:, -1], 5).tolist()}")
    assert not gate[0, :3].any() and gate[0, 3:cross + 8].all() and not gate[0, cross + 8:].any() and 24 <= cross <= 38
    assert not gate[1].any() and not gate[2, :3].any() and gate[2, 3:].all()
    if carrier_squelch:
        assert carrier[[0, 2]].all() and not carrier[[1, 3]].any() and not gate[3].any()       # the carrier gate outlasts the station: its decay is slow
    else:
        assert carrier.all() and not gate[3, :3].any() and gate[3, 3:].all()
    e.close()


def test_gpu_noise_off_changes_nothing(rdsp):
    """NFM, LSB and AM groups (5 + 3 + 4 receivers), meter and squelch on: an engine that enabled the detector with every group at
    mode 0 gives the audio, the meter records and the active list of one that never enabled it, and reads zero records; the blob
    of the engine that never enabled it has the size and the flags it always had (sources none, meter 2, FM 8) and is, byte for
    byte, the other's without its last part, which is zeros"""
    from test_engine_meter import _bursts
    n, nb, first = 12, 6, [0, 5, 8]
    x = _bursts(83, n, nb)
    x[:5] = FM.station(90, nb, 4000.0, 1000.0, 9000.0, 3.0)[None]
    x[1] = _bursts(84, 1, nb)[0]                                                              # an NFM receiver whose carrier is keyed
    engines = []
    for with_noise in (True, False):
        e = _engine(n, 4, meter=True, noise=with_noise, nfm=False)
        e.set_squelch(2e-3, 1e-3, 1)
        e.set_groups(first)
        e.select_group(0); assert e.setDemodMode(NFM) == 0.0
        e.select_group(2); e.setDemodMode(4); e.setAudioFilter(0)
        e.select_group(-1)
        engines.append(e)
    a, b = engines
    assert a.noise_enabled and not b.noise_enabled
    for k0, k in ((0, 4), (4, 2)):
        d = _cuda(x[:, k0 * 128:(k0 + k) * 128])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        assert np.array_equal(ya, yb) and ya[:5].any() and ya[5:].any()
        for va, vb in zip(a.read_meter(k), b.read_meter(k)):
            assert np.array_equal(bits(va.cpu().numpy().astype(F32)), bits(vb.cpu().numpy().astype(F32)))
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        N, nopen = _records(a, k)
        assert not N.any() and not nopen.any()
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert len(blob_b) == 16 + n * (CH_WORDS + 3 + 50) * 4 == b.lib.rdsp_engine_state_bytes(b.h, n) and blob_b.view(np.uint32)[3] == 2 | 8
    assert len(blob_a) == len(blob_b) + n * NZ.WORDS * 4 == a.lib.rdsp_engine_state_bytes(a.h, n) and blob_a.view(np.uint32)[3] == 2 | 8 | 128
    assert np.array_equal(blob_a[16:len(blob_b)], blob_b[16:]) and not blob_a[len(blob_b):].any()
    with pytest.raises(rdsp.RdspError) as ex:
        b.read_noise(0)
    assert ex.value.code == -4
    for e in engines:
        e.close()


@functools.lru_cache(maxsize=None)
def _both_case():
    """two receivers, 128 blocks: a station that carries a 254.1 Hz tone at 0.12 of the deviation and code 023 at 0.3 under
    voice-band noise, and an empty channel"""
    nb = 128
    t = np.arange(nb * 128)
    r = np.random.default_rng(31)
    mod = np.clip(0.12 * np.sin(2 * np.pi * 254.1 / 44100.0 * t + 0.7) + 0.3 * D.nrz(D.codeword(0o023), len(t), 4.4) + T.voice_noise(31, len(t)), -1.0, 1.0)
    z = 8000.0 * np.exp(1j * 2 * np.pi * 5000.0 / 44100.0 * np.cumsum(mod)) + 3.0 * (r.standard_normal(len(t)) + 1j * r.standard_normal(len(t)))
    x = np.stack([np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16), NZ.station(32, nb, 0, 212.0)])
    y, lvl = FM.Fm(2).run(x)
    return x, y, lvl, _tail(2).run(y)


def test_gpu_noise_beside_tone_and_dcs(rdsp):
    """a station with a 254.1 Hz tone and code 023, its receiver set to both, and an empty channel whose receiver has neither;
    the meter's squelch off; tone squelch (K = 32), code squelch (K = 16, max_err 1, on 4, off 2) and noise squelch (mode 2, the
    defaults) on.  The records of all three detectors are their models'; the open records are the models' AND -- the station opens
    when the last of its three gates does, the empty channel is shut by the noise gate alone --, the audio is the tail's gated by
    that, and the blob carries all three parts"""
    nb, call, n = 128, 32, 2
    x, y, lvl, tail = _both_case()
    tones, codes = [254.1, 0.0], [0o023, 0]
    e = _engine(n, call, meter=True, tone=True, dcs=True)
    e.set_tones(0, tones)
    e.set_tone_squelch(32, 0.06, 0.045)
    e.set_dcs_codes(0, codes)
    e.set_dcs_squelch(16, 1, 4, 2)
    e.set_noise_squelch()
    mt, md, mn = T.Tone(n, table(rdsp), tones, 32, 0.06, 0.045), D.Dcs(n, codes, 16, 1, 4, 2), NZ.Noise(n)
    gates, parts = [], []
    for k0 in range(0, nb, call):
        sl = slice(k0 * 128, (k0 + call) * 128)
        audio = e.update(_cuda(x[:, sl])).cpu().numpy()
        wa, wt = mt.run(y[:, sl])
        rec = md.run(y[:, sl])
        wN, wo = mn.run(y[:, sl])
        N, nopen = _records(e, call)
        a2, tone = (v.cpu().numpy() for v in e.read_tone(call))
        assert np.array_equal(bits(N), bits(wN)) and np.array_equal(nopen, wo)
        assert np.array_equal(bits(a2), bits(wa)) and np.array_equal(tone, wt) and np.array_equal(e.read_dcs(call)[0].cpu().numpy(), rec[0])
        both = md.gate(mt.gate(mn.gate(np.ones((n, call), np.uint8), wo), wt), rec[0])
        assert np.array_equal(e.read_meter(call)[2].cpu().numpy(), both)
        want = gated(tail[:, sl], both)
        assert np.array_equal(audio[..., 0], want) and np.array_equal(audio[..., 1], want)
        assert np.array_equal(e.active()[0].cpu().numpy(), np.flatnonzero(both.any(1)))
        gates.append(both); parts.append((wo, wt, rec[0]))
    gate = np.concatenate(gates, 1)
    firsts = [int(np.argmax(np.concatenate([p[k] for p in parts], 1)[0])) for k in range(3)]
    assert gate[0].any() and int(np.argmax(gate[0])) == max(firsts) >= 31 and firsts[0] == 3 and not gate[1].any()
    blob = e.save_state(0, n)
    assert blob.view(np.uint32)[3] == 2 | 8 | 16 | 64 | 128 and np.array_equal(_noise_words(blob, n), mn.words())
    e.close()


def test_gpu_noise_state(rdsp):
    """the detector's words are signal state.  A receiver in mid-hang, with a nonzero history, moves by blob to an engine with
    another channel count, another index and another max_blocks and continues bit for bit.  An engine without the detector
    refuses the part with nothing changed; a blob without the part zeroes the words and the receiver comes up CLOSED, N from 1.0.
    A regrouping with the same settings keeps the detector; a changed mode, a regrouping into a group at another mode, a changed W
    and a changed tau_us (0 <-> not 0) each restart it as the model says; outside NFM the words are not maintained and coming
    back restarts it; rdsp_engine_reset zeroes the words"""
    nb, cut = 40, 12
    x = np.stack([NZ.station(41, nb, 8000.0, 3.0, until=4 * 128), NZ.station(42, nb, 6000.0, 3.0, 900.0), NZ.station(43, nb, 0, 212.0),
                  NZ.station(44, nb, 3000.0, 30.0, -1200.0), NZ.station(45, nb, 9000.0, 3.0)])
    fm = FM.Fm(5)
    a = _engine(5, 8)
    a.enable_noise()                                                                          # again: a no-op
    a.set_noise_squelch()
    m = NZ.Noise(5)
    at = 0

    def step(k, e=a, model=m, rows=None):
        nonlocal at
        e.update(_cuda(x[:, at * 128:(at + k) * 128]))
        wN, wo = model.run(fm.run(x[:, at * 128:(at + k) * 128])[0] if rows is None else rows)
        N, nopen = _records(e, k)
        assert np.array_equal(bits(N), bits(wN)) and np.array_equal(nopen, wo), at
        assert np.array_equal(_noise_words(e.save_state(0, 5), 5), model.words()), at
        at += k
        return wN, wo
    step(8); step(cut - 8)
    blob = a.save_state(0, 1)
    w0 = m.words()[0]
    assert w0[NZ.OPEN] == 1 and 0 < w0[NZ.HANG] < 8 and w0[NZ.HIST0:].all() and np.array_equal(_noise_words(blob, 1)[0], w0)
    assert blob.view(np.uint32)[3] == 8 | 128
    plain = _engine(3, 8, noise=False)
    assert len(blob) == a.lib.rdsp_engine_state_bytes(a.h, 1) == plain.lib.rdsp_engine_state_bytes(plain.h, 1) + NZ.WORDS * 4
    before = plain.save_state(0, 3)
    with pytest.raises(rdsp.RdspError) as ex:                                                 # an engine without the detector refuses the part
        plain.load_state(0, blob)
    assert ex.value.code == -4 and np.array_equal(plain.save_state(0, 3), before)
    # the receiver continues in another engine: 7 channels, index 4, 16 blocks a call, a past of its own
    b = _engine(7, 16)
    b.set_noise_squelch()
    b.update(_cuda(np.broadcast_to(x[1:2, :128], (7, 128, 2)).copy()))
    b.load_state(4, blob)
    assert np.array_equal(_noise_words(b.save_state(4, 1), 1)[0], w0)
    rest = np.zeros((7, 16 * 128, 2), np.int16)
    rest[4] = x[0, cut * 128:(cut + 16) * 128]
    b.update(_cuda(rest))
    N, nopen = _records(b, 16)
    fm_b, m_b = FM.Fm(5), NZ.Noise(5)
    fm_b.run(x[:, :cut * 128])
    m_b.w[:] = m.words()
    cN, co = m_b.run(fm_b.run(x[:, cut * 128:(cut + 16) * 128])[0])
    assert np.array_equal(bits(N[4]), bits(cN[0])) and np.array_equal(nopen[4], co[0]) and co[0, 0] == 1 and not co[0, -1]   # it closes there as here
    # a blob without the part zeroes the words: the receiver comes up closed, N from 1.0, whatever it was
    b.load_state(4, plain.save_state(0, 1))
    assert not _noise_words(b.save_state(4, 1), 1).any()
    one = np.broadcast_to(NZ.station(45, 5, 9000.0, 3.0), (7, 5 * 128, 2)).copy()
    b.update(_cuda(one))
    N, nopen = _records(b, 5)
    zN, zo = NZ.Noise(5).run(FM.Fm(5).run(one[:5])[0])                                         # the blob's FM words are a fresh detector's too
    assert np.array_equal(bits(N[4]), bits(zN[0])) and np.array_equal(nopen[4], zo[0]) and not zo[0, :3].any() and zo[0, -1] == 1 and zN[0, 0] > 0.01
    # a's own stream goes on.  A regrouping with the same settings keeps the detector
    a.set_groups([0, 2])
    wN, wo = step(3)
    assert wo[1].all() and wo[4].all() and not wo[2].any()
    # group 1 (channels 2, 3, 4) measures only: a changed mode restarts its receivers -- closed, N from 1.0
    a.select_group(1); a.set_noise_squelch(1); a.select_group(-1)
    m.set(NZ.MEASURE, channels=slice(2, None))
    wN, wo = step(5)
    assert np.array_equal(wo[4], [0, 0, 0, 1, 1]) and wo[1].all() and not wo[2:, :3].any() and m.words()[4, NZ.KEY] == NZ.key_of(1, 2, 750.0)
    # one group again, group 0's settings: channels 2 ... 4 restart once more
    a.set_groups([0])
    m.set(NZ.GATE, channels=slice(2, None))
    wN, wo = step(4)
    assert np.array_equal(wo[4], [0, 0, 0, 1]) and wo[1].all()
    # a changed W, then a changed tau_us: every receiver restarts (the FM detector goes on: set_fm resets nothing)
    a.set_fm(3, 5000.0, 750.0)
    fm.set(3, 5000.0, 750.0); m.set(NZ.GATE, 3, 750.0)
    wN, wo = step(4)
    assert not wo[:, :3].any() and wo[4, 3]
    a.set_fm(3, 5000.0, 0.0)
    fm.set(3, 5000.0, 0.0); m.set(NZ.GATE, 3, 0.0)
    wN, wo = step(4)
    assert not wo[:, :3].any() and wo[[1, 3, 4], 3].all() and at == 32                         # no de-emphasis to undo: a station's DC is no step
    # leaving NFM: the words are not maintained outside the mode; coming back starts the detector
    w = m.words()
    a.setDemodMode(4)
    a.update(_cuda(x[:, :128]))
    assert np.array_equal(_noise_words(a.save_state(0, 5), 5), w) and not _records(a, 1)[0].any()   # untouched, and no records
    a.setDemodMode(NFM)
    fm.reset(); m.reset()
    wN, wo = step(5)
    assert not wo[:, :3].any() and wo[4, 3:].all() and wo[[1, 3], 4].all()
    # rdsp_engine_reset zeroes the words and keeps the settings
    a.reset()
    assert not _noise_words(a.save_state(0, 5), 5).any()
    fm.reset(); m.reset()
    step(3)
    for e in (a, b, plain):
        e.close()


def test_gpu_noise_refusals(rdsp):
    """every refusal that needs an engine, each with the object unchanged: rdsp_engine_enable_noise before rdsp_engine_enable_fm;
    rdsp_engine_read_noise before rdsp_engine_enable_noise; a mode outside 0 ... 2; thresholds that are zero, negative, crossed,
    infinite or NaN; a hang outside 0 ... 65535; coefficients outside (0, 1] or NaN; n_blocks above the last call's; a short stride"""
    import torch
    from test_engine_meter import _engine as plain_engine
    p = plain_engine(2, 4, meter=False)
    assert p.lib.rdsp_engine_enable_noise(p.h) == -4 and b"rdsp_engine_enable_fm" in p.lib.rdsp_last_error() and not p.noise_enabled
    p.set_noise_squelch(2)                                                                    # a setting: it may precede the detector
    p.enable_fm()
    with pytest.raises(rdsp.RdspError) as ex:
        p.read_noise(0)
    assert ex.value.code == -4
    p.close()
    x = np.stack([NZ.station(51, 8, 8000.0, 3.0), NZ.station(52, 8, 0, 212.0), NZ.station(53, 8, 5000.0, 3.0, 1400.0)])
    y = FM.Fm(3).run(x)[0]
    e = _engine(3, 8)
    e.set_noise_squelch(2, 0.01, 0.025, 3, 0.75, 0.125)
    m = NZ.Noise(3, hang_blocks=3)
    e.update(_cuda(x[:, :3 * 128]))
    m.run(y[:, :3 * 128])
    nan, inf = float("nan"), float("inf")
    for bad in ((3, 0.01, 0.025, 8, 0.75, 0.125), (-1, 0.01, 0.025, 8, 0.75, 0.125), (2, 0.0, 0.025, 8, 0.75, 0.125), (2, -0.01, 0.025, 8, 0.75, 0.125),
                (2, 0.03, 0.025, 8, 0.75, 0.125), (2, 0.01, inf, 8, 0.75, 0.125), (2, nan, 0.025, 8, 0.75, 0.125), (2, 0.01, nan, 8, 0.75, 0.125),
                (2, 0.01, 0.025, -1, 0.75, 0.125), (2, 0.01, 0.025, 65536, 0.75, 0.125), (2, 0.01, 0.025, 8, 0.0, 0.125), (2, 0.01, 0.025, 8, 1.01, 0.125),
                (2, 0.01, 0.025, 8, 0.75, 0.0), (2, 0.01, 0.025, 8, 0.75, 1.5), (2, 0.01, 0.025, 8, nan, 0.125), (2, 0.01, 0.025, 8, 0.75, nan)):
        with pytest.raises(rdsp.RdspError) as ex:
            e.set_noise_squelch(*bad)
        assert ex.value.code == -1, bad
    N = torch.full((3, 4), 7.0, dtype=torch.float32, device="cuda")
    nopen = torch.full((3, 4), 7, dtype=torch.uint8, device="cuda")
    for nblk, s_n, s_o in ((4, 4, 4), (-1, 4, 4), (3, 2, 4), (3, 4, 2)):
        assert e.lib.rdsp_engine_read_noise(e.h, nblk, N.data_ptr(), s_n, nopen.data_ptr(), s_o, None) == -1, (nblk, s_n, s_o)
        assert b"rdsp_engine_read_noise" in e.lib.rdsp_last_error()
    torch.cuda.synchronize()
    assert (N == 7.0).all() and (nopen == 7).all()
    assert e.lib.rdsp_engine_read_noise(e.h, 3, None, 0, nopen.data_ptr(), 4, None) == 0       # either pointer may be NULL
    assert e.lib.rdsp_engine_read_noise(e.h, 3, N.data_ptr(), 4, None, 0, None) == 0
    # nothing of all that changed the object: the stream goes on as the model's
    e.update(_cuda(x[:, 3 * 128:]))
    wN, wo = m.run(y[:, 3 * 128:])
    got = _records(e, 5)
    assert np.array_equal(bits(got[0]), bits(wN)) and np.array_equal(got[1], wo) and wo[0].all() and not wo[1].any()
    assert np.array_equal(_noise_words(e.save_state(0, 3), 3), m.words())
    e.close()
