"""The DCS code squelch of rdsp_engine_t on the GPU (include/rdsp.h "code squelch"; csrc/rdsp_engine_dcs.hip,
csrc/rdsp_engine_dcs_host.hip) against tests/engine_dcs_model.py on the demodulated rows of tests/engine_fm_model.py.  Every
comparison with the model is exact.  The three records, all 232 state words (through a blob), the combined gate, the active list
and the gated int16 audio for 1, 5, 97 and 300 receivers, K = 8 and 12, four call splits, with and without the meter, aligned and
unaligned output rows; a station at the defaults with the active list and both packs, and with its code switched off; an engine
that enabled the detector with every code 0 against one that never did; the detector beside the tone squelch and the tone search;
the state through blobs, regroupings, changed settings, mode changes and resets; the refusals.  tests/test_engine_dcs.py has what
needs no GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import engine_dcs_model as D
import engine_fm_model as FM
import engine_pack_model as P
import engine_tail_model as TM
import engine_tone_model as T
import engine_tone_search_model as TS
import engine_voice_model as V
from engine_meter_model import Meter, Squelch, gated
from engine_sources_model import table

F32 = np.float32
NFM = 7
CH_WORDS = 96 + 2 * 512 + 3 * 384 + 320      # a channel's words in a blob, in front of the optional parts
POOL = 48                                    # distinct stations; receivers beyond share them with settings of their own
pytestmark = pytest.mark.gpu


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _engine(n, max_blocks, meter=False, dcs=True, nfm=True, tone=False, search=False):
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
    if dcs:
        e.enable_dcs()
    if nfm:
        assert e.setDemodMode(NFM) == 0.0
    return e


def _tail(n):
    return TM.Tail(n).setAGCmode(0)


@functools.lru_cache(maxsize=None)
def _pool(nb=96):
    """POOL stations of nb blocks, computed once: (iq int16 [POOL, t, 2], the code each carries, whether inverted, whether too
    weak to slice, y, lvl float32 [POOL, t], tail int16 [POOL, t]).  Code, bit phase, amplitude (0.1 ... 0.3 of the deviation; every
    sixth 0.004: too weak under the voice) and carrier (500 ... 20000 counts: some open the carrier squelch, some do not) are
    drawn; station 1 is on the rails and station 2 all zeros"""
    r = np.random.default_rng(2300)
    code = r.choice(np.array(D.STANDARD), POOL)
    code[0] = 0o023
    inv = r.integers(0, 2, POOL).astype(bool)
    inv[0] = False
    weak = np.arange(POOL) % 6 == 5
    x = np.stack([D.station(700 + s, nb, D.codeword(int(code[s])) ^ (D.MASK if inv[s] else 0), 0.004 if weak[s] else r.uniform(0.1, 0.3),
                            r.uniform(0, 23), r.uniform(500, 20000)) for s in range(POOL)])
    x[1] = r.choice(np.array([32767, -32768], np.int16), (nb * 128, 2))
    x[2] = 0
    y, lvl = FM.Fm(POOL).run(x)
    return x, code, inv, weak, y, lvl, _tail(POOL).run(y)


@functools.lru_cache(maxsize=None)
def _drawn(n):
    """n receivers: (their stations' indices into the pool, their settings uint16 [n]).  A receiver's setting is drawn from: none,
    its station's code in its polarity, ANY, a wrong code, the right code in the wrong polarity; the first five are one of each on
    station 0 (023, normal)"""
    r = np.random.default_rng(2400 + n)
    st = np.arange(n) % POOL
    _, code, inv, _, _, _, _ = _pool()
    kind = r.integers(0, 5, n)
    if n >= 5:
        st[:5], kind[:5] = 0, (1, 2, 0, 3, 4)
    else:
        st[0], kind[0] = 0, 1
    right = code[st].astype(np.int64) | np.where(inv[st], D.INVERTED, 0)
    wrong = np.array([D.STANDARD[(D.STANDARD.index(int(c)) + 1 + int(k)) % 104] for c, k in zip(code[st], r.integers(0, 50, n))], np.int64)
    codes = np.choose(kind, [np.zeros(n, np.int64), right, np.full(n, D.ANY), wrong, right ^ D.INVERTED])
    return st, codes.astype(np.uint16)


def _dcs_words(blob, n):
    """the detector words of a blob of n channels: its last part"""
    return blob[-n * D.WORDS * 4:].view(np.uint32).reshape(n, D.WORDS)


SQUELCH = Squelch(F32(2e-3), F32(1e-3), 1)     # a carrier of 2000 counts reads 3.7e-3: some of the drawn stations open it, some do not


def _update(e, x, out=None):
    """one call; out: a (tensor, stride in pairs) pair for rows that are not 16-byte aligned -> the int16 rows [n, t, 2] on the host"""
    if out is None:
        return e.update(_cuda(x)).cpu().numpy()
    rows, stride = out
    d = _cuda(x)
    assert e.lib.rdsp_engine_update(e.h, d.data_ptr(), x.shape[1], x.shape[1] // 128, rows.data_ptr(), stride, None) == 0, e.lib.rdsp_last_error()
    return rows[:, :x.shape[1]].cpu().numpy()


def _records(e, k):
    dcs, hits, word = (v.cpu().numpy() for v in e.read_dcs(k))
    return dcs, hits, word.view(np.uint32)


def _same(got, want):
    return all(np.array_equal(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("meter", [False, True])
@pytest.mark.parametrize("n", [1, 5, 97, 300])
def test_gpu_dcs_rows_are_the_model(rdsp, n, meter):
    """1, 5, 97 and 300 receivers (a ragged last workgroup, more than one workgroup) with drawn settings -- none, standard codes,
    inverted codes, ANY, a wrong code, the wrong polarity -- on stations with drawn codes, bit phases and amplitudes, some too weak
    to slice; K = 8 (max_err 1, on 2, off 1) and K = 12 (max_err 2, on 4, off 2); 80 blocks, because 23 bits take 59 blocks before
    anything can match, as [80], [7, 64, 9], eighty calls of 1 and [40, 40] -- windows end in mid-call, at a call boundary and inside
    the eight-block trip -- each from a reset: rdsp_engine_read_dcs's three records, all 232 state words (through a blob) and, with
    the meter, rdsp_engine_read_meter's open records (the carrier gate of engine_meter_model on the model's level rows, and the dcs
    records), the active list and the int16 audio (engine_tail_model, gated) equal the models.  Without the meter nothing is gated:
    the audio is the tail's.  [40, 40] runs once more into output rows that are not 16-byte aligned.  At 97 and 300 receivers
    every combination of carrier gate and code decision occurs"""
    import torch
    nb = 80
    px, _, _, _, py, plvl, ptail = _pool()
    st, codes = _drawn(n)
    x, y, lvl, tail = px[st, :nb * 128], py[st, :nb * 128], plvl[st, :nb * 128], ptail[st, :nb * 128]
    e = _engine(n, nb, meter)
    e.set_dcs_codes(0, codes)
    if meter:
        e.set_squelch(float(SQUELCH.open_ms), float(SQUELCH.close_ms), SQUELCH.hang_blocks)
    stride = nb * 128 + 3
    buf = torch.zeros(n * stride * 2 + 8, dtype=torch.int16, device="cuda")
    odd = buf[2:2 + n * stride * 2].view(n, stride, 2)
    assert odd.data_ptr() % 16 == 4
    seen = set()
    for K, err, on, off in ((8, 1, 2, 1), (12, 2, 4, 2)):
        e.set_dcs_squelch(K, err, on, off)
        for pattern, out in (([80], None), ([7, 64, 9], None), ([1] * 80, None), ([40, 40], None), ([40, 40], (odd, stride))):
            e.reset()
            m, mm = D.Dcs(n, codes, K, err, on, off), Meter(n)
            a = 0
            for i, k in enumerate(pattern):
                s = slice(a * 128, (a + k) * 128)
                audio = _update(e, x[:, s], out)
                want_rec = m.run(y[:, s])
                got = _records(e, k)
                assert _same(got, want_rec), (K, pattern, a, [np.argwhere(g != w)[:3] for g, w in zip(got, want_rec)])
                if k > 1 or i % 8 == 7:
                    assert np.array_equal(_dcs_words(e.save_state(0, n), n), m.words()), (K, pattern, a)
                want = tail[:, s]
                if meter:
                    carrier = mm.run(lvl[:, s], SQUELCH)[2]
                    both = m.gate(carrier, want_rec[0])
                    assert np.array_equal(e.read_meter(k)[2].cpu().numpy(), both), (K, pattern, a)
                    assert np.array_equal(e.active()[0].cpu().numpy(), np.flatnonzero(both.any(1)))
                    assert np.array_equal(e.meter()[:, 3], mm.open.astype(F32))               # the carrier gate's state is the meter's own
                    want = gated(want, both)
                    seen |= {(int(c), int(t)) for c, t in zip(carrier[codes != 0].ravel(), want_rec[0][codes != 0].ravel())}
                assert np.array_equal(audio[..., 0], want) and np.array_equal(audio[..., 1], want), (K, pattern, a)
                a += k
            assert a == nb
            dcs, hits, word = want_rec
            w = m.words()
            assert dcs[0, -1] and word[0, -1] == D.canon(D.codeword(0o023))
            if n >= 5:
                assert dcs[1, -1] and D.code_of_word(int(word[1, -1])) == (0o023, False)       # ANY reads the station's code
                assert not w[2].any() and not dcs[2].any() and not dcs[3].any() and not dcs[4].any() and not hits[3:5].any()
                hyp = w[0, D.HDR:].reshape(D.HYP, D.HYP_WORDS)
                assert (hyp[:, D.NB] == 23).all() and hyp[:, D.RING:].all() and w[0, D.MS] == (nb * 4 * D.STEP) & 0xFFFFFFFF
    if meter and n >= 97:
        assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)}                                       # every combination of the two gates occurred
    e.close()


@functools.lru_cache(maxsize=None)
def _gate_case(stops):
    nb = 256
    x = np.broadcast_to(D.station(7, nb, D.codeword(0o023), 0.15, 9.3, until=128 * 128 if stops else None), (4, nb * 128, 2)).copy()
    y, lvl = FM.Fm(4).run(x)
    return x, y, lvl, _tail(4).run(y)


@pytest.mark.parametrize("stops", [False, True])
def test_gpu_dcs_gate(rdsp, stops):
    """four receivers on one synthetic station that carries code 023 at 0.15 of the deviation under voice-band noise, set to 023,
    to 025, to ANY and to no code, at the defaults (K = 64, max_err 1, on_hits 16, off_hits 12); 256 blocks in four calls.  The
    first and the third receiver open at the second window's end (block 127: the first window holds the 59 blocks 23 bits take),
    the third reads 023 through dcs_code_of_word, the second never opens, the fourth follows the carrier gate alone.  The int16
    audio is the model's gated audio; the open records, the active list, rdsp_engine_pack_active and rdsp_engine_pack_voice (R = 2)
    are their models' on the combined gate, while rdsp_engine_get_meter still reports the carrier gate.  stops: the code is
    switched off half-way through (block 128) -- the gate closes one window later, after block 191, while the carrier gate stays
    open"""
    from radiodsp_sdr_rx_amd.engine import dcs_code_of_word, ms_of_db
    nb, call = 256, 64
    x, y, lvl, tail = _gate_case(stops)
    s = Squelch(F32(ms_of_db(-30.0)), F32(ms_of_db(-36.0)), 2)                              # the carrier of 8000 counts is -9 dB
    codes = [0o023, 0o025, D.ANY, 0]
    e = _engine(4, call, meter=True)
    assert e.dcs_enabled
    e.set_squelch(float(s.open_ms), float(s.close_ms), s.hang_blocks)
    e.set_dcs_codes(0, codes)
    e.enable_voice(2)
    m, mm, voice = D.Dcs(4, codes), Meter(4), V.Voice(4, 2)
    gates, carriers, hits, words = [], [], [], []
    for a in range(0, nb, call):
        sl = slice(a * 128, (a + call) * 128)
        yd = e.update(_cuda(x[:, sl]))
        audio = yd.cpu().numpy()
        rec = m.run(y[:, sl])
        carrier = mm.run(lvl[:, sl], s)[2]
        both = m.gate(carrier, rec[0])
        assert _same(_records(e, call), rec)
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
        gates.append(both); carriers.append(carrier); hits.append(rec[1][:, -1]); words.append(rec[2][:, -1])
    gate, carrier = np.concatenate(gates, 1), np.concatenate(carriers, 1)
    print("hits at the ends of the four windows, per receiver:", np.stack(hits, 1).tolist())
    assert carrier[:, 2:].all() and np.array_equal(gate[3], carrier[3]) and not gate[1].any()
    last = 191 if stops else nb
    for c in (0, 2):
        assert not gate[c, :127].any() and gate[c, 127:last].all() and not gate[c, last:].any(), c
    assert dcs_code_of_word(int(words[1][2])) == (0o023, False) and words[1][0] == D.canon(D.codeword(0o023))
    e.close()


def test_gpu_dcs_off_changes_nothing(rdsp):
    """NFM, LSB and AM groups (5 + 3 + 4 receivers), meter and squelch on: an engine that enabled the detector with every code 0
    gives the audio, the meter records and the active list of one that never enabled it, and reads zero records; the blob of the
    engine that never enabled it has the size and the flags it always had (sources none, meter 2, FM 8) and is, byte for byte,
    the other's without its last part"""
    from test_engine_meter import _bursts
    n, nb, first = 12, 6, [0, 5, 8]
    x = _bursts(83, n, nb)
    x[:5] = FM.station(90, nb, 4000.0, 1000.0, 9000.0, 3.0)[None]
    x[1] = _bursts(84, 1, nb)[0]                                                              # an NFM receiver whose carrier is keyed
    engines = []
    for with_dcs in (True, False):
        e = _engine(n, 4, meter=True, dcs=with_dcs, nfm=False)
        e.set_squelch(2e-3, 1e-3, 1)
        e.set_groups(first)
        e.select_group(0); assert e.setDemodMode(NFM) == 0.0
        e.select_group(2); e.setDemodMode(4); e.setAudioFilter(0)
        e.select_group(-1)
        engines.append(e)
    a, b = engines
    assert a.dcs_enabled and not b.dcs_enabled
    gates = []
    for k0, k in ((0, 4), (4, 2)):
        d = _cuda(x[:, k0 * 128:(k0 + k) * 128])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        assert np.array_equal(ya, yb) and ya[:5].any() and ya[5:].any()
        for va, vb in zip(a.read_meter(k), b.read_meter(k)):
            assert np.array_equal(va.cpu().numpy().astype(F32).view(np.uint32), vb.cpu().numpy().astype(F32).view(np.uint32))
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        assert not any(v.any() for v in a.read_dcs(k))
        gates.append(b.read_meter(k)[2].cpu().numpy())
    gate = np.concatenate(gates, 1)
    assert np.array_equal(gate[1], [0, 0, 1, 1, 1, 1]) and gate[0].all()                      # the keyed NFM receiver: closed blocks, then open ones
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert len(blob_b) == 16 + n * (CH_WORDS + 3 + 50) * 4 == b.lib.rdsp_engine_state_bytes(b.h, n) and blob_b.view(np.uint32)[3] == 2 | 8
    assert len(blob_a) == len(blob_b) + n * D.WORDS * 4 == a.lib.rdsp_engine_state_bytes(a.h, n) and blob_a.view(np.uint32)[3] == 2 | 8 | 64
    assert np.array_equal(blob_a[16:len(blob_b)], blob_b[16:]) and not blob_a[len(blob_b):].any()
    with pytest.raises(rdsp.RdspError) as ex:
        b.read_dcs(0)
    assert ex.value.code == -4
    for e in engines:
        e.close()


@functools.lru_cache(maxsize=None)
def _both_case():
    """one station that carries a 254.1 Hz tone at 0.12 of the deviation AND code 023 at 0.3 under voice-band noise, five times"""
    nb, n = 128, 5
    t = np.arange(nb * 128)
    r = np.random.default_rng(31)
    mod = np.clip(0.12 * np.sin(2 * np.pi * 254.1 / 44100.0 * t + 0.7) + 0.3 * D.nrz(D.codeword(0o023), len(t), 4.4) + T.voice_noise(31, len(t)), -1.0, 1.0)
    z = 8000.0 * np.exp(1j * 2 * np.pi * 5000.0 / 44100.0 * np.cumsum(mod)) + 3.0 * (r.standard_normal(len(t)) + 1j * r.standard_normal(len(t)))
    x = np.broadcast_to(np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16), (n, nb * 128, 2)).copy()
    y, lvl = FM.Fm(n).run(x)
    return x, y, lvl, _tail(n).run(y)


def test_gpu_dcs_beside_tone_and_search(rdsp):
    """five receivers on a station that carries a tone and a code, tone squelch (K = 32), tone search (K = 32) and code squelch
    (K = 16, max_err 1, on 4, off 2) on: receiver 0 has the tone and the code and is gated by both -- it opens when the later of
    the two does --, receiver 1 the tone and a wrong code and never opens, receiver 2 the tone only, receiver 3 a wrong tone,
    receiver 4 nothing.  Against an engine without the code squelch: the tone and search records of every receiver, and the open
    records and audio of receivers 2 ... 4, are the same; receivers 0 and 1 have the other engine's open records ANDed with the
    model's dcs records and the audio gated by that"""
    nb, call, n = 128, 32, 5
    x, y, lvl, tail = _both_case()
    s = Squelch(F32(2e-3), F32(1e-3), 1)
    tones, codes = [254.1, 254.1, 254.1, 100.0, 0.0], [0o023, 0o025, 0, 0, 0]
    engines = []
    for with_dcs in (True, False):
        e = _engine(n, call, meter=True, dcs=with_dcs, tone=True, search=True)
        e.set_squelch(float(s.open_ms), float(s.close_ms), s.hang_blocks)
        e.set_tones(0, tones)
        e.set_tone_squelch(32, 0.06, 0.045)
        e.set_tone_search(32)
        if with_dcs:
            e.set_dcs_codes(0, codes)
            e.set_dcs_squelch(16, 1, 4, 2)
        engines.append(e)
    a, b = engines
    m = D.Dcs(n, codes, 16, 1, 4, 2)
    gates, others, decisions = [], [], []
    for k0 in range(0, nb, call):
        sl = slice(k0 * 128, (k0 + call) * 128)
        d = _cuda(x[:, sl])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        rec = m.run(y[:, sl])
        assert _same(_records(a, call), rec)
        for va, vb in zip(a.read_tone(call) + a.read_tone_search(call), b.read_tone(call) + b.read_tone_search(call)):
            assert np.array_equal(va.cpu().numpy().view(np.uint8), vb.cpu().numpy().view(np.uint8))
        oa, ob = a.read_meter(call)[2].cpu().numpy(), b.read_meter(call)[2].cpu().numpy()
        both = m.gate(ob, rec[0])
        assert np.array_equal(oa, both) and np.array_equal(oa[2:], ob[2:]) and np.array_equal(ya[2:], yb[2:])
        want = gated(yb[..., 0], both)
        assert np.array_equal(ya[..., 0], want) and np.array_equal(ya[..., 1], want)
        assert np.array_equal(a.active()[0].cpu().numpy(), np.flatnonzero(both.any(1)))
        gates.append(oa); others.append(ob); decisions.append(rec[0])
    gate, other = np.concatenate(gates, 1), np.concatenate(others, 1)
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert blob_a.view(np.uint32)[3] == 2 | 8 | 16 | 32 | 64 and np.array_equal(blob_a[16:len(blob_b)], blob_b[16:])
    assert np.array_equal(_dcs_words(blob_a, n), m.words())
    decided = np.concatenate(decisions, 1)
    first_tone, first_code = int(np.argmax(other[0])), int(np.argmax(decided[0]))
    assert other[0].any() and other[1].any() and gate[0].any() and not gate[1].any() and not other[3].any() and other[4].all()
    assert int(np.argmax(gate[0])) == max(first_tone, first_code) >= 31 and min(first_tone, first_code) >= 31 and first_tone != first_code
    assert not decided[1:].any()
    for e in engines:
        e.close()


def test_gpu_dcs_state(rdsp):
    """the detector's words are signal state.  A coded receiver whose rings are all nonzero moves by blob to an engine with
    another channel count, another index and another max_blocks, set to the same code and K, and continues bit for bit; moved onto
    a channel with another code it restarts from zeros, as the model does.  An engine without the detector refuses the part with
    nothing changed; a blob without the part zeroes the words.  A regrouping into a group with another K, a changed K, max_err
    or code, leaving NFM and coming back and rdsp_engine_reset each restart the detector as the model says; a regrouping with the
    same K keeps it"""
    nb, cut, K = 96, 74, 8
    px, _, _, _, py, _, _ = _pool()
    codes = np.array([0o023, D.ANY, 0o023, 0, 0o025], np.uint16)                              # five receivers on station 0, which carries 023
    x, y = px[np.zeros(5, int)], py[np.zeros(5, int)]
    a = _engine(5, 80)
    a.enable_dcs()                                                                            # again: a no-op
    a.set_dcs_codes(0, codes)
    a.set_dcs_squelch(K, 1, 2, 1)
    m = D.Dcs(5, codes, K, 1, 2, 1)
    a.update(_cuda(x[:, :cut * 128]))
    rec = m.run(y[:, :cut * 128])
    assert _same(_records(a, cut), rec)
    blob = a.save_state(0, 1)
    w0 = m.words()[0]
    assert w0[D.HDR:].reshape(8, -1)[:, D.RING:].all() and w0[[D.KEY, D.CNT, D.DCS, D.H_, D.WORD, D.MS]].all()
    assert np.array_equal(_dcs_words(blob, 1)[0], w0) and blob.view(np.uint32)[3] == 8 | 64
    plain = _engine(3, 8, dcs=False)
    assert len(blob) == a.lib.rdsp_engine_state_bytes(a.h, 1) == plain.lib.rdsp_engine_state_bytes(plain.h, 1) + D.WORDS * 4
    before = plain.save_state(0, 3)
    with pytest.raises(rdsp.RdspError) as ex:                                                 # an engine without the detector refuses the part
        plain.load_state(0, blob)
    assert ex.value.code == -4 and np.array_equal(plain.save_state(0, 3), before)
    # the receiver continues in another engine: 7 channels, index 4, 32 blocks a call, a past of its own; index 5 has another code
    b = _engine(7, 32)
    b.set_dcs_squelch(K, 1, 2, 1)
    b.set_dcs_codes(4, [0o023, 0o047])
    b.update(_cuda(np.broadcast_to(px[3:4, :128], (7, 128, 2)).copy()))
    b.load_state(4, blob)
    b.load_state(5, blob)
    assert np.array_equal(_dcs_words(b.save_state(4, 2), 2), np.stack([w0, w0]))
    k = nb - cut
    rest = np.zeros((7, k * 128, 2), np.int16)
    rest[4] = rest[5] = x[0, cut * 128:(cut + k) * 128]
    b.update(_cuda(rest))
    got = _records(b, k)
    m1 = D.Dcs(5, codes, K, 1, 2, 1)
    m1.w[:] = m.words()
    cont = m1.run(y[:, cut * 128:(cut + k) * 128])
    assert all(np.array_equal(g[4], c[0]) for g, c in zip(got, cont)) and cont[0][0].all()    # the same code and K: bit for bit, and still open
    other = D.Dcs(1, [0o047], K, 1, 2, 1)
    other.w[0] = w0                                                                           # another code: the key does not match, zeros
    orec = other.run(y[:1, cut * 128:(cut + k) * 128])
    fresh = D.Dcs(1, [0o047], K, 1, 2, 1).run(y[:1, cut * 128:(cut + k) * 128])
    assert all(np.array_equal(g[5], o[0]) for g, o in zip(got, orec)) and _same(orec, fresh) and not orec[0].any()
    assert np.array_equal(_dcs_words(b.save_state(4, 2), 2), np.stack([m1.words()[0], other.words()[0]]))
    b.load_state(4, plain.save_state(0, 1))                                                   # a blob without the part zeroes the words
    assert not _dcs_words(b.save_state(4, 1), 1).any()
    # a's own stream goes on.  A regrouping with the same K keeps the detector
    a.set_groups([0, 2])
    at = cut

    def step(k):
        nonlocal at
        a.update(_cuda(x[:, at * 128:(at + k) * 128]))
        want = m.run(y[:, at * 128:(at + k) * 128])
        assert _same(_records(a, k), want), at
        assert np.array_equal(_dcs_words(a.save_state(0, 5), 5), m.words()), at
        at += k
        return m.words()
    w = step(3)
    assert w[0, D.MS] == ((cut + 3) * 4 * D.STEP) & 0xFFFFFFFF and w[4, D.CNT] == (cut + 3) % K
    # group 1 (channels 2, 3, 4) gets K = 12: a changed K restarts its receivers
    a.select_group(1); a.set_dcs_squelch(12, 1, 2, 1); a.select_group(-1)
    m.set_squelch(12, 1, 2, 1, slice(2, None))
    w = step(4)
    assert w[4, D.CNT] == 4 and w[4, D.K_] == 12 and w[4, D.MS] == (16 * D.STEP) & 0xFFFFFFFF and w[0, D.CNT] == (cut + 7) % K
    # a regrouping into a group with another K: channel 2 joins group 0 (K = 8) and restarts, channel 4 goes on (3 has no code)
    a.set_groups([0, 3])
    m.set_squelch(K, 1, 2, 1, slice(2, 3))
    w = step(2)
    assert w[2, D.CNT] == 2 and w[2, D.K_] == K and w[4, D.CNT] == 6 and not w[3].any() and w[0, D.CNT] == (cut + 9) % K
    # a changed max_err restarts group 0's receivers only
    a.select_group(0); a.set_dcs_squelch(K, 0, 2, 1); a.select_group(-1)
    m.set_squelch(K, 0, 2, 1, slice(0, 3))
    w = step(2)
    assert w[0, D.CNT] == 2 and w[0, D.MS] == (8 * D.STEP) & 0xFFFFFFFF and w[4, D.CNT] == 8
    # a changed code in mid-stream restarts that receiver only
    a.set_dcs_codes(4, [0o023])
    m.set_codes([0o023], 4)
    w = step(2)
    assert w[4, D.CNT] == 2 and w[4, D.KEY] == m.keys()[4] and w[0, D.CNT] == 4 and at == cut + 13
    # leaving NFM and coming back: the words are not maintained outside the mode and start from zeros at the next NFM update
    a.set_groups([0])
    a.set_dcs_squelch(K, 1, 2, 1)
    codes2 = codes.copy()
    codes2[4] = 0o023
    m3 = D.Dcs(5, codes2, K, 1, 2, 1)
    a.setDemodMode(4)
    a.update(_cuda(x[:, :128]))
    assert np.array_equal(_dcs_words(a.save_state(0, 5), 5), w) and not any(v.any() for v in a.read_dcs(1))   # untouched, and no records
    a.setDemodMode(NFM)
    a.update(_cuda(x[:, :72 * 128]))
    ya = FM.Fm(5).run(x[:, :72 * 128])[0]
    r3 = m3.run(ya)
    assert _same(_records(a, 72), r3) and np.array_equal(_dcs_words(a.save_state(0, 5), 5), m3.words()) and r3[0][0, -1]
    # rdsp_engine_reset zeroes the words and keeps the codes and the settings
    a.reset()
    assert not _dcs_words(a.save_state(0, 5), 5).any()
    a.update(_cuda(x[:, :72 * 128]))
    m3.reset()
    assert _same(_records(a, 72), m3.run(ya))
    for e in (a, b, plain):
        e.close()


def test_gpu_dcs_refusals(rdsp):
    """every refusal that needs an engine, each with the object unchanged: rdsp_engine_enable_dcs before rdsp_engine_enable_fm;
    rdsp_engine_read_dcs before rdsp_engine_enable_dcs; K outside 8 ... 512; max_err outside 0 ... 3; off_hits below 1 or above
    on_hits, on_hits above the bits of a window; codes above 511, an inverted 0, a range outside the object, a NULL array;
    n_blocks above the last call's; a short stride"""
    import torch
    from test_engine_meter import _engine as plain_engine
    p = plain_engine(2, 4, meter=False)
    assert p.lib.rdsp_engine_enable_dcs(p.h) == -4 and b"rdsp_engine_enable_fm" in p.lib.rdsp_last_error() and not p.dcs_enabled
    p.set_dcs_codes(0, [0o023, 0])                                                            # a setting: it may precede the detector
    p.enable_fm()
    with pytest.raises(rdsp.RdspError) as ex:
        p.read_dcs(0)
    assert ex.value.code == -4
    p.close()
    px, _, _, _, py, _, _ = _pool()
    st, codes = _drawn(5)
    x, y = px[st], py[st]
    e = _engine(5, 80)
    e.set_dcs_codes(0, codes)
    e.set_dcs_squelch(8, 1, 2, 1)
    m = D.Dcs(5, codes, 8, 1, 2, 1)
    e.update(_cuda(x[:, :3 * 128]))
    m.run(y[:, :3 * 128])
    for bad in ((7, 1, 2, 1), (513, 1, 2, 1), (-1, 1, 2, 1), (8, -1, 2, 1), (8, 4, 2, 1), (8, 1, 2, 0), (8, 1, 1, 2), (8, 1, 4, 1), (64, 1, 25, 6), (512, 1, 200, 6)):
        with pytest.raises(rdsp.RdspError) as ex:
            e.set_dcs_squelch(*bad)
        assert ex.value.code == -1, bad
    for first, bad in ((0, [0o023, 512]), (0, [0x8000]), (2, [0x7FFF]), (0, [19, 19, 0xFFFE]), (4, [19, 19]), (-1, [19]), (5, [19])):
        with pytest.raises(rdsp.RdspError) as ex:
            e.set_dcs_codes(first, bad)
        assert ex.value.code == -1, (first, bad)
    assert e.lib.rdsp_engine_set_dcs_codes(e.h, 0, 1, None) == -1 and e.lib.rdsp_engine_set_dcs_codes(e.h, 0, 0, (C.c_uint16 * 1)(19)) == -1
    dcs = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    hits = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    word = torch.full((5, 4), 7, dtype=torch.int32, device="cuda")
    for nblk, s_d, s_h, s_w in ((4, 4, 4, 4), (-1, 4, 4, 4), (3, 2, 4, 4), (3, 4, 2, 4), (3, 4, 4, 2)):
        assert e.lib.rdsp_engine_read_dcs(e.h, nblk, dcs.data_ptr(), s_d, hits.data_ptr(), s_h, word.data_ptr(), s_w, None) == -1, (nblk, s_d, s_h, s_w)
        assert b"rdsp_engine_read_dcs" in e.lib.rdsp_last_error()
    torch.cuda.synchronize()
    assert (dcs == 7).all() and (hits == 7).all() and (word == 7).all()
    assert e.lib.rdsp_engine_read_dcs(e.h, 3, None, 0, None, 0, word.data_ptr(), 4, None) == 0  # any pointer may be NULL
    assert e.lib.rdsp_engine_read_dcs(e.h, 3, dcs.data_ptr(), 4, None, 0, None, 0, None) == 0
    # nothing of all that changed the object: the stream goes on as the model's
    e.update(_cuda(x[:, 3 * 128:80 * 128]))
    want = m.run(y[:, 3 * 128:80 * 128])
    assert _same(_records(e, 77), want) and want[0][0, -1]
    assert np.array_equal(_dcs_words(e.save_state(0, 5), 5), m.words())
    e.close()
