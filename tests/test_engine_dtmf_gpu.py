"""The DTMF decoder of rdsp_engine_t on the GPU (include/rdsp.h "DTMF decoder"; csrc/rdsp_engine_dtmf.hip,
csrc/rdsp_engine_dtmf_host.hip) against tests/engine_dtmf_model.py on the demodulated rows of tests/engine_fm_model.py.  Every
comparison with the model is exact: floats as uint32, audio as int16.  The four records, n_digits with the ring and all 168 state
words (through a blob) for 1, 5, 97 and 300 receivers, K = 4 and 5, on_frames / off_frames of 1 and 2 and four call splits; a
station's keys read back once each with the model's stamps; a long key; a key with drop-outs; a full ring; the decoder beside the
meter, the tone squelch, the code squelch, the noise squelch and the voice stage, none of which it changes; an engine that enabled
the decoder with K = 0 everywhere against one that never did; the state through blobs, regroupings, mode changes, resets, a
changed K and changed thresholds; the refusals.  tests/test_engine_dtmf.py has what needs no GPU."""
import functools

import numpy as np
import pytest

import engine_dtmf_model as D
import engine_fm_model as FM
import engine_tone_model as T
from engine_sources_model import table

F32 = np.float32
NFM = 7
CH_WORDS = 96 + 2 * 512 + 3 * 384 + 320      # a channel's words in a blob, in front of the optional parts
LOOSE = dict(min_amp=0.05, ratio=2.0, twist=8.0, share=0.3)
SETTINGS = (dict(K=4, on_frames=1, off_frames=1, **LOOSE), dict(K=4, on_frames=2, off_frames=2), dict(K=5, on_frames=1, off_frames=2),
            dict(K=5, on_frames=2, off_frames=1, **LOOSE))
pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _engine(n, max_blocks, meter=False, dtmf=True, nfm=True, others=False):
    """sketch set-up, NFM at its defaults (W = 2, 5000 Hz, 750 us), the tail's AGC and ALS off, audio filter 2700"""
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
    if dtmf:
        e.enable_dtmf()
    if nfm:
        assert e.setDemodMode(NFM) == 0.0
    return e


def _station(seed, mod, carrier=8000.0, noise=3.0):
    """int16 [t, 2]: a carrier frequency-modulated (5000 Hz peak deviation) by mod (+-1.0: the deviation), `noise` counts of noise"""
    r = np.random.default_rng(seed)
    n = len(mod)
    z = carrier * np.exp(1j * (2 * np.pi * 5000.0 / 44100.0 * np.cumsum(np.clip(mod, -1.0, 1.0)) + r.uniform(0, 6))) + \
        noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16)


@functools.lru_cache(maxsize=None)
def _drawn(n, nb=17):
    """n receivers, nb blocks: (iq int16 [n, t, 2], y float32 [n, t]).  Every receiver's station sends drawn keys, each for 5 to 12
    blocks with pauses of 2 to 4 blocks, at drawn tone amplitudes of 0.25 to 0.5 of the deviation (the de-emphasis leaves 0.03 to
    0.15 of them), every fourth one nothing; with three or more, channel 1 is on the rails and channel 2 all zeros"""
    r = np.random.default_rng(800 + n)
    x = []
    for c in range(n):
        keys = "".join(r.choice(list(D.KEYS), 4))
        mod = D.keyed(keys, int(r.integers(5, 13)) * 128, int(r.integers(2, 5)) * 128, r.uniform(0.25, 0.5), r.uniform(0.25, 0.5),
                      lead=int(r.integers(0, 256)), phase=r.uniform(0, 6), total=nb * 128)[:nb * 128]
        x.append(_station(900 + c, mod * (c % 4 != 3), r.uniform(500, 20000)))
    x = np.stack(x)
    if n >= 3:
        x[1] = r.choice(np.array([32767, -32768], np.int16), (nb * 128, 2))
        x[2] = 0
    return x, FM.Fm(n).run(x)[0]


def _dtmf_words(blob, n):
    """the DTMF words of a blob of n channels: its last part"""
    return blob[-n * D.WORDS * 4:].view(np.uint32).reshape(n, D.WORDS)


def _update(e, x):
    return e.update(_cuda(x)).cpu().numpy()


def _records(e, k):
    return tuple(v.cpu().numpy() for v in e.read_dtmf(k))


def _digits(e):
    return tuple(v.cpu().numpy().view(np.uint32) for v in e.read_dtmf_digits())


def _same(got, want, where):
    """the four records of a call against the model's"""
    for k in (0, 1):
        assert np.array_equal(got[k], want[k]), (where, k, np.argwhere(got[k] != want[k])[:3])
    for k in (2, 3):
        assert np.array_equal(bits(got[k]), bits(want[k])), (where, k, np.argwhere(bits(got[k]) != bits(want[k]))[:3])


def _same_digits(e, m, where):
    (gc, gr), (wc, wr) = _digits(e), m.digits()
    assert np.array_equal(gc, wc) and np.array_equal(gr, wr), where


@pytest.mark.parametrize("n", [1, 5, 97, 300])
def test_gpu_dtmf_rows_are_the_model(rdsp, n):
    """1, 5, 97 and 300 receivers (a ragged last workgroup, more than one workgroup; channel 1 on the rails, channel 2 all zeros),
    K = 4 and 5 with on_frames / off_frames of 1 and 2 and two sets of thresholds, 17 blocks as [17], [7, 8, 2], seventeen calls of
    1 and [9, 8] -- frames end in mid-call, at a call boundary and inside the eight-block trip -- each from a reset: after every
    call rdsp_engine_read_dtmf's four records, rdsp_engine_read_dtmf_digits' counts and rings and all 168 state words (through a
    blob) equal the model's, and the int16 audio is that of an engine that never enabled the decoder"""
    nb = 17
    x, y = _drawn(n)
    tab = table(rdsp)
    plain = _engine(n, nb, dtmf=False)
    audio_ref = _update(plain, x)
    plain.close()
    e = _engine(n, nb)
    emitted = 0
    for setting in SETTINGS:
        K = setting["K"]
        e.set_dtmf(**setting)
        for pattern in ([17], [7, 8, 2], [1] * 17, [9, 8]):
            e.reset()
            m = D.Dtmf(n, tab, **setting)
            a = 0
            for k in pattern:
                s = slice(a * 128, (a + k) * 128)
                audio = _update(e, x[:, s])
                want = m.run(y[:, s])
                _same(_records(e, k), want, (setting, pattern, a))
                _same_digits(e, m, (setting, pattern, a))
                assert np.array_equal(_dtmf_words(e.save_state(0, n), n), m.words()), (setting, pattern, a)
                assert np.array_equal(audio, audio_ref[:, s]), (setting, pattern, a)
                a += k
            w = m.words()
            assert (w[:, D.CNT] == 17 % K).all() and (w[:, D.TBLOCKS] == 17).all()
            if n >= 3:
                assert w[1, D.PL] and not w[2, D.PL] and not w[2, D.NDIGITS] and (want[0][2] == 255).all()   # the rails read something, silence nothing
        emitted += int(m.words()[:, D.NDIGITS].sum())
    assert emitted > 0 or n == 1                                                               # keys were read
    e.close()


_LONG = {}


def _long_case(rdsp):
    """four receivers in four groups through the FM model and the engine, 224 blocks in calls of 32, computed once: a station that
    sends "159D*0#A" at 40 ms on / 40 ms off, each tone at 0.2 of the deviation, under voice-band noise of rms 0.03 (the
    defaults); key 7 held for 25 frames and a little (the defaults); key 3 held for 200 blocks with four drop-outs of 8 blocks
    (off_frames 4); twenty keys of 8 blocks (which always hold a whole frame) with pauses of 3 (on_frames 1, off_frames 1).
    -> the engine's and the model's records of every call, the model, the engine's final digits and words"""
    if _LONG:
        return _LONG
    nb, call = 224, 32
    t = nb * 128
    sent = "159D*0#A"
    station = D.keyed(sent, 1764, 1764, 0.2, 0.2, lead=100, total=t) + T.voice_noise(77, t, 0.03)
    held = D.keyed("7", 101 * 128, 0, 0.25, 0.25, lead=300, total=t)
    dropped = D.keyed("3", 200 * 128, 0, 0.25, 0.25, lead=0, total=t)
    for g in range(4):
        dropped[(30 + 40 * g) * 128:(38 + 40 * g) * 128] = 0.0
    many = "0123456789ABCD*#1470"
    ring = D.keyed(many, 8 * 128, 3 * 128, 0.3, 0.3, lead=50, total=t)
    x = np.stack([_station(60 + k, mod) for k, mod in enumerate((station, held, dropped, ring))])
    y = FM.Fm(4).run(x)[0]
    settings = (dict(K=4), dict(K=4), dict(K=4, off_frames=4), dict(K=4, on_frames=1, off_frames=1))
    e = _engine(4, call)
    e.set_groups([0, 1, 2, 3])
    m = D.Dtmf(4, table(rdsp))
    for g, s in enumerate(settings):
        e.select_group(g)
        e.set_dtmf(**s)
        m.set(channels=slice(g, g + 1), **s)
    e.select_group(-1)
    got, want = [], []
    for a in range(0, nb, call):
        sl = slice(a * 128, (a + call) * 128)
        e.update(_cuda(x[:, sl]))
        got.append(_records(e, call))
        want.append(m.run(y[:, sl]))
    _LONG.update(sent=sent, many=many, model=m, got=[np.concatenate([g[k] for g in got], 1) for k in range(4)],
                 want=[np.concatenate([w[k] for w in want], 1) for k in range(4)], digits=_digits(e), words=_dtmf_words(e.save_state(0, 4), 4))
    e.close()
    return _LONG


def test_gpu_dtmf_reads_a_stations_keys(rdsp):
    """a station through the FM model sends "159D*0#A" at 40 ms on / 40 ms off under voice-band noise; K = 4 and the defaults: the
    engine's records, counts, rings and words equal the model's, and on them the eight keys are read back exactly once each, in
    order, with the model's block stamps, each stamped inside its key's 40 ms plus one frame"""
    c = _long_case(rdsp)
    _same(c["got"], c["want"], "station")
    m = c["model"]
    assert np.array_equal(c["digits"][0], m.digits()[0]) and np.array_equal(c["digits"][1], m.digits()[1]) and np.array_equal(c["words"], m.words())
    count, ring = c["digits"]
    keys = [(D.KEYS[int(ring[0, k]) & 0xFF], int(ring[0, k]) >> 8) for k in range(int(count[0]))]
    print("read back:", keys)
    assert "".join(k for k, _ in keys) == c["sent"] and keys == m.keys(0)
    new = c["got"][1][0]
    assert [D.KEYS[s] for s in new[new != 255]] == list(c["sent"]) and [int(b) + 1 for b in np.flatnonzero(new != 255)] == [t for _, t in keys]
    for k, (_, stamp) in enumerate(keys):
        assert 100 + k * 3528 < stamp * 128 <= 100 + k * 3528 + 1764 + 512 + 64, (k, stamp)


def test_gpu_dtmf_long_key_emits_once(rdsp):
    """key 7 held for 25 frames is emitted once and held until it ends; key 3 with four drop-outs of two frames each under
    off_frames = 4 is emitted once too (misses do not add up across matches) and held through the drop-outs"""
    c = _long_case(rdsp)
    count, ring = c["digits"]
    key, new = c["got"][0], c["got"][1]
    assert count[1] == 1 and D.KEYS[int(ring[1, 0]) & 0xFF] == "7" and (new[1] != 255).sum() == 1
    assert (key[1] == D.symbol_of("7")).sum() >= 24 * 4 and key[1, -1] == 255
    assert count[2] == 1 and D.KEYS[int(ring[2, 0]) & 0xFF] == "3" and (new[2] != 255).sum() == 1
    first = int(np.argmax(key[2] != 255))
    assert (key[2, first:200] == D.symbol_of("3")).all() and key[2, -1] == 255 and c["words"][2, D.MISS] >= 4
    assert c["want"][2][2, 35] < c["want"][2][2, 23] * 0.01                   # a frame inside a drop-out read next to nothing


def test_gpu_dtmf_full_ring(rdsp):
    """twenty keys wrap the ring of 16: n_digits is 20, digit k lies in ring[k mod 16], so the ring holds digits 16 ... 19 in front of
    digits 4 ... 15, with ascending block stamps in that order"""
    c = _long_case(rdsp)
    count, ring = c["digits"]
    assert count[3] == 20
    order = [16, 17, 18, 19] + list(range(4, 16))
    assert [D.KEYS[int(w) & 0xFF] for w in ring[3]] == [c["many"][k] for k in order]
    stamps = np.array([int(w) >> 8 for w in ring[3]])
    assert (np.diff(stamps[np.argsort(order)]) > 0).all() and c["model"].keys(3) == [(c["many"][k], int(stamps[order.index(k)])) for k in range(4, 20)]


def test_gpu_dtmf_beside_the_other_detectors(rdsp):
    """meter with its squelch, tone squelch, code squelch, noise squelch (mode 2), voice stage (R = 2) and the decoder together
    against the same engine without the decoder, 97 receivers, 17 blocks as [9, 8], K = 4: the int16 audio, rdsp_engine_read_meter's
    records (the combined gate among them), the active list, the tone, code and noise records, the voice rows and every blob part
    with a flag below 256 are the same bytes, the gate is neither shut nor open everywhere, and the decoder's records, digits and
    words equal the model's"""
    n, nb = 97, 17
    x, y = _drawn(n)
    r = np.random.default_rng(5)
    tones = np.where(np.arange(n) % 3 == 0, F32(100.0), F32(0.0)).astype(F32)
    engines = []
    for with_dtmf in (True, False):
        e = _engine(n, nb, meter=True, dtmf=with_dtmf, others=True)
        e.set_squelch(2e-3, 1e-3, 1)
        e.set_tones(0, tones)
        e.set_tone_squelch(4, 0.06, 0.045)
        e.set_dcs_codes(0, [0o023 if c % 5 == 0 else 0 for c in range(n)])
        e.set_noise_squelch()
        e.enable_voice(2)
        engines.append(e)
    a, b = engines
    setting = dict(K=4, on_frames=1, off_frames=1, **LOOSE)
    a.set_dtmf(**setting)
    m = D.Dtmf(n, table(rdsp), **setting)
    at, seen = 0, set()
    same = lambda va, vb: np.array_equal(va.cpu().numpy().view(np.uint8), vb.cpu().numpy().view(np.uint8))
    for k in (9, 8):
        s = slice(at * 128, (at + k) * 128)
        d = _cuda(x[:, s])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        assert np.array_equal(ya, yb)
        for read in ("read_meter", "read_tone", "read_dcs", "read_noise"):
            for va, vb in zip(getattr(a, read)(k), getattr(b, read)(k)):
                assert same(va, vb), read
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        assert same(a.read_voice(k), b.read_voice(k))
        _same(_records(a, k), m.run(y[:, s]), at)
        _same_digits(a, m, at)
        seen |= set(a.read_meter(k)[2].cpu().numpy().ravel().tolist())
        at += k
    assert seen == {0, 1} and m.words()[:, D.NDIGITS].any()
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert blob_b.view(np.uint32)[3] == 2 | 4 | 8 | 16 | 64 | 128 and blob_a.view(np.uint32)[3] == 2 | 4 | 8 | 16 | 64 | 128 | 256
    assert len(blob_a) == len(blob_b) + n * D.WORDS * 4 and np.array_equal(blob_a[16:len(blob_b)], blob_b[16:])
    assert np.array_equal(_dtmf_words(blob_a, n), m.words())
    for e in engines:
        e.close()


def test_gpu_dtmf_off_changes_nothing(rdsp):
    """NFM, LSB and AM groups (5 + 3 + 4 receivers), meter and squelch on: an engine that enabled the decoder with K = 0 everywhere
    gives the audio, the meter records and the active list of one that never enabled it, and reads 255 / 255 / 0 / 0 and no
    digits; the blob of the engine that never enabled it has the size and the flags it always had (meter 2, FM 8) and is, byte for
    byte, the other's without its header flag 256 and its ninth part, which is zeros"""
    from test_engine_meter import _bursts
    n, nb, first = 12, 6, [0, 5, 8]
    x = _bursts(83, n, nb)
    x[:5] = FM.station(90, nb, 4000.0, 1000.0, 9000.0, 3.0)[None]
    engines = []
    for with_dtmf in (True, False):
        e = _engine(n, 4, meter=True, dtmf=with_dtmf, nfm=False)
        e.set_squelch(2e-3, 1e-3, 1)
        e.set_groups(first)
        e.select_group(0); assert e.setDemodMode(NFM) == 0.0
        e.select_group(2); e.setDemodMode(4); e.setAudioFilter(0)
        e.select_group(-1)
        engines.append(e)
    a, b = engines
    assert a.dtmf_enabled and not b.dtmf_enabled
    for k0, k in ((0, 4), (4, 2)):
        d = _cuda(x[:, k0 * 128:(k0 + k) * 128])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        assert np.array_equal(ya, yb) and ya[:5].any() and ya[5:].any()
        for va, vb in zip(a.read_meter(k), b.read_meter(k)):
            assert np.array_equal(bits(va.cpu().numpy().astype(F32)), bits(vb.cpu().numpy().astype(F32)))
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        key, new, lo, hi = _records(a, k)
        assert (key == 255).all() and (new == 255).all() and not lo.any() and not hi.any()
        count, ring = _digits(a)
        assert not count.any() and not ring.any()
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert len(blob_b) == 16 + n * (CH_WORDS + 3 + 50) * 4 == b.lib.rdsp_engine_state_bytes(b.h, n) and blob_b.view(np.uint32)[3] == 2 | 8
    assert len(blob_a) == len(blob_b) + n * D.WORDS * 4 == a.lib.rdsp_engine_state_bytes(a.h, n) and blob_a.view(np.uint32)[3] == 2 | 8 | 256
    assert np.array_equal(blob_a[16:len(blob_b)], blob_b[16:]) and not blob_a[len(blob_b):].any()
    assert np.array_equal(blob_a[:12], blob_b[:12])
    with pytest.raises(rdsp.RdspError) as ex:
        b.read_dtmf(0)
    assert ex.value.code == -4
    for e in engines:
        e.close()


def test_gpu_dtmf_state(rdsp):
    """the decoder's words are signal state.  A receiver in mid-frame with nonzero chains moves by blob to an engine with another
    channel count, another index and another max_blocks and the same K, and continues bit for bit.  An engine without the decoder
    refuses the part with nothing changed; a blob without the part zeroes the words.  A regrouping with the same K keeps the
    detector; a changed K and a regrouping into a group with another K restart it as the model says; changed thresholds and
    on_frames / off_frames do not; outside NFM the words are left alone and coming back restarts them; K = 0 zeroes them;
    rdsp_engine_reset zeroes them and keeps the settings"""
    nb, cut, K = 17, 6, 4
    S1 = dict(K=K, on_frames=1, off_frames=1, **LOOSE)
    x, y = _drawn(5)
    tab = table(rdsp)
    a = _engine(5, 8)
    a.enable_dtmf()                                                                           # again: a no-op
    a.set_dtmf(**S1)
    m = D.Dtmf(5, tab, **S1)
    a.update(_cuda(x[:, :cut * 128]))
    _same(_records(a, cut), m.run(y[:, :cut * 128]), "cut")
    blob = a.save_state(0, 1)
    w0 = m.words()[0]
    assert w0[D.CNT] == cut % K and w0[D.TBLOCKS] == cut and w0[D.RE:D.RE + 64].all() and w0[D.IM:D.IM + 64].all() and w0[D.E:D.E + 8].all() and w0[D.PL]
    assert np.array_equal(_dtmf_words(blob, 1)[0], w0) and blob.view(np.uint32)[3] == 8 | 256
    plain = _engine(3, 8, dtmf=False)
    assert len(blob) == a.lib.rdsp_engine_state_bytes(a.h, 1) == plain.lib.rdsp_engine_state_bytes(plain.h, 1) + D.WORDS * 4
    before = plain.save_state(0, 3)
    with pytest.raises(rdsp.RdspError) as ex:                                                 # an engine without the decoder refuses the part
        plain.load_state(0, blob)
    assert ex.value.code == -4 and np.array_equal(plain.save_state(0, 3), before)
    # the receiver continues in another engine: 7 channels, index 4, 16 blocks a call, a past of its own
    b = _engine(7, 16)
    b.set_dtmf(**S1)
    b.update(_cuda(np.broadcast_to(x[1:2, :128], (7, 128, 2)).copy()))
    b.load_state(4, blob)
    assert np.array_equal(_dtmf_words(b.save_state(4, 1), 1)[0], w0)
    rest = np.zeros((7, (nb - cut) * 128, 2), np.int16)
    rest[4] = x[0, cut * 128:]
    b.update(_cuda(rest))
    want = m.run(y[:, cut * 128:])
    got = _records(b, nb - cut)
    _same(tuple(v[4:5] for v in got), tuple(v[:1] for v in want), "moved")
    assert np.array_equal(_dtmf_words(b.save_state(4, 1), 1)[0], m.words()[0])
    b.load_state(4, plain.save_state(0, 1))                                                   # a blob without the part zeroes the words
    assert not _dtmf_words(b.save_state(4, 1), 1).any()
    # a's own stream goes on.  A regrouping with the same K keeps the detector
    a.set_groups([0, 2])
    m2 = D.Dtmf(5, tab, **S1)
    m2.run(y[:, :cut * 128])
    at = cut

    def step(k):
        nonlocal at
        a.update(_cuda(x[:, at * 128:(at + k) * 128]))
        _same(_records(a, k), m2.run(y[:, at * 128:(at + k) * 128]), at)
        assert np.array_equal(_dtmf_words(a.save_state(0, 5), 5), m2.words()), at
        _same_digits(a, m2, at)
        at += k
        return m2.words()
    w = step(3)
    assert w[3, D.CNT] == (cut + 3) % K and (w[:, D.TBLOCKS] == cut + 3).all()
    # group 1 (channels 2, 3, 4) gets K = 8: a changed K restarts its receivers
    S8 = dict(S1, K=8)
    a.select_group(1); a.set_dtmf(**S8); a.select_group(-1)
    m2.set(channels=slice(2, None), **S8)
    w = step(3)
    assert w[3, D.CNT] == 3 and w[3, D.K_] == 8 and w[3, D.TBLOCKS] == 3 and w[0, D.CNT] == (cut + 6) % K and w[0, D.TBLOCKS] == cut + 6
    # a regrouping into a group with another K: channel 2 joins group 0 (K = 4) and restarts, channels 3 and 4 go on
    a.set_groups([0, 3])
    m2.set(channels=slice(2, 3), **S1)
    w = step(2)
    assert w[2, D.TBLOCKS] == 2 and w[2, D.K_] == K and w[4, D.CNT] == 5 and w[4, D.TBLOCKS] == 5 and w[0, D.TBLOCKS] == cut + 8
    # changed thresholds and frame counts do not restart anything
    S2 = dict(K=K, min_amp=0.02, ratio=3.0, twist=12.0, share=0.4, on_frames=2, off_frames=3)
    a.select_group(0); a.set_dtmf(**S2); a.select_group(-1)
    m2.set(channels=slice(0, 3), **S2)
    w = step(3)
    assert w[0, D.TBLOCKS] == nb == at and w[0, D.CNT] == nb % K and w[4, D.TBLOCKS] == 8
    # leaving NFM and coming back: the words are not maintained outside the mode and start from zeros at the next NFM update
    a.set_groups([0])
    a.set_dtmf(**S1)
    a.setDemodMode(4)
    a.update(_cuda(x[:, :128]))
    key, new, lo, hi = _records(a, 1)
    assert np.array_equal(_dtmf_words(a.save_state(0, 5), 5), w) and (key == 255).all() and (new == 255).all() and not lo.any() and not hi.any()
    a.setDemodMode(NFM)
    a.update(_cuda(x[:, :5 * 128]))
    ya = FM.Fm(5).run(x[:, :5 * 128])[0]
    m3 = D.Dtmf(5, tab, **S1)
    _same(_records(a, 5), m3.run(ya), "back in NFM")
    assert np.array_equal(_dtmf_words(a.save_state(0, 5), 5), m3.words()) and (m3.words()[:, D.TBLOCKS] == 5).all() and m3.words()[:, D.PL].any()
    # K = 0: the words are zeros and the records 255 / 255 / 0 / 0
    a.set_dtmf(0)
    a.update(_cuda(x[:, :128]))
    key, new, lo, hi = _records(a, 1)
    assert not _dtmf_words(a.save_state(0, 5), 5).any() and (key == 255).all() and (new == 255).all() and not lo.any() and not hi.any()
    # rdsp_engine_reset zeroes the words and keeps the settings
    a.set_dtmf(**S1)
    a.update(_cuda(x[:, :3 * 128]))
    assert _dtmf_words(a.save_state(0, 5), 5).any()
    a.reset()
    assert not _dtmf_words(a.save_state(0, 5), 5).any()
    a.update(_cuda(x[:, :5 * 128]))
    m3.reset()
    _same(_records(a, 5), m3.run(ya), "after the reset")
    for e in (a, b, plain):
        e.close()


def test_gpu_dtmf_refusals(rdsp):
    """every refusal that needs an engine, each with the object unchanged: rdsp_engine_enable_dtmf before rdsp_engine_enable_fm; the
    reads before rdsp_engine_enable_dtmf; the records before a call; K outside {0} and 4 ... 32; min_amp zero, negative, above 1
    or NaN; ratio and twist below 1, above 1e6, NaN or infinite; share zero, above 1 or NaN; on_frames and off_frames outside
    1 ... 16; n_blocks above the last call's; short strides; a digit range outside the object"""
    import torch
    from test_engine_meter import _engine as plain_engine
    p = plain_engine(2, 4, meter=False)
    assert p.lib.rdsp_engine_enable_dtmf(p.h) == -4 and b"rdsp_engine_enable_fm" in p.lib.rdsp_last_error() and not p.dtmf_enabled
    p.set_dtmf(8)                                                                             # a setting: it may precede the decoder
    p.enable_fm()
    for f in (lambda: p.read_dtmf(0), p.read_dtmf_digits):
        with pytest.raises(rdsp.RdspError) as ex:
            f()
        assert ex.value.code == -4
    p.enable_dtmf()                                                                           # without the meter and the other detectors
    assert p.dtmf_enabled and not p.tone_enabled
    with pytest.raises(rdsp.RdspError) as ex:                                                 # no call yet: there are no records
        p.read_dtmf(1)
    assert ex.value.code == -1
    count, ring = _digits(p)                                                                  # the words exist: no digits
    assert not count.any() and not ring.any()
    p.close()
    x, y = _drawn(5)
    e = _engine(5, 8)
    S1 = dict(K=4, on_frames=1, off_frames=1, **LOOSE)
    e.set_dtmf(**S1)
    m = D.Dtmf(5, table(rdsp), **S1)
    e.update(_cuda(x[:, :3 * 128]))
    m.run(y[:, :3 * 128])
    nan, inf = float("nan"), float("inf")
    ok = (4, 0.015, 4.0, 16.0, 0.5, 2, 2)
    bad_values = {0: (3, 1, 33, -1), 1: (0.0, -0.01, 1.01, nan), 2: (0.99, 1.01e6, nan, inf), 3: (0.99, 1.01e6, nan, inf), 4: (0.0, -0.1, 1.01, nan),
                  5: (0, 17, -1), 6: (0, 17, -1)}
    for k, values in bad_values.items():
        for v in values:
            bad = ok[:k] + (v,) + ok[k + 1:]
            with pytest.raises(rdsp.RdspError) as ex:
                e.set_dtmf(*bad)
            assert ex.value.code == -1 and b"rdsp_engine_set_dtmf" in e.lib.rdsp_last_error(), bad
    with pytest.raises(rdsp.RdspError):
        e.set_dtmf(0, 0.0)                                                                    # K = 0 does not excuse the rest
    key = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    new = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    lo = torch.full((5, 4), 7.0, dtype=torch.float32, device="cuda")
    hi = torch.full((5, 4), 7.0, dtype=torch.float32, device="cuda")
    for nblk, sk, sn, sl, sh in ((4, 4, 4, 4, 4), (-1, 4, 4, 4, 4), (3, 2, 4, 4, 4), (3, 4, 2, 4, 4), (3, 4, 4, 2, 4), (3, 4, 4, 4, 2)):
        assert e.lib.rdsp_engine_read_dtmf(e.h, nblk, key.data_ptr(), sk, new.data_ptr(), sn, lo.data_ptr(), sl, hi.data_ptr(), sh, None) == -1, (nblk, sk, sn, sl, sh)
        assert b"rdsp_engine_read_dtmf" in e.lib.rdsp_last_error()
    count = torch.full((5,), 7, dtype=torch.int32, device="cuda")
    ring = torch.full((5, 16), 7, dtype=torch.int32, device="cuda")
    for c0, cn in ((-1, 1), (0, 6), (5, 1), (0, 0), (3, 3)):
        assert e.lib.rdsp_engine_read_dtmf_digits(e.h, c0, cn, count.data_ptr(), ring.data_ptr(), None) == -1, (c0, cn)
        assert b"rdsp_engine_read_dtmf_digits" in e.lib.rdsp_last_error()
    torch.cuda.synchronize()
    assert (key == 7).all() and (new == 7).all() and (lo == 7.0).all() and (hi == 7.0).all() and (count == 7).all() and (ring == 7).all()
    assert e.lib.rdsp_engine_read_dtmf(e.h, 3, None, 0, None, 0, lo.data_ptr(), 4, None, 0, None) == 0   # any pointer may be NULL
    assert e.lib.rdsp_engine_read_dtmf(e.h, 3, key.data_ptr(), 4, new.data_ptr(), 4, None, 0, hi.data_ptr(), 4, None) == 0
    assert e.lib.rdsp_engine_read_dtmf_digits(e.h, 1, 3, count.data_ptr(), None, None) == 0
    assert e.lib.rdsp_engine_read_dtmf_digits(e.h, 1, 3, None, ring.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(count[:3].cpu().numpy().view(np.uint32), m.digits()[0][1:4]) and (count[3:] == 7).all()
    assert np.array_equal(ring[:3].cpu().numpy().view(np.uint32), m.digits()[1][1:4]) and (ring[3:] == 7).all() and (lo[:, 3] == 7.0).all()
    # nothing of all that changed the object: the stream goes on as the model's
    e.update(_cuda(x[:, 3 * 128:8 * 128]))
    _same(_records(e, 5), m.run(y[:, 3 * 128:8 * 128]), "goes on")
    assert np.array_equal(_dtmf_words(e.save_state(0, 5), 5), m.words())
    e.close()
