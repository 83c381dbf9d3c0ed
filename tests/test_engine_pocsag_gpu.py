"""The POCSAG pager decoder of rdsp_engine_t on the GPU (include/rdsp.h "POCSAG pager decoder"; csrc/rdsp_engine_pocsag.hip,
csrc/rdsp_engine_pocsag_host.hip) against tests/engine_pocsag_model.py.  Every comparison with the model is exact: floats as
uint32, audio as int16.  The five records, n_msgs with the ring and all 456 state words (through a blob) for 1, 5, 97 and 300
receivers on the demodulated rows of tests/engine_fm_model.py at 2400, 1200 and 512 baud under several call splits; the edges: a
codeword that ends with a call's first sampled bit while a transition falls on a trip's first sample, a message across a batch
and a call boundary, corrected and uncorrectable words inside a message, 81 codewords, a full ring, both polarities under invert
2; the decoder beside the other detectors, none of which it changes; an engine that enabled the decoder but has no baud anywhere
against one that never did; two groups at different baud; the state through blobs, regroupings, mode changes, resets and a
changed baud; the refusals.  A paging channel is set_fm(2, 7500, 0).  tests/test_engine_pocsag.py has what needs no GPU."""
import functools

import numpy as np
import pytest

import engine_fm_model as FM
import engine_pocsag_model as M

F32 = np.float32
NFM = 7
CH_WORDS = 96 + 2 * 512 + 3 * 384 + 320      # a channel's words in a blob, in front of the optional parts
DISTINCT = 8
NB = {2400: 87, 1200: 175, 512: 434}
PATTERNS = {2400: ([87], [7, 8, 9, 63], [1] * 87), 1200: ([175],), 512: ([200, 234],)}
pytestmark = pytest.mark.gpu


def _P():
    from radiodsp_sdr_rx_amd import pocsag
    return pocsag


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _engine(n, max_blocks, meter=False, pocsag=True, nfm=True, others=False):
    """sketch set-up, NFM as a paging channel (W = 2, 7500 Hz, no de-emphasis), the tail's AGC and ALS off"""
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
        e.enable_afsk()
    if pocsag:
        e.enable_pocsag()
    if nfm:
        assert e.setDemodMode(NFM) == 0.0
        e.set_fm(2, 7500.0, 0.0)
    return e


def _station(seed, mod, carrier=8000.0, noise=3.0):
    """int16 [t, 2]: a carrier frequency-modulated (7500 Hz peak deviation) by mod (+-0.6: the usual +-4.5 kHz shift)"""
    r = np.random.default_rng(seed)
    n = len(mod)
    z = carrier * np.exp(1j * (2 * np.pi * 7500.0 / 44100.0 * np.cumsum(np.clip(mod, -1.0, 1.0)) + r.uniform(0, 6))) + \
        noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16)


def _flip(word, *at):
    for b in at:
        word ^= 1 << b
    return word


def _messages(r):
    """the five keyed stations' messages: seven words from frame 1; a tone-only page and a numeric one; five words (this row is
    sent inverted); four words of which one gets two errors and one three; two words from frame 3"""
    P = _P()
    draw = lambda k: [int(v) for v in r.integers(0, 1 << 20, k)]
    return [[(801, 3, draw(7))], [(16, 1, []), (1002, 0, P.numeric_words("0123456789"))], [(2048, 2, draw(5))], [(52, 0, draw(4))], [(99003, 3, draw(2))]]


@functools.lru_cache(maxsize=None)
def _distinct(baud):
    """eight distinct receivers, NB[baud] blocks: (iq int16 [8, t, 2], y float32 [8, t] by the FM model, the messages of rows
    0 ... 4).  Rows 0 ... 4: keyed stations that send a 64-bit preamble and one batch, row 2 inverted, row 3 with a corrected and
    a hurt word, row 4 weak under noise; at 512 baud only the preamble, the sync word and two frames, then random bits to the
    batch's end and through the next sync word's place: uncorrectable words, then the `cut`.  Row 5 all zeros; row 6 on the
    rails; row 7 an idle discriminator (noise and no carrier)"""
    P = _P()
    r = np.random.default_rng(4000 + baud)
    nb = NB[baud]
    t = nb * 128
    sent = _messages(r)
    if baud == 512:
        sent = [[(8 * k + 1024, k % 4, [int(v) for v in r.integers(0, 1 << 20, 3)])] for k in range(5)]   # frames 0 and 1: the address and three words
    x = []
    for c, msgs in enumerate(sent):
        words = P.batches(msgs)
        assert len(words) == 17
        if c == 3 and baud != 512:
            at = words.index(P.address_word(52, 0))
            words[at + 2], words[at + 3] = _flip(words[at + 2], 5, 20), _flip(words[at + 3], 1, 12, 25)
        stream = P.bits(words, 64)
        if baud == 512:
            stream = stream[:64 + 32 * 5] + [1 if k % 32 == 0 else int(v) for k, v in enumerate(r.integers(0, 2, 32 * 13))]   # no address words
        mod = P.transmit(stream, baud, 0.6 if c != 1 else 0.45, ppm=r.uniform(-100, 100), lead=int(r.integers(0, 60)), total=t, invert=c == 2)
        x.append(_station(900 + c, mod, r.uniform(2000, 20000), 300.0 if c == 4 else 3.0))
    x.append(np.zeros((t, 2), np.int16))
    x.append(r.choice(np.array([32767, -32768], np.int16), (t, 2)))
    x.append(np.rint(300.0 * r.standard_normal((t, 2))).astype(np.int16))
    x = np.stack(x)
    return x, FM.Fm(DISTINCT, 2, 7500.0, 0.0).run(x)[0], sent


@functools.lru_cache(maxsize=None)
def _model_runs(baud, p):
    """the model on the eight distinct rows at the defaults under call pattern p, computed once for every receiver count: per
    call (records, n_msgs, ring, words)"""
    x, y, sent = _distinct(baud)
    m = M.Pocsag(DISTINCT, baud)
    out, a = [], 0
    for k in PATTERNS[baud][p]:
        rec = m.run(y[:, a * 128:(a + k) * 128])
        out.append((rec,) + m.ring() + (m.words(),))
        a += k
    return out, [m.messages(c) for c in range(DISTINCT)]


def _pocsag_words(blob, n):
    """the POCSAG words of a blob of n channels: its last part"""
    return blob[-n * M.WORDS * 4:].view(np.uint32).reshape(n, M.WORDS)


def _records(e, k):
    return tuple(v.cpu().numpy() for v in e.read_pocsag(k))


def _ring(e):
    return tuple(v.cpu().numpy().view(np.uint32) for v in e.read_pocsag_ring())


def _same(got, want, where):
    """the five records of a call against the model's"""
    for k in (0, 1, 2):
        assert np.array_equal(got[k], want[k]), (where, k, np.argwhere(got[k] != want[k])[:3])
    for k in (3, 4):
        assert np.array_equal(bits(got[k]), bits(want[k])), (where, k, np.argwhere(bits(got[k]) != bits(want[k]))[:3])


def _same_all(e, m, got, want, where, sel=slice(None)):
    _same(got, want, where)
    (gc, gr), (wc, wr) = _ring(e), m.ring()
    assert np.array_equal(gc[sel], wc) and np.array_equal(gr[sel], wr), where
    n = e.n_channels
    assert np.array_equal(_pocsag_words(e.save_state(0, n), n)[sel], m.words()), where


def _msgs(listing):
    """(address, function, words) and flags of read_slot tuples"""
    return [((a, f, w), fl) for _, a, f, w, fl, _ in listing]


@pytest.mark.parametrize("n", [1, 5, 97, 300])
def test_gpu_pocsag_rows_are_the_model(rdsp, n):
    """1, 5, 97 and 300 receivers (a ragged last workgroup, more than one workgroup) that cycle the eight rows of _distinct (keyed
    stations through the FM model, one inverted, silence, the rails, an idle discriminator) at the defaults.  2400 baud: a 64-bit
    preamble and one batch, 87 blocks as [87], [7, 8, 9, 63] and 87 calls of one.  1200 baud: one batch in one call.  512 baud
    (97 receivers at most): preamble, sync and two frames, then noise, 434 blocks as [200, 234] -- the carry of W = 20 across
    trips and the `cut`.  Each from a reset: after every call rdsp_engine_read_pocsag's five records,
    rdsp_engine_read_pocsag_messages' counts and rings and all 456 state words (through a blob) equal the model's.  The
    stations' messages are read as sent"""
    idx = np.arange(n) % DISTINCT
    for baud in (2400, 1200, 512):
        if baud == 512 and n > 97:
            continue
        x, y, sent = _distinct(baud)
        xs = np.ascontiguousarray(x[idx])
        e = _engine(n, max(max(p) for p in PATTERNS[baud]))
        e.set_pocsag(baud)
        for p, pattern in enumerate(PATTERNS[baud]):
            e.reset()
            a = 0
            runs, read = _model_runs(baud, p)
            for k, (rec, count, ring, words) in zip(pattern, runs):
                e.update(_cuda(xs[:, a * 128:(a + k) * 128]))
                _same(_records(e, k), tuple(v[idx] for v in rec), (baud, pattern, a))
                gc, gr = _ring(e)
                assert np.array_equal(gc, count[idx]) and np.array_equal(gr, ring[idx]), (baud, pattern, a)
                assert np.array_equal(_pocsag_words(e.save_state(0, n), n), words[idx]), (baud, pattern, a)
                a += k
            assert (words[:, M.TBLOCKS] == NB[baud]).all() and not words[5, M.NMSGS] and not rec[3][5].any() and rec[3][6].all()
            if baud == 512:
                for c in range(5):
                    (got, fl), = _msgs(read[c])
                    assert got[:2] == sent[c][0][:2] and got[2][:3] == sent[c][0][2] and len(got[2]) > 3 and fl & M.FLAG_CUT, c
                assert words[:5, M.NBAD].all()
            else:
                for c in (0, 1, 2, 4):
                    assert _msgs(read[c]) == [(s, 0) for s in sent[c]], (baud, c)
                assert [p for *_, p in read[2]] == [1] and [p for *_, p in read[0]] == [0]
                (got, fl), = _msgs(read[3])
                assert got[:2] == (52, 0) and got[2][:2] == sent[3][0][2][:2] and ring[3, 0, 4 + 1] >> 24 == 2 and fl == M.FLAG_UNCORRECTABLE
        e.close()


def _edge_signals(nb):
    """six stations at 2400 baud: a message of six words from frame 7, so that five lie behind the second sync word; a message
    with a word of two errors and one of three; a message of 81 words; six messages in one batch; one message sent
    inverted; the same as sent"""
    P = _P()
    r = np.random.default_rng(31)
    draw = lambda k: [int(v) for v in r.integers(0, 1 << 20, k)]
    two, hurt, long, one = [(4007, 3, draw(6))], [(52, 0, draw(4))], [(77, 3, draw(81))], [(1234561, 1, draw(3))]
    six = sorted([(800 + 9 * k, k % 4, draw(k % 2)) for k in range(6)], key=lambda m: m[0] & 7)
    wh = P.batches(hurt)
    at = wh.index(P.address_word(52, 0))
    wh[at + 2], wh[at + 3] = _flip(wh[at + 2], 5, 20), _flip(wh[at + 3], 1, 12, 25)
    rows = [(P.batches(two), False), (wh, False), (P.batches(long), False), (P.batches(six), False), (P.batches(one), True), (P.batches(one), False)]
    x = np.stack([_station(70 + c, P.transmit(P.bits(w, 64), 2400, 0.6, ppm=40.0 * c - 90.0, lead=50 + 37 * c, total=nb * 128, invert=inv)) for c, (w, inv) in enumerate(rows)])
    return x, dict(two=two, hurt=hurt, long=long, six=six, one=one)


_EDGE = {}


def _edge_case():
    """the six stations through an engine in calls of 32 blocks, one call cut short so that a call boundary falls into the second
    sync word of row 0 (a message across a batch and a call boundary); the model runs on the rows rdsp_engine_read_demod returns;
    compared after every call"""
    if _EDGE:
        return _EDGE
    nb = 500
    x, sent = _edge_signals(nb)
    second_sync = int((50 + (64 + 17 * 32 + 16) * 18.375) // 128)                            # the block in the middle of row 0's second sync word
    cuts, a = [], 0
    while a < nb:
        k = min(32, nb - a, second_sync - a if a < second_sync else 32)
        cuts.append(k)
        a += k
    assert second_sync in np.cumsum(cuts)
    e = _engine(6, 32)
    e.set_pocsag(2400)
    m = M.Pocsag(6, 2400)
    trace, raws, a = [], [], 0
    for k in cuts:
        e.update(_cuda(x[:, a * 128:(a + k) * 128]))
        want = m.run(e.read_demod(k).cpu().numpy(), trace=trace, raws=raws)
        _same_all(e, m, _records(e, k), want, a)
        if a + k == second_sync:
            w0 = m.words()[0]
            assert w0[M.OPEN] == 1 and w0[M.M_NCW] == 1 and w0[M.NCW] == 16 and 0 < w0[M.NBITS] < 32   # inside the sync word, the message open
        a += k
    _EDGE.update(x=x, sent=sent, model=m, trace=trace, raw=np.concatenate(raws, 1), listed=e.read_pocsag_messages())
    e.close()
    return _EDGE


def test_gpu_pocsag_edges(rdsp):
    """a message across a batch boundary and a call boundary is read whole; a word with two errors is corrected (ne 2) and the
    word with three is appended as received and flagged uncorrectable; 81 words are read as 80 and flagged
    truncated; six messages leave the last four in slots 4, 5, 2, 3; under invert 2 the inverted station is read with polarity
    1 and the plain one with polarity 0; Engine.read_pocsag_messages returns what the model's ring holds"""
    P = _P()
    c = _edge_case()
    m, sent = c["model"], c["sent"]
    assert _msgs(m.messages(0)) == [(sent["two"][0], 0)]
    (got, fl), = _msgs(m.messages(1))
    slot = m.ring()[1][1, 0]
    assert got[:2] == (52, 0) and got[2][:2] == sent["hurt"][0][2][:2] and got[2][3] == sent["hurt"][0][2][3] and slot[4 + 1] >> 24 == 2
    assert fl == M.FLAG_UNCORRECTABLE and slot[4 + 2] >> 31 and slot[3] == 2 | 1 << 16 and m.words()[1, M.NBAD] == 1   # three errors are never accepted
    a, f, w = sent["long"][0]
    assert _msgs(m.messages(2)) == [((a, f, w[:80]), M.FLAG_TRUNCATED)]
    count, ring = m.ring()
    assert count[3] == 6 and _msgs(m.messages(3)) == [(s, 0) for s in sent["six"][2:]]
    assert [int(ring[3, s, 2]) & 0x1FFFFF for s in range(4)] == [sent["six"][k][0] for k in (4, 5, 2, 3)]
    assert _msgs(m.messages(4)) == _msgs(m.messages(5)) == [(sent["one"][0], 0)]
    assert [p for *_, p in m.messages(4)] == [1] and [p for *_, p in m.messages(5)] == [0]
    want = [(ch, P.from_slot(ring[ch, k % 4])) for ch in range(6) for k in range(max(0, int(count[ch]) - 4), int(count[ch]))]
    assert c["listed"] == want and c["listed"][0][1].words == sent["two"][0][2]


def test_gpu_pocsag_word_ends_on_a_calls_first_bit(rdsp):
    """row 0 of the edge case again, cut so that a codeword's 32nd bit is the FIRST bit a call samples (the shift register, the
    bit count and the clock all come from the words) and so that a transition falls on the first sample of a call's second trip
    (prev_raw and the clock cross the trip): records, ring and words equal the model's at every call"""
    c = _edge_case()
    raw = c["raw"][0]
    ends = [(m0, k) for m0, k, _ in c["trace"] if k >= 0 and m0 % 32 < 4 and m0 // 32 > 40]   # 4.59 samples a bit: the bit before lies in an earlier block
    assert ends, "no codeword ends in a block's first samples"
    for m_end, _ in ends:                                                                     # the first such word with a suitable transition before it
        E = m_end // 32
        first = raw[32 * np.arange(1, E)] != raw[32 * np.arange(1, E) - 1]
        J = [int(j) for j in np.flatnonzero(first) + 1 if 8 <= j and j + 24 <= E]
        if J:
            break
    assert J, "no transition on a block's first sample"
    j = J[len(J) // 2]
    pattern, a = [], 0
    for stop in (j - 8, E, E + 40):
        while a < stop:
            k = min(32, stop - a)
            pattern.append(k)
            a += k
    assert j - 8 in np.cumsum([0] + pattern) and E in np.cumsum([0] + pattern)
    e = _engine(1, 32)
    e.set_pocsag(2400)
    m = M.Pocsag(1, 2400)
    a = 0
    for k in pattern:
        before = m.words()[0]
        e.update(_cuda(c["x"][:1, a * 128:(a + k) * 128]))
        _same_all(e, m, _records(e, k), m.run(e.read_demod(k).cpu().numpy()), a)
        if a == E:
            assert before[M.NBITS] == 31 and before[M.INSYNC] == 1
        a += k
    assert _msgs(m.messages(0)) == [(c["sent"]["two"][0], 0)]
    e.close()


def test_gpu_pocsag_beside_the_other_detectors(rdsp):
    """meter with its squelch, tone squelch, code squelch, noise squelch, DTMF decoder, AFSK decoder, voice stage (R = 2) and the
    decoder together against the same engine without the decoder, 97 receivers, 87 blocks as [7, 8, 9, 63]: the int16 audio, the
    other detectors' records, the active list, the voice rows and every blob part with a flag below 1024 are the same bytes,
    and the decoder's records, ring and words equal the model's"""
    n = 97
    x, y, sent = _distinct(2400)
    idx = np.arange(n) % DISTINCT
    xs = np.ascontiguousarray(x[idx])
    engines = []
    for with_pocsag in (True, False):
        e = _engine(n, 63, meter=True, pocsag=with_pocsag, others=True)
        e.set_squelch(2e-3, 1e-3, 1)
        e.set_tones(0, np.where(np.arange(n) % 3 == 0, F32(100.0), F32(0.0)).astype(F32))
        e.set_tone_squelch(4, 0.06, 0.045)
        e.set_dcs_codes(0, [0o023 if c % 5 == 0 else 0 for c in range(n)])
        e.set_noise_squelch()
        e.set_dtmf(4)
        e.set_afsk(1)
        e.enable_voice(2)
        engines.append(e)
    a, b = engines
    a.set_pocsag(2400)
    same = lambda va, vb: np.array_equal(va.cpu().numpy().view(np.uint8), vb.cpu().numpy().view(np.uint8))
    at = 0
    runs, read = _model_runs(2400, 1)
    for k, (rec, count, ring, words) in zip(PATTERNS[2400][1], runs):
        d = _cuda(xs[:, at * 128:(at + k) * 128])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        assert np.array_equal(ya, yb)
        for read_ in ("read_meter", "read_tone", "read_dcs", "read_noise", "read_dtmf", "read_afsk"):
            for va, vb in zip(getattr(a, read_)(k), getattr(b, read_)(k)):
                assert same(va, vb), read_
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        assert same(a.read_voice(k), b.read_voice(k))
        _same(_records(a, k), tuple(v[idx] for v in rec), at)
        gc, gr = _ring(a)
        assert np.array_equal(gc, count[idx]) and np.array_equal(gr, ring[idx])
        at += k
    assert count[:5].all()
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert blob_b.view(np.uint32)[3] == 2 | 4 | 8 | 16 | 64 | 128 | 256 | 512 and blob_a.view(np.uint32)[3] == 2 | 4 | 8 | 16 | 64 | 128 | 256 | 512 | 1024
    assert len(blob_a) == len(blob_b) + n * M.WORDS * 4 and np.array_equal(blob_a[16:len(blob_b)], blob_b[16:])
    assert np.array_equal(_pocsag_words(blob_a, n), words[idx])
    for e in engines:
        e.close()


def test_gpu_pocsag_off_changes_nothing(rdsp):
    """NFM, LSB and AM groups (5 + 3 + 4 receivers), meter and squelch on: an engine that enabled the decoder with baud 0
    everywhere gives the audio, the meter records and the active list of one that never enabled it, and reads zero records and no
    messages; the blob of the engine that never enabled it has the size and the flags it always had (meter 2, FM 8) and is, byte
    for byte, the other's without its header flag 1024 and its eleventh part, which is zeros"""
    from test_engine_meter import _bursts
    n, nb, first = 12, 6, [0, 5, 8]
    x = _bursts(83, n, nb)
    x[:5] = FM.station(90, nb, 4000.0, 1000.0, 9000.0, 3.0)[None]
    engines = []
    for with_pocsag in (True, False):
        e = _engine(n, 4, meter=True, pocsag=with_pocsag, nfm=False)
        e.set_squelch(2e-3, 1e-3, 1)
        e.set_groups(first)
        e.select_group(0); assert e.setDemodMode(NFM) == 0.0
        e.select_group(2); e.setDemodMode(4); e.setAudioFilter(0)
        e.select_group(-1)
        engines.append(e)
    a, b = engines
    assert a.pocsag_enabled and not b.pocsag_enabled
    for k0, k in ((0, 4), (4, 2)):
        d = _cuda(x[:, k0 * 128:(k0 + k) * 128])
        ya, yb = a.update(d).cpu().numpy(), b.update(d).cpu().numpy()
        assert np.array_equal(ya, yb) and ya[:5].any() and ya[5:].any()
        for va, vb in zip(a.read_meter(k), b.read_meter(k)):
            assert np.array_equal(bits(va.cpu().numpy().astype(F32)), bits(vb.cpu().numpy().astype(F32)))
        assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy()) and np.array_equal(a.meter(), b.meter())
        assert not any(v.any() for v in _records(a, k))
        count, ring = _ring(a)
        assert not count.any() and not ring.any() and a.read_pocsag_messages() == []
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)
    assert len(blob_b) == 16 + n * (CH_WORDS + 3 + 50) * 4 == b.lib.rdsp_engine_state_bytes(b.h, n) and blob_b.view(np.uint32)[3] == 2 | 8
    assert len(blob_a) == len(blob_b) + n * M.WORDS * 4 == a.lib.rdsp_engine_state_bytes(a.h, n) and blob_a.view(np.uint32)[3] == 2 | 8 | 1024
    assert np.array_equal(blob_a[16:len(blob_b)], blob_b[16:]) and not blob_a[len(blob_b):].any()
    assert np.array_equal(blob_a[:12], blob_b[:12])
    with pytest.raises(rdsp.RdspError) as ex:
        b.read_pocsag(0)
    assert ex.value.code == -4
    for e in engines:
        e.close()


def test_gpu_pocsag_two_bauds_side_by_side(rdsp):
    """five receivers in two groups, channels 0 and 1 at 2400 baud and 2, 3 and 4 at 1200: the groups' launches lie in one
    call and each reads with its own window and step; records, rings and words equal the model's with per-channel settings, and
    every station's message is read"""
    x24, _, s24 = _distinct(2400)
    x12, _, s12 = _distinct(1200)
    nb = NB[1200]
    x = np.zeros((5, nb * 128, 2), np.int16)
    x[:2, :NB[2400] * 128] = x24[:2]
    x[2:] = x12[:3]
    e = _engine(5, 64)
    e.set_groups([0, 2])
    e.select_group(0); e.set_pocsag(2400); e.select_group(1); e.set_pocsag(1200, 2, 2, 1, 1, 1); e.select_group(-1)
    m = M.Pocsag(5, 2400)
    m.set(1200, 2, 2, 1, 1, 1, channels=slice(2, None))
    for a in range(0, nb, 64):
        k = min(64, nb - a)
        e.update(_cuda(x[:, a * 128:(a + k) * 128]))
        _same_all(e, m, _records(e, k), m.run(e.read_demod(k).cpu().numpy()), a)
    assert [_msgs(m.messages(c)) for c in range(5)] == [[(s, 0) for s in s24[0]], [(s, 0) for s in s24[1]], [(s, 0) for s in s12[0]], [(s, 0) for s in s12[1]],
                                                        [(s, 0) for s in s12[2]]]
    assert list(m.words()[:, M.BAUD]) == [2400, 2400, 1200, 1200, 1200]
    e.close()


def test_gpu_pocsag_state(rdsp):
    """the decoder's words are signal state.  A receiver in the middle of a message (in sync, words in the open message) moves by
    blob to an engine with another channel count, another index and another max_blocks, and continues bit for bit to the
    message's end.  An engine without the decoder refuses the part with nothing changed; a blob without the part zeroes the
    words.  A regrouping keeps the detector; changed invert, pull, sync_errs and fix_* do not restart it; baud 0 zeroes a
    group's words; another baud restarts them from zeros; outside NFM the words are left alone and coming back restarts them;
    rdsp_engine_reset zeroes them and keeps the settings"""
    nb, cut = NB[2400], 40
    x, y, sent = _distinct(2400)
    x, y = x[:5], y[:5]
    a = _engine(5, 16)
    a.enable_pocsag()                                                                         # again: a no-op
    a.set_pocsag(2400)
    m = M.Pocsag(5, 2400)
    for k0 in (0, 16, 32):
        k = min(16, cut - k0)
        a.update(_cuda(x[:, k0 * 128:(k0 + k) * 128]))
        _same(_records(a, k), m.run(y[:, k0 * 128:(k0 + k) * 128]), k0)
    blob = a.save_state(0, 1)
    w0 = m.words()[0]
    assert w0[M.INSYNC] == 1 and w0[M.OPEN] == 1 and w0[M.M_NCW] > 1 and w0[M.TBLOCKS] == cut and w0[M.HIST_:M.HIST_ + 19].all() and w0[M.PLL]
    assert np.array_equal(_pocsag_words(blob, 1)[0], w0) and blob.view(np.uint32)[3] == 8 | 1024
    plain = _engine(3, 8, pocsag=False)
    assert len(blob) == a.lib.rdsp_engine_state_bytes(a.h, 1) == plain.lib.rdsp_engine_state_bytes(plain.h, 1) + M.WORDS * 4
    before = plain.save_state(0, 3)
    with pytest.raises(rdsp.RdspError) as ex:                                                 # an engine without the decoder refuses the part
        plain.load_state(0, blob)
    assert ex.value.code == -4 and np.array_equal(plain.save_state(0, 3), before)
    # the receiver continues in another engine: 7 channels, index 4, 64 blocks a call, a past of its own
    b = _engine(7, 64)
    b.set_pocsag(2400)
    b.update(_cuda(np.broadcast_to(x[1:2, :128], (7, 128, 2)).copy()))
    b.load_state(4, blob)
    assert np.array_equal(_pocsag_words(b.save_state(4, 1), 1)[0], w0)
    rest = np.zeros((7, (nb - cut) * 128, 2), np.int16)
    rest[4] = x[0, cut * 128:]
    b.update(_cuda(rest))
    want = m.run(y[:, cut * 128:])
    got = _records(b, nb - cut)
    _same(tuple(v[4:5] for v in got), tuple(v[:1] for v in want), "moved")
    assert np.array_equal(_pocsag_words(b.save_state(4, 1), 1)[0], m.words()[0]) and _msgs(m.messages(0)) == [(sent[0][0], 0)]
    assert [(ch, msg.address, msg.words) for ch, msg in b.read_pocsag_messages() if ch == 4] == [(4, sent[0][0][0], sent[0][0][2])]
    b.load_state(4, plain.save_state(0, 1))                                                   # a blob without the part zeroes the words
    assert not _pocsag_words(b.save_state(4, 1), 1).any()
    # a's own stream goes on from block `cut`.  A regrouping keeps the detector
    a.set_groups([0, 2])
    m2 = M.Pocsag(5, 2400)
    m2.run(y[:, :cut * 128])
    at = cut

    def step(k):
        nonlocal at
        a.update(_cuda(x[:, at * 128:(at + k) * 128]))
        _same_all(a, m2, _records(a, k), m2.run(y[:, at * 128:(at + k) * 128]), at)
        at += k
        return m2.words()
    w = step(3)
    assert (w[:, M.TBLOCKS] == cut + 3).all()
    # changed settings restart nothing
    S2 = dict(invert=0, pull=2, sync_errs=1, fix_addr=2, fix_data=1)
    a.select_group(1); a.set_pocsag(2400, **S2); a.select_group(-1)
    m2.set(2400, channels=slice(2, None), **S2)
    w = step(4)
    assert (w[:, M.TBLOCKS] == cut + 7).all()
    # group 0 (channels 0, 1) switches the decoder off: its words are zeros, its records too; group 1 goes on
    a.select_group(0); a.set_pocsag(0); a.select_group(-1)
    m2.set(0, channels=slice(0, 2))
    w = step(3)
    assert not w[:2].any() and (w[2:, M.TBLOCKS] == cut + 10).all()
    # and on again at another baud, and group 1 changes its baud: fresh detectors
    a.select_group(0); a.set_pocsag(1200); a.select_group(1); a.set_pocsag(512, **S2); a.select_group(-1)
    m2.set(1200, channels=slice(0, 2))
    m2.set(512, channels=slice(2, None), **S2)
    w = step(5)
    assert (w[:, M.TBLOCKS] == 5).all() and list(w[:, M.BAUD]) == [1200, 1200, 512, 512, 512]
    # a regrouping into a group with another baud restarts the channel that moved: channel 2 joins group 0
    a.set_groups([0, 3])
    m2.set(1200, channels=slice(2, 3))
    step(16)
    step(10)
    w = step(nb - at)
    assert list(w[:, M.BAUD]) == [1200, 1200, 1200, 512, 512] and w[2, M.TBLOCKS] < w[3, M.TBLOCKS] and at == nb
    # leaving NFM and coming back: the words are not maintained outside the mode and start from zeros at the next NFM update
    a.set_groups([0])
    a.set_pocsag(2400)
    a.setDemodMode(4)
    a.update(_cuda(x[:, :128]))
    assert np.array_equal(_pocsag_words(a.save_state(0, 5), 5), w) and not any(v.any() for v in _records(a, 1))
    a.setDemodMode(NFM)
    a.update(_cuda(x[:, :9 * 128]))
    ya = FM.Fm(5, 2, 7500.0, 0.0).run(x[:, :9 * 128])[0]
    m3 = M.Pocsag(5, 2400)
    _same(_records(a, 9), m3.run(ya), "back in NFM")
    assert np.array_equal(_pocsag_words(a.save_state(0, 5), 5), m3.words()) and (m3.words()[:, M.TBLOCKS] == 9).all()
    # rdsp_engine_reset zeroes the words and keeps the settings
    a.reset()
    assert not _pocsag_words(a.save_state(0, 5), 5).any()
    a.update(_cuda(x[:, :9 * 128]))
    m3.reset()
    _same(_records(a, 9), m3.run(ya), "after the reset")
    assert np.array_equal(_pocsag_words(a.save_state(0, 5), 5), m3.words())
    for e in (a, b, plain):
        e.close()


def test_gpu_pocsag_refusals(rdsp):
    """every refusal that needs an engine, each with the object unchanged: rdsp_engine_enable_pocsag before rdsp_engine_enable_fm;
    the reads before rdsp_engine_enable_pocsag; the records before a call; a baud outside 0, 512, 1200, 2400; invert outside
    0 ... 2; pull outside 1 ... 4; sync_errs outside 0 ... 3; fix_* outside 0 ... 2; n_blocks above the last call's; short strides;
    a message range outside the object"""
    import torch
    from test_engine_meter import _engine as plain_engine
    p = plain_engine(2, 4, meter=False)
    assert p.lib.rdsp_engine_enable_pocsag(p.h) == -4 and b"rdsp_engine_enable_fm" in p.lib.rdsp_last_error() and not p.pocsag_enabled
    p.set_pocsag(1200, 1, 2, 3, 2, 0)                                                         # a setting: it may precede the decoder
    p.enable_fm()
    for f in (lambda: p.read_pocsag(0), p.read_pocsag_ring, p.read_pocsag_messages):
        with pytest.raises(rdsp.RdspError) as ex:
            f()
        assert ex.value.code == -4
    p.enable_pocsag()                                                                         # without the meter and the other detectors
    assert p.pocsag_enabled and not p.afsk_enabled
    with pytest.raises(rdsp.RdspError) as ex:                                                 # no call yet: there are no records
        p.read_pocsag(1)
    assert ex.value.code == -1
    count, ring = _ring(p)                                                                    # the words exist: no messages
    assert not count.any() and not ring.any()
    p.close()
    x, y, sent = _distinct(2400)
    x, y = x[:5], y[:5]
    e = _engine(5, 8)
    e.set_pocsag(2400)
    m = M.Pocsag(5, 2400)
    e.update(_cuda(x[:, :3 * 128]))
    m.run(y[:, :3 * 128])
    ok = (1200, 2, 3, 2, 1, 2)
    bad_values = {0: (-1, 1, 600, 4800, 511), 1: (-1, 3), 2: (0, 5, -1), 3: (-1, 4), 4: (-1, 3), 5: (-1, 3)}
    for k, values in bad_values.items():
        for v in values:
            bad = ok[:k] + (v,) + ok[k + 1:]
            with pytest.raises(rdsp.RdspError) as ex:
                e.set_pocsag(*bad)
            assert ex.value.code == -1 and b"rdsp_engine_set_pocsag" in e.lib.rdsp_last_error(), bad
    with pytest.raises(rdsp.RdspError):
        e.set_pocsag(0, 3)                                                                    # baud 0 does not excuse the rest
    sync = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    new = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    bad = torch.full((5, 4), 7, dtype=torch.uint8, device="cuda")
    lvl = torch.full((5, 4), 7.0, dtype=torch.float32, device="cuda")
    dc = torch.full((5, 4), 7.0, dtype=torch.float32, device="cuda")
    for nblk, s0, s1, s2, s3, s4 in ((4, 4, 4, 4, 4, 4), (-1, 4, 4, 4, 4, 4), (3, 2, 4, 4, 4, 4), (3, 4, 2, 4, 4, 4), (3, 4, 4, 2, 4, 4), (3, 4, 4, 4, 2, 4),
                                     (3, 4, 4, 4, 4, 2)):
        assert e.lib.rdsp_engine_read_pocsag(e.h, nblk, sync.data_ptr(), s0, new.data_ptr(), s1, bad.data_ptr(), s2, lvl.data_ptr(), s3, dc.data_ptr(), s4,
                                             None) == -1, (nblk, s0, s1, s2, s3, s4)
        assert b"rdsp_engine_read_pocsag" in e.lib.rdsp_last_error()
    count = torch.full((5,), 7, dtype=torch.int32, device="cuda")
    ring = torch.full((5, 4, 84), 7, dtype=torch.int32, device="cuda")
    for c0, cn in ((-1, 1), (0, 6), (5, 1), (0, 0), (3, 3)):
        assert e.lib.rdsp_engine_read_pocsag_messages(e.h, c0, cn, count.data_ptr(), ring.data_ptr(), None) == -1, (c0, cn)
        assert b"rdsp_engine_read_pocsag_messages" in e.lib.rdsp_last_error()
    torch.cuda.synchronize()
    assert (sync == 7).all() and (new == 7).all() and (bad == 7).all() and (lvl == 7.0).all() and (dc == 7.0).all() and (count == 7).all() and (ring == 7).all()
    assert e.lib.rdsp_engine_read_pocsag(e.h, 3, None, 0, None, 0, None, 0, lvl.data_ptr(), 4, None, 0, None) == 0   # any pointer may be NULL
    assert e.lib.rdsp_engine_read_pocsag(e.h, 3, sync.data_ptr(), 4, new.data_ptr(), 4, bad.data_ptr(), 4, None, 0, dc.data_ptr(), 4, None) == 0
    assert e.lib.rdsp_engine_read_pocsag_messages(e.h, 1, 3, count.data_ptr(), None, None) == 0
    assert e.lib.rdsp_engine_read_pocsag_messages(e.h, 1, 3, None, ring.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(count[:3].cpu().numpy().view(np.uint32), m.ring()[0][1:4]) and (count[3:] == 7).all()
    assert np.array_equal(ring[:3].cpu().numpy().view(np.uint32), m.ring()[1][1:4]) and (ring[3:] == 7).all() and (lvl[:, 3] == 7.0).all()
    # nothing of all that changed the object: the stream goes on as the model's
    e.update(_cuda(x[:, 3 * 128:8 * 128]))
    _same(_records(e, 5), m.run(y[:, 3 * 128:8 * 128]), "goes on")
    assert np.array_equal(_pocsag_words(e.save_state(0, 5), 5), m.words())
    e.close()
