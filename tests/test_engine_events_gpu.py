"""rdsp_engine_gather_events on the GPU (include/rdsp.h "Decoder events"; csrc/rdsp_engine_events.hip,
csrc/rdsp_engine_events_host.hip) against tests/engine_events_model.py.  Every comparison is exact.  The expected sequence is the
model applied to THE ENGINE'S OWN read_dtmf / read_afsk / read_pocsag records and read_dtmf_digits / read_afsk_ring /
read_pocsag_ring counts and rings of the same call, so these tests pin the gather and not the decoders (their own files hold
those to their models).  The stimuli come from the decoders' builders: pocsag.transmit, engine_afsk_model's Bell 202 audio and
engine_dtmf_model's keypad, through an FM station at 7500 Hz of deviation; every NFM group is set_fm(2, 7500, 0), a paging channel,
on which the flat packet and keypad stations read as well.  tests/test_engine_events.py has what needs no GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import engine_afsk_model as A
import engine_dtmf_model as D
import engine_events_model as M

NFM, LSB = 7, 0
U32 = np.uint32
NB = 87
SENTINEL = 0x5EA15EA1
LOOSE = dict(K=4, min_amp=0.05, ratio=2.0, twist=8.0, share=0.3, on_frames=1, off_frames=1)
pytestmark = pytest.mark.gpu


def _P():
    from radiodsp_sdr_rx_amd import pocsag
    return pocsag


def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _engine(n, max_blocks=NB, kinds=(True, True, True), groups=None):
    """sketch set-up, the tail's AGC and ALS off, every group NFM as a paging channel with the enabled decoders on: DTMF frames of
    4 blocks that emit a key after one frame (LOOSE), AFSK at its defaults, POCSAG at 2400 baud"""
    from radiodsp_sdr_rx_amd.engine import Engine
    import oracle_lib
    e = Engine(n, max_blocks_per_call=max_blocks, tables=oracle_lib.engine_tables())
    e.sketch_setup()
    e.setAGCmode(0)
    e.enable_fm()
    if kinds[0]:
        e.enable_dtmf()
    if kinds[1]:
        e.enable_afsk()
    if kinds[2]:
        e.enable_pocsag()
    if groups:
        e.set_groups(groups)
    assert e.setDemodMode(NFM) == 0.0
    e.set_fm(2, 7500.0, 0.0)
    if kinds[0]:
        e.set_dtmf(**LOOSE)
    if kinds[1]:
        e.set_afsk(1)
    if kinds[2]:
        e.set_pocsag(2400)
    return e


def station(seed, mod, carrier=8000.0, noise=3.0):
    """int16 [t, 2]: a carrier frequency-modulated (7500 Hz peak deviation) by mod, `noise` counts of noise"""
    r = np.random.default_rng(seed)
    n = len(mod)
    z = carrier * np.exp(1j * (2 * np.pi * 7500.0 / 44100.0 * np.cumsum(np.clip(mod, -1.0, 1.0)) + r.uniform(0, 6))) + \
        noise * (r.standard_normal(n) + 1j * r.standard_normal(n))
    return np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16)


def page(messages, baud=2400, lead=0, total=None, whole=True):
    """the modulating signal of a paging transmitter: a 64-bit preamble and the messages' batches; whole False: cut behind the
    idle word that closes the last message"""
    P = _P()
    words = P.batches(messages)
    if not whole:
        last = max(k for k, w in enumerate(words) if w != P.IDLE and w != P.SYNC)
        words = words[:last + 2]
    return P.transmit(P.bits(words, 64), baud, 0.6, lead=lead, total=total)


def packet(payload, lead=0, total=None, amp=0.4):
    """the modulating signal of a flat packet station: one frame behind 3 flags"""
    return A.audio(A.nrzi(A.frame_bits(payload, 3, 2)), amp, lead=lead, total=total)


def keypad(keys, on=6, off=3, lead=0, total=None):
    """the modulating signal of a keypad: every key `on` blocks of its tone pair and `off` blocks of nothing"""
    return D.keyed(keys, on * 128, off * 128, 0.3, 0.3, lead=lead, total=total)


def placed(total, *parts):
    """the sum of (signal, first sample) parts in `total` samples"""
    out = np.zeros(total)
    for sig, at in parts:
        k = max(0, min(len(sig), total - at))
        out[at:at + k] += sig[:k]
    return out


PAYLOADS = [bytes(np.random.default_rng(60 + k).integers(0, 256, 15 + 4 * k, dtype=np.uint8)) for k in range(3)]


@functools.lru_cache(maxsize=None)
def rows(nb=NB):
    """nine distinct receivers, nb blocks, int16 [9, t, 2]: 0 a paging station with a message of seven words; 1 one with a
    tone-only page and a numeric one; 2 a packet station; 3 a keypad run of eight keys; 4 silence; 5 the rails; 6 an idle
    discriminator; 7 a tone-only page, then a packet (a channel with an AFSK and a POCSAG item in one call); 8 a tone-only page at
    1200 baud"""
    P = _P()
    r = np.random.default_rng(7100)
    t = nb * 128
    draw = lambda k: [int(v) for v in r.integers(0, 1 << 20, k)]
    short = page([(8, 2, [])], whole=False)
    mods = [page([(801, 3, draw(7))], lead=20, total=t), page([(16, 1, []), (1002, 0, P.numeric_words("0123456789"))], lead=45, total=t),
            packet(PAYLOADS[0], lead=700, total=t), keypad("159D*0#A", lead=128, total=t), None, None, None,
            placed(t, (short, 30), (packet(PAYLOADS[1]), 30 + len(short) + 200)), page([(24, 1, [])], 1200, lead=10, total=t, whole=False)]
    x = [station(900 + c, m, r.uniform(2000, 20000)) if m is not None else None for c, m in enumerate(mods)]
    x[4] = np.zeros((t, 2), np.int16)
    x[5] = r.choice(np.array([32767, -32768], np.int16), (t, 2))
    x[6] = np.rint(300.0 * r.standard_normal((t, 2))).astype(np.int16)
    return np.stack(x)


def snapshot(e, k):
    """the engine's own records of the last call's k blocks, counts and rings, by kind; None for a decoder that is off"""
    new, count, ring = [None] * 3, [None] * 3, [None] * 3
    host = lambda v: v.cpu().numpy()
    if e.dtmf_enabled:
        new[0], (count[0], ring[0]) = host(e.read_dtmf(k)[1]), (host(v).view(U32) for v in e.read_dtmf_digits())
    if e.afsk_enabled:
        new[1], (count[1], ring[1]) = host(e.read_afsk(k)[1]), (host(v).view(U32) for v in e.read_afsk_ring())
    if e.pocsag_enabled:
        new[2], (count[2], ring[2]) = host(e.read_pocsag(k)[1]), (host(v).view(U32) for v in e.read_pocsag_ring())
    return new, count, ring


def gather(e, ce=None, cw=None, stream=None):
    records, words, counts = e.gather_events(ce, cw, stream=stream)
    return records.cpu().numpy().view(U32), words.cpu().numpy().view(U32), tuple(counts)


def raw_gather(e, ce, cw, tail=5):
    """the entry point itself into buffers with `tail` sentinel entries behind the capacities: the sentinels behind `written` are
    asserted here"""
    import torch
    records = torch.full((ce + tail, 4), SENTINEL, dtype=torch.int32, device="cuda")
    words = torch.full((cw + tail,), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    rc = e.lib.rdsp_engine_gather_events(e.h, records.data_ptr() if ce else None, ce, words.data_ptr() if cw else None, cw, cnt.data_ptr(), None)
    assert rc == 0, e.lib.rdsp_last_error()
    torch.cuda.synchronize()
    counts = tuple(int(v) for v in cnt.tolist())
    records, words = records.cpu().numpy(), words.cpu().numpy()
    assert (records[counts[1]:] == SENTINEL).all() and (words[counts[3]:] == SENTINEL).all(), ("written behind `written`", ce, cw, counts)
    return records[:counts[1]].view(U32), words[:counts[3]].view(U32), counts


def same(got, want, where):
    assert got[2] == want[2], (where, got[2], want[2])
    assert np.array_equal(got[0], want[0]), (where, np.argwhere(got[0] != want[0])[:3])
    assert np.array_equal(got[1], want[1]), (where, np.argwhere(got[1] != want[1])[:3])


def check(e, k, where):
    """the gather of the last call (k blocks) is the model on the engine's own records -> (events, lost) of the model"""
    snap = snapshot(e, k)
    events, lost = M.sequence(*snap)
    same(gather(e), M.cut(events, lost), where)
    return events, lost


def kinds_of(events):
    return {k for _, k, _, _ in events}


@pytest.mark.parametrize("n", [1, 5, 97, 300])
def test_gpu_events_rows_are_the_model(rdsp, n):
    """1, 5, 97 and 300 receivers (a ragged last workgroup, more than one workgroup) that cycle the first eight rows of rows(), all
    three decoders on, 87 blocks as [87] and as [7, 8, 9, 63] from a reset each, a gather after every call: records, words and
    counts are the model's on the engine's own records.  Over a pattern's calls every seq of every channel and kind appears exactly
    once, 0 ... n - 1 of its final count; nothing is lost; from eight receivers on all three kinds occur, and the channel of row 7
    has an AFSK and a POCSAG item in one call"""
    from radiodsp_sdr_rx_amd import events as EV
    idx = np.arange(n) % 8
    x = np.ascontiguousarray(rows()[idx])
    e = _engine(n)
    both = False
    for pattern in ([87], [7, 8, 9, 63]):
        e.reset()
        a, seen = 0, {}
        for k in pattern:
            e.update(_cuda(x[:, a * 128:(a + k) * 128]))
            events, lost = check(e, k, (n, pattern, a))
            assert lost == 0
            for ch, kind, seq, _ in events:
                seen.setdefault((ch, kind), []).append(seq)
            both |= n >= 8 and {1, 2} <= {kind for ch, kind, _, _ in events if ch == 7}
            a += k
        _, count, _ = snapshot(e, k)
        for kind in range(3):
            for ch in range(n):
                assert seen.get((ch, kind), []) == list(range(int(count[kind][ch]))), (pattern, ch, kind)
        if n >= 8:
            assert {kind for _, kind in seen} == {0, 1, 2}
            assert count[0][3] >= 4 and count[1][2] == 1 and count[2][0] == 1 and count[2][1] == 2 and not count[0][4:7].any()
    assert both == (n >= 8)                                                   # in the call of 87 blocks
    got = e.events()                                                          # the last call of [7, 8, 9, 63], read on the host
    assert [(v.channel, v.kind, v.seq) for v in got] == [(ch, kind, seq) for ch, kind, seq, _ in events]
    if n >= 8:
        assert any(v.kind == EV.AFSK and v.value == PAYLOADS[0] for v in got) and any(v.kind == EV.POCSAG and v.value.address == 801 for v in got)
        assert all(v.value in "159D*0#A" for v in got if v.kind == EV.DTMF and v.channel == 3)


@pytest.mark.parametrize("n", [1025, 2049])
def test_gpu_events_scan_chunks(rdsp, n):
    """1025 and 2049 receivers (two and three chunks of the scan, the last of one channel), silence but for channels 0, 1023, 1024
    and the last: a call of 79 blocks, then one of 8 in which a page closes on 0 (and on 2048), a packet on 1023 and a key is
    read on 1024.  The gather of the second call is the model's and its events lie on exactly those four channels"""
    t = NB * 128
    short = page([(8, 2, [])], whole=False)
    frame = packet(PAYLOADS[0])
    at = {0: placed(t, (short, 82 * 128 - len(short))), 1023: placed(t, (frame, 83 * 128 - len(frame))), 1024: keypad("7", 8, 0, lead=79 * 128, total=t)}
    if n - 1 not in at:
        at[n - 1] = placed(t, (short, 84 * 128 - len(short)))
    kind_at = {0: 2, 1023: 1, 1024: 0, n - 1: 0 if n - 1 == 1024 else 2}
    x = np.zeros((n, t, 2), np.int16)
    for ch, mod in at.items():
        x[ch] = station(500 + ch % 7, mod)
    e = _engine(n)
    e.update(_cuda(x[:, :79 * 128]))
    first, _ = check(e, 79, (n, 0))
    e.update(_cuda(x[:, 79 * 128:]))
    events, lost = check(e, 8, (n, 79))
    assert sorted({ch for ch, *_ in events}) == sorted(at) and lost == 0, [(ch, k, s) for ch, k, s, _ in events]
    assert {ch: k for ch, k, _, _ in events} == kind_at and not {ch for ch, *_ in first} & set(at)


def test_gpu_events_more_than_a_trip(rdsp):
    """three receivers, max_blocks 130, one call of 129 blocks (three trips of the record reduction, the last of one block): a key
    read in block 63, a packet whose closing flag ends in block 64, a page that closes in block 128 -- the engine's own records say so -- and the
    gather is the model's"""
    t = 129 * 128
    short = page([(8, 2, [])], whole=False)
    frame = packet(PAYLOADS[0])
    x = np.stack([station(41, keypad("5", 8, 0, lead=60 * 128, total=t)), station(42, placed(t, (frame, 66 * 128 + 100 - len(frame)))),
                  station(43, placed(t, (short, 128 * 128 + 64 - len(short))))])
    e = _engine(3, 130)
    e.update(_cuda(x))
    events, lost = check(e, 129, "trip")
    new, _, _ = snapshot(e, 129)
    assert new[0][0, 63] != 255 and new[1][1, 64] == 1 and new[2][2, 128] == 1, (np.flatnonzero(new[0][0] != 255), np.flatnonzero(new[1][1]), np.flatnonzero(new[2][2]))
    assert [(ch, k) for ch, k, _, _ in events] == [(0, 0), (1, 1), (2, 2)] and lost == 0


def test_gpu_events_lost(rdsp):
    """six tone-only pages in one batch at 2400 baud.  In one call of 87 blocks c = 6: the four newest are gathered, seq n - 4 ...
    n - 1 = 2 ... 5, and lost is 2.  The same stream as calls of 46 and 41 blocks loses nothing: seq 0 ... 5 over the two"""
    x = station(77, page([(8 * k + k, k % 4, []) for k in range(6)], lead=30, total=NB * 128))[None]
    e = _engine(1)
    e.update(_cuda(x))
    events, lost = check(e, NB, "one call")
    rec, words, counts = gather(e)
    assert lost == 2 and counts == (4, 4, 16, 16, 2) and [seq for *_, seq, _ in events] == [2, 3, 4, 5]
    assert [v.value.address for v in e.events()] == [8 * k + k for k in range(2, 6)]
    e.reset()
    seqs, a = [], 0
    for k in (46, 41):
        e.update(_cuda(x[:, a * 128:(a + k) * 128]))
        events, lost = check(e, k, ("two calls", a))
        assert lost == 0 and 0 < len(events) <= 4
        seqs += [seq for *_, seq, _ in events]
        a += k
    assert seqs == list(range(6))


def test_gpu_events_capacity(rdsp):
    """the first eight rows in one call: under cuts in events only, in words only, in both, and a cut inside channel 7 between its
    AFSK and its POCSAG item (by events and by one word too few), the written prefix is the model's and both buffers keep their
    sentinels behind `written` (raw_gather asserts it); the sizing call; a repeat with another capacity gives the same prefix"""
    e = _engine(8)
    e.update(_cuda(rows()[:8]))
    events, lost = check(e, NB, "all")
    ne, nw = len(events), sum(len(p) for *_, p in events)
    offs = np.cumsum([0] + [len(p) for *_, p in events])
    full = raw_gather(e, ne, nw)
    same(full, M.cut(events, lost), "full")
    (inside,) = [k for k, (ch, kind, _, _) in enumerate(events) if ch == 7 and kind == 2]
    assert events[inside - 1][:2] == (7, 1)
    cuts = [(0, 0), (ne // 2, nw), (1, nw), (ne, int(offs[ne // 2]) + 1), (ne, 1), (ne, 0), (0, nw), (ne // 3, int(offs[ne // 2])), (inside, nw),
            (ne, int(offs[inside + 1]) - 1), (ne, int(offs[inside])), (ne - 1, nw), (ne, nw - 1), (ne + 3, nw + 3)]
    for ce, cw in cuts:
        want = M.cut(events, lost, ce, cw)
        got = raw_gather(e, ce, cw)
        same(got, want, (ce, cw))
        we, ww = want[2][1], want[2][3]
        assert np.array_equal(got[0], full[0][:we]) and np.array_equal(got[1], full[1][:ww])
        same(gather(e, ce, cw), want, ("Engine.gather_events", ce, cw))
    assert M.cut(events, lost, inside, nw)[2][1] == inside == M.cut(events, lost, ne, int(offs[inside + 1]) - 1)[2][1]
    same(raw_gather(e, ne, nw), full, "again")


def test_gpu_events_kinds_subset(rdsp):
    """engines with only DTMF, only POCSAG, and AFSK with POCSAG, nine receivers in three groups: group 0 with POCSAG at baud 0,
    group 1 at 2400, group 2 at 1200 (row 8's page).  Call 1, all NFM: the gather is the model's.  Then group 1 -- between two NFM
    groups -- goes to LSB and the same rows run again: no decoder runs on its receivers, their count words stay what call 1 left
    (the detectors' words and record buffers still hold call 1's values: its read calls patch them, the raw counts show them), and
    the gather has nothing of them while call 1's had"""
    order = [0, 2, 3, 7, 2, 3, 8, 7, 3]
    x = _cuda(rows()[order])
    for kinds in ((True, False, False), (False, False, True), (False, True, True)):
        e = _engine(9, kinds=kinds, groups=[0, 3, 6])
        if kinds[2]:
            e.select_group(0)
            e.set_pocsag(0)
            e.select_group(2)
            e.set_pocsag(1200)
            e.select_group(-1)
        e.update(x)
        first, lost = check(e, NB, (kinds, 1))
        _, count1, _ = snapshot(e, NB)
        assert kinds_of(first) == {k for k in range(3) if kinds[k]} and lost == 0
        mid = {(ch, k) for ch, k, _, _ in first if 3 <= ch < 6}
        assert mid
        if kinds[2]:
            assert not any(k == 2 and ch < 3 for ch, k, _, _ in first) and any(k == 2 and ch == 6 for ch, k, _, _ in first)
        e.select_group(1)
        e.setDemodMode(LSB)
        e.select_group(-1)
        e.update(x)
        second, _ = check(e, NB, (kinds, 2))
        new2, count2, _ = snapshot(e, NB)
        assert not any(3 <= ch < 6 for ch, *_ in second)
        for ch, k in mid:                                                     # the words still hold call 1's items; only the rows list keeps them out
            assert count2[k][ch] == count1[k][ch] > 0 and M.fresh_count(k, new2[k])[ch] == 0
        assert {ch for ch, *_ in second} <= {0, 1, 2, 6, 7, 8}
    e = _engine(2, kinds=(False, False, False))
    import torch
    cnt = torch.zeros(5, dtype=torch.int32, device="cuda")
    assert e.lib.rdsp_engine_gather_events(e.h, None, 0, None, 0, cnt.data_ptr(), None) == -4 and b"no decoder" in e.lib.rdsp_last_error()


def test_gpu_events_restart_in_the_call(rdsp):
    """a group's baud changes between two updates, so its detectors start from zeros in the next call: after a call at 2400 baud
    that read row 1's two pages, the same receiver at 1200 baud reads row 8's page -- the gather has that call's own message, seq
    0 of a count of 1 with a block stamp inside the call, not what the ring held before"""
    e = _engine(1)
    e.update(_cuda(rows()[1:2]))
    events, _ = check(e, NB, 2400)
    assert [(k, seq) for _, k, seq, _ in events if k == 2] == [(2, 0), (2, 1)]
    e.set_pocsag(1200)
    e.update(_cuda(rows()[8:9]))
    events, lost = check(e, NB, 1200)
    _, count, _ = snapshot(e, NB)
    (got,) = [v for v in e.events() if v.kind == 2]
    assert count[2][0] == 1 and got.seq == 0 and got.value.address == 24 and 0 < got.t_blocks <= NB and lost == 0


def test_gpu_events_invalidated(rdsp):
    """the counts are all 0 with no update made yet, after an update of 0 blocks, after rdsp_engine_reset and after
    rdsp_engine_load_state, each until the next update, which gathers again"""
    import torch
    x = _cuda(rows()[:3])
    e = _engine(3)
    zero = (0, 0, 0, 0, 0)
    assert gather(e)[2] == zero
    e.update(x)
    events, _ = check(e, NB, "first")
    assert len(events) >= 3
    out = torch.empty_like(x)
    assert e.lib.rdsp_engine_update(e.h, x.data_ptr(), NB * 128, 0, out.data_ptr(), NB * 128, None) == 0
    assert gather(e)[2] == zero and raw_gather(e, 4, 100)[2] == zero
    e.update(x)
    assert gather(e)[2][0] > 0
    e.reset()
    assert gather(e)[2] == zero
    e.update(x)
    assert check(e, NB, "behind the reset")[0]
    blob = e.save_state(0, 3)
    assert gather(e)[2][0] > 0                                                # saving reads only
    e.load_state(0, blob)
    assert gather(e)[2] == zero
    e.update(x)
    check(e, NB, "behind the load")


def test_gpu_events_refusals(rdsp):
    """RDSP_ERR_INVALID with nothing written: d_counts NULL, a capacity with a NULL buffer, a buffer off a 16-byte boundary, a
    capacity above INT32_MAX; RDSP_ERR_NOT_READY is test_gpu_events_kinds_subset's"""
    import torch
    e = _engine(2)
    e.update(_cuda(rows()[2:4]))
    rec = torch.full((8, 4), SENTINEL, dtype=torch.int32, device="cuda")
    wd = torch.full((400,), SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((5,), -7, dtype=torch.int32, device="cuda")
    g = lambda *a: e.lib.rdsp_engine_gather_events(e.h, *a, None)
    r, w, c = rec.data_ptr(), wd.data_ptr(), cnt.data_ptr()
    for args in ((r, 8, w, 400, None), (None, 8, w, 400, c), (r, 8, None, 400, c), (r + 4, 4, w, 400, c), (r, 8, w + 8, 300, c), (r, 2 ** 31, w, 400, c),
                 (r, 8, w, 2 ** 31, c)):
        assert g(*args) == -1 and b"rdsp_engine_gather_events" in e.lib.rdsp_last_error(), args
    torch.cuda.synchronize()
    assert (cnt == -7).all() and (rec == SENTINEL).all() and (wd == SENTINEL).all()
    assert g(r, 8, w, 400, c) == 0 and int(cnt[0]) > 0


def test_gpu_events_never_called_changes_nothing(rdsp):
    """an engine that gathers after every call against a twin that never does, five receivers under [7, 8, 9, 63]: the audio, every
    decoder's records, counts and rings and the state blob are the same bits after every call"""
    x = np.ascontiguousarray(rows()[[0, 2, 3, 7, 6]])
    a_, b_ = _engine(5), _engine(5)
    a = 0
    for k in (7, 8, 9, 63):
        d = _cuda(x[:, a * 128:(a + k) * 128])
        ya, yb = a_.update(d), b_.update(d)
        gather(a_)
        raw_gather(a_, 2, 9)
        assert np.array_equal(ya.cpu().numpy(), yb.cpu().numpy())
        for kind_a, kind_b in zip(zip(*snapshot(a_, k)), zip(*snapshot(b_, k))):
            for va, vb in zip(kind_a, kind_b):
                assert np.array_equal(va, vb)
        for fa, fb in ((a_.read_dtmf, b_.read_dtmf), (a_.read_afsk, b_.read_afsk), (a_.read_pocsag, b_.read_pocsag)):
            for va, vb in zip(fa(k), fb(k)):
                assert np.array_equal(va.cpu().numpy().view(np.uint8), vb.cpu().numpy().view(np.uint8))
        assert np.array_equal(a_.save_state(0, 5), b_.save_state(0, 5))
        a += k


def test_gpu_events_on_a_callers_stream(rdsp):
    """update and gather on a non-blocking stream: the raw call's counts are read after the stream's synchronise, and
    Engine.gather_events, which waits itself, gives the model's sequence"""
    import torch
    x = _cuda(rows()[:8])
    e = _engine(8)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        e.update(x, stream=s)
        cnt = torch.full((5,), -7, dtype=torch.int32, device="cuda")
        rec = torch.zeros((64, 4), dtype=torch.int32, device="cuda")
        wd = torch.zeros((2048,), dtype=torch.int32, device="cuda")
        assert e.lib.rdsp_engine_gather_events(e.h, rec.data_ptr(), 64, wd.data_ptr(), 2048, cnt.data_ptr(), C.c_void_p(s.cuda_stream)) == 0
        s.synchronize()
        counts = tuple(cnt.tolist())
        got = gather(e, stream=s)
    snap = snapshot(e, NB)
    want = M.gather(*snap)
    same(got, want, "stream")
    assert counts == want[2]
    assert np.array_equal(rec.cpu().numpy()[:counts[1]].view(U32), want[0]) and np.array_equal(wd.cpu().numpy()[:counts[3]].view(U32), want[1])
