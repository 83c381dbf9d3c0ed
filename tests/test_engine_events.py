"""rdsp_engine_gather_events without a GPU (include/rdsp.h "Decoder events"; csrc/rdsp_events.h, csrc/rdsp_engine_events_host.hip):
the exports, the refusals that need no device, tests/engine_events_model.py against the library's rdsp_events_reference bit for
bit on drawn synthetic states, the prefix rule under every pair of capacities, events.parse against what read_afsk_frames and
read_pocsag_messages make of the same rings, and tests/host/host_events_check.cpp -- csrc/rdsp_events.h as a program of its own,
plain and under ASan + UBSan, run directly.  tests/test_engine_events_gpu.py holds the kernels to the same model."""
import ctypes as C
import itertools
import os
import subprocess

import numpy as np
import pytest

import engine_events_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
U32 = np.uint32
SENTINEL = 0xDEADBEEF
AFSK_LENS = (0, 1, 3, 4, 5, 328)
POCSAG_NCW = (0, 80)


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def reference(lib, new, states, n_channels, n_blocks, ce, cw, tail=3):
    """rdsp_events_reference into buffers with `tail` sentinel entries behind the capacities -> (records, words, counts, rc); the
    sentinels behind `written` are asserted here"""
    new = [None if v is None else np.ascontiguousarray(v, np.uint8) for v in new]
    stride = max([v.shape[1] for v in new if v is not None] + [n_blocks])
    records = np.full((ce + tail, 4), SENTINEL, U32)
    words = np.full(cw + tail, SENTINEL, U32)
    counts = np.full(5, -7, np.int32)
    rc = lib.rdsp_events_reference(_ptr(new[0]), _ptr(new[1]), _ptr(new[2]), stride, _ptr(states[0]), _ptr(states[1]), _ptr(states[2]), n_channels,
                                   n_blocks, _ptr(records) if ce else None, ce, _ptr(words) if cw else None, cw, _ptr(counts))
    assert rc >= 0, lib.rdsp_last_error()
    we, ww = int(counts[1]), int(counts[3])
    assert (records[we:] == SENTINEL).all() and (words[ww:] == SENTINEL).all(), "written behind `written`"
    return records[:we], words[:ww], tuple(int(v) for v in counts), rc


def draw(r, n, nb, on=(True, True, True), busy=0.5):
    """a synthetic state of n channels behind a call of nb blocks: (new, count, ring) by kind, None for a kind that is off.  Per
    channel and kind c is one of 0, 1, R, R + 1, 255 (where the records can hold it) or drawn; n is c (a detector that started in
    the call), c + a drawn number, or chosen so that the items cross the ring's wrap; the slots' headers run through AFSK_LENS
    and POCSAG_NCW and drawn values, the other words are drawn"""
    new, count, ring = [], [], []
    for k in range(3):
        if not on[k]:
            new.append(None), count.append(None), ring.append(None)
            continue
        R, S = M.RING[k], M.SLOT[k]
        rec = np.full((n, nb), 255 if k == M.DTMF else 0, np.uint8)
        cnt = np.zeros(n, U32)
        rg = r.integers(0, 1 << 32, (n, R, S), dtype=np.uint64).astype(U32)
        if k == M.DTMF:
            rg = (rg & 0xFFFFFF00) | (rg & 0xF)
        elif k == M.AFSK:
            rg[:, :, 0] = r.choice(np.array(AFSK_LENS + tuple(r.integers(0, 329, 4)), U32), (n, R))
        else:
            rg[:, :, 0] = r.choice(np.array(POCSAG_NCW + tuple(r.integers(0, 81, 4)), U32), (n, R)) | (r.integers(0, 8, (n, R)).astype(U32) << 8)
        most = nb if k == M.DTMF else 255 * nb
        menu = [c for c in (1, R, R + 1, 255, int(r.integers(0, 2 * R))) if c <= most]
        for ch in np.flatnonzero(r.random(n) < busy):
            c = int(r.choice(menu))
            if k == M.DTMF:
                rec[ch, r.choice(nb, c, replace=False)] = r.integers(0, 16, c)
            else:
                left = c
                while left:
                    b, v = int(r.integers(0, nb)), min(left, int(r.integers(1, 256)))
                    if int(rec[ch, b]) + v <= 255:
                        rec[ch, b] += v
                        left -= v
            take = min(c, R)
            how = int(r.integers(0, 3))
            cnt[ch] = c if how == 0 else c + int(r.integers(0, 1000)) if how == 1 else max(c, (c // R + 1) * R + int(r.integers(0, max(take, 1))))
        new.append(rec), count.append(cnt), ring.append(rg)
    return new, count, ring


def same(got, want, where):
    assert got[2] == want[2], (where, got[2], want[2])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), where


def test_events_exports(rdsp):
    from radiodsp_sdr_rx_amd import engine, events
    lib = rdsp.load()
    assert hasattr(lib, "rdsp_engine_gather_events") and hasattr(lib, "rdsp_events_reference")
    assert callable(engine.Engine.gather_events) and callable(engine.Engine.events) and callable(events.parse)
    assert events.Event._fields == ("channel", "kind", "seq", "t_blocks", "value")
    assert events.Counts._fields == ("needed_events", "written_events", "needed_words", "written_words", "lost")
    assert (events.DTMF, events.AFSK, events.POCSAG) == (M.DTMF, M.AFSK, M.POCSAG) == (0, 1, 2)


def test_events_refusals_without_a_device(rdsp):
    """no object: rdsp_engine_gather_events refuses.  rdsp_events_reference refuses, with nothing written: counts NULL, a capacity
    with a NULL buffer, a capacity above INT32_MAX, n_channels x 688 above INT32_MAX, a negative n_blocks, a stride below
    n_blocks.  The refusals that need an object are test_engine_events_gpu's"""
    lib = rdsp.load()
    cnt = np.full(5, -7, np.int32)
    assert lib.rdsp_engine_gather_events(None, None, 0, None, 0, _ptr(cnt), None) == -1
    rec, wd = np.full((4, 4), SENTINEL, U32), np.full(8, SENTINEL, U32)
    new, state = np.zeros((1, 4), np.uint8), np.zeros((1, 448), U32)
    ok = lambda *a: lib.rdsp_events_reference(None, _ptr(new), None, 4, None, _ptr(state), None, *a)
    assert ok(1, 4, _ptr(rec), 4, _ptr(wd), 8, _ptr(cnt)) == 0 and list(cnt) == [0] * 5
    cnt[:] = -7
    for args in ((1, 4, _ptr(rec), 4, _ptr(wd), 8, None), (1, 4, None, 4, _ptr(wd), 8, _ptr(cnt)), (1, 4, _ptr(rec), 4, None, 8, _ptr(cnt)),
                 (1, 4, _ptr(rec), 2 ** 31, _ptr(wd), 8, _ptr(cnt)), (1, 4, _ptr(rec), 4, _ptr(wd), 2 ** 31, _ptr(cnt)),
                 ((2 ** 31 - 1) // 688 + 1, 4, _ptr(rec), 4, _ptr(wd), 8, _ptr(cnt)), (-1, 4, _ptr(rec), 4, _ptr(wd), 8, _ptr(cnt)),
                 (1, -1, _ptr(rec), 4, _ptr(wd), 8, _ptr(cnt)), (1, 5, _ptr(rec), 4, _ptr(wd), 8, _ptr(cnt))):
        assert ok(*args) == -1 and b"rdsp_events_reference" in lib.rdsp_last_error(), args
    assert (cnt == -7).all() and (rec == SENTINEL).all() and (wd == SENTINEL).all()
    assert ok(1, 4, None, 0, None, 0, _ptr(cnt)) == 0 and list(cnt) == [0] * 5    # the sizing call


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 2049])
def test_events_model_is_the_reference(rdsp, n):
    """drawn states of 1 to 2049 channels (draw: c of 0, 1, R, R + 1 and 255 per kind, n = c and counts across the wrap, every
    AFSK length of 0, 1, 3, 4, 5 and 328, POCSAG n_cw of 0 and 80), each under all eight combinations of kinds: the model's
    records, words and counts are rdsp_events_reference's, at the needed capacity and from a sizing call"""
    lib = rdsp.load()
    r = np.random.default_rng(5100 + n)
    nb = 256 if n <= 5 else 9
    seen = {k: set() for k in range(3)}
    wrapped = set()
    for on in itertools.product((False, True), repeat=3):
        for rep in range(6 if n <= 5 else 1):
            new, count, ring = draw(r, n, nb, on, 0.9 if n <= 5 else 0.05)
            events, lost = M.sequence(new, count, ring)
            want = M.cut(events, lost)
            st = M.states(count, ring)
            ne, nw = want[2][0], want[2][2]
            got = reference(lib, new, st, n, nb, ne, nw)
            assert got[3] == 0
            same(got, want, (n, on, rep))
            sizing = reference(lib, new, st, n, nb, 0, 0)
            assert sizing[2] == (ne, 0, nw, 0, want[2][4])
            assert want[2][4] == sum(max(0, int(c) - M.RING[k]) for k in range(3) if on[k] for c in M.fresh_count(k, new[k]))
            for k in range(3):
                if on[k]:
                    c, cn = M.fresh_count(k, new[k]), count[k].astype(np.int64)
                    seen[k] |= set(int(v) for v in c)
                    take = np.minimum(c, M.RING[k])
                    if ((take > 0) & (cn % M.RING[k] < take) & (cn % M.RING[k] > 0)).any():
                        wrapped.add(k)
                    if (c > 0).any() and (c == cn)[c > 0].any():
                        wrapped.add(("started", k))
            if not any(on):
                assert want[2] == (0, 0, 0, 0, 0)
    if n <= 5:
        for k in range(3):
            assert {0, 1, M.RING[k], M.RING[k] + 1, 255} <= seen[k], (k, sorted(seen[k]))
            assert k in wrapped and ("started", k) in wrapped, (k, wrapped)


def test_events_lengths(rdsp):
    """one channel with a full AFSK and a full POCSAG ring under every length named: n_words is 2 + ceil(len / 4) and 4 + n_cw, the
    payload is the slot's first n_words words"""
    lib = rdsp.load()
    r = np.random.default_rng(77)
    for lens, ncw in ((AFSK_LENS[:4], (0, 80, 1, 79)), (AFSK_LENS[2:], (80, 0, 80, 0))):
        new = [None, np.full((1, 1), 4, np.uint8), np.full((1, 1), 4, np.uint8)]
        ring = [None] + [r.integers(0, 1 << 32, (1, 4, 84), dtype=np.uint64).astype(U32) for _ in range(2)]
        ring[1][0, :, 0], ring[2][0, :, 0] = lens, np.array(ncw, U32) | 0x10200
        count = [None, np.array([8], U32), np.array([4], U32)]
        want = M.gather(new, count, ring)
        assert [int(v) >> 8 for v in want[0][:, 1]] == [2 + (v + 3) // 4 for v in lens] + [4 + v for v in ncw]
        got = reference(lib, new, M.states(count, ring), 1, 1, want[2][0], want[2][2])
        same(got, want, lens)
        at = 0
        for k, s in [(1, s) for s in range(4)] + [(2, s) for s in range(4)]:
            nw = M.n_words(k, ring[k][0, s, 0])
            assert np.array_equal(got[1][at:at + nw], ring[k][0, s, :nw])
            at += nw


def test_events_prefix_rule(rdsp):
    """a drawn case of about a dozen events of all three kinds over five channels: every capacity_events in 0 ... needed + 1 with
    every capacity_words in 0 ... needed_words + 1 -- the written prefix is the model's and every word and record behind
    `written` keeps its sentinel (reference() asserts it)"""
    lib = rdsp.load()
    r = np.random.default_rng(12)
    while True:
        new, count, ring = draw(r, 5, 6, busy=0.45)
        for k in (1, 2):
            ring[k][:, :, 0] = np.minimum(ring[k][:, :, 0] & 0xFF, 30) | (ring[k][:, :, 0] & 0xFF00 if k == 2 else 0)   # short payloads: a small product
        events, lost = M.sequence(new, count, ring)
        if 10 <= len(events) <= 14 and {k for _, k, _, _ in events} == {0, 1, 2} and sum(len(p) for *_, p in events) < 200:
            break
    st = M.states(count, ring)
    ne, nw = len(events), sum(len(p) for *_, p in events)
    seen = set()
    for ce in range(ne + 2):
        for cw in range(nw + 2):
            want = M.cut(events, lost, ce, cw)
            got = reference(lib, new, st, 5, 6, ce, cw)
            same(got, want, (ce, cw))
            seen.add(want[2][1])
    assert seen == set(range(ne + 1))


def test_events_parse_reads_the_rings(rdsp):
    """events.parse on a gathered sequence gives, per channel, what read_afsk_frames and read_pocsag_messages make of the same
    rings (their loops restated on numpy arrays) for the items gathered, and the keys of the DTMF ring words"""
    from radiodsp_sdr_rx_amd import events, pocsag
    r = np.random.default_rng(31)
    new, count, ring = draw(r, 40, 12, busy=0.6)
    rec, words, counts = M.gather(new, count, ring)
    got = events.parse(rec.view(np.int32), words.view(np.int32))
    assert len(got) == counts[0] > 30 and {e.kind for e in got} == {0, 1, 2}
    frames, msgs = {}, {}
    for c in range(40):                                                       # Engine.read_afsk_frames / read_pocsag_messages, restated
        n = int(count[1][c])
        for k in range(max(0, n - 4), n):
            slot = ring[1][c, k % 4]
            frames[c, k] = (int(slot[1]), slot[2:].astype("<u4").tobytes()[:int(slot[0])])
        n = int(count[2][c])
        for k in range(max(0, n - 4), n):
            msgs[c, k] = pocsag.from_slot(ring[2][c, k % 4])
    for e, (ch, kw, seq, off) in zip(got, rec.tolist()):
        assert (e.channel, e.kind, e.seq) == (ch, kw & 0xFF, seq)
        if e.kind == events.AFSK:
            assert (e.t_blocks, e.value) == frames[ch, seq]
        elif e.kind == events.POCSAG:
            assert e.value == msgs[ch, seq] and e.t_blocks == msgs[ch, seq].t_blocks
        else:
            w = int(ring[0][ch, seq % 16, 0])
            assert e.value == events.DTMF_KEYS[w & 0xF] and e.t_blocks == w >> 8
    with pytest.raises(ValueError):
        events.parse(rec[:1], words[:0])


@pytest.mark.parametrize("sanitize", [False, True])
def test_events_host_program(rdsp, tmp_path, sanitize):
    """tests/host/host_events_check.cpp, plain and under ASan + UBSan, a program of its own run on the CPU: its own cases (states
    whose c exceeds n -- the clamp --, capacities 0, the largest slot lengths and lengths above them), then drawn states of 5 and
    1025 channels at the needed capacities, cut in events and cut in words, whose output is the model's"""
    exe = str(tmp_path / ("host_events_check_san" if sanitize else "host_events_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_events_check.cpp"), "-o", exe])
    fin, fout = str(tmp_path / "state.bin"), str(tmp_path / "out.bin")
    r = np.random.default_rng(99)
    for n, nb, on in ((5, 256, (True, True, True)), (1025, 9, (True, True, True)), (5, 20, (False, True, True)), (5, 20, (True, False, False))):
        new, count, ring = draw(r, n, nb, on, 0.9 if n == 5 else 0.05)
        events, lost = M.sequence(new, count, ring)
        ne, nw = len(events), sum(len(p) for *_, p in events)
        st = M.states(count, ring)
        with open(fin, "wb") as f:
            for k in range(3):
                f.write((new[k] if on[k] else np.zeros((n, nb), np.uint8)).tobytes())
            for k in range(3):
                f.write((st[k] if on[k] else np.zeros((n, M.WORDS[k]), U32)).tobytes())
        kinds = sum(1 << k for k in range(3) if on[k])
        for ce, cw in ((ne, nw), (ne // 2, nw), (ne, nw // 2), (0, 0)):
            out = subprocess.run([exe, fin, fout, str(n), str(nb), str(ce), str(cw), str(kinds)], capture_output=True, text=True, timeout=600)
            assert out.returncode == 0 and out.stdout.endswith("host_events_check OK\n"), out.stdout + out.stderr
            assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
            w = np.fromfile(fout, U32)
            want = M.cut(events, lost, ce, cw)
            assert tuple(int(v) for v in w[:5]) == want[2] and w[5] == 0, (n, ce, cw)
            we, ww = want[2][1], want[2][3]
            assert np.array_equal(w[6:6 + 4 * we].reshape(-1, 4), want[0]) and np.array_equal(w[6 + 4 * we:], want[1]) and len(w) == 6 + 4 * we + ww
    assert subprocess.run([exe], capture_output=True, text=True).stdout == "host_events_check OK\n"
    assert subprocess.run([exe, fin, fout, "0", "1", "1", "1", "7"], capture_output=True).returncode == 2
