"""Voice-rate audio of rdsp_engine_t (include/rdsp.h "voice-rate audio"; csrc/rdsp_voice.h, csrc/rdsp_engine_voice.hip,
csrc/rdsp_engine_voice_host.hip): the left words of every receiver's output row, behind the gate, low-passed and decimated by
R = 2 or 4 on the device.  Every comparison is exact.

`-m "not gpu"`: rdsp_engine_voice_taps against tests/engine_voice_model.py and the filter figures of the definition;
tests/host/host_voice_check.cpp -- csrc/rdsp_voice.h as a program of its own, plain and under ASan + UBSan, run directly --
against the model on crafted rows (the clamps, the tie and the floor on both sides of zero, the history hand-over at every call
length from 1 to 3 blocks); the model against a float64 convolution; the exports; the refusals of the host-only call.
`-m gpu`: the engine's voice rows against the model applied to the left words the call returned; the pack of those rows
against the model's pack on the gates rdsp_engine_read_meter returns; history through regroupings, resets and state blobs;
the refusals."""
import functools
import os
import subprocess

import numpy as np
import pytest

import engine_pack_model as P
import engine_voice_model as V
from test_engine_meter import _bursts, _engine, _on_sources
from test_engine_pack import _between, _call, _cuda, _grouped, _twelve

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RATES = (2, 4)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def _response_db(q, R):
    """(largest pass-band deviation from 0 dB on |f| <= 0.544 fs / (2 R), stop-band attenuation from 1.456 fs / (2 R) on), dB"""
    n = 1 << 16
    h = np.abs(np.fft.rfft(q.astype(np.float64) / 262144.0, n))
    f = np.arange(len(h)) * 44100.0 / n
    nyq = 44100.0 / (2 * R)
    return np.abs(20 * np.log10(h[f <= 0.544 * nyq])).max(), -20 * np.log10(h[f >= 1.456 * nyq].max())


@pytest.mark.parametrize("R", RATES)
def test_voice_taps(rdsp, R):
    """rdsp_engine_voice_taps equals the model bit for bit and is symmetric; sum q - 2^18 is 0 (R = 2) and 2 (R = 4), sum |q| /
    2^18 is 1.649 and 1.603; the family's limits hold: ripple <= 0.001 dB on |f| <= 0.544 fs / (2 R) (6 000 / 3 000 Hz), at least
    90 dB down from 1.456 fs / (2 R) (16 050 / 8 025 Hz) to 22 050 Hz.  The measured figures are printed."""
    from radiodsp_sdr_rx_amd.engine import ddc_taps, voice_taps
    q = voice_taps(R)
    assert q.dtype == np.int32 and q.shape == (16 * R,)
    assert np.array_equal(q, V.taps(R)) and np.array_equal(q, q[::-1])
    assert np.array_equal(q, np.rint(ddc_taps(R).astype(np.float64) * 262144.0).astype(np.int32))
    total, absolute = int(q.astype(np.int64).sum()), float(np.abs(q.astype(np.int64)).sum()) / 262144.0
    ripple, stop = _response_db(q, R)
    print(f"voice taps R = {R}: sum q - 2^18 = {total - 262144}, sum |q| / 2^18 = {absolute:.4f}, ripple {ripple:.5f} dB, stop band {stop:.2f} dB")
    assert total - 262144 == {2: 0, 4: 2}[R]
    assert abs(absolute - {2: 1.649, 4: 1.603}[R]) < 0.0006
    assert ripple <= 0.001 and stop >= 90.0
    assert 32767 * np.abs(q.astype(np.int64)).sum() + 32768 < 2 ** 34                    # |acc| < 2^34


def test_voice_taps_refusals(rdsp):
    import ctypes as C
    from radiodsp_sdr_rx_amd.engine import voice_taps
    lib = rdsp.load()
    buf = (C.c_int32 * 64)(*([77] * 64))
    for R in (0, 1, 3, 5, 8, -2):
        assert lib.rdsp_engine_voice_taps(R, buf) == -1 and b"rdsp_engine_voice_taps" in lib.rdsp_last_error(), R
        with pytest.raises(rdsp.RdspError):
            voice_taps(R)
    assert lib.rdsp_engine_voice_taps(2, None) == -1 and list(buf) == [77] * 64
    assert lib.rdsp_engine_voice_taps(4, buf) == 0 and list(buf) == V.taps(4).tolist()


def test_voice_exports(rdsp):
    from radiodsp_sdr_rx_amd import engine
    lib = rdsp.load()
    for name in ("voice_taps", "enable_voice", "voice_rate", "read_voice", "pack_voice"):
        assert hasattr(lib, "rdsp_engine_" + name), name
    assert callable(engine.voice_taps) and all(callable(getattr(engine.Engine, n)) for n in ("enable_voice", "read_voice", "pack_voice"))
    assert isinstance(engine.Engine.voice_rate, property)


def _convolved(left, R):
    """a fresh channel's voice rows by a float64 convolution, floor(acc / 2^18 + 1 / 2) and a clamp: every product and sum is
    an integer below 2^53, so the doubles are exact"""
    q = V.taps(R).astype(np.float64)
    out = []
    for row in left:
        full = np.convolve(row.astype(np.float64), q)[:len(row)]                          # full[n] = sum_k q_k x[n - k]
        out.append(np.clip(np.floor(full[R - 1::R] / 262144.0 + 0.5), -32768, 32767))
    return np.array(out).astype(np.int16)


@pytest.mark.parametrize("R", RATES)
def test_voice_model_is_the_convolution(R):
    """the model on drawn rows -- full-range words, small words around the ties, a row in three calls -- equals the float64
    convolution followed by floor and clamp"""
    r = np.random.default_rng(5 + R)
    left = np.concatenate([r.integers(-32768, 32768, (6, 5 * 128)), r.integers(-3, 4, (3, 5 * 128))]).astype(np.int16)
    want = _convolved(left, R)
    assert np.array_equal(V.Voice(len(left), R).run(left), want)
    m = V.Voice(len(left), R)
    got = np.concatenate([m.run(left[:, :128]), m.run(left[:, 128:384]), m.run(left[:, 384:])], 1)
    assert np.array_equal(got, want) and np.array_equal(m.hist, left[:, -60:])
    assert (want[:6] == 32767).any() or np.abs(want[:6]).max() > 20000


def _solve_tie(q, x, target_mod):
    """change the window x (int64 [T], x[k] multiplies q[k]) a little so that sum q x = target_mod (mod 2^18): the large taps
    take the residue down greedily, the three outermost taps (small, coprime) finish it exactly by search"""
    x = x.copy()
    mod = 1 << 18

    def res():
        r = (target_mod - int((q * x).sum())) % mod
        return r - mod if r > mod // 2 else r
    for k in np.argsort(-np.abs(q)):
        if abs(q[k]) < 100:
            break
        d = int(np.clip(round(res() / int(q[k])), -2000, 2000))
        x[k] += d
    d = np.arange(-60, 61)
    d0, d1, d2 = np.meshgrid(d, d, d, indexing="ij")
    hit = np.argwhere((d0 * int(q[0]) + d1 * int(q[1]) + d2 * int(q[2]) - res()) % mod == 0)
    assert len(hit), "no exact solution in the search range"
    best = hit[np.abs(d[hit]).sum(1).argmin()]
    x[:3] += d[best]
    assert (int((q * x).sum()) - target_mod) % mod == 0 and np.abs(x).max() <= 32767
    return x


@functools.lru_cache(maxsize=None)
def _crafted(R):
    """int16 [rows, 6 * 128]: all +32767, all -32768, 32767 sign(q) and its negative in the window of one output (the model
    must saturate on both sides), windows searched so that acc = 2^17 (mod 2^18) with acc positive and with acc negative (the tie
    and the floor), drawn full-range rows -> (rows, {name: (row, output index)})"""
    q = V.taps(R).astype(np.int64)
    T, n = 16 * R, 6 * 128
    r = np.random.default_rng(40 + R)
    rows, at = [], {}

    def window_row(name, w, m):                                                           # x[R m + R - 1 - k] = w[k]
        row = np.zeros(n, np.int64)
        row[R * m + R - 1 - np.arange(T)] = w
        at[name] = (len(rows), m)
        rows.append(row)
    rows.append(np.full(n, 32767, np.int64))
    rows.append(np.full(n, -32768, np.int64))
    sign = np.where(q >= 0, 1, -1)
    window_row("sat_hi", 32767 * sign, 100)
    window_row("sat_lo", -32767 * sign, 101)
    big = np.abs(q) > 20000
    window_row("tie_pos", _solve_tie(q, r.integers(-300, 301, T) + 9000 * big, 1 << 17), 77)
    window_row("tie_neg", _solve_tie(q, r.integers(-300, 301, T) - 9000 * big, 1 << 17), 90)
    least = np.zeros(T, np.int64)                                                         # acc = -2^17 exactly: -0.5 goes up to 0
    least[np.abs(q).argmax()] = round(-(1 << 17) / int(q.max()))
    window_row("tie_small_neg", _solve_tie(q, least, 1 << 17), 133)
    for _ in range(3):
        rows.append(r.integers(-32768, 32768, n))
    return np.array(rows).astype(np.int16), at


@pytest.mark.parametrize("sanitize", [False, True])
def test_voice_host_program(tmp_path, sanitize):
    """tests/host/host_voice_check.cpp, plain and under ASan + UBSan, a program of its own run on the CPU: on the crafted rows,
    for R = 2 and 4 and calls of 1, 2 and 3 blocks, its taps, outputs and final histories equal the model's; the crafted rows
    do what they were made for -- both clamps reached, acc on the tie with either sign"""
    exe = str(tmp_path / ("host_voice_check_san" if sanitize else "host_voice_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_voice_check.cpp"), "-o", exe])
    for R in RATES:
        rows, at = _crafted(R)
        n, t = rows.shape
        q = V.taps(R).astype(np.int64)
        want = V.Voice(n, R).run(rows)
        x = np.concatenate([np.zeros((n, V.HIST), np.int64), rows.astype(np.int64)], 1)
        acc = V.accumulate(x, R)
        assert np.all(want[0, 16:] == 32767) and np.all(want[1, 16:] == -32768)
        assert want[at["sat_hi"]] == 32767 and acc[at["sat_hi"]] == 32767 * np.abs(q).sum() > 32767 * 2 ** 18 + 2 ** 17
        assert want[at["sat_lo"]] == -32768 and acc[at["sat_lo"]] == -32767 * np.abs(q).sum() < -32768 * 2 ** 18 - 2 ** 17
        for name, sign in (("tie_pos", 1), ("tie_neg", -1), ("tie_small_neg", -1)):
            a = int(acc[at[name]])
            assert a % (1 << 18) == (1 << 17) and np.sign(a) == sign, (name, a)
            assert int(want[at[name]]) == (a + (1 << 17)) // (1 << 18) == (a - (1 << 17)) // (1 << 18) + 1, name   # the tie goes up
        assert int(acc[at["tie_small_neg"]]) == -(1 << 17) and int(want[at["tie_small_neg"]]) == 0
        fin, fout = str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")
        rows.tofile(fin)
        for call_blocks in (1, 2, 3, 6):
            out = subprocess.run([exe, fin, fout, str(R), str(n), str(t // 128), str(call_blocks)], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0 and out.stdout.endswith("host_voice_check OK\n"), out.stdout + out.stderr
            assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
            w = np.fromfile(fout, np.int32)
            assert np.array_equal(w[:16 * R], q)
            assert np.array_equal(w[16 * R:16 * R + n * (t // R)].reshape(n, t // R), want), (R, call_blocks)
            assert np.array_equal(w[16 * R + n * (t // R):].reshape(n, V.HIST), rows[:, -V.HIST:]), (R, call_blocks)
    assert subprocess.run([exe, fin, fout, "3", "1", "1", "1"], capture_output=True).returncode == 2


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _voice_engine(R, n, max_blocks, meter=True):
    e = _engine(n, max_blocks, meter)
    e.enable_voice(R)
    assert e.voice_rate == R
    return e


def _play(eng, model, x, cuts):
    """x int16 [n, t, 2] through eng in calls of `cuts` blocks; after every call read_voice equals the model on the left words
    the call returned -> (left words [n, t], voice rows [n, t / R])"""
    left, voice, a = [], [], 0
    for nb in cuts:
        y = eng.update(_cuda(x[:, a * 128:(a + nb) * 128])).cpu().numpy()
        assert np.array_equal(y[..., 0], y[..., 1])
        got = eng.read_voice().cpu().numpy()
        want = model.run(y[..., 0])
        assert got.shape == want.shape and np.array_equal(got, want), (cuts, a)
        left.append(y[..., 0]); voice.append(got)
        a += nb
    return np.concatenate(left, 1), np.concatenate(voice, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 5, 97])
@pytest.mark.parametrize("R", RATES)
def test_gpu_voice_rows_are_the_model(rdsp, R, n):
    """1, 5 and 97 channels (the ragged last workgroup): 3 blocks as [3], [1, 2] and [1, 1, 1] -- a one-block call at R = 4 fills
    half a trip and renews the history from 128 samples -- with a reset between them, after which the outputs equal the fresh
    engine's; then 9 blocks in one call (a row spans several trips), whose first 3 blocks are the same again"""
    x = _bursts(70 + n, n, 9)
    eng = _voice_engine(R, n, 9)
    model = V.Voice(n, R)
    seen = []
    for cuts in ([3], [1, 2], [1, 1, 1], [9]):
        seen.append(_play(eng, model, x, cuts))
        eng.reset()
        model.reset()
    assert all(voice.any() for _, voice in seen)                                               # not zeros against zeros
    for left, voice in seen[1:]:
        assert np.array_equal(left[:, :3 * 128], seen[0][0]) and np.array_equal(voice[:, :3 * 128 // R], seen[0][1])
    assert np.array_equal(seen[3][1], V.Voice(n, R).run(seen[3][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("R", RATES)
def test_gpu_voice_many_channels(rdsp, R):
    """300 channels x 2 blocks, then one more block: 75 workgroups, every channel against the model"""
    base = _bursts(81, 48, 3)
    x = np.tile(base, (7, 1, 1))[:300]
    x[48:] = np.roll(x[48:], 17, 1)
    eng = _voice_engine(R, 300, 2)
    _, voice = _play(eng, V.Voice(300, R), x, [2, 1])
    assert voice.any(1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("R", RATES)
def test_gpu_voice_unaligned_rows(rdsp, R):
    """update writes into rows 3 x 128 + 2 pairs apart that start at an odd pair (4-byte loads), in calls of 1 and 2 blocks; and
    into 16-byte aligned rows whose stride is no multiple of four pairs: the voice rows equal the model on the words written,
    and the aligned run's"""
    import torch
    n = 97
    x = _bursts(90, n, 3)
    eng = _voice_engine(R, n, 3)
    _, want = _play(eng, V.Voice(n, R), x, [1, 2])
    stride = 3 * 128 + 2
    for offset in (4, 0):
        eng.reset()
        model = V.Voice(n, R)
        buf = torch.full((n * stride + 1, 2), 7, dtype=torch.int16, device="cuda")
        ptr = buf.data_ptr() + offset
        assert (ptr % 16 != 0) == (offset == 4) and stride % 4 != 0
        got = []
        for a, nb in ((0, 1), (1, 2)):
            d = _cuda(x[:, a * 128:(a + nb) * 128])
            assert eng.lib.rdsp_engine_update(eng.h, d.data_ptr(), nb * 128, nb, ptr, stride, None) == 0
            rows = buf.reshape(-1)[offset // 2:offset // 2 + n * stride * 2].view(n, stride, 2)[:, :nb * 128].cpu().numpy()
            w = nb * 128 // R
            out = torch.full((n, w + 3), 99, dtype=torch.int16, device="cuda")                 # a destination stride of its own
            assert eng.lib.rdsp_engine_read_voice(eng.h, nb, out.data_ptr(), w + 3, None) == 0
            out = out.cpu().numpy()
            assert np.array_equal(out[:, :w], model.run(rows[..., 0])) and np.all(out[:, w:] == 99)
            got.append(out[:, :w])
        assert np.array_equal(np.concatenate(got, 1), want)


@pytest.mark.gpu
@pytest.mark.parametrize("R", RATES)
def test_gpu_voice_full_range_words(rdsp, R):
    """the settings of fixture case wrap_agc_off (AGC off, output gain past full scale: the engine's store wraps), so the words
    the stage reads spread over the whole int16 range -- asserted: magnitudes above 30 000, both signs -- in calls of 1, 2 and 3
    blocks"""
    import json
    kat = np.load(os.path.join(HERE, "golden", "engine_kat.npz"))
    iq = kat["wrap_agc_off_iq"][:6 * 128]
    x = np.stack([iq, iq[::-1].copy(), -iq, (iq * 0.9).astype(np.int16), np.roll(iq, 50, 0)])
    eng = _voice_engine(R, 5, 6)
    for c in json.loads(str(kat["wrap_agc_off_calls"])):
        assert c[0] == 0
        getattr(eng, c[1])(*c[2:])
    left, voice = _play(eng, V.Voice(5, R), x, [1, 2, 3])
    assert (left > 30000).any() and (left < -30000).any()
    assert np.abs(np.diff(left[0].astype(np.int32))).max() > 40000                             # a wrapped store
    assert voice.any(1).all()


def _is_voice_pack(eng, voice, gate, R, **kw):
    a, r, needed = eng.pack_voice(**kw)
    cap = kw.get("capacity")
    nb = kw.get("n_blocks")
    if nb is not None:
        voice, gate = voice[:, :nb * 128 // R], gate[:, :nb]
    want = V.pack(voice, gate, R, cap)
    a, r = a.cpu().numpy(), r.cpu().numpy()
    assert needed == want[2] and a.shape == want[0].shape and r.shape == want[1].shape
    assert np.array_equal(r, want[1]) and np.array_equal(a, want[0])
    return a, r


@pytest.mark.gpu
@pytest.mark.parametrize("R", RATES)
def test_gpu_voice_squelch_and_pack(rdsp, R):
    """97 channels x 12 blocks of keyed tones in three groups (open, never open, a squelch between the loud and quiet levels), in
    calls of 5 and 7 blocks: closed blocks enter as zeros, the block behind an opening gate carries the zeros' memory (it differs
    from the ungated engine's), pack_voice equals the model's pack on read_meter's gates for capacity None, 0, needed - 1 and
    needed + 5 with the sentinels behind `written` untouched, the sizing call returns the counts, a repeated call gives the same
    bytes, n_blocks below the call's works, pack_runs on the records agrees with the model; with the squelch off the pack is
    the voice rows themselves"""
    import torch
    from radiodsp_sdr_rx_amd.engine import pack_runs
    x, s = _twelve()
    n, w = x.shape[0], 128 // R
    free = _voice_engine(R, n, 12)
    free.set_meter(1.0, 1.0)
    y, free_left, gate = _call(free, x)
    free_voice = free.read_voice().cpu().numpy()
    assert gate.all() and np.array_equal(free_voice, V.Voice(n, R).run(free_left))
    a, r = _is_voice_pack(free, free_voice, gate, R)
    assert np.array_equal(a.reshape(n, 12 * w), free_voice)                                    # squelch off: the voice rows themselves
    eng = _grouped(n, 12, [0, 10, 20], ["open", "closed", "bursts"], s)
    eng.enable_voice(R)
    model = V.Voice(n, R)
    lefts, voices, gates = [], [], []
    for lo, hi in ((0, 5), (5, 12)):
        y, left, g = _call(eng, x[:, lo * 128:hi * 128])
        v = eng.read_voice().cpu().numpy()
        assert np.array_equal(v, model.run(left))
        assert not left.reshape(n, hi - lo, 128)[g == 0].any() and not v.reshape(n, hi - lo, w)[g == 0][:, 16:].any()
        lefts.append(left); voices.append(v); gates.append(g)
    left, voice, gate_all = np.concatenate(lefts, 1), np.concatenate(voices, 1), np.concatenate(gates, 1)
    opening = np.argwhere((gate_all[:, 1:] == 1) & (gate_all[:, :-1] == 0)) + [0, 1]
    assert len(opening) >= 5
    head = np.array([voice.reshape(n, 12, w)[c, b, :4] for c, b in opening])
    assert (head != np.array([free_voice.reshape(n, 12, w)[c, b, :4] for c, b in opening])).any(1).sum() >= len(opening) // 2
    assert np.array_equal(left.reshape(n, 12, 128)[gate_all == 1], free_left.reshape(n, 12, 128)[gate_all == 1])
    v, g = voices[1], gates[1]                                                                  # the last call: 7 blocks
    blocks, rec, needed = V.pack(v, g, R)
    assert needed > 8 and 0 < g.mean() < 1
    cnt = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    assert eng.lib.rdsp_engine_pack_voice(eng.h, 7, None, None, 0, cnt.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [needed, 0]
    for cap in (None, 0, needed - 1, needed + 5):
        _is_voice_pack(eng, v, g, R, capacity=cap)
        if cap:
            a = torch.full((needed + 8, w), -21846, dtype=torch.int16, device="cuda")
            r = torch.full((needed + 8, 2), -7, dtype=torch.int32, device="cuda")
            assert eng.lib.rdsp_engine_pack_voice(eng.h, 7, a.data_ptr(), r.data_ptr(), cap, cnt.data_ptr(), None) == 0
            torch.cuda.synchronize()
            k = min(needed, cap)
            assert cnt.tolist() == [needed, k]
            a, r = a.cpu().numpy(), r.cpu().numpy()
            assert np.array_equal(a[:k], blocks[:k]) and np.array_equal(r[:k], rec[:k]) and np.all(a[k:] == -21846) and np.all(r[k:] == -7), cap
    one, two = _is_voice_pack(eng, v, g, R), _is_voice_pack(eng, v, g, R)
    assert one[0].tobytes() == two[0].tobytes() and one[1].tobytes() == two[1].tobytes()
    part = _is_voice_pack(eng, v, g, R, n_blocks=3)
    assert 0 < len(part[0]) < needed
    assert np.array_equal(pack_runs(one[1], 5), P.runs(rec, 5))
    a, r, need0 = eng.pack_voice(n_blocks=0)
    assert need0 == 0 and len(a) == 0 and len(r) == 0


@pytest.mark.gpu
def test_gpu_voice_on_the_sources_path(rdsp):
    """two int16 sources at D = 4, twelve receivers on keyed stations, the squelch between their levels, R = 4: behind
    update_sources the voice rows are the model's on that call's audio, and the pack the model's on its gates"""
    nb, D, R = 12, 4, 4
    stations = -33000.0 + 6000.0 * np.arange(12)
    source_of = [c % 2 for c in range(12)]
    src = _on_sources(_bursts(27, 12, nb, quiet=(2, 3)), stations, source_of, D)
    eng = _voice_engine(R, 12, nb)
    eng.set_meter(1.0, 1.0)
    eng.set_sources(2, source_of)
    eng.set_source_decimation(D)
    eng.tune(0, stations)
    eng.update_sources(_cuda(src))
    s = _between(eng.read_meter(nb)[0].cpu().numpy())
    eng.reset()
    eng.set_squelch(s.open_ms, s.close_ms, s.hang_blocks)
    model = V.Voice(12, R)
    for k in range(2):
        y = eng.update_sources(_cuda(src))
        left, gate = y.cpu().numpy()[..., 0], eng.read_meter(nb)[2].cpu().numpy()
        voice = eng.read_voice().cpu().numpy()
        assert 0 < gate.mean() < 1 and np.array_equal(voice, model.run(left))
        a, _ = _is_voice_pack(eng, voice, gate, R)
        assert a.any()


def _left(eng, x):
    y = eng.update(_cuda(x)).cpu().numpy()
    return y[..., 0]


@pytest.mark.gpu
def test_gpu_voice_state(rdsp):
    """set_groups between two calls keeps every channel's history; a blob from an R = 4 engine continues bit for bit in an R = 2
    engine at another channel index and another channel count; a blob from an engine without the stage zeroes the history; a
    blob with the part is refused by an engine without the stage, nothing changed; rdsp_engine_state_bytes grows by 240 bytes a
    channel only with the stage on; the blob of an engine that never enabled the stage carries no flag of it and is, byte for
    byte, the blob of an engine with the stage without its part"""
    lib = rdsp.load()
    x = _bursts(55, 7, 4)
    a = _voice_engine(4, 5, 4, meter=False)
    ma = V.Voice(5, 4)
    left = [_left(a, x[:5, :128])]
    assert np.array_equal(a.read_voice().cpu().numpy(), ma.run(left[0]))
    a.set_groups([0, 2])
    left.append(_left(a, x[:5, 128:256]))
    assert np.array_equal(a.read_voice().cpu().numpy(), ma.run(left[1]))                       # regrouped: the history stayed
    plain = _engine(5, 4, meter=False)
    plain.set_groups([0, 2])
    for k in range(2):
        assert np.array_equal(_left(plain, x[:5, k * 128:(k + 1) * 128]), left[k])
    assert plain.voice_rate == 0
    assert lib.rdsp_engine_state_bytes(a.h, 3) - lib.rdsp_engine_state_bytes(plain.h, 3) == 3 * 240
    blob, plain_blob = a.save_state(1, 3), plain.save_state(1, 3)
    hdr, plain_hdr = blob[:16].view(np.uint32), plain_blob[:16].view(np.uint32)
    assert hdr[3] == 4 and plain_hdr[3] == 0 and len(blob) == len(plain_blob) + 720
    assert np.array_equal(blob[16:len(plain_blob)], plain_blob[16:])                            # the stage changed nothing else
    assert np.array_equal(blob[len(plain_blob):].view(np.int32).reshape(3, 60), left[1][1:4, -60:])
    # into an R = 2 engine of 7 channels, at channel 3
    b = _voice_engine(2, 7, 4, meter=False)
    mb = V.Voice(7, 2)
    first = _left(b, x[:, :128])
    assert np.array_equal(b.read_voice().cpu().numpy(), mb.run(first))
    b.load_state(3, blob)
    mb.hist[3:6] = left[1][1:4, -60:]
    x2 = x[:, 256:512].copy()
    x2[3:6] = x[1:4, 256:512]
    got = _left(b, x2)
    cont = _left(a, x[:5, 256:512])
    assert np.array_equal(got[3:6], cont[1:4])                                                  # the engine's own state moved, as ever
    assert np.array_equal(b.read_voice().cpu().numpy(), mb.run(got))
    # a blob without the part zeroes the history of the channels it lands on
    b.load_state(0, plain.save_state(0, 2))
    mb.hist[0:2] = 0
    got = _left(b, x[:, :128])
    assert np.array_equal(b.read_voice().cpu().numpy(), mb.run(got))
    # a blob with the part is refused by an engine without the stage
    before = plain.save_state(0, 5)
    with pytest.raises(rdsp.RdspError) as ex:
        plain.load_state(0, blob)
    assert ex.value.code == -4 and b"rdsp_engine_enable_voice" in lib.rdsp_last_error()
    assert np.array_equal(plain.save_state(0, 5), before)
    # with the meter too: the voice words stand behind the meter's
    c = _voice_engine(4, 2, 4, meter=True)
    lc = _left(c, x[:2, :256])
    cb = c.save_state(0, 2)
    assert cb[:16].view(np.uint32)[3] == 6 and np.array_equal(cb[-2 * 240:].view(np.int32).reshape(2, 60), lc[:, -60:])


@pytest.mark.gpu
def test_gpu_voice_refusals(rdsp):
    """rdsp_engine_enable_voice: R other than 2 or 4 and a second R are RDSP_ERR_INVALID with the rate as it was, the same R
    again is RDSP_OK; read_voice and pack_voice before it RDSP_ERR_NOT_READY (pack_voice also without the meter);
    RDSP_ERR_INVALID for a NULL destination, n_blocks negative or above the last call's, a short stride, a capacity with a NULL
    buffer, a d_audio that is not 16-byte aligned, a capacity above INT32_MAX: buffers keep their sentinels and the rows and the
    history are as they were.  No call yet, or n_blocks 0: counts {0, 0}."""
    import torch
    x = _bursts(26, 5, 6)
    e = _engine(5, 8, meter=False)
    lib = e.lib
    out = torch.full((5, 6 * 64), 77, dtype=torch.int16, device="cuda")
    a = torch.full((40, 64), 77, dtype=torch.int16, device="cuda")
    r = torch.full((40, 2), 77, dtype=torch.int32, device="cuda")
    cnt = torch.full((2,), 77, dtype=torch.int32, device="cuda")
    po, pa, pr, pc = out.data_ptr(), a.data_ptr(), r.data_ptr(), cnt.data_ptr()
    e.update(_cuda(x))
    assert e.voice_rate == 0 and lib.rdsp_engine_voice_rate(None) == 0
    assert lib.rdsp_engine_read_voice(e.h, 6, po, 6 * 64, None) == -4 and b"rdsp_engine_enable_voice" in lib.rdsp_last_error()
    assert lib.rdsp_engine_pack_voice(e.h, 6, pa, pr, 40, pc, None) == -4 and b"rdsp_engine_enable_meter" in lib.rdsp_last_error()
    for R in (0, 1, 3, 8, -4):
        assert lib.rdsp_engine_enable_voice(e.h, R) == -1 and e.voice_rate == 0, R
    assert lib.rdsp_engine_enable_voice(None, 2) == -1
    e.enable_voice(2)
    assert lib.rdsp_engine_enable_voice(e.h, 4) == -1 and b"rdsp_engine_enable_voice" in lib.rdsp_last_error() and e.voice_rate == 2
    assert lib.rdsp_engine_enable_voice(e.h, 2) == 0 and e.voice_rate == 2
    assert lib.rdsp_engine_pack_voice(e.h, 6, pa, pr, 40, pc, None) == -4 and b"rdsp_engine_enable_meter" in lib.rdsp_last_error()
    assert lib.rdsp_engine_read_voice(e.h, 1, po, 6 * 64, None) == -1                           # the stage has seen no call yet
    assert lib.rdsp_engine_read_voice(e.h, 0, po, 0, None) == 0
    m = _engine(5, 8, meter=True)
    assert lib.rdsp_engine_pack_voice(m.h, 0, pa, pr, 40, pc, None) == -4 and b"rdsp_engine_enable_voice" in lib.rdsp_last_error()
    e.set_squelch(1e-4, 1e-5, 2)
    e.enable_meter()
    assert lib.rdsp_engine_pack_voice(e.h, 1, pa, pr, 40, pc, None) == -1                       # no call yet
    assert lib.rdsp_engine_pack_voice(e.h, 0, pa, pr, 40, pc, None) == 0
    torch.cuda.synchronize()
    assert cnt.tolist() == [0, 0]
    cnt.fill_(77)
    e.reset()
    left = e.update(_cuda(x)).cpu().numpy()[..., 0]
    want = V.Voice(5, 2).run(left)
    gate = e.read_meter(6)[2].cpu().numpy()
    assert gate.any() and not gate.all()
    for args in ((6, None, 6 * 64), (-1, po, 6 * 64), (7, po, 8 * 64), (6, po, 6 * 64 - 1)):
        assert lib.rdsp_engine_read_voice(e.h, *args, None) == -1 and b"rdsp_engine_read_voice" in lib.rdsp_last_error(), args
    assert lib.rdsp_engine_read_voice(None, 6, po, 6 * 64, None) == -1
    for args in ((6, pa, pr, 40, None), (-1, pa, pr, 40, pc), (7, pa, pr, 40, pc), (6, None, pr, 40, pc), (6, pa, None, 40, pc),
                 (6, None, None, 1, pc), (6, pa + 8, pr, 39, pc), (6, pa + 2, pr, 39, pc), (6, pa, pr, 2 ** 31, pc), (6, pa + 8, None, 0, pc)):
        assert lib.rdsp_engine_pack_voice(e.h, *args, None) == -1, args
        assert b"rdsp_engine_pack_voice" in lib.rdsp_last_error()
    assert lib.rdsp_engine_pack_voice(None, 6, pa, pr, 40, pc, None) == -1
    torch.cuda.synchronize()
    assert bool((out == 77).all()) and bool((a == 77).all()) and bool((r == 77).all()) and cnt.tolist() == [77, 77]
    assert np.array_equal(e.read_voice().cpu().numpy(), want)                                  # the rows are as they were
    _is_voice_pack(e, want, gate, 2)
    _is_voice_pack(e, want, gate, 2, capacity=2)
    assert np.array_equal(e.save_state(0, 5)[-5 * 240:].view(np.int32).reshape(5, 60), left[:, -60:])
