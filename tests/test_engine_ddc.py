"""rdsp_engine_t on wide-band sources: rows at D x 44 100 Hz, every receiver tuned, low-passed and decimated by D
(rdsp_engine_set_source_decimation, include/rdsp.h; kernel csrc/rdsp_engine_ddc.hip, arithmetic csrc/rdsp_tune.h).

`-m "not gpu"`: the prototype filter is the one specified (and the numpy evaluation of its formula, bit for bit: the
library uses no libm function for it); the numpy restatement (tests/engine_sources_model.py, at Q = 1) is rdsp_tune.h's
arithmetic compiled on the host (tests/host/host_source_pass_check.cpp), bit for bit; the restated row stays within a derived
bound of a float64 evaluation of the definition; it is a receiver (a station at +200 kHz comes out at the IF, what folds onto
the IF is gone); it does not depend on how the stream is cut into calls.
`-m gpu`: the audio of every receiver, bit for bit, against oracle_lib.OracleEngine run on the restated row, as
tests/test_engine_tuning.py does for D = 1."""
import ctypes
import subprocess

import numpy as np
import pytest

from engine_sources_model import (F32, HIST, M32, S16, TUNING_OFFSET, Rx, _band, _int16, _phasor_modulus_error, _script_97, _tone, ddc_rows,
                                  dphi_of, engine, host_program, host_rows, lib_taps, receiver_taps, stream, table, taps_of, wide)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check():
    return host_program()


def test_ddc_filter_is_the_one_specified(rdsp):
    """rdsp_engine_ddc_taps for every D in 2 ... 64 at gain 1: symmetric bit for bit; sum 1 within the rounding of 16 D
    floats (2^-25 each); ripple <= 0.001 dB on |f| <= 12 000 Hz and <= -89 dB from 32 100 Hz on (the design conditions; the
    worst measured values are printed); and EQUAL BIT FOR BIT to the numpy evaluation of the same formula
    (engine_sources_model.taps_of): the library evaluates sine and I0 by series of + - * / only and sqrt, so no libm stands
    between the two.  The gain multiplies before the rounding; refusals of the host-only call."""
    worst_ripple, worst_stop = 0.0, -1e9
    for D in range(2, 65):
        h = lib_taps(D)
        T = 16 * D
        assert h.dtype == F32 and len(h) == T and np.array_equal(h, h[::-1]), D
        assert abs(float(h.astype(np.float64).sum()) - 1.0) <= T * 2.0 ** -25, D
        assert np.array_equal(h.view(np.uint32), taps_of(D).view(np.uint32)), D
        fs = D * 44100.0
        nfft = 64 * T
        H = np.abs(np.fft.rfft(h.astype(np.float64), nfft))
        f = np.fft.rfftfreq(nfft, 1 / fs)
        ripple = np.abs(20 * np.log10(H[f <= 12000.0])).max()
        stop = (20 * np.log10(np.maximum(H[f >= 32100.0], 1e-300))).max()
        assert ripple <= 0.001 and stop <= -89.0, (D, ripple, stop)
        assert np.abs(h.astype(np.float64)).sum() <= 1.65, D
        worst_ripple, worst_stop = max(worst_ripple, ripple), max(worst_stop, stop)
    print(f"ddc taps: worst ripple {worst_ripple:.6f} dB, worst stop band {worst_stop:.2f} dB")
    assert np.array_equal(lib_taps(16, 1, 37.5).view(np.uint32), taps_of(16, 1, 37.5).view(np.uint32))
    lib = rdsp.load()
    o = np.zeros(16 * 64, F32)
    p = o.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for D, g in ((0, 1.0), (65, 1.0), (4, 0.0), (4, -1.0), (4, float("nan")), (4, float("inf"))):
        assert lib.rdsp_engine_ddc_taps(D, g, p) == -1, (D, g)
    assert not o.any()


@pytest.mark.parametrize("D", [2, 3, 16, 64])
def test_ddc_numpy_restatement_is_the_headers_arithmetic(host_check, tmp_path, rdsp, D):
    """ddc_rows / receiver_taps / taps_of / dphi_of against rdsp_tune.h compiled on the host, bit for bit: 256 outputs of 24
    receivers at the steps of drawn stations in every mode (anywhere in |f| < D x 22 050, and 0, and the band's edges) from
    drawn phases, on a drawn row under a gain of 3 with edge pairs (+-32767, -32768, 0, +-1 in every combination),
    full-scale stretches that saturate, and a history; the host check's own checks (symmetry, the series against libm,
    the step at D, the DC gain) pass too"""
    out = subprocess.run([host_check, "check"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout + out.stderr
    r = np.random.default_rng(100 + D)
    n_out, n_rx, gain = 256, 24, 3.0
    n = HIST * D + n_out * D
    xh = r.integers(-9000, 9000, (n, 2)).astype(np.int16)
    edge = np.array([-32768, -32767, -1, 0, 1, 32767], np.int16)
    e = np.stack(np.meshgrid(edge, edge), -1).reshape(-1, 2)
    at = r.integers(0, n - 1, len(e))
    xh[at] = e
    for a, pair in ((40 * D, [32767, 32767]), (90 * D, [-32768, 32767]), (150 * D, [-32768, -32768])):
        xh[a:a + 20 * D] = pair
    lim = D * 22050.0
    stations = np.concatenate([r.uniform(-lim + 1, lim - 1, n_rx - 4), [0.0, 8390.0, lim - 0.1, -lim + 0.1]])
    modes = np.arange(n_rx) % 7
    to = np.array([TUNING_OFFSET[int(m)] for m in modes], F32)
    dphi = np.array([dphi_of(t, s, D) for t, s in zip(to, stations)], np.uint64)
    ph0 = r.integers(0, 1 << 32, n_rx, dtype=np.uint64)
    ph0[:3] = 0
    want = host_rows(host_check, tmp_path, S16, xh[HIST * D:], xh[:HIST * D], D, 1, 0, gain, dphi, ph0, n_out, to, stations)
    tab = table(rdsp)
    h = np.fromfile(tmp_path / "taps.bin", F32)
    assert np.array_equal(h.view(np.uint32), taps_of(D, 1, gain).view(np.uint32))
    assert np.array_equal(h.view(np.uint32), lib_taps(D, 1, gain).view(np.uint32))
    assert list(np.fromfile(tmp_path / "dphi.bin", np.uint32)) == [int(d) for d in dphi]
    g = np.fromfile(tmp_path / "g.bin", F32).reshape(n_rx, 16 * D, 2)
    gx, gy = receiver_taps(h, dphi, tab)
    assert np.array_equal(gx.view(np.uint32), g[..., 0].view(np.uint32)) and np.array_equal(gy.view(np.uint32), g[..., 1].view(np.uint32))
    got = np.ascontiguousarray(ddc_rows(xh, D, h, dphi, ph0, tab)).view(np.uint32)[..., 0]
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert (np.abs(ddc_rows(xh, D, h, dphi, ph0, tab).astype(int)) >= 32767).sum() > 50      # the rails were reached


@pytest.mark.parametrize("D", [2, 5, 16, 64])
def test_ddc_restatement_against_exact_arithmetic(rdsp, D):
    """the restated rows of 6 receivers against a float64 evaluation of the definition (numpy's cos / sin, the same float32
    taps, gain 2, a busy band with full-scale stretches), every sample of both components:
        |diff| <= 0.5 + A (2 x 2^-17 + gamma) counts,  A[m] = sum_k |h_k| |x[(m + 1) D - 1 - k]|  (|x| the modulus),
    0.5 for the one rounding to int16 (saturation moves two values no further apart).  Derivation: with |h_k| |x| summed,
    A bounds |sum g_k x| and every partial sum of either component (|gx xi| + |gy xq| <= |g| |x|).  The translated taps carry
    the table's phasor error, below 2^-17 as a modulus (_phasor_modulus_error, asserted here): at most 2^-17 A; the rotation to the IF carries it
    once more: 2^-17 A.  gamma, the roundings: the product h_k c: 2^-24 A; the chain of n = 2 T fmaf per component, each
    rounding a partial sum of at most A: 2 T x 2^-24 A; the rotation's product and its fmaf: 2 x 2^-24 A; one more 2^-24 A
    for every second-order term: gamma = (2 T + 4) 2^-24."""
    tab = table(rdsp)
    assert _phasor_modulus_error(tab) < 2.0 ** -17
    T, nb, gain = 16 * D, 6, 2.0
    src = wide(7 + D, 1, nb, D, level=0.08)[0]
    h = lib_taps(D, 1, gain)
    r = np.random.default_rng(D)
    lim = D * 22050.0
    stations = np.concatenate([r.uniform(-lim + 1, lim - 1, 4), [0.0, lim - 1.0]])
    dphi = np.array([dphi_of(TUNING_OFFSET[m % 7], s, D) for m, s in enumerate(stations)], np.uint64)
    got, _ = stream(src, D, 1, h, np.repeat(dphi[:, None], nb, 1), tab)
    x = np.concatenate([np.zeros(HIST * D), src[:, 0].astype(np.float64) + 1j * src[:, 1].astype(np.float64)])
    n_out = nb * 128
    A = np.convolve(np.abs(x), np.abs(h.astype(np.float64)))[T - 1::D][:n_out]
    gamma = (2 * T + 4) * 2.0 ** -24
    bound = 0.5 + A * (2 * 2.0 ** -17 + gamma)
    k = np.arange(T)
    worst = 0.0
    for i, d in enumerate(dphi):
        g = h.astype(np.float64) * np.exp(-2j * np.pi * ((k * int(d)) % (1 << 32)) / 4294967296.0)
        z = np.convolve(x, g)[T - 1::D][:n_out]
        z = z * np.exp(2j * np.pi * ((np.arange(n_out) * ((int(d) * D) & M32)) & M32) / 4294967296.0)
        for comp, want in ((0, z.real), (1, z.imag)):
            diff = np.abs(got[i, :, comp].astype(np.float64) - np.clip(want, -32768, 32767))
            worst = max(worst, float((diff / bound).max()))
            assert np.all(diff <= bound), (D, i, comp, int(np.argmax(diff - bound)), float(diff.max()))
    print(f"ddc D {D}: worst |diff| / bound = {worst:.3f}")


def test_ddc_is_a_receiver(rdsp):
    """D = 16 (a source at 705 600 Hz), a USB station at +200 kHz carrying a tone 1 000 Hz above it at a quarter of full
    scale: the tuned row holds it at TuningOffset + 1 000 = 6 390 Hz (the strongest bin of 4 410 samples, 10 Hz apart) with
    the amplitude within the ripple bound (0.001 dB) plus one count.  Then a 0.9 full-scale interferer at station -
    TuningOffset + 44 100 + 7 890 = 246 600 Hz, which the shift puts at 51 990 Hz and the decimation would fold onto 7 890 Hz in
    the IF band: no sample of the tuned row moves by more than 2 counts (0.9 x 32767 x 10^(-89 / 20) = 1.05 before rounding)"""
    tab = table(rdsp)
    D, nb = 16, 36
    fs, n = D * 44100.0, nb * 128 * D
    h = lib_taps(D)
    to = TUNING_OFFSET[1]
    steps = np.full((1, nb), dphi_of(to, 200000.0, D), np.uint64)
    amp = 0.25 * 32767
    y = stream(_int16(_tone(201000.0, n, fs, amp)), D, 1, h, steps, tab)[0][0]
    z = (y[128:128 + 4410, 0] + 1j * y[128:128 + 4410, 1]).astype(np.complex128)
    spec = np.abs(np.fft.fft(z))
    assert abs(np.fft.fftfreq(4410, 1 / 44100.0)[np.argmax(spec)] - (to + 1000.0)) < 1e-6
    got = abs(np.mean(z * np.exp(-2j * np.pi * (to + 1000.0) / 44100.0 * np.arange(4410))))
    print(f"ddc receiver: amplitude {got:.3f} of {amp:.3f}")
    assert abs(got - amp) <= amp * (10 ** (0.001 / 20) - 1) + 1.0
    f_int = 200000.0 - to + 44100.0 + 7890.0
    a = 0.09 * 32767
    clean = stream(_int16(_tone(201000.0, n, fs, a)), D, 1, h, steps, tab)[0][0]
    dirty = stream(_int16(_tone(201000.0, n, fs, a) + _tone(f_int, n, fs, 0.9 * 32767, 1.0)), D, 1, h, steps, tab)[0][0]
    moved = np.abs(dirty.astype(int) - clean.astype(int))[16:].max()       # behind the filter's own length
    print(f"ddc receiver: the folding interferer moves a sample by at most {moved} counts")
    assert moved <= 2


@pytest.mark.parametrize("D", [2, 16])
def test_ddc_restatement_does_not_depend_on_the_call_split(rdsp, D):
    """32 blocks in one call, against calls of 1, 7 and 32 blocks with the history and the phases carried: sample for
    sample; and the phases after the stream are the closed form 32 x 128 x D x dphi"""
    tab = table(rdsp)
    nb = 32
    src = wide(3, 1, nb, D)[0]
    h = lib_taps(D, 1, 1.5)
    r = np.random.default_rng(4)
    dphi = np.array([dphi_of(TUNING_OFFSET[m], s, D) for m, s in zip((0, 1, 4), r.uniform(-D * 22000.0, D * 22000.0, 3))], np.uint64)
    steps = np.repeat(dphi[:, None], nb, 1)
    whole, ph = stream(src, D, 1, h, steps, tab)
    assert [int(p) for p in ph] == [(nb * 128 * D * int(d)) & M32 for d in dphi]
    for split in (1, 7, 32):
        cut, ph2 = stream(src, D, 1, h, steps, tab, cuts=range(0, nb, split))
        assert np.array_equal(cut, whole) and np.array_equal(ph, ph2), split


# ---- GPU ------------------------------------------------------------------------------------------------------------------
_stream_cache = {}


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 7, 32])
@pytest.mark.parametrize("D", [2, 5, 16, 64])
def test_gpu_ddc_against_the_restatement(rdsp, D, split):
    """3 sources x 97 receivers (the sources' last workgroups ragged) at stations anywhere in |f| < D x 22 050, gain 2.5, 40
    blocks cut into calls of `split`, with a retune, a regrouping and a mode change in mid-stream (_script_97): every
    receiver against the restatement of its own row and calls, bit for bit.  What the CPU side computes does not depend on
    the split, so it is computed once per D."""
    nch, nb, gain = 97, 40, 2.5
    r = np.random.default_rng(20 + D)
    src = wide(40 + D, 3, nb, D)
    source_of = r.integers(0, 3, nch)
    lim = D * 22050.0
    stations = r.uniform(-lim + 1, lim - 1, nch)
    stations[:3] = [lim - 0.5, -lim + 0.5, 0.0]
    eng = engine(nch, 32)
    eng.sketch_setup()
    R = Rx(eng, src, source_of, [0, 19, 40, 58, 77], stations, D, 1, gain)
    _script_97(R, split, nb)
    y = R.result()
    if D not in _stream_cache:
        R.restate(range(nch))
        _stream_cache[D] = (R.steps, R.calls, [R.want(c) for c in range(nch)])
    steps, calls, want = _stream_cache[D]
    assert steps == R.steps and calls == R.calls
    for c in range(nch):
        assert np.array_equal(y[c], want[c]), (c, int(np.argmax(y[c] != want[c])))
    eng.close()


@pytest.mark.gpu
def test_gpu_ddc_decimation_one_is_the_tuning_pass(rdsp):
    """set_source_decimation(1, 1.0), then the 97-receiver stream of test_engine_tuning.py (its data, its script, calls of 7
    blocks): the audio is the D = 1 restatement's, bit for bit -- the path without a filter"""
    split = 7
    r = np.random.default_rng(20 + split)
    nch, nb = 97, 256
    src = _band(40, 3, nb)
    source_of = r.integers(0, 3, nch)
    eng = engine(nch, 64)
    eng.sketch_setup()
    R = Rx(eng, src, source_of, [0, 19, 40, 58, 77], r.uniform(-21500, 21500, nch))
    eng.set_source_decimation(1, 1.0)
    assert eng.source_decimation() == 1
    for g, m in enumerate([0, 1, 2, 4, 5]):
        R.call(0, g, "setDemodMode", m)
    R.run(0, 90, split)
    R.tune(5, r.uniform(-21500, 21500, 32))
    R.run(90, 150, split)
    R.call(150, 2, "setDemodMode", 3)
    R.call(150, 4, "setDemodMode", 1)
    R.call(150, 1, "setAudioFilter", 3)
    R.run(150, nb, split)
    R.check(R.result())


@pytest.mark.gpu
def test_gpu_ddc_reset_history_and_state_as_data(rdsp):
    """D = 5.  Reset zeroes the source histories: the same rows after a reset give the same audio as the first time and
    as a fresh engine.  A receiver saved in one engine after 9 blocks and loaded into another engine (another channel
    count, index and call size) that heard the same source stream continues bit for bit; the blob sizes are those of an
    engine with sources at D = 1 (16 + n (10 368 + 4) bytes): the history is not in them"""
    import torch
    D, nb, k, gain = 5, 24, 9, 2.0
    r = np.random.default_rng(9)
    src = wide(61, 2, nb, D)
    lim = D * 22050.0
    a = engine(6, 8)
    a.sketch_setup()
    A = Rx(a, src, [0, 1, 1, 0, 1, 0], [0], r.uniform(-lim + 1, lim - 1, 6), D, 1, gain)
    A.run(0, nb, 8)
    first = A.result()
    A.check(first)
    a.reset()
    A.outs = []
    A.run(0, nb, 8)
    assert np.array_equal(A.result(), first)
    fresh = engine(6, 8)
    fresh.sketch_setup()
    Fr = Rx(fresh, src, A.source_of, [0], A.station, D, 1, gain)
    Fr.run(0, 1, 8)
    assert np.array_equal(Fr.result(), first[:, :128])
    # state as data: a runs 9 blocks, b hears the same 9 blocks with receivers of its own, then takes a's channels 2, 3
    a.reset()
    A.outs = []
    A.run(0, k, 8)
    blob = a.save_state(2, 2)
    assert blob.size == a.lib.rdsp_engine_state_bytes(a.h, 2) == 16 + 2 * (10368 + 4)
    assert list(blob[:16].view(np.uint32)) == [0x45534452, 1, 2, 1]
    b = engine(9, 16)
    b.sketch_setup()
    B = Rx(b, src, [0] * 5 + [1, 0] + [1] * 2, [0], r.uniform(-lim + 1, lim - 1, 9), D, 1, gain)
    B.tune(5, A.station[2:4])
    B.run(0, k, 16)
    b.load_state(5, blob)
    B.outs = []
    B.run(k, nb, 16)
    y = B.result()
    assert np.array_equal(y[5], first[2, k * 128:]) and np.array_equal(y[6], first[3, k * 128:])


@pytest.mark.gpu
def test_gpu_ddc_at_the_bench_shape(rdsp):
    """`bench.py --config ENGINE`'s shape -- 4096 receivers x 32 blocks in one call -- on 16 sources at D = 16 (705 600 Hz),
    receiver c on source c % 16 (so the pass's source order is not the channel order), gain 4: the first and the last
    receiver of every source in the pass's order, the receivers around two workgroup boundaries and 32 drawn ones -- 68 or
    more -- bit for bit"""
    nch, nblk, nsrc, D = 4096, 32, 16, 16
    src = wide(5, nsrc, nblk, D)
    eng = engine(nch, nblk)
    eng.sketch_setup()
    lim = D * 22050.0
    R = Rx(eng, src, np.arange(nch) % nsrc, [0], np.random.default_rng(5).uniform(-lim + 1, lim - 1, nch), D, 1, 4.0)
    R.run(0, nblk, nblk)
    y = R.result()
    per = nch // nsrc                                       # position p of source s in the pass's order is channel p nsrc + s
    pick = {p * nsrc + s for s in range(nsrc) for p in (0, per - 1)} | {p * nsrc + 3 for p in (15, 16, 17, 31, 32)}
    pick |= set(int(c) for c in np.random.default_rng(2).integers(0, nch, 32))
    assert len(pick) >= 64
    R.check(y, sorted(pick))


@pytest.mark.gpu
def test_gpu_ddc_refusals(rdsp):
    """refused with nothing changed: set_source_decimation before set_sources (NOT_READY); D of 0 and 65; a gain of 0, NaN,
    inf; a D under which a tuned station falls outside the band; then at D = 4 a station at and beyond 4 x 22 050 Hz, a
    src_stride shorter than n_blocks x 128 x D -- the object then runs on exactly as a twin that never saw those calls"""
    import torch
    from radiodsp_sdr_rx_amd._lib import RdspError
    D = 4
    src = torch.from_numpy(wide(95, 2, 16, D)).cuda()
    out = torch.empty((4, 8 * 128, 2), dtype=torch.int16, device="cuda")
    eng, twin = engine(4, 8), engine(4, 8)
    for e in (eng, twin):
        e.sketch_setup()
    with pytest.raises(RdspError) as ex:
        eng.set_source_decimation(D, 1.0)
    assert ex.value.code == -4 and b"set_sources" in eng.lib.rdsp_last_error()
    for e in (eng, twin):
        e.set_sources(2, [0, 1, 1, 0])
        e.set_source_decimation(D, 3.0)
        e.tune(0, [-80000.0, 100.0, 40000.0, 88000.0])
    w = 128 * D
    y = [e.update_sources(src[:, :8 * w].contiguous()).cpu().numpy() for e in (eng, twin)]
    for d, g in ((0, 1.0), (65, 1.0), (-1, 1.0), (D, 0.0), (D, -2.0), (D, float("nan")), (D, float("inf")), (3, 1.0), (1, 1.0)):
        with pytest.raises(RdspError) as ex:                 # D = 3 and D = 1: channel 3 sits at 88 kHz
            eng.set_source_decimation(d, g)
        assert ex.value.code == -1, (d, g)
    assert eng.source_decimation() == D
    for first, st in ((0, [88200.0]), (1, [-88200.0]), (0, [float("nan")]), (0, [1000.0, 2000.0, 90000.0])):
        with pytest.raises(RdspError) as ex:
            eng.tune(first, st)
        assert ex.value.code == -1
    lib, p, o = eng.lib, src.data_ptr(), out.data_ptr()
    row = src.shape[1]
    assert lib.rdsp_engine_update_sources(eng.h, p, 8 * w - 4, 8, o, 8 * 128, None) == -1     # shorter than 8 blocks at D
    assert lib.rdsp_engine_update_sources(eng.h, p, 8 * 128, 8, o, 8 * 128, None) == -1       # long enough at D = 1 only
    assert lib.rdsp_engine_update_sources(eng.h, p, row, 9, o, 8 * 128, None) == -1           # more than max_blocks
    with pytest.raises(AssertionError):
        eng.update_sources(src[:, :8 * w + 128].contiguous())                                 # not a multiple of 128 D
    y2 = [e.update_sources(src[:, 8 * w:].contiguous()).cpu().numpy() for e in (eng, twin)]
    assert np.array_equal(y[0], y[1]) and np.array_equal(y2[0], y2[1])
    assert y[0].any() and y2[0].any()
