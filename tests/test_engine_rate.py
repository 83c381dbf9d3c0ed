"""rdsp_engine_t on sources at any rational multiple of 44 100 Hz: rows at 44 100 P / Q Hz, every receiver tuned, low-passed
and resampled by Q / P in one polyphase pass (rdsp_engine_set_source_rate, include/rdsp.h; kernel
csrc/rdsp_engine_rate.hip, schedule and arithmetic csrc/rdsp_tune.h).

`-m "not gpu"`: the prototype filter is the one specified (and the numpy evaluation of its formula, bit for bit); the schedule
is the one specified, in Python integers; the numpy restatement (tests/engine_sources_model.py) is rdsp_tune.h's arithmetic
compiled on the host (tests/host/host_source_pass_check.cpp), bit for bit; the restated row stays within a derived bound of a
float64 evaluation of the definition; it is a receiver at 2.4 MHz; it does not depend on how the stream is cut into calls.
`-m gpu`: the audio of every receiver, bit for bit, against oracle_lib.OracleEngine run on the restated row, as
tests/test_engine_ddc.py does for integer rates."""
import ctypes
import math
import subprocess

import numpy as np
import pytest

from engine_sources_model import (F32, M32, S16, TUNING_OFFSET, Rx, _dc, _fs, _int16, _pairs, _phasor_modulus_error, _script_97, _tone, dphi_of,
                                  engine, host_program, host_rows, lib_taps, rate_rows, schedule, stream, table, taps_of, wide)

RATES = [(3, 2), (65, 64), (160, 147), (640, 147), (2500, 441), (8000, 147), (20480, 441)]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check():
    return host_program()


def test_rate_filter_is_the_one_specified(rdsp):
    """rdsp_engine_rate_taps over RATES at gain 1: EQUAL BIT FOR BIT to the numpy evaluation of the same formula
    (engine_sources_model.taps_of; no libm stands between the two); symmetric bit for bit; sum Q gain within the rounding of
    Tp floats (Tp 2^-25 Q); ripple <= 0.001 dB on |f| <= 12 000 Hz; <= -89 dB from 32 100 Hz to the prototype's Nyquist frequency (the
    images of the source spectrum included); every branch's sum |hb[r][j]| <= 2.5 (the worst values are printed).  For Q = 1
    the taps are rdsp_engine_ddc_taps' bit for bit; (882, 294) is (3, 1); the refusals of the host-only call."""
    from radiodsp_sdr_rx_amd.engine import ddc_taps, rate_taps
    worst_ripple, worst_stop, worst_abs = 0.0, -1e9, 0.0
    for P, Q in RATES:
        h = lib_taps(P, Q)
        Tb = 16 * _dc(P, Q)
        Tp = Tb * Q
        assert h.dtype == F32 and len(h) == Tp and np.array_equal(h, h[::-1]), (P, Q)
        assert np.array_equal(h.view(np.uint32), taps_of(P, Q).view(np.uint32)), (P, Q)
        assert abs(float(h.astype(np.float64).sum()) - Q) <= Tp * 2.0 ** -25 * Q, (P, Q)
        fs = 44100.0 * P                                             # the prototype's rate
        nfft = 1 << int(math.ceil(math.log2(16 * Tp)))
        H = np.abs(np.fft.rfft(h.astype(np.float64) / Q, nfft))
        f = np.fft.rfftfreq(nfft, 1 / fs)
        ripple = np.abs(20 * np.log10(H[f <= 12000.0])).max()
        stop = (20 * np.log10(np.maximum(H[f >= 32100.0], 1e-300))).max()
        branch = np.abs(h.astype(np.float64)).reshape(Tb, Q).sum(0).max()
        assert ripple <= 0.001 and stop <= -89.0 and branch <= 2.5, (P, Q, ripple, stop, branch)
        worst_ripple, worst_stop, worst_abs = max(worst_ripple, ripple), max(worst_stop, stop), max(worst_abs, branch)
    print(f"rate taps: worst ripple {worst_ripple:.6f} dB, worst stop band {worst_stop:.2f} dB, worst branch sum |h| {worst_abs:.3f}")
    assert np.array_equal(lib_taps(160, 147, 37.5).view(np.uint32), taps_of(160, 147, 37.5).view(np.uint32))
    for D in (2, 16, 64):
        assert np.array_equal(rate_taps(D, 1, 2.5).view(np.uint32), ddc_taps(D, 2.5).view(np.uint32)), D
        assert np.array_equal(rate_taps(D, 1, 2.5).view(np.uint32), taps_of(D, 1, 2.5).view(np.uint32)), D
    assert np.array_equal(rate_taps(882, 294, 1.5).view(np.uint32), ddc_taps(3, 1.5).view(np.uint32))
    lib = rdsp.load()
    o = np.zeros(16 * 64 * 441, F32)
    p = o.ctypes.data_as(ctypes.POINTER(ctypes.c_float))
    for P, Q, g in ((3, 0, 1.0), (885, 442, 1.0), (1770, 884, 1.0), (146, 147, 1.0), (2, 3, 1.0), (65 * 147 + 1, 147, 1.0), (129, 2, 1.0),
                    (0, 1, 1.0), (-3, 2, 1.0), (3, -2, 1.0), (3, 2, 0.0), (3, 2, -1.0), (3, 2, float("nan")), (3, 2, float("inf"))):
        assert lib.rdsp_engine_rate_taps(P, Q, g, p) == -1, (P, Q, g)         # 1770 / 884 reduces to 885 / 442
    assert not o.any()


def test_rate_of_hz(rdsp):
    """the ratios of the rates that matter, and the refusals: 44 101 Hz (Q = 44 100), 32 000 Hz (P < Q), 3.2 MHz (above 64),
    48 000.5 Hz (not an integer)"""
    from radiodsp_sdr_rx_amd._lib import RdspError
    from radiodsp_sdr_rx_amd.engine import rate_of_hz
    for fs, want in ((48000, (160, 147)), (96000, (320, 147)), (192000, (640, 147)), (2400000, (8000, 147)), (2048000, (20480, 441)),
                     (1024000, (10240, 441)), (250000, (2500, 441)), (44100, (1, 1)), (705600, (16, 1)), (2822400, (64, 1))):
        assert rate_of_hz(fs) == want, fs
        assert math.gcd(*want) == 1 and want[0] * 44100 == fs * want[1]
    for fs in (44101, 32000, 3200000, 48000.5, 0, -48000, float("nan"), float("inf"), 2822401):
        with pytest.raises(RdspError) as ex:
            rate_of_hz(fs)
        assert ex.value.code == -1, fs


@pytest.mark.parametrize("P,Q", [(3, 2), (160, 147), (20480, 441)])
def test_rate_schedule(host_check, tmp_path, P, Q):
    """rdsp_tune.h's schedule (rate_step, rate_pairs, rate_frac_after, compiled on the host) over 64 blocks cut into calls of 1,
    7 and 32 blocks, against Python integers: the pairs of the calls add up to floor(M P / Q) and differ by at most one
    between equal calls; with S the pairs before the call and m the output's index since the reset, every n(i) + S is
    floor(((m + 1) P - Q) / Q) and every r(i) is ((m + 1) P - Q) mod Q"""
    nb = 64
    for split in (1, 7, 32):
        M, S, seen = 0, 0, set()
        for a in range(0, nb, split):
            n_out = (min(nb, a + split) - a) * 128
            frac = (M * P) % Q
            np.array([P, Q, frac, n_out], np.uint32).tofile(tmp_path / "params.bin")
            out = subprocess.run([host_check, "sched", str(tmp_path)], capture_output=True, text=True)
            assert out.returncode == 0, out.stdout + out.stderr
            pairs, after = (int(v) for v in np.fromfile(tmp_path / "pairs.bin", np.uint64))
            s = np.fromfile(tmp_path / "sched.bin", np.int32).reshape(n_out, 2)
            f2, p2, n, r = schedule(P, Q, M, n_out)
            assert (frac, pairs) == (f2, p2) and after == ((M + n_out) * P) % Q
            m = [M + i for i in range(n_out)]
            assert [int(v) + S for v in s[:, 0]] == [((k + 1) * P - Q) // Q for k in m]
            assert [int(v) for v in s[:, 1]] == [((k + 1) * P - Q) % Q for k in m]
            assert np.array_equal(s[:, 0], n) and np.array_equal(s[:, 1], r) and s[0, 0] >= 0 and s[-1, 0] == pairs - 1
            if n_out == split * 128:
                seen.add(pairs)
            M, S = M + n_out, S + pairs
        assert S == (M * P) // Q and M == nb * 128
        assert max(seen) - min(seen) <= 1, seen


@pytest.mark.parametrize("P,Q", [(3, 2), (160, 147), (2500, 441), (8000, 147)])
def test_rate_numpy_restatement_is_the_headers_arithmetic(host_check, tmp_path, rdsp, P, Q):
    """rate_rows / taps_of / schedule / dphi_of against rdsp_tune.h compiled on the host, bit for bit: 256 outputs of 24
    receivers from a NON-ZERO frac (37 outputs into a stream) at the steps of drawn stations in every mode (anywhere in |f| <
    22 050 P / Q, and 0, and the band's edges) from drawn phases, on a drawn row under a gain of 3 with edge pairs (+-32767,
    -32768, 0, +-1 in every combination), full-scale stretches that saturate, and a history; the host check's own checks
    (Q = 1 is the decimating pass's filter, step and window; the schedule over calls; the limits; the DC gain) pass too"""
    out = subprocess.run([host_check, "check"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout + out.stderr
    r = np.random.default_rng(100 + P)
    n_out, n_rx, gain, m0 = 256, 24, 3.0, 37
    Dc = _dc(P, Q)
    Tb = 16 * Dc
    frac, pairs, _, _ = schedule(P, Q, m0, n_out)
    assert frac != 0
    n = Tb + pairs
    xh = r.integers(-9000, 9000, (n, 2)).astype(np.int16)
    edge = np.array([-32768, -32767, -1, 0, 1, 32767], np.int16)
    e = np.stack(np.meshgrid(edge, edge), -1).reshape(-1, 2)
    xh[r.integers(0, n - 1, len(e))] = e
    for a, pair in ((40 * Dc, [32767, 32767]), (90 * Dc, [-32768, 32767]), (150 * Dc, [-32768, -32768])):
        xh[a:a + 20 * Dc] = pair
    lim = (22050.0 * P) / Q
    stations = np.concatenate([r.uniform(-lim + 1, lim - 1, n_rx - 4), [0.0, 8390.0, lim - 0.1, -lim + 0.1]])
    modes = np.arange(n_rx) % 7
    to = np.array([TUNING_OFFSET[int(m)] for m in modes], F32)
    dphi = np.array([dphi_of(t, s, P, Q) for t, s in zip(to, stations)], np.uint64)
    ph0 = r.integers(0, 1 << 32, n_rx, dtype=np.uint64)
    ph0[:3] = 0
    want = host_rows(host_check, tmp_path, S16, xh[Tb:], xh[:Tb], P, Q, frac, gain, dphi, ph0, n_out, to, stations)
    tab = table(rdsp)
    h = np.fromfile(tmp_path / "taps.bin", F32)
    assert np.array_equal(h.view(np.uint32), taps_of(P, Q, gain).view(np.uint32))
    assert np.array_equal(h.view(np.uint32), lib_taps(P, Q, gain).view(np.uint32))
    assert list(np.fromfile(tmp_path / "dphi.bin", np.uint32)) == [int(d) for d in dphi]
    rows = rate_rows(xh, P, Q, frac, h, dphi, ph0, tab, n_out)
    got = np.ascontiguousarray(rows).view(np.uint32)[..., 0]
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    assert (np.abs(rows.astype(int)) >= 32767).sum() > 50                                # the rails were reached


@pytest.mark.parametrize("P,Q", [(3, 2), (160, 147), (2500, 441), (8000, 147)])
def test_rate_restatement_against_exact_arithmetic(rdsp, P, Q):
    """the restated rows of 6 receivers against a float64 evaluation of the definition (numpy's cos / sin, the same float32
    taps, gain 2, a busy band with full-scale stretches), every sample of both components:
        |diff| <= 0.5 + A (2 x 2^-17 + gamma) counts,  A[i] = sum_j |hb[r(i)][j]| |x[n(i) - j]|  (|x| the modulus),
    0.5 for the one rounding to int16 (saturation moves two values no further apart).  Derivation, test_engine_ddc's for the
    new order: with |hb| |x| summed, A bounds |sum e_j u_j| and every partial sum of either component (|ex ux| + |ey uy| <=
    |e| |u|, |e| <= 1 + 2^-17).  The phasors e_j carry the table's error, below 2^-17 as a modulus (asserted here): at most
    2^-17 A; the rotation to the IF carries it once more: 2^-17 A.  gamma, the roundings: the product hb x rounds ONCE per
    component where the decimating pass's h c did: 2^-24 A; the chain of 2 Tb fmaf per component, each rounding a partial
    sum of at most A: 2 Tb x 2^-24 A; the rotation's product and its fmaf: 2 x 2^-24 A; one more 2^-24 A for every
    second-order term: gamma = (2 Tb + 4) 2^-24."""
    tab = table(rdsp)
    assert _phasor_modulus_error(tab) < 2.0 ** -17
    Dc = _dc(P, Q)
    Tb, nb, gain = 16 * Dc, 6, 2.0
    src = wide(7 + P, 1, nb, P, Q, level=0.08)[0]
    h = lib_taps(P, Q, gain)
    r = np.random.default_rng(P)
    lim = (22050.0 * P) / Q
    stations = np.concatenate([r.uniform(-lim + 1, lim - 1, 4), [0.0, lim - 1.0]])
    dphi = np.array([dphi_of(TUNING_OFFSET[m % 7], s, P, Q) for m, s in enumerate(stations)], np.uint64)
    got, _ = stream(src, P, Q, h, np.repeat(dphi[:, None], nb, 1), tab)
    n_out = nb * 128
    _, _, n, br = schedule(P, Q, 0, n_out)
    x = np.concatenate([np.zeros(Tb), src[:, 0].astype(np.float64) + 1j * src[:, 1].astype(np.float64)])
    j = np.arange(Tb)
    X = x[Tb + n[:, None] - j[None, :]]                                                   # [n_out, Tb]
    H = h.astype(np.float64)[j[None, :] * Q + br[:, None]]
    A = (np.abs(H) * np.abs(X)).sum(1)
    gamma = (2 * Tb + 4) * 2.0 ** -24
    bound = 0.5 + A * (2 * 2.0 ** -17 + gamma)
    worst = 0.0
    for i, d in enumerate(dphi):
        e = np.exp(-2j * np.pi * ((j * int(d)) % (1 << 32)) / 4294967296.0)
        k = np.array([((int(v) + 1 - Dc) * int(d)) & M32 for v in n], np.float64)
        z = (H * X * e[None, :]).sum(1) * np.exp(2j * np.pi * k / 4294967296.0)
        for comp, want in ((0, z.real), (1, z.imag)):
            diff = np.abs(got[i, :, comp].astype(np.float64) - np.clip(want, -32768, 32767))
            worst = max(worst, float((diff / bound).max()))
            assert np.all(diff <= bound), (P, Q, i, comp, int(np.argmax(diff - bound)), float(diff.max()))
    print(f"rate {P} / {Q}: worst |diff| / bound = {worst:.3f}")


def test_rate_is_a_receiver_at_2400_kHz(rdsp):
    """8000 / 147 (a source at 2.4 MHz), 36 blocks, a USB station at +600 kHz carrying a tone 1 000 Hz above it at a quarter of
    full scale: the tuned row holds it at TuningOffset + 1 000 = 6 390 Hz exactly on its bin (4 410 samples, bins 10 Hz
    apart) with the amplitude within the ripple bound (0.001 dB) plus one count, and EVERY OTHER BIN at least 85 dB below it:
    the images are >= 89 dB down, the phasor error 2^-17 is about -102 dB, int16 rounding at this amplitude over 4 410 bins
    about -120 dB -- a wrong branch or window anywhere in the schedule shows at about -40 dB.  Then a 0.9 full-scale interferer
    at station - TuningOffset + 44 100 + 7 890 Hz, which the shift puts at 51 990 Hz and the resampling would fold onto 7 890 Hz
    in the IF band: no sample of the tuned row moves by more than 2 counts (0.9 x 32767 x 10^(-89 / 20) = 1.05 before
    rounding; test_engine_ddc's derivation)"""
    tab = table(rdsp)
    P, Q, nb = 8000, 147, 36
    fs, n = _fs(P, Q), _pairs(P, Q, nb)
    assert fs == 2400000.0
    h = lib_taps(P, Q)
    to = TUNING_OFFSET[1]
    steps = np.full((1, nb), dphi_of(to, 600000.0, P, Q), np.uint64)
    amp = 0.25 * 32767
    y = stream(_int16(_tone(601000.0, n, fs, amp)), P, Q, h, steps, tab)[0][0]
    z = (y[128:128 + 4410, 0] + 1j * y[128:128 + 4410, 1]).astype(np.complex128)
    spec = np.abs(np.fft.fft(z))
    peak = int(np.argmax(spec))
    assert abs(np.fft.fftfreq(4410, 1 / 44100.0)[peak] - (to + 1000.0)) < 1e-6
    got = abs(np.mean(z * np.exp(-2j * np.pi * (to + 1000.0) / 44100.0 * np.arange(4410))))
    print(f"rate receiver: amplitude {got:.3f} of {amp:.3f}")
    assert abs(got - amp) <= amp * (10 ** (0.001 / 20) - 1) + 1.0
    rest = np.delete(spec, peak).max()
    print(f"rate receiver: the strongest other bin is {20 * np.log10(rest / spec[peak]):.2f} dB")
    assert 20 * np.log10(rest / spec[peak]) <= -85.0
    f_int = 600000.0 - to + 44100.0 + 7890.0
    a = 0.09 * 32767
    clean = stream(_int16(_tone(601000.0, n, fs, a)), P, Q, h, steps, tab)[0][0]
    dirty = stream(_int16(_tone(601000.0, n, fs, a) + _tone(f_int, n, fs, 0.9 * 32767, 1.0)), P, Q, h, steps, tab)[0][0]
    moved = np.abs(dirty.astype(int) - clean.astype(int))[16:].max()       # behind the filter's own length
    print(f"rate receiver: the folding interferer moves a sample by at most {moved} counts")
    assert moved <= 2


@pytest.mark.parametrize("P,Q", [(160, 147), (2500, 441)])
def test_rate_restatement_does_not_depend_on_the_call_split(rdsp, P, Q):
    """32 blocks in one call, against calls of 1, 7 and 32 blocks with frac, the history and the phases carried: sample for
    sample; and the phases after the stream are the closed form floor(M P / Q) x dphi"""
    tab = table(rdsp)
    nb = 32
    src = wide(3, 1, nb, P, Q)[0]
    h = lib_taps(P, Q, 1.5)
    r = np.random.default_rng(4)
    lim = (22000.0 * P) / Q
    dphi = np.array([dphi_of(TUNING_OFFSET[m], s, P, Q) for m, s in zip((0, 1, 4), r.uniform(-lim, lim, 3))], np.uint64)
    steps = np.repeat(dphi[:, None], nb, 1)
    whole, ph = stream(src, P, Q, h, steps, tab)
    assert [int(p) for p in ph] == [(((nb * 128 * P) // Q) * int(d)) & M32 for d in dphi]
    for split in (1, 7, 32):
        cut, ph2 = stream(src, P, Q, h, steps, tab, cuts=range(0, nb, split))
        assert np.array_equal(cut, whole) and np.array_equal(ph, ph2), split


# ---- GPU ------------------------------------------------------------------------------------------------------------------
_stream_cache = {}


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 7, 32])
@pytest.mark.parametrize("P,Q", [(3, 2), (160, 147), (2500, 441), (8000, 147)])
def test_gpu_rate_against_the_restatement(rdsp, P, Q, split):
    """3 sources x 97 receivers (the sources' workgroups ragged) at stations anywhere in |f| < 22 050 P / Q, gain 2.5, 40
    blocks (24 at 8000 / 147) cut into calls of `split`, with a retune, a regrouping and mode changes in mid-stream
    (engine_sources_model._script_97): every receiver against the restatement of its own row and calls, bit for bit.  The calls
    walk through one long device buffer without a copy; in the 7-block runs every call's rows start at an odd pair offset
    (rows 4-byte aligned only).  What the CPU side computes does not depend on the split: once per rate."""
    nch, nb, gain = 97, (24 if (P, Q) == (8000, 147) else 40), 2.5
    r = np.random.default_rng(20 + P)
    src = wide(40 + P, 3, nb, P, Q)
    source_of = r.integers(0, 3, nch)
    lim = (22050.0 * P) / Q
    stations = r.uniform(-lim + 1, lim - 1, nch)
    stations[:3] = [lim - 0.5, -lim + 0.5, 0.0]
    eng = engine(nch, 32)
    eng.sketch_setup()
    R = Rx(eng, src, source_of, [0, 19, 40, 58, 77], stations, P, Q, gain, odd=split == 7)
    assert R.nb == nb
    _script_97(R, split, nb)
    y = R.result()
    if (P, Q) not in _stream_cache:
        R.restate(range(nch))
        _stream_cache[(P, Q)] = (R.steps, R.calls, [R.want(c) for c in range(nch)])
    steps, calls, want = _stream_cache[(P, Q)]
    assert steps == R.steps and calls == R.calls
    for c in range(nch):
        assert np.array_equal(y[c], want[c]), (c, int(np.argmax(y[c] != want[c])))
    eng.close()


@pytest.mark.gpu
def test_gpu_rate_more_than_a_workgroup_of_receivers_on_one_source(rdsp):
    """one source at 160 / 147, 4 blocks, 256 + 44 receivers: one full workgroup of the kernel (four waves: two halves of 128
    receivers, two receivers a lane) and a ragged one whose only wave with receivers is ragged (44 of its lanes have one
    receiver, none has two): the first and the last receiver of each workgroup, of each wave's half and of each lane block,
    bit for bit"""
    P, Q, nch, nb = 160, 147, 300, 4
    src = wide(11, 1, nb, P, Q)
    lim = (22050.0 * P) / Q
    eng = engine(nch, nb)
    eng.sketch_setup()
    R = Rx(eng, src, [0] * nch, [0], np.random.default_rng(12).uniform(-lim + 1, lim - 1, nch), P, Q, 2.0)
    R.run(0, nb, nb)
    R.check(R.result(), [0, 1, 63, 64, 127, 128, 191, 192, 254, 255, 256, 257, 298, 299])
    eng.close()


@pytest.mark.gpu
def test_gpu_rate_q_one_is_the_integer_pass(rdsp):
    """set_source_rate(10, 2, g) IS set_source_decimation(5, g): equal audio on the same stream, source_decimation() 5 and
    source_rate() (5, 1); after a rational rate source_decimation() is 0; a later set_source_decimation replaces the
    rational rate (the audio is again that of an engine that only ever had D = 5)"""
    import torch
    D, nb, g = 5, 8, 2.0
    src = torch.from_numpy(wide(31, 2, nb, D)).cuda()
    st = np.random.default_rng(5).uniform(-D * 22000.0, D * 22000.0, 6)
    engs = [engine(6, nb) for _ in range(3)]
    for k, e in enumerate(engs):
        e.sketch_setup()
        e.set_sources(2, [0, 1, 1, 0, 1, 0])
        if k == 0:
            e.set_source_decimation(D, g)
        elif k == 1:
            e.set_source_rate(10, 2, g)
        else:
            e.set_source_rate(160, 147, g)
            assert e.source_decimation() == 0 and e.source_rate() == (160, 147) and e.source_pairs(1) == 139
            e.set_source_decimation(D, g)
        assert e.source_decimation() == D and e.source_rate() == (D, 1) and e.source_pairs(3) == 3 * 128 * D
        e.tune(0, st)
    y = [e.update_sources(src).cpu().numpy() for e in engs]
    assert y[0].any() and np.array_equal(y[0], y[1]) and np.array_equal(y[0], y[2])
    y1 = engs[1].update_sources(src, n_blocks=nb).cpu().numpy()               # n_blocks is allowed with an integer rate
    assert np.array_equal(y1, engs[0].update_sources(src).cpu().numpy())
    for e in engs:
        e.close()


@pytest.mark.gpu
def test_gpu_rate_reset_and_state_as_data(rdsp):
    """160 / 147.  Reset zeroes frac and the source histories: the same rows after a reset (made after 9 blocks, where frac is
    not 0) give the same audio as the first time and as a fresh engine.  A receiver saved in one engine after 9 blocks and
    loaded into another engine (another channel count, index and call size) that heard the same source stream continues bit
    for bit; the blob sizes are those of an engine with sources at D = 1 (16 + n (10 368 + 4) bytes)"""
    P, Q, nb, k, gain = 160, 147, 24, 9, 2.0
    assert (k * 128 * P) % Q != 0
    r = np.random.default_rng(9)
    src = wide(61, 2, nb, P, Q)
    lim = (22050.0 * P) / Q
    a = engine(6, 8)
    a.sketch_setup()
    A = Rx(a, src, [0, 1, 1, 0, 1, 0], [0], r.uniform(-lim + 1, lim - 1, 6), P, Q, gain)
    A.run(0, nb, 8)
    first = A.result()
    A.check(first)
    a.reset()
    A.outs = []
    A.run(0, k, 3)
    a.reset()
    A.outs = []
    assert a.source_pairs(8) == _pairs(P, Q, 8)
    A.run(0, nb, 8)
    assert np.array_equal(A.result(), first)
    fresh = engine(6, 8)
    fresh.sketch_setup()
    Fr = Rx(fresh, src, A.source_of, [0], A.station, P, Q, gain)
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
    B = Rx(b, src, [0] * 5 + [1, 0] + [1] * 2, [0], r.uniform(-lim + 1, lim - 1, 9), P, Q, gain)
    B.tune(5, A.station[2:4])
    B.run(0, k, 16)
    b.load_state(5, blob)
    B.outs = []
    B.run(k, nb, 16)
    y = B.result()
    assert np.array_equal(y[5], first[2, k * 128:]) and np.array_equal(y[6], first[3, k * 128:])


@pytest.mark.gpu
def test_gpu_rate_refusals(rdsp):
    """refused with nothing changed: set_source_rate before set_sources (NOT_READY); Q of 0, Q = 442 after reduction, P < Q, P >
    64 Q, a gain of 0, NaN, inf; a rate under which a tuned station falls outside the band; a station at and beyond 22 050 P /
    Q; a src_stride below source_pairs; more than max_blocks; the Python method without n_blocks -- the object then runs on
    exactly as a twin that never saw those calls"""
    import torch
    from radiodsp_sdr_rx_amd._lib import RdspError
    P, Q = 160, 147
    src = torch.from_numpy(wide(95, 2, 16, P, Q)).cuda()
    out = torch.empty((4, 8 * 128, 2), dtype=torch.int16, device="cuda")
    eng, twin = engine(4, 8), engine(4, 8)
    for e in (eng, twin):
        e.sketch_setup()
    with pytest.raises(RdspError) as ex:
        eng.set_source_rate(P, Q, 1.0)
    assert ex.value.code == -4 and b"set_sources" in eng.lib.rdsp_last_error()
    lim = (22050.0 * P) / Q
    for e in (eng, twin):
        e.set_sources(2, [0, 1, 1, 0])
        e.set_source_rate(P, Q, 3.0)
        e.tune(0, [-20000.0, 100.0, 4000.0, 23900.0])
    p0 = eng.source_pairs(8)
    assert p0 == _pairs(P, Q, 8)
    y = [e.update_sources(src[:, :p0], n_blocks=8).cpu().numpy() for e in (eng, twin)]
    frac_pairs = eng.source_pairs(8)
    for p, q, g in ((3, 0, 1.0), (885, 442, 1.0), (146, 147, 1.0), (65 * 147 + 1, 147, 1.0), (0, 1, 1.0), (-160, 147, 1.0), (P, Q, 0.0), (P, Q, -2.0),
                    (P, Q, float("nan")), (P, Q, float("inf")), (65, 64, 1.0), (1, 1, 1.0), (2, 2, 1.0)):
        with pytest.raises(RdspError) as ex:                 # 65 / 64, 1 / 1 and 2 / 2: channel 3 sits at 23.9 kHz
            eng.set_source_rate(p, q, g)
        assert ex.value.code == -1, (p, q, g)
    with pytest.raises(RdspError):
        eng.set_source_decimation(1, 1.0)                    # the same station, through the integer setter
    assert eng.source_rate() == (P, Q) and eng.source_decimation() == 0 and eng.source_pairs(8) == frac_pairs
    for first, st in ((0, [lim]), (1, [-lim]), (0, [float("nan")]), (0, [1000.0, 2000.0, 24001.0])):
        with pytest.raises(RdspError) as ex:
            eng.tune(first, st)
        assert ex.value.code == -1
    lib, o = eng.lib, out.data_ptr()
    rest = src[:, p0:]
    ptr, row = rest.data_ptr(), src.shape[1]
    assert lib.rdsp_engine_update_sources(eng.h, ptr, frac_pairs - 1, 8, o, 8 * 128, None) == -1    # shorter than source_pairs
    assert lib.rdsp_engine_update_sources(eng.h, ptr, 8 * 128, 8, o, 8 * 128, None) == -1           # long enough at 44 100 Hz only
    assert lib.rdsp_engine_update_sources(eng.h, ptr, row, 9, o, 8 * 128, None) == -1               # more than max_blocks
    assert lib.rdsp_engine_update_sources(eng.h, ptr + 2, row, 8, o, 8 * 128, None) == -1           # not on an int16 pair
    with pytest.raises(AssertionError):
        eng.update_sources(rest)                                                                    # a rational rate needs n_blocks
    with pytest.raises(AssertionError):
        eng.update_sources(rest[:, :frac_pairs - 1], n_blocks=8)                                    # fewer pairs than source_pairs
    assert eng.source_pairs(8) == frac_pairs
    y2 = [e.update_sources(rest, n_blocks=8).cpu().numpy() for e in (eng, twin)]
    assert np.array_equal(y[0], y[1]) and np.array_equal(y2[0], y2[1])
    assert y[0].any() and y2[0].any()
