"""rdsp_channelizer_t, the part that needs no GPU (include/rdsp.h "channelizer"; host half csrc/rdsp_channelizer_host.cpp): the
rate, the prototype, the twiddles and the placement against tests/channelizer_model.py; the model's float32 arithmetic against a
float64 evaluation of the definition inside the bound of its fmaf chains; the signal path of a receiver behind a sub-band in
the model alone (stage 1, then the engine's decimating pass as tests/engine_sources_model.py restates it); and
tests/host/host_channelizer_check.cpp, a program of its own, plain and under the address and undefined-behaviour sanitizers.

The bound of test_model_against_float64: every fold chain has at most ceil(Tb / M) fmaf, the DFT chain of a component 2 M, and
each twiddle carries one rounding: (ceil(Tb / M) + 2 M + 1) 2^-24 A to first order, A = sum_j |hb[r][j]| (|xI| + |xQ|) (every
twiddle is at most 1 in magnitude, so A bounds the sum of the magnitudes of either chain's terms); the issue's constant has
+ 2, which leaves room for the second-order terms.  Worst observed fraction of it: 0.07 on the six configurations, 0.13 on the
edges of CM.EDGE (printed).  The model's own parts have tests here too: the EDGE list's facts, Model.call's at=, and fma32 and
fmaf against rational arithmetic where results are subnormal."""
import math
import os
import subprocess

import numpy as np
import pytest

import channelizer_model as CM
from engine_sources_model import (FL, HERE, ROOT, S16, TUNING_OFFSET, _int16, _tone, call_rows, dphi_of, lib_taps, table, taps_of, values)

F32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- taps, twiddles, place, rate --------------------------------------------------------------------------------------------
def test_rate_and_taps(rdsp):
    """rdsp_channelizer_rate is P / (Q D2) in lowest terms; rdsp_channelizer_taps is rdsp_engine_rate_taps(P1, Q1, 1.0) times
    2^-15 bit for bit (and the numpy formula's); over the six configurations the float taps (times 2^15 / Q1) keep the family's
    figures: ripple <= 0.001 dB on |f| <= 12000 D2, <= -89 dB from 32100 D2 to the prototype's Nyquist frequency, branch sum <= 2.5"""
    from radiodsp_sdr_rx_amd import channelizer as ch
    for P, Q, M, D2 in CM.CONFIGS:
        P1, Q1 = ch.rate(P, Q, D2)
        assert (P1, Q1) == CM.rate(P, Q, D2) and CM.accepted(P, Q, M, D2)
        h = ch.taps(P, Q, D2)
        Tb = 16 * -(-P1 // Q1)
        assert h.dtype == F32 and h.size == Tb * Q1
        assert np.array_equal(_bits(h), _bits(lib_taps(P1, Q1, 1.0) * F32(2.0 ** -15))), (P, Q, D2)
        assert np.array_equal(_bits(h), _bits(CM.taps(P, Q, D2))) and np.array_equal(_bits(h), _bits(h[::-1]))
        g = h.astype(np.float64) * 32768.0
        fs = 44100.0 * D2 * P1                                       # the prototype's rate: the source's times Q1
        nfft = 1 << int(math.ceil(math.log2(16 * g.size)))
        H = np.abs(np.fft.rfft(g / Q1, nfft))
        f = np.fft.rfftfreq(nfft, 1 / fs)
        ripple = np.abs(20 * np.log10(H[f <= 12000.0 * D2])).max()
        stop = (20 * np.log10(np.maximum(H[f >= 32100.0 * D2], 1e-300))).max()
        branch = np.abs(g).reshape(Tb, Q1).sum(0).max()
        print(f"({P}, {Q}, {M}, {D2}): P1 / Q1 = {P1} / {Q1}, Tb = {Tb}, ripple {ripple:.6f} dB, stop band {stop:.2f} dB, worst branch sum |hb| {branch:.3f}")
        assert ripple <= 0.001 and stop <= -89.0 and branch <= 2.5, (P, Q, M, D2, ripple, stop, branch)


@pytest.mark.parametrize("M", [8, 16, 32, 64])
def test_twiddles(rdsp, M):
    """within half an ulp of the float64 values, exactly 0 and +-1 at quarter turns, the same magnitudes in every octant, and
    the numpy restatement's bits"""
    from radiodsp_sdr_rx_amd import channelizer as ch
    t = ch.twiddles(M)
    assert t.dtype == F32 and t.shape == (M, 2) and np.array_equal(_bits(t), _bits(CM.twiddles(M)))
    a = 2.0 * np.pi * np.arange(M) / M
    want = np.stack([np.cos(a), np.sin(a)], 1)
    ulp = np.spacing(np.abs(want).astype(F32)).astype(np.float64)     # of the float below or at the value: the float's own or half of it
    at_quarter = (np.arange(M) % (M // 4) == 0)
    err = np.abs(t.astype(np.float64) - want)
    assert np.all(err[~at_quarter] <= 0.5 * ulp[~at_quarter]), float((err[~at_quarter] / ulp[~at_quarter]).max())
    for turn, (c, s) in enumerate([(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]):
        assert t[turn * M // 4, 0] == c and t[turn * M // 4, 1] == s
    assert not np.any(np.signbit(t[t == 0.0]))
    for m in range(M):
        assert t[(M - m) % M, 0] == t[m, 0] and t[(M - m) % M, 1] == -t[m, 1]           # conjugate
        assert t[(m + M // 4) % M, 0] == -t[m, 1] and t[(m + M // 4) % M, 1] == t[m, 0]  # a quarter turn on
        assert t[(M // 4 - m) % M, 0] == t[m, 1]                                        # mirrored in the octant's edge
    with pytest.raises(rdsp.RdspError):
        ch.twiddles(12)


def test_place(rdsp):
    """kk = round half away from zero (station / spacing), subband = kk mod M >= 0, residual = station - kk spacing: at +-half a
    spacing, at sub-band M / 2, at negative stations, over drawn stations (the array form equals the scalar call), and the
    refusals at and beyond +-fs / 2 and for NaN"""
    from radiodsp_sdr_rx_amd import channelizer as ch
    for P, Q, M, D2 in CM.CONFIGS:
        fs = (P * 44100.0) / Q
        sp = fs / M
        assert ch.place(P, Q, M, sp / 2) == (1, -sp / 2) and ch.place(P, Q, M, -sp / 2) == (M - 1, sp / 2)
        assert ch.place(P, Q, M, np.nextafter(sp / 2, 0.0)) == (0, np.nextafter(sp / 2, 0.0))
        assert ch.place(P, Q, M, 0.0) == (0, 0.0) and ch.place(P, Q, M, -1.0) == (0, -1.0)
        k, res = ch.place(P, Q, M, -(fs / 2 - 1.0))                   # the band's lower edge belongs to sub-band M / 2
        assert k == M // 2 and res == -(fs / 2 - 1.0) + (M // 2) * sp
        k, res = ch.place(P, Q, M, fs / 2 - 1.0)
        assert k == M // 2 and res == (fs / 2 - 1.0) - (M // 2) * sp
        assert ch.place(P, Q, M, -3 * sp + 100.0) == (M - 3, 100.0)
        st = np.random.default_rng(M + D2).uniform(-fs / 2, fs / 2, 500)
        st[:4] = [sp / 2, -sp / 2, 2.5 * sp, -2.5 * sp]
        ks, rs = ch.place(P, Q, M, st)
        for s, k, r in zip(st, ks, rs):
            assert (k, r) == ch.place(P, Q, M, float(s)) == CM.place(P, Q, M, float(s)) and abs(r) <= sp / 2
            assert abs(CM.centre_hz(P, Q, M, k) + r - s) <= 1e-9 * fs or abs(abs(CM.centre_hz(P, Q, M, k) + r - s) - fs) <= 1e-9 * fs
        for bad in (fs / 2, -fs / 2, fs, float("nan")):
            with pytest.raises(rdsp.RdspError):
                ch.place(P, Q, M, bad)
            with pytest.raises(rdsp.RdspError):
                ch.place(P, Q, M, np.array([0.0, bad]))
    with pytest.raises(rdsp.RdspError):
        ch.place(16, 1, 12, 0.0)


def test_refusals_of_the_host_calls(rdsp):
    """what include/rdsp.h lists: 8000 / 147 with M = 32, D2 = 4 and 2500 / 441 with M = 8, D2 = 2 fail the band condition (the
    rate itself is fine), 10240 / 441 with D2 = 3 has Q1 = 1323; and the limits of D2 and of the source rate"""
    from radiodsp_sdr_rx_amd import channelizer as ch
    assert [CM.accepted(*c) for c in CM.REFUSED] == [False] * 3 and all(CM.accepted(*c) for c in CM.CONFIGS)
    assert ch.rate(8000, 147, 4) == (2000, 147) and ch.rate(2500, 441, 2) == (1250, 441)
    assert CM.rate(10240, 441, 3) == (10240, 1323)
    for P, Q, D2 in ((10240, 441, 3), (2, 1, 4), (16, 1, 1), (16, 1, 65), (65, 1, 2), (147, 160, 2), (0, 1, 2)):
        with pytest.raises(rdsp.RdspError):
            ch.rate(P, Q, D2)
        with pytest.raises(rdsp.RdspError):
            ch.taps(P, Q, D2)
    assert rdsp.Channelizer is ch.Channelizer


# ---- the model against a float64 evaluation of the definition --------------------------------------------------------------
def _rails(rng, S, pairs):
    x = rng.integers(-32768, 32768, (S, pairs, 2)).astype(np.int16)
    x[0, :200] = [[-32768, 32767], [32767, -32768]] * 100
    x[0, 200:300] = 32767
    return x


@pytest.mark.parametrize("cfg", CM.CONFIGS + CM.EDGE)
def test_model_against_float64(cfg):
    """every output of the float32 restatement lies within (ceil(Tb / M) + 2 M + 2) 2^-24 A of the float64 evaluation (the
    module's docstring has the derivation), on full-scale noise with rows on the rails, over two calls; the six configurations
    and the edges of CM.EDGE"""
    P, Q, M, D2 = cfg
    m = CM.Model(2, P, Q, M, D2)
    rng = np.random.default_rng(5)
    worst = 0.0
    for nb in (1, 1):
        pairs = m.source_pairs(nb)
        vals = values(S16, _rails(rng, 2, pairs))
        want, A = m.call(vals, nb, exact=True)
        got = m.call(vals, nb).astype(np.float64)
        bound = (-(-m.Tb // M) + 2 * M + 2) * 2.0 ** -24 * np.repeat(A, M, 0)[..., None]
        frac = np.abs(got - want) / bound
        worst = max(worst, float(frac.max()))
        assert np.all(np.abs(got - want) <= bound), (cfg, float(frac.max()))
    print(f"{cfg}: worst fraction of the bound {worst:.4f}")


def test_edge_list_keeps_its_purpose():
    """CM.EDGE beside CM.EDGE_FACTS: every entry is accepted and new, has the Tb and the T mod M after 1, 2 and 3 blocks that the
    list states, and the list still holds what it was made for: M = 16 with T mod M != 0 (one entry at Q1 = 441), P1 = Q1,
    Tb < M, Tb = M, the top rate with the largest tile the GPU tests stage, M = 64 at D2 = 2, and D2 = 16"""
    assert len(CM.EDGE) == len(CM.EDGE_FACTS) == len(set(CM.EDGE)) and not set(CM.EDGE) & set(CM.CONFIGS)
    seen = {}
    for cfg, (Tb, tmods, why) in zip(CM.EDGE, CM.EDGE_FACTS):
        P, Q, M, D2 = cfg
        assert CM.accepted(*cfg), cfg
        m = CM.Model(1, *cfg)
        got = tuple(m.source_pairs(nb) % M for nb in (1, 2, 3))
        print(f"{cfg}: P1 / Q1 = {m.P1} / {m.Q1}, Tb = {m.Tb}, T mod M after 1, 2, 3 blocks {got}: {why}")
        assert m.Tb == Tb and got == tmods, (cfg, m.Tb, got)
        seen[cfg] = (m, got)
    m16 = [c for c in CM.EDGE if c[2] == 16 and all(seen[c][1])]
    assert len(m16) >= 2 and any(seen[c][0].Q1 == 441 for c in m16)
    assert any(m.P1 == m.Q1 for m, _ in seen.values())
    assert any(m.Tb < m.M and m.M == 64 for m, _ in seen.values()) and any(m.Tb == m.M for m, _ in seen.values())
    assert any(c[0] == 64 * c[1] and c[2] == 64 for c in CM.EDGE)
    assert any(c[2] == 64 and c[3] == 2 and all(seen[c][1]) for c in CM.EDGE) and max(c[3] for c in CM.EDGE) == 16

    def tile(c):                                            # the kernel's LDS plan in bytes: (M 64 + 79 Dc1) float2
        P1, Q1 = CM.rate(c[0], c[1], c[3])
        return (c[2] * 64 + 79 * -(-P1 // Q1)) * 8

    assert max(map(tile, CM.EDGE)) == tile((64, 1, 64, 3)) == 46672 > max(map(tile, CM.CONFIGS))


def test_call_at():
    """Model.call(..., at=idx) gives the columns idx of the whole call, bit for bit, and leaves the state the whole call leaves:
    the next call's rows are the same either way.  (640, 147, 8, 2): frac and T mod M are non-zero after the first call"""
    cfg = (640, 147, 8, 2)
    a, b = CM.Model(2, *cfg), CM.Model(2, *cfg)
    rng = np.random.default_rng(11)
    vals = values(S16, _rails(rng, 2, a.source_pairs(3)))
    idx = np.concatenate([[0, 1, 63, 64, 255, 256, 2 * 256 - 1], rng.integers(0, 2 * 256, 40)])
    p2 = a.source_pairs(2)
    whole = a.call(vals[:, :p2], 2)
    some = b.call(vals[:, :p2], 2, at=idx)
    assert some.shape == (2 * 8, len(idx), 2) and np.array_equal(_bits(some), _bits(whole[:, idx]))
    assert (a.frac, a.T) == (b.frac, b.T) and a.frac != 0 and a.T % 8 != 0 and np.array_equal(_bits(a.hist), _bits(b.hist))
    assert b.call(vals[:, :p2], 0, at=[]).shape == (16, 0, 2) and (a.frac, a.T) == (b.frac, b.T)
    p1 = a.source_pairs(1)
    assert np.array_equal(_bits(a.call(vals[:, p2:p2 + p1], 1)), _bits(b.call(vals[:, p2:p2 + p1], 1)))


def _round_f32(x):
    """a Fraction rounded to the nearest float32, ties to even, subnormals included (no overflow here)"""
    from fractions import Fraction
    if x == 0:
        return F32(0.0)
    e = -126
    while abs(x) >= Fraction(2) ** (e + 1):
        e += 1
    quantum = Fraction(2) ** (e - 23)                       # float32's spacing at |x|; 2^-149 below 2^-125
    q = x / quantum
    n = q.numerator // q.denominator
    rem = q - n
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return F32(float(n * quantum))                          # n quantum has at most 25 bits: exact in double, exact or 2^e+1 in float32


def test_fma32_where_results_are_subnormal():
    """fma32 and fmaf against a b + c in rational arithmetic, rounded once: 480 triples whose results are subnormal (drawn),
    lie on a midpoint of the subnormal grid or 2^-196 beside one (where the double sum lands ON the midpoint and only the
    TwoSum error says which side), or lie just above 2^-126 up to 2^-124; taken as one array and one by one (above 2^-125 a
    lone triple takes fma32's short cut)"""
    from fractions import Fraction
    from engine_sources_model import fma32, fmaf
    r = np.random.default_rng(17)
    u = lambda e: F32(2.0 ** e)
    trip = []
    for lo, hi in ((0, 1 << 10), (1 << 18, 1 << 23), (1 << 23, 1 << 24), (1 << 24, 1 << 25)):      # c = +-k 2^-149 (k even above 2^24)
        for _ in range(24):
            k = int(r.integers(lo, hi))
            k -= k % 2 if k >= 1 << 24 else 0
            c = F32(float(k) * 2.0 ** -149) * F32(r.choice([-1.0, 1.0]))
            for a, b in ((u(-100), F32(r.choice([1.0, 3.0, -1.0, -3.0])) * u(-50)),                  # a b = +-j 2^-150: half a step
                         (u(-75) * F32(1 + 2.0 ** -23), u(-75) * F32(1 - 2.0 ** -23) * F32(r.choice([-1.0, 1.0]))),   # +-(2^-150 - 2^-196)
                         (u(-75) * F32(1 + 2.0 ** -23), u(-75) * F32(1 + 2.0 ** -23) * F32(r.choice([-1.0, 1.0]))),   # +-(2^-150 + 2^-172 + 2^-196)
                         (F32(r.uniform(-2, 2)) * u(-60), F32(r.uniform(-2, 2)) * u(-80)),
                         (F32(r.uniform(-2, 2)) * u(-70), F32(r.uniform(-2, 2)) * u(-75))):
                trip.append((a, b, c))
    a, b, c = (np.array(v, F32) for v in zip(*trip))
    want = np.array([_round_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in trip], F32)
    tiny = np.abs(want) < F32(2.0 ** -126)
    assert len(trip) == 480 and tiny.sum() >= 200 and (~tiny).sum() >= 150 and (np.abs(want) >= F32(2.0 ** -125)).sum() >= 60
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    assert (np.abs(s).astype(F32) != np.abs(want)).sum() >= 10, "no triple on which rounding the double sum goes wrong"
    assert np.array_equal(_bits(fmaf(a, b, c)), _bits(want)) and np.array_equal(_bits(fma32(a, b, c)), _bits(want))
    one = np.array([fma32(x, y, z) for x, y, z in trip], F32)
    assert np.array_equal(_bits(one), _bits(want)), int(np.argmax(_bits(one) != _bits(want)))


# ---- signal path, model only ------------------------------------------------------------------------------------------------
def _receiver_amplitude(rdsp, cfg, k, tone_hz, station_hz, amp, nb=36):
    """a complex tone of `amp` counts at tone_hz in an int16 source; a receiver (LSB, gain 1) placed on station_hz: sub-band k of
    stage 1, then the decimating pass at D2 on the float row -> the amplitude of the IF line (TuningOffset, on its bin of 4410
    samples) in counts"""
    P, Q, M, D2 = cfg
    fs = (P * 44100.0) / Q
    kk, res = CM.place(P, Q, M, station_hz)
    assert kk == k
    m = CM.Model(1, P, Q, M, D2)
    src = _int16(_tone(tone_hz, m.source_pairs(nb), fs, amp))[None]
    row = m.call(values(S16, src), nb, ks=[k])[0]                               # float32 [n_out, 2], full scale +-1
    xh = np.concatenate([np.zeros((15 * D2, 2), F32), values(FL, row)])
    to = TUNING_OFFSET[0]
    y = call_rows(xh, D2, 1, 0, taps_of(D2, 1, 1.0), [dphi_of(to, res, D2, 1)], [0], table(rdsp), nb * 128)[0]
    z = (y[128:128 + 4410, 0] + 1j * y[128:128 + 4410, 1]).astype(np.complex128)
    return abs(np.mean(z * np.exp(-2j * np.pi * to / 44100.0 * np.arange(4410))))


@pytest.mark.parametrize("cfg,k", [((640, 147, 8, 2), 3), ((16, 1, 16, 3), 5)])
def test_signal_path(rdsp, cfg, k):
    """a tone of 8000 counts at a station half a spacing less 1 Hz above sub-band k's centre arrives at the receiver's IF with
    A gain (gain 1) within 0.002 dB (two stages' ripple) plus one count; moved by +-fo = +-44100 D2 Hz it would fold onto the
    station: it reads at most A 10^(-89 / 20) plus one count"""
    P, Q, M, D2 = cfg
    sp = (P * 44100.0) / Q / M
    station = CM.centre_hz(P, Q, M, k) + sp / 2 - 1.0
    A = 8000.0
    got = _receiver_amplitude(rdsp, cfg, k, station, station, A)
    print(f"{cfg}: station {station:.1f} Hz, sub-band {k}: {got:.3f} counts of {A:.0f} ({20 * np.log10(got / A):+.5f} dB)")
    assert abs(got - A) <= A * (10 ** (0.002 / 20) - 1) + 1.0
    for sign in (1.0, -1.0):
        leak = _receiver_amplitude(rdsp, cfg, k, station + sign * 44100.0 * D2, station, A)
        print(f"{cfg}: the tone at station {sign * 44100.0 * D2:+.0f} Hz reads {leak:.4f} counts")
        assert leak <= A * 10 ** (-89.0 / 20) + 1.0


# ---- the host program --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_host_program(tmp_path, sanitize):
    """tests/host/host_channelizer_check.cpp with csrc/rdsp_channelizer_host.cpp, plain and under ASan + UBSan, run directly:
    what it prints for the six configurations equals the numpy restatement, and its own checks and refusals pass"""
    exe = str(tmp_path / ("host_channelizer_check_san" if sanitize else "host_channelizer_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    csrc = os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "include"), "-I", csrc,
                           os.path.join(HERE, "host", "host_channelizer_check.cpp"), os.path.join(csrc, "rdsp_channelizer_host.cpp"), "-o", exe])
    out = subprocess.run([exe] + [str(v) for c in CM.CONFIGS for v in c], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.endswith("host_channelizer_check OK\n"), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
    lines = out.stdout.splitlines()[:-1]
    assert len(lines) == 5 * len(CM.CONFIGS)
    for (P, Q, M, D2), at in zip(CM.CONFIGS, range(0, len(lines), 5)):
        h = CM.taps(P, Q, D2)
        fnv = 1469598103934665603
        for b in h.tobytes():
            fnv = ((fnv ^ b) * 1099511628211) & ((1 << 64) - 1)
        P1, Q1 = CM.rate(P, Q, D2)
        assert lines[at] == f"config {P} {Q} {M} {D2} rate {P1} {Q1} taps {h.size} {fnv:016x}"
        assert lines[at + 1] == "twiddles " + " ".join(f"{int(b):08x}" for b in _bits(CM.twiddles(M)).reshape(-1))
        fs = (P * 44100.0) / Q
        for i, st in enumerate((fs / M / 2, -(fs / M) / 2, -(fs / 2 - 1.0))):
            w = lines[at + 2 + i].split()
            k, r = CM.place(P, Q, M, st)
            assert w[0] == "place" and float.fromhex(w[1]) == st and int(w[2]) == k and float.fromhex(w[3]) == r
