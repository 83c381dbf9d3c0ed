"""The noise squelch of rdsp_engine_t without a GPU (include/rdsp.h "noise squelch"; csrc/rdsp_noise.h,
csrc/rdsp_engine_noise_host.hip): the exports, every refusal that needs no device, rdsp_engine_noise_taps against
tests/engine_noise_model.py bit for bit with the filter's figures printed, the float32 model against a float64 evaluation of the
same taps, the detector's figures on the demodulated rows of tests/engine_fm_model.py (empty channels, strong, off-centre and
weak stations; both W, both time constants) with the defaults held to them, a station that stops, and
tests/host/host_noise_check.cpp -- csrc/rdsp_noise.h as a program of its own, plain and under ASan + UBSan, run directly --
against the model's bits at every cut of 1 to 3 blocks.  tests/test_engine_noise_gpu.py holds the kernel to the same model."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import engine_fm_model as FM
import engine_noise_model as NZ

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
D = NZ.DEFAULTS


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_noise_exports(rdsp):
    from radiodsp_sdr_rx_amd import engine
    lib = rdsp.load()
    for name in ("enable_noise", "noise_enabled", "set_noise_squelch", "read_noise", "noise_taps"):
        assert hasattr(lib, "rdsp_engine_" + name), name
    assert callable(engine.noise_taps) and (engine.NOISE_OFF, engine.NOISE_MEASURE, engine.NOISE_GATE) == (0, 1, 2)
    assert all(callable(getattr(engine.Engine, n)) for n in ("enable_noise", "set_noise_squelch", "read_noise"))
    assert isinstance(engine.Engine.noise_enabled, property)


def test_noise_refusals_without_a_device(rdsp):
    """no object: every entry point refuses; rdsp_engine_noise_taps refuses a NULL array and a time constant rdsp_engine_set_fm
    refuses, with the array untouched.  The refusals that need an object are test_engine_noise_gpu's"""
    from radiodsp_sdr_rx_amd.engine import noise_taps
    lib = rdsp.load()
    assert lib.rdsp_engine_enable_noise(None) == -1 and lib.rdsp_engine_noise_enabled(None) == 0
    assert lib.rdsp_engine_set_noise_squelch(None, 2, 0.01, 0.025, 8, 0.75, 0.125) == -1 and b"rdsp_engine_set_noise_squelch" in lib.rdsp_last_error()
    assert lib.rdsp_engine_read_noise(None, 0, None, 0, None, 0, None) == -1
    out = (C.c_float * 65)(*([7.0] * 65))
    assert lib.rdsp_engine_noise_taps(750.0, None) == -1 and b"rdsp_engine_noise_taps" in lib.rdsp_last_error()
    for tau in (24.0, 1001.0, -1.0, float("nan"), float("inf")):
        assert lib.rdsp_engine_noise_taps(tau, out) == -1, tau
        with pytest.raises(rdsp.RdspError):
            noise_taps(tau)
    assert all(v == 7.0 for v in out)


def test_noise_taps_are_the_model_and_the_filter(rdsp):
    """rdsp_engine_noise_taps equals the model bit for bit at tau_us 0, 75 and 750; g[64] is 0 without de-emphasis.  The
    filter's figures, from the float taps, printed and held to the definition's: the prototype reads 0.0 dB at 6 kHz, -6 dB at
    8 kHz (and at 4.5 kHz), at most -63 dB up to 3 kHz, -37.6 dB at 3.4 kHz; the compensated taps at 750 us read -40 dB at
    3 kHz, and behind the de-emphasis they are the prototype again; sum |g| is 45.4 at 750 us and 1.55 at 0"""
    from radiodsp_sdr_rx_amd.engine import noise_taps
    for tau in (0.0, 75.0, 750.0):
        g, m = noise_taps(tau), NZ.taps(tau)
        assert g.dtype == F32 and g.shape == (65,) and np.array_equal(bits(g), bits(m)), tau
    g0, g750 = noise_taps(0.0), noise_taps(750.0)
    assert g0[64] == 0.0 and g750[64] != 0.0
    low = NZ.response_db(g0, np.arange(0.0, 3000.1, 25.0)).max()
    at = dict(zip((3400, 4500, 6000, 8000), NZ.response_db(g0, [3400.0, 4500.0, 6000.0, 8000.0])))
    comp = float(NZ.response_db(g750, 3000.0)[0])
    print(f"prototype: {at[6000]:+.3f} dB at 6 kHz, {at[8000]:.2f} dB at 8 kHz, {at[4500]:.2f} dB at 4.5 kHz, {at[3400]:.1f} dB at 3.4 kHz, "
          f"at most {low:.1f} dB up to 3 kHz; compensated (750 us): {comp:.1f} dB at 3 kHz; sum |g| = {np.abs(g750).sum():.2f} (750 us), "
          f"{np.abs(g0).sum():.3f} (0)")
    assert abs(at[6000]) < 0.01 and abs(at[8000] + 6.0) < 0.05 and abs(at[4500] + 6.0) < 0.05 and low <= -63.0 and abs(at[3400] + 37.6) < 0.1
    assert abs(comp + 40.0) < 0.1 and abs(np.abs(g750).sum() - 45.4) < 0.05 and abs(np.abs(g0).sum() - 1.55) < 0.01
    # behind the de-emphasis y <- y + a (u - y), whose response is a / (1 - r z^-1), the compensated taps are the prototype
    a = float(FM.constants(5000.0, 750.0)[1])
    f = np.array([500.0, 3000.0, 5000.0, 6000.0, 7500.0])
    z = np.exp(-2j * np.pi * f / 44100.0)
    de = 20.0 * np.log10(np.abs(a / (1.0 - (1.0 - a) * z)))
    assert np.abs(NZ.response_db(g750, f) + de - NZ.response_db(g0, f))[1:].max() < 0.01
    print(f"the de-emphasis at 6 kHz, 750 us: {de[3]:.1f} dB")


@functools.lru_cache(maxsize=None)
def _rows(W, tau_us, nb=400):
    """the demodulated rows of the figures, float32 [8, nb * 128]: empty channels at sigma 2120 and 21.2 counts (40 dB apart), a
    strong station (8000 counts, voice-band noise modulation at 0.35 rms of the deviation), the same 1500 Hz above and below the
    centre, weak stations of 1200, 750 and 480 counts over sigma 212"""
    x = np.stack([NZ.station(1, nb, 0, 2120.0), NZ.station(2, nb, 0, 21.2), NZ.station(3, nb, 8000.0, 3.0), NZ.station(4, nb, 8000.0, 3.0, 1500.0),
                  NZ.station(5, nb, 8000.0, 3.0, -1500.0), NZ.station(6, nb, 1200.0, 212.0), NZ.station(7, nb, 750.0, 212.0), NZ.station(8, nb, 480.0, 212.0)])
    return FM.Fm(len(x), W, 5000.0, tau_us).run(x)[0]


def test_noise_model_against_float64():
    """every computed output v_j of the float32 model lies within 66 x 2^-24 x sum_k |g_k| |a[.]| of the float64 sum on the same
    taps and samples -- the bound of a 65-term fused chain -- on the rows of the figures (32 blocks, W = 2, 750 us: the taps with
    the largest sum |g|), on a row on the rails and on uniform noise; the worst fraction of the bound is printed"""
    r = np.random.default_rng(5)
    y = np.concatenate([_rows(2, 750.0)[:, :32 * 128], r.choice(np.array([1.0, -1.0], F32), (1, 32 * 128)),
                        r.uniform(-1.0, 1.0, (1, 32 * 128)).astype(F32)])
    worst = 0.0
    for tau in (750.0, 0.0):
        g = np.broadcast_to(NZ.taps(tau), (len(y), 65))
        x = np.concatenate([np.zeros((len(y), 64), F32), y], 1)
        v, (v64, mag) = NZ.outputs(g, x, 32), NZ.outputs64(g, x, 32)
        bound = 66.0 * 2.0 ** -24 * mag
        assert np.all(np.abs(v.astype(np.float64) - v64) <= bound), tau
        worst = max(worst, float((np.abs(v.astype(np.float64) - v64) / np.maximum(bound, 1e-300)).max()))
    print(f"float32 chain against float64: worst error {worst:.3f} of the bound 66 x 2^-24 x sum |g| |a|")


@pytest.mark.parametrize("tau_us", [0.0, 750.0])
@pytest.mark.parametrize("W", [2, 3])
def test_noise_figures_and_defaults(W, tau_us):
    """the detector's figures on the float32 model, 400 blocks a row, printed; and the rule the defaults (0.01, 0.025, 8, 0.75,
    0.125) are held to: the empty-channel rows never open; the strong and the off-centre stations are open from at most the
    fourth block on and never close.  The two empty channels, 40 dB apart in level, read medians closer than either's
    block-to-block spread (its 10th to 90th percentile).  The weak stations read between the strong and the empty ones, in order
    (medians; printed, not held to a figure).  With fall = 0.5, the value proposed first, the strong station opens at the seventh
    block only: N has to come down from 1.0"""
    y = _rows(W, tau_us)
    m = NZ.Noise(len(y), NZ.GATE, W, tau_us)
    N, nopen = m.run(y)
    g = np.broadcast_to(NZ.taps(tau_us), (len(y), 65))
    s = np.sqrt(NZ.readings(NZ.outputs(g, np.concatenate([np.zeros((len(y), 64), F32), y], 1), y.shape[1] // 128)).astype(np.float64))
    med = np.median(s, 1)
    names = ("empty, sigma 2120", "empty, sigma 21.2", "strong", "+1500 Hz", "-1500 Hz", "1200 counts", "750 counts", "480 counts")
    for c, name in enumerate(names):
        print(f"W = {W}, tau_us = {tau_us:g}: {name:18s} sqrt(nz) median {med[c]:.4f}, range {s[c].min():.4f} ... {s[c].max():.4f} (after the first block "
              f"at most {s[c, 1:].max():.4f}); N {N[c].min():.5f} ... {N[c, 4:].max():.5f}; first open block {int(np.argmax(nopen[c])) if nopen[c].any() else None}")
    assert not nopen[:2].any()
    assert nopen[2:5, 3:].all()
    spread = [np.percentile(s[c], 90) - np.percentile(s[c], 10) for c in (0, 1)]
    assert abs(med[0] - med[1]) < min(spread), (med[:2], spread)
    assert med[2:5].max() < med[5] < med[6] < med[7] < med[:2].min()
    half = NZ.Noise(len(y), NZ.GATE, W, tau_us, fall=0.5).run(y[:, :16 * 128])[1]
    assert not half[2, :6].any() and half[2, 6:].all()


def test_noise_station_that_stops():
    """a strong station that stops after block 24 of 48, the channel empty behind it (noise of 3 counts): the gate is open from
    the fourth block on, N crosses close_n within a few blocks of the stop -- at most 15, what rise = 0.125 needs from N = 0 on
    the smallest empty-channel reading of the figures, rms 0.17; the model's count is printed -- and the gate closes exactly
    hang_blocks blocks after the crossing"""
    nb, stop = 48, 24
    x = NZ.station(9, nb, 8000.0, 3.0, until=stop * 128)[None]
    y = FM.Fm(1).run(x)[0]
    N, nopen = NZ.Noise(1).run(y)
    cross = stop + int(np.argmax(N[0, stop:] > F32(D["close_n"])))
    closed = int(np.flatnonzero(nopen[0] == 0)[-1]) if not nopen[0, -1] else None
    first_closed = stop + int(np.argmax(nopen[0, stop:] == 0))
    print(f"the station stops after block {stop - 1}: N crosses close_n at block {cross} ({cross - stop + 1} blocks), the gate closes at block {first_closed}; "
          f"N then reads {N[0, -1]:.4f}")
    assert nopen[0, 3:stop].all() and N[0, stop:].max() > D["close_n"] and cross - stop + 1 <= 15
    assert first_closed == cross + D["hang_blocks"] and closed == nb - 1 and not nopen[0, first_closed:].any()


def _crafted_rows(nb):
    """float32 [5, nb * 128]: a station that stops after block 8, an empty channel, a row on the rails (+-1 drawn), an all-zero
    row, a station 1500 Hz off centre"""
    r = np.random.default_rng(31)
    x = np.stack([NZ.station(11, nb, 8000.0, 3.0, until=8 * 128), NZ.station(12, nb, 0, 212.0), NZ.station(13, nb, 8000.0, 3.0, 1500.0)])
    y = FM.Fm(3).run(x)[0]
    return np.stack([y[0], y[1], r.choice(np.array([1.0, -1.0], F32), nb * 128), np.zeros(nb * 128, F32), y[2]]).astype(F32)


@pytest.mark.parametrize("sanitize", [False, True])
def test_noise_host_program(rdsp, tmp_path, sanitize):
    """tests/host/host_noise_check.cpp, plain and under ASan + UBSan, a program of its own run on the CPU: on the crafted rows (a
    station that stops, an empty channel, on the rails, all zeros, off centre), at mode 2 / W 2 / 750 us with the defaults and at
    mode 1 / W 3 / 0 us with other settings, in calls of 1, 2 and 3 blocks (which it holds to one long call itself), its key,
    taps, records and final words equal the model's.  The station that stops opens and closes; the empty channel and the rails
    stay closed; the all-zero row OPENS at its fourth block (N decays from 1.0: a dead source is not an empty channel); mode 0
    leaves zero words and zero records"""
    exe = str(tmp_path / ("host_noise_check_san" if sanitize else "host_noise_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_noise_check.cpp"), "-o", exe])
    nb = 30
    rows = _crafted_rows(nb)
    n = len(rows)
    fin, fout = str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")
    rows.tofile(fin)

    def run(mode, W, tau, s, call_blocks):
        out = subprocess.run([exe, fin, fout, str(mode), str(W), str(tau)] + [repr(float(F32(s[k]))) if k != "hang_blocks" else str(s[k]) for k in
                             ("open_n", "close_n", "hang_blocks", "fall", "rise")] + [str(n), str(nb), str(call_blocks)], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and out.stdout.endswith("host_noise_check OK\n"), out.stdout + out.stderr
        assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
        w = np.fromfile(fout, np.uint32)
        return w[0], w[1:66], w[66:].reshape(n, 2 * nb + NZ.WORDS)

    for mode, W, tau, s in ((NZ.GATE, 2, 750.0, D), (NZ.MEASURE, 3, 0.0, dict(open_n=0.02, close_n=0.02, hang_blocks=0, fall=1.0, rise=0.5))):
        m = NZ.Noise(n, mode, W, tau, **s)
        N, nopen = m.run(rows)
        for call_blocks in (1, 2, 3):
            key, g, body = run(mode, W, tau, s, call_blocks)
            assert key == NZ.key_of(mode, W, tau) and np.array_equal(g, bits(NZ.taps(tau))), (mode, call_blocks)
            assert np.array_equal(body[:, :nb], bits(N)) and np.array_equal(body[:, nb:2 * nb], nopen), (mode, call_blocks)
            assert np.array_equal(body[:, 2 * nb:], m.words()), (mode, call_blocks)
        if mode == NZ.GATE:
            assert nopen[0, 3:8].all() and not nopen[0, -1] and not nopen[1].any() and not nopen[2].any() and nopen[4, 3:].all()
            assert not nopen[3, :3].any() and nopen[3, 3:].all() and N[2].min() > 1.0                  # silence opens; the rails read above full scale
    key, g, body = run(NZ.OFF, 2, 750.0, D, 3)
    assert not body.any()
    bad = [fin, fout, "2", "2", "750", "0.01", "0.025", "8", "0.75", "0.125", "1", "1", "1"]
    for at, v in ((2, "3"), (3, "4"), (4, "24"), (5, "0"), (6, "0.005"), (7, "65536"), (8, "0"), (9, "1.5"), (12, "0")):
        assert subprocess.run([exe] + bad[:at] + [v] + bad[at + 1:], capture_output=True).returncode == 2, (at, v)
