"""The CTCSS tone squelch of rdsp_engine_t without a GPU (include/rdsp.h "tone squelch"; csrc/rdsp_tone.h,
csrc/rdsp_engine_tone_host.hip): the step, the scale and rdsp_engine_tone_gain against tests/engine_tone_model.py, the exports,
every refusal that needs no device, tests/host/host_tone_check.cpp -- csrc/rdsp_tone.h as a program of its own, plain and under
ASan + UBSan, run directly -- against the model's bits at every cut of 1 to 3 blocks, and the detector's figures on a synthetic
demodulated row (a 100.0 Hz tone of 0.12 under voice-band noise of rms 0.25, clipped, de-emphasised), printed and asserted on
the model.  tests/test_engine_tone_gpu.py holds the kernel to the same model."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import engine_sources_model as S
import engine_tone_model as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
STANDARD = (67.0, 71.9, 88.5, 100.0, 103.5, 151.4, 203.5, 254.1)


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_tone_exports(rdsp):
    from radiodsp_sdr_rx_amd import engine
    lib = rdsp.load()
    for name in ("enable_tone", "tone_enabled", "set_tones", "set_tone_squelch", "read_tone", "tone_gain"):
        assert hasattr(lib, "rdsp_engine_" + name), name
    assert callable(engine.tone_gain)
    assert all(callable(getattr(engine.Engine, n)) for n in ("enable_tone", "set_tones", "set_tone_squelch", "read_tone"))
    assert isinstance(engine.Engine.tone_enabled, property)


def test_tone_refusals_without_a_device(rdsp):
    """no object: every entry point refuses; rdsp_engine_tone_gain answers 0.0 to a frequency outside (0, 22050), a NaN, or a
    time constant rdsp_engine_set_fm refuses.  The refusals that need an object are test_engine_tone_gpu's"""
    from radiodsp_sdr_rx_amd.engine import tone_gain
    lib = rdsp.load()
    hz = (C.c_float * 2)(100.0, 0.0)
    assert lib.rdsp_engine_enable_tone(None) == -1 and lib.rdsp_engine_tone_enabled(None) == 0
    assert lib.rdsp_engine_set_tones(None, 0, 2, hz) == -1 and b"rdsp_engine_set_tones" in lib.rdsp_last_error()
    assert lib.rdsp_engine_set_tone_squelch(None, 128, 0.04, 0.025) == -1 and b"rdsp_engine_set_tone_squelch" in lib.rdsp_last_error()
    assert lib.rdsp_engine_read_tone(None, 0, None, 0, None, 0, None) == -1
    nan = float("nan")
    for f, tau in ((0.0, 750.0), (-100.0, 750.0), (22050.0, 750.0), (nan, 750.0), (100.0, 24.0), (100.0, 1001.0), (100.0, nan), (float("inf"), 0.0)):
        assert lib.rdsp_engine_tone_gain(f, tau) == 0.0 and b"rdsp_engine_tone_gain" in lib.rdsp_last_error(), (f, tau)
        with pytest.raises(rdsp.RdspError):
            tone_gain(f, tau)


def test_tone_gain_is_the_model_and_the_filters(rdsp):
    """rdsp_engine_tone_gain equals the model's double on the standard tones and time constants, is 1.0 without de-emphasis, and
    is what the de-emphasis does to a sine: the amplitude of a 100 Hz sine of 0.12 behind the model's float32 recursion, measured
    over 50 whole periods after the transient, is 0.12 x gain within 1e-4"""
    from radiodsp_sdr_rx_amd.engine import tone_gain
    for f in STANDARD:
        assert tone_gain(f, 0.0) == 1.0
        for tau in (25.0, 50.0, 75.0, 750.0, 1000.0):
            g, m = tone_gain(f, tau), T.gain(f, tau)
            assert abs(g - m) <= 4e-16 * m and 0.0 < g < 1.0, (f, tau, g, m)
    g = tone_gain(100.0, 750.0)
    print(f"tone_gain(100 Hz, 750 us) = {g:.5f}; (254.1 Hz, 750 us) = {tone_gain(254.1, 750.0):.5f}; (100 Hz, 75 us) = {tone_gain(100.0, 75.0):.5f}")
    analog = 1.0 / np.sqrt(1.0 + (2 * np.pi * 100.0 * 750e-6) ** 2)                          # the RC network the recursion stands for: 0.9046
    assert abs(g / analog - 1.0) < 0.005
    n = 441 * 60
    y = T.deemph((0.12 * np.sin(2 * np.pi * 100.0 / 44100.0 * np.arange(n))).astype(F32), 750.0).astype(np.float64)[441 * 10:]
    amp = 2.0 * abs(np.mean(y * np.exp(-2j * np.pi * 100.0 / 44100.0 * np.arange(len(y)))))
    assert abs(amp - 0.12 * g) < 1e-4, (amp, 0.12 * g)


def _crafted_rows(nb):
    """float32 [rows, nb * 128] with their tones: toned rows under voice noise, a row on the rails (+-1 drawn), an all-zero row,
    a tone that stops after 4.5 blocks, full-range noise without a tone set, a row without a tone"""
    r = np.random.default_rng(23)
    rows = [T.demod_row(1, nb, 100.0), T.demod_row(2, nb, 254.1, 0.15, 0.3), r.choice(np.array([1.0, -1.0], F32), nb * 128),
            np.zeros(nb * 128, F32), T.demod_row(3, nb, 67.0, 0.5, 0.0, 0.0, tone_until=576), r.uniform(-1.0, 1.0, nb * 128).astype(F32),
            T.demod_row(4, nb, 151.4)]
    return np.stack(rows).astype(F32), [100.0, 254.1, 88.5, 203.5, 67.0, 0.0, 151.4]


@pytest.mark.parametrize("sanitize", [False, True])
def test_tone_host_program(rdsp, tmp_path, sanitize):
    """tests/host/host_tone_check.cpp, plain and under ASan + UBSan, a program of its own run on the CPU: on the crafted rows (on
    the rails, all zeros, a tone that stops, no tone), for K = 4 and 5 and calls of 1, 2 and 3 blocks (which it holds to one long
    call itself), its steps, scale, thresholds, records and final words equal the model's.  The tone that stops is detected and
    then lost; the row of zeros never has one; the row without a tone leaves zero words"""
    exe = str(tmp_path / ("host_tone_check_san" if sanitize else "host_tone_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_tone_check.cpp"), "-o", exe])
    nb = 13
    rows, hz = _crafted_rows(nb)
    n = len(rows)
    fin, fout = str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")
    rows.tofile(fin)
    tab = S.table(rdsp)
    for K, on, off in ((4, 0.06, 0.045), (5, 0.04, 0.025)):
        m = T.Tone(n, tab, hz, K, on, off)
        a2, tone = m.run(rows)
        for call_blocks in (1, 2, 3):
            out = subprocess.run([exe, fin, fout, str(K), str(on), str(off), str(n), str(nb), str(call_blocks)] + [str(v) for v in hz],
                                 capture_output=True, text=True, timeout=120)
            assert out.returncode == 0 and out.stdout.endswith("host_tone_check OK\n"), out.stdout + out.stderr
            assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
            w = np.fromfile(fout, np.uint32)
            assert w[0] == bits(T.scale_of(K)) and w[1] == bits(m.on2[0]) and w[2] == bits(m.off2[0])
            body = w[3:].reshape(n, 1 + 2 * nb + 8)
            assert np.array_equal(body[:, 0], m.dphi), (K, call_blocks)
            assert np.array_equal(body[:, 1:1 + nb], bits(a2)) and np.array_equal(body[:, 1 + nb:1 + 2 * nb], tone), (K, call_blocks)
            assert np.array_equal(body[:, 1 + 2 * nb:], m.words()), (K, call_blocks)
        if K == 4:
            assert tone[4, 3] and not tone[4, -1] and tone[0].any() and not tone[3].any() and not a2[3].any()   # found, then lost; silence
            assert not m.words()[5].any() and not a2[5].any() and a2[2].any()
    assert subprocess.run([exe, fin, fout, "3", "0.04", "0.025", "1", "1", "1", "100"], capture_output=True).returncode == 2
    assert subprocess.run([exe, fin, fout, "4", "0.04", "0.05", "1", "1", "1", "100"], capture_output=True).returncode == 2
    assert subprocess.run([exe, fin, fout, "4", "0.04", "0.025", "1", "1", "1", "59"], capture_output=True).returncode == 2


def test_tone_steps_and_scales():
    """dphi = llround(tone_hz 2^32 / 44100) on the float the setter receives: 100 Hz is 9 739 155 (9739155.01...), 0 is 0, and the
    model's rounding is half away from zero; scale = 4 / (128 K)^2 makes a sinusoid of amplitude A read a2 = A^2 -- so a detector
    fed its own table's sine reads 1.0 within the table's 2^-17"""
    assert T.dphi_of(100.0) == 9739155 and T.dphi_of(0.0) == 0 and T.dphi_of(300.0) == round(300.0 * 2 ** 32 / 44100.0)
    assert T.dphi_of(67.0) == round(float(F32(67.0)) * 2 ** 32 / 44100.0) and T.dphi_of(254.1) == round(float(F32(254.1)) * 2 ** 32 / 44100.0)
    for K in (4, 32, 128, 512):
        assert float(T.scale_of(K)) == float(F32(4.0 / (128.0 * K) ** 2))
    assert bits(T.scale_of(128)) == bits(F32(2.0 ** -26))


@functools.lru_cache(maxsize=None)
def _toned(n_blocks, seed=11):
    return T.demod_row(seed, n_blocks, 100.0, 0.12, 0.25, 750.0)


def _readings(rdsp, row, tones, K):
    """the amplitudes sqrt(a2) of every completed window, one detector per tone on the same row: float64 [len(tones), windows]"""
    m = T.Tone(len(tones), S.table(rdsp), list(tones), K)
    a2, _ = m.run(np.broadcast_to(row, (len(tones), len(row))))
    return T.amplitude(a2[:, K - 1::K])


def test_tone_figures(rdsp):
    """the detector's figures on the model, printed; the row: a 100.0 Hz tone of 0.12, band-limited noise of 300 ... 3000 Hz and rms
    0.25 standing in for voice, the sum clipped to +-1, the 750 us de-emphasis.  Asserted: the set tone reads at least 0.10, a
    detector at 151.4 Hz at most 0.01 (K = 32 and K = 128); at K = 128 a detector at the adjacent standard tone 103.5 Hz stays below
    the default off_amp 0.025, and uniform +-1 noise behind the de-emphasis (an idle discriminator) reads below the default
    on_amp 0.04 at 100 Hz"""
    row = _toned(512)
    for K in (32, 128):
        own, other, adjacent = _readings(rdsp, row, (100.0, 151.4, 103.5), K)
        print(f"K = {K}: the set tone reads {own.min():.4f} ... {own.max():.4f}, 151.4 Hz at most {other.max():.4f}, 103.5 Hz {adjacent.min():.4f} ... "
              f"{adjacent.max():.4f} ({len(own)} windows)")
        assert own.min() >= 0.10 and other.max() <= 0.01, K
        if K == 128:
            assert adjacent.max() < T.DEFAULT_OFF
    quiet = T.demod_row(12, 256, 100.0, 0.0)
    print(f"K = 32: the noise alone reads at most {_readings(rdsp, quiet, (100.0,), 32).max():.4f} at 100 Hz")
    r = np.random.default_rng(13)
    idle = T.deemph(r.uniform(-1.0, 1.0, 1024 * 128).astype(F32), 750.0)
    for K in (32, 128):
        worst = _readings(rdsp, idle, (100.0,), K).max()
        print(f"K = {K}: uniform +-1 noise behind the de-emphasis reads at most {worst:.4f} at 100 Hz ({1024 // K} windows)")
        if K == 128:
            assert worst < T.DEFAULT_ON
