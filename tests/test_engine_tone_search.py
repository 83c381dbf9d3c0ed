"""The CTCSS tone search of rdsp_engine_t without a GPU (include/rdsp.h "tone search"; csrc/rdsp_tone_search.h,
csrc/rdsp_engine_tone_search_host.hip): the exports, every refusal that needs no device, the steps, the bank's key and the scale
against tests/engine_tone_search_model.py, rdsp_engine_tone_search_gain against a float64 formula and against a sine pushed
through the de-emphasis and the model, the standard list, tests/host/host_tone_search_check.cpp -- csrc/rdsp_tone_search.h as a
program of its own, plain and under ASan + UBSan, run directly -- against the model's bits at every cut of 1 to 3 blocks and
banks of 50, 64, 3 and 1 tones, and the search's figures on the float32 model, printed and asserted.
tests/test_engine_tone_search_gpu.py holds the kernel to the same model."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import engine_sources_model as S
import engine_tone_model as T
import engine_tone_search_model as TS
from test_engine_tone import _crafted_rows

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
BANK64 = tuple(np.round(np.linspace(60.0, 300.0, 64), 1))
BANKS = (TS.STANDARD, BANK64, (88.5, 100.0, 254.1), (151.4,))


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_tone_search_exports(rdsp):
    from radiodsp_sdr_rx_amd import engine
    lib = rdsp.load()
    for name in ("enable_tone_search", "tone_search_enabled", "set_tone_bank", "tone_bank", "set_tone_search", "read_tone_search",
                 "read_tone_spectrum", "tone_standard", "tone_search_gain"):
        assert hasattr(lib, "rdsp_engine_" + name), name
    assert callable(engine.standard_tones) and callable(engine.tone_search_gain)
    assert all(callable(getattr(engine.Engine, n)) for n in ("enable_tone_search", "set_tone_bank", "tone_bank", "set_tone_search",
                                                             "read_tone_search", "read_tone_spectrum"))
    assert isinstance(engine.Engine.tone_search_enabled, property)


def test_tone_search_refusals_without_a_device(rdsp):
    """no object: every entry point refuses; rdsp_engine_tone_standard refuses NULL; rdsp_engine_tone_search_gain answers 0.0 to
    what rdsp_engine_tone_gain refuses.  The refusals that need an object are test_engine_tone_search_gpu's"""
    from radiodsp_sdr_rx_amd.engine import tone_search_gain
    lib = rdsp.load()
    hz = (C.c_float * 2)(100.0, 103.5)
    assert lib.rdsp_engine_enable_tone_search(None) == -1 and lib.rdsp_engine_tone_search_enabled(None) == 0
    assert lib.rdsp_engine_set_tone_bank(None, hz, 2) == -1 and b"rdsp_engine_set_tone_bank" in lib.rdsp_last_error()
    assert lib.rdsp_engine_tone_bank(None, hz) == -1
    assert lib.rdsp_engine_set_tone_search(None, 128, 0.04, 4.0) == -1 and b"rdsp_engine_set_tone_search" in lib.rdsp_last_error()
    assert lib.rdsp_engine_read_tone_search(None, 0, None, 0, None, 0, None, 0, None) == -1
    assert lib.rdsp_engine_read_tone_spectrum(None, 0, 1, None, 64, None) == -1
    assert lib.rdsp_engine_tone_standard(None) == -1
    nan = float("nan")
    for f, tau in ((0.0, 750.0), (-100.0, 750.0), (22050.0, 750.0), (nan, 750.0), (100.0, 24.0), (100.0, 1001.0), (100.0, nan), (float("inf"), 0.0)):
        assert lib.rdsp_engine_tone_search_gain(f, tau) == 0.0 and b"rdsp_engine_tone_search_gain" in lib.rdsp_last_error(), (f, tau)
        with pytest.raises(rdsp.RdspError):
            tone_search_gain(f, tau)


def test_tone_search_standard_list(rdsp):
    """rdsp_engine_tone_standard is the 50-entry EIA list, ascending, 67.0 ... 254.1 Hz, and the model's"""
    from radiodsp_sdr_rx_amd.engine import standard_tones
    s = standard_tones()
    assert s.dtype == F32 and len(s) == 50 and np.all(np.diff(s) > 0) and s[0] == F32(67.0) and s[-1] == F32(254.1)
    assert np.array_equal(s, np.array(TS.STANDARD, F32)) and {F32(100.0), F32(88.5), F32(151.4), F32(203.5)} <= set(s)
    assert np.diff(s).min() > 2.2                                                            # the closest neighbours are 2.3 Hz apart


def test_tone_search_steps_key_and_scale():
    """dphi_t = llround(tone_hz 2^32 32 / 44100) on the float: 32 times the tone squelch's step but for the rounding; the key is
    FNV-1a over the bytes of n_tones and the steps (the empty hash and one known vector pin the constants); scale is the tone
    squelch's"""
    assert TS.dphi_of(100.0) == round(100.0 * 32 * 2 ** 32 / 44100.0) == 311652956
    for f in TS.STANDARD:
        assert TS.dphi_of(f) == round(float(F32(f)) * 32 * 2 ** 32 / 44100.0) and abs(TS.dphi_of(f) - 32 * T.dphi_of(f)) <= 16
    assert TS.dphi_of(300.0) < 2 ** 31                                                       # every tone lies below the decimated Nyquist
    h = 2166136261
    for byte in (1, 0, 0, 0) + tuple((TS.dphi_of(100.0) >> (8 * k)) & 0xff for k in range(4)):
        h = ((h ^ byte) * 16777619) & 0xffffffff
    assert TS.bank_key([TS.dphi_of(100.0)]) == h
    keys = {TS.bank_key([TS.dphi_of(f) for f in b]) for b in BANKS} | {TS.bank_key([TS.dphi_of(f) for f in TS.STANDARD[:49]])}
    assert len(keys) == 5 and 0 not in keys


def test_tone_search_gain_is_the_formula_and_the_filters(rdsp):
    """rdsp_engine_tone_search_gain equals |sin(32 pi f / 44100) / (32 sin(pi f / 44100))| x tone_gain in float64 within 4e-16
    relative on the standard tones and time constants, and is what the de-emphasis and the decimator do to a sine: a 100 Hz sine
    of 0.12 behind the model's float32 de-emphasis reads sqrt(a2) = 0.12 x gain in the model's second window of K = 128.  The
    bound: a window of N = 512 decimated samples correlates A cos(w n + p) into (A / 2)(N e^{jp} + e^{-jp} sum e^{-2 j w n}), and
    |sum| <= 1 / sin w = 2.27 at w = 2 pi 100 / 1378.125, so the reading is off by at most 2.27 / 512 = 0.45 % (plus the table's
    2^-17)"""
    from radiodsp_sdr_rx_amd.engine import tone_gain, tone_search_gain
    for f in TS.STANDARD:
        for tau in (0.0, 25.0, 75.0, 750.0, 1000.0):
            w = math.pi * float(F32(f)) / 44100.0
            want = abs(math.sin(32.0 * w) / (32.0 * math.sin(w))) * tone_gain(f, tau)
            g = tone_search_gain(f, tau)
            assert abs(g - want) <= 4e-16 * want and abs(g - TS.gain(f, tau)) <= 4e-16 * want and 0.0 < g < 1.0, (f, tau, g, want)
    g = tone_search_gain(100.0, 750.0)
    print(f"tone_search_gain(100 Hz, 750 us) = {g:.5f}; (254.1 Hz, 750 us) = {tone_search_gain(254.1, 750.0):.5f}; boxcar alone at 254.1 Hz "
          f"{tone_search_gain(254.1, 0.0):.5f}")
    y = T.deemph((0.12 * np.sin(2 * np.pi * 100.0 / 44100.0 * np.arange(256 * 128))).astype(F32), 750.0)
    m = TS.Search(1, S.table(rdsp), (100.0,), 128)
    best, a2, nxt = m.run(y[None])
    amp = math.sqrt(float(a2[0, -1]))
    print(f"a 100 Hz sine of 0.12 reads {amp:.5f}; 0.12 x gain = {0.12 * g:.5f}")
    assert best[0, -1] == 0 and abs(amp / (0.12 * g) - 1.0) < 2.27 / 512 + 2.0 ** -17


@pytest.mark.parametrize("sanitize", [False, True])
def test_tone_search_host_program(rdsp, tmp_path, sanitize):
    """tests/host/host_tone_search_check.cpp, plain and under ASan + UBSan, a program of its own run on the CPU: on the crafted
    rows of test_engine_tone (on the rails, all zeros, a tone that stops, no tone), for K = 4 and 5, calls of 1, 2 and 3 blocks
    (which it holds to one long call itself) and banks of 50, 64, 3 and 1 tones, its steps, key, scale, thresholds, records and
    final words equal the model's.  The row of zeros never finds a tone; a bank of one tone has no `next`; a row whose only
    nonzero decimated sample is the first gives every tone the same power, and the lowest index wins the tie"""
    exe = str(tmp_path / ("host_tone_search_check_san" if sanitize else "host_tone_search_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_tone_search_check.cpp"), "-o", exe])
    nb = 13
    rows, _ = _crafted_rows(nb)
    tie = np.zeros((1, nb * 128), F32)
    tie[0, :32] = 1.0                                                                         # d = 32 at m = 0 and 0 after it: every P_t is equal
    rows = np.concatenate([rows, tie])
    n = len(rows)
    fin, fout = str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")
    rows.tofile(fin)
    tab = S.table(rdsp)
    for bank in BANKS:
        for K, lo, ratio in ((4, 0.06, 1.0), (5, 0.04, 4.0)):
            m = TS.Search(n, tab, bank, K, lo, ratio)
            best, a2, nxt = m.run(rows)
            for call_blocks in (1, 2, 3):
                out = subprocess.run([exe, fin, fout, str(K), str(lo), str(ratio), str(n), str(nb), str(call_blocks)] + [str(v) for v in bank],
                                     capture_output=True, text=True, timeout=120)
                assert out.returncode == 0 and out.stdout.endswith("host_tone_search_check OK\n"), out.stdout + out.stderr
                assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
                w = np.fromfile(fout, np.uint32)
                assert w[0] == bits(T.scale_of(K)) and w[1] == bits(m.min2[0]) and w[2] == bits(m.ratio[0]), (K, len(bank))
                assert w[3] == len(bank) and w[4] == m.key and np.array_equal(w[5:69], m.dphi), (K, len(bank))
                body = w[69:].reshape(n, 3 * nb + 200)
                assert np.array_equal(body[:, :nb], best), (K, len(bank), call_blocks)
                assert np.array_equal(body[:, nb:2 * nb], bits(a2)) and np.array_equal(body[:, 2 * nb:3 * nb], bits(nxt)), (K, len(bank), call_blocks)
                assert np.array_equal(body[:, 3 * nb:], m.words()), (K, len(bank), call_blocks)
            assert (best[3] == 255).all() and not a2[3].any() and a2[2].any() and (best[:, :K - 1] == 255).all()   # silence; before the first window
            if len(bank) == 1:
                assert not nxt.any() and set(best.ravel()) <= {0, 255}
            tied = TS.Search(1, tab, bank, K, lo, ratio)
            tied.run(rows[-1:, :K * 128])
            spec = tied.spectrum()[0]
            assert (bits(spec) == bits(spec[0])).all() and spec[0] > lo * lo                  # the tie: the lowest index wins, and is found at ratio 1
            assert best[-1, K - 1] == (0 if ratio == 1.0 else 255 if len(bank) > 2 else 0) and (best[-1, 2 * K - 1:] == 255).all()
            nt, w = len(bank), m.words()
            assert not w[:, TS.RE + nt:TS.IM].any() and not w[:, TS.IM + nt:TS.P].any() and not w[:, TS.P + nt:].any() and w[2, TS.P:TS.P + nt].all()
    for bad in (["3", "0.04", "4", "1", "1", "1", "100"], ["0", "0.04", "4", "1", "1", "1", "100"], ["4", "0.04", "0.5", "1", "1", "1", "100"],
                ["4", "0.04", "4", "1", "1", "1", "59"], ["4", "0.04", "4", "1", "1", "1", "100", "100"], ["4", "0.04", "4", "1", "1", "1", "103.5", "100"]):
        assert subprocess.run([exe, fin, fout] + bad, capture_output=True).returncode == 2, bad


def test_tone_search_figures(rdsp):
    """the search's figures on the float32 model, printed and asserted.  The signal is engine_tone_model.demod_row: a tone of 0.12
    under voice-band noise of rms 0.25, clipped, behind the 750 us de-emphasis -- one row per standard tone.  K = 128, the default
    bank and the defaults 0.04 / 4.0, four windows: every one of the 50 tones is found as itself in every window after the first.
    Uniform +-1 noise behind the de-emphasis (an idle discriminator), 16 windows: nothing is found.  K = 32: the arg-max is the
    tone everywhere, but the ratio to `next` falls below the default at the low end of the list, where the search then declines
    to decide: printed, only the arg-max asserted"""
    tab = S.table(rdsp)
    n = len(TS.STANDARD)
    rows = np.stack([T.demod_row(100 + t, 512, f, 0.12, 0.25, 750.0) for t, f in enumerate(TS.STANDARD)])
    m = TS.Search(n, tab, TS.STANDARD, 128)
    best, a2, nxt = m.run(rows)
    ends = slice(2 * 128 - 1, None, 128)                                                      # the windows after the first
    with np.errstate(divide="ignore"):
        ratio = a2[:, ends].astype(np.float64) / nxt[:, ends]
    amp = np.sqrt(a2[:, ends].astype(np.float64))
    print(f"K = 128: sqrt(a2) {amp.min():.4f} ... {amp.max():.4f} (lowest at {TS.STANDARD[int(amp.min(1).argmin())]} Hz), worst P_i / next "
          f"{ratio.min():.1f} at {TS.STANDARD[int(ratio.min(1).argmin())]} Hz, {int((best[:, ends] != np.arange(n)[:, None]).sum())} wrong decisions")
    assert np.array_equal(best[:, ends], np.broadcast_to(np.arange(n, dtype=np.uint8)[:, None], (n, 3)))
    assert amp.min() >= TS.DEFAULT_MIN and ratio.min() >= TS.DEFAULT_RATIO
    r = np.random.default_rng(13)
    idle = T.deemph(r.uniform(-1.0, 1.0, 16 * 128 * 128).astype(F32), 750.0)
    q = TS.Search(1, tab, TS.STANDARD, 128)
    ibest, ia2, inxt = q.run(idle[None])
    e = slice(127, None, 128)
    print(f"K = 128, idle: sqrt(a2) at most {np.sqrt(ia2[0, e].max()):.4f}, P_i / next at most {(ia2[0, e] / inxt[0, e]).max():.2f} (16 windows)")
    assert (ibest == 255).all()
    s = TS.Search(n, tab, TS.STANDARD, 32)
    worst, declined, windows = np.full(n, np.inf), 0, 0
    for k in range(16):                                                                       # a window a call: the spectrum of each
        sbest, sa2, snxt = s.run(rows[:, k * 32 * 128:(k + 1) * 32 * 128])
        if k == 0:
            continue
        assert np.array_equal(s.spectrum().argmax(1), np.arange(n)), k
        worst = np.minimum(worst, sa2[:, -1].astype(np.float64) / snxt[:, -1])
        declined, windows = declined + int((sbest[:, -1] == 255).sum()), windows + n
    print(f"K = 32: the arg-max is the tone everywhere; worst P_i / next {worst.min():.2f} at {TS.STANDARD[int(worst.argmin())]} Hz; "
          f"{declined} of {windows} windows decline to decide")
