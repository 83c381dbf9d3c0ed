"""Narrow-band FM of rdsp_engine_t (include/rdsp.h "narrow-band FM"; csrc/rdsp_fm.h, csrc/rdsp_engine_fm.hip,
csrc/rdsp_engine_fm_host.hip): the detector an NFM group runs where the other modes run the IF filter and their detector, and the
carrier squelch it gives the meter.  Every comparison with the model is exact: floats as uint32, audio as int16.

`-m "not gpu"`: rdsp_engine_fm_atan2 and rdsp_engine_fm_constants against tests/engine_fm_model.py, the arctangent's error
against float64, the refusals of rdsp_engine_fm_constants (rdsp_engine_set_fm shares its limits; its own need an engine object, so
a device: test_gpu_fm_state), the exports, the channel filters' figures on the float taps, the model
against a float64 evaluation of the same definition on a synthetic station, the level row on a carrier,
tests/host/host_fm_check.cpp -- csrc/rdsp_fm.h as a program of its own, plain and under ASan + UBSan, run directly -- against the
model, and tests/engine_tail_model.py against the stage taps and the audio of tests/golden/engine_kat.npz.
`-m gpu`: an NFM group's demodulated rows, level rows and int16 audio against the models for every call split; unaligned rows;
the decay into subnormals; NFM beside LSB and AM groups; the carrier squelch, the active list and both packs; the sources path;
the state through blobs, regroupings, mode changes and resets; the refusals."""
import functools
import json
import os
import subprocess

import numpy as np
import pytest

import engine_fm_model as FM
import engine_pack_model as P
import engine_tail_model as TM
import engine_voice_model as V
from engine_meter_model import Meter, Squelch, gated

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
ATAN_BOUND = 2.0 ** -19
NFM = 7


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def _drawn_pairs(n, seed=3):
    r = np.random.default_rng(seed)
    mag = lambda: (r.uniform(1.0, 2.0, n) * 2.0 ** r.integers(-60, 61, n) * r.choice([-1.0, 1.0], n)).astype(F32)
    return mag(), mag()


def test_fm_atan2_is_the_model_and_within_its_bound(rdsp):
    """rdsp_engine_fm_atan2 equals the model bit for bit on drawn pairs of every scale and sign and on the special cases -- both
    arguments zero with either sign, one zero (the axes), |x| = |y| (the diagonals), huge with tiny (a quotient that underflows)
    -- and the model's worst error against float64 atan2 over every t = j / 2^20 and a million drawn pairs is within 2^-19"""
    from radiodsp_sdr_rx_amd.engine import fm_atan2
    y, x = _drawn_pairs(20000)
    huge, tiny = F32(3.0e38), F32(1.0e-44)
    special = [(0.0, 0.0), (-0.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (0.0, 2.0), (-0.0, 2.0), (0.0, -2.0), (-0.0, -2.0), (3.0, 0.0), (-3.0, 0.0),
               (3.0, -0.0), (1.0, 1.0), (1.0, -1.0), (-1.0, 1.0), (-1.0, -1.0), (huge, huge), (tiny, tiny), (huge, tiny), (tiny, huge),
               (-tiny, -huge), (-huge, -tiny), (huge, -tiny), (tiny, -huge), (5.0e-39, 1.0e-38), (1.0, 3.0e38)]
    y = np.concatenate([y, np.array([s[0] for s in special], F32)])
    x = np.concatenate([x, np.array([s[1] for s in special], F32)])
    got = np.array([fm_atan2(a, b) for a, b in zip(y, x)], F32)
    assert np.array_equal(bits(got), bits(FM.atan2(y, x)))
    assert bits(FM.atan2(F32(-0.0), F32(-0.0))) == 0 and FM.atan2(F32(-0.0), F32(-2.0)) == -FM.PI and FM.atan2(F32(3.0), F32(0.0)) == FM.PI_2
    t = (np.arange((1 << 20) + 1) / float(1 << 20)).astype(F32)
    one = np.ones_like(t)
    worst = 0.0
    for yy, xx in ((t, one), (one, t), (t, -one), (-one, -t)) + (_drawn_pairs(1000000, 4),):
        worst = max(worst, float(np.abs(FM.atan2(yy, xx).astype(np.float64) - np.arctan2(yy.astype(np.float64), xx.astype(np.float64))).max()))
    print(f"fm_atan2: worst error against float64 atan2 {worst:.3e} rad, {worst / ATAN_BOUND:.3f} of the bound 2^-19")
    assert worst <= ATAN_BOUND


def test_fm_constants_and_refusals(rdsp):
    """rdsp_engine_fm_constants equals the model's k and a; out-of-range arguments are refused with nothing written"""
    import ctypes as C
    from radiodsp_sdr_rx_amd.engine import fm_constants
    for dev in (1000.0, 2500.0, 5000.0, 7500.0, 3333.3):
        for tau in (0.0, 25.0, 50.0, 75.0, 750.0, 1000.0):
            k, a = fm_constants(dev, tau)
            mk, ma = FM.constants(dev, tau)
            assert bits(k) == bits(mk) and bits(a) == bits(ma), (dev, tau)
    assert abs(float(FM.constants(2500.0, 750.0)[0]) - 2.81) < 0.005 and abs(float(FM.constants(5000.0, 750.0)[1]) - 0.0293) < 0.0001
    lib = rdsp.load()
    buf = (C.c_float * 2)(77.0, 77.0)
    for dev, tau in ((999.0, 750.0), (7501.0, 750.0), (float("nan"), 750.0), (5000.0, 24.0), (5000.0, 1001.0), (5000.0, -1.0), (5000.0, float("nan"))):
        assert lib.rdsp_engine_fm_constants(dev, tau, buf) == -1 and b"rdsp_engine_fm_constants" in lib.rdsp_last_error()
        with pytest.raises(rdsp.RdspError):
            fm_constants(dev, tau)
    assert lib.rdsp_engine_fm_constants(5000.0, 750.0, None) == -1 and list(buf) == [77.0, 77.0]


def test_fm_exports(rdsp):
    from radiodsp_sdr_rx_amd import engine
    lib = rdsp.load()
    for name in ("enable_fm", "fm_enabled", "set_fm", "read_fm_level", "fm_atan2", "fm_constants"):
        assert hasattr(lib, "rdsp_engine_" + name), name
    assert engine.NFMmode == NFM and callable(engine.fm_atan2) and callable(engine.fm_constants)
    assert all(callable(getattr(engine.Engine, n)) for n in ("enable_fm", "set_fm", "read_fm_level")) and isinstance(engine.Engine.fm_enabled, property)
    assert lib.rdsp_engine_set_fm(None, 2, 5000.0, 750.0) == -1 and lib.rdsp_engine_fm_enabled(None) == 0 and lib.rdsp_engine_enable_fm(None) == -1
    # rdsp_engine_set_fm's other refusals need an engine object, which only exists with a device: test_gpu_fm_state makes them.  Its
    # limits are rdsp_fm.h's deviation_ok and tau_ok, which rdsp_engine_fm_constants shares (test_fm_constants_and_refusals, a NaN included)
    assert lib.rdsp_engine_set_fm(None, 5, float("nan"), 24.0) == -1 and b"rdsp_engine_set_fm" in lib.rdsp_last_error()


def _gain_db(h, f_hz):
    f = np.atleast_1d(np.asarray(f_hz, np.float64))
    k = np.arange(len(h))
    return 20 * np.log10(np.abs((h.astype(np.float64)[None] * np.exp(-2j * np.pi * f[:, None] / 44100.0 * k[None])).sum(1)))


@pytest.mark.parametrize("W", [2, 3])
def test_fm_channel_filter_figures(rdsp, W):
    """the definition's table recomputed on the float taps of rdsp_engine_ddc_taps(W): the flat band, the -6 dB point, the stop
    band, sum |h|.  Printed; ripple <= 0.001 dB to 7 kHz (W = 2) / 4 kHz (W = 3), at least 90 dB from 16.05 kHz / 80 dB from 10 kHz"""
    from radiodsp_sdr_rx_amd.engine import ddc_taps
    h = ddc_taps(W)
    assert np.array_equal(bits(h), bits(FM.taps(W))) and h.shape == (16 * W,)
    flat_to, stop_from, stop_db, marks = {2: (7000.0, 16050.0, 90.0, (8000.0, 11000.0, 12500.0)), 3: (4000.0, 10000.0, 80.0, (5500.0, 7350.0))}[W]
    ripple = float(np.abs(_gain_db(h, np.arange(0.0, flat_to + 1, 10.0))).max())
    stop = float(-_gain_db(h, np.arange(stop_from, 22050.0 + 1, 10.0)).max())
    at = ", ".join(f"{g:.2f} dB at {f / 1000:g} kHz" for f, g in zip(marks, _gain_db(h, marks)))
    total = float(np.abs(h.astype(np.float64)).sum())
    print(f"FM channel filter W = {W}: within {ripple:.5f} dB to {flat_to / 1000:g} kHz, {at}, >= {stop:.1f} dB from {stop_from / 1000:g} kHz, sum |h| = {total:.4f}")
    assert ripple <= 0.001 and stop >= stop_db and total <= 1.65
    assert abs(_gain_db(h, marks[1])[0] + 6.0) < 0.5


def _tone_amplitude(y, f_hz):
    """the amplitude of the f_hz component of y over a whole number of its periods"""
    n = int(len(y) // (44100.0 / f_hz) * (44100.0 / f_hz))
    t = np.arange(n)
    return 2.0 * abs(np.mean(y[:n] * np.exp(-2j * np.pi * f_hz / 44100.0 * t)))


@pytest.mark.parametrize("W, deviation", [(2, 5000.0), (3, 2500.0)])
def test_fm_model_against_float64_on_a_station(W, deviation):
    """a carrier of 8000 counts, frequency-modulated by a 1 kHz tone at the set deviation, in noise of 3 counts, no de-emphasis:
    the recovered tone is within 0.5 % of sinc(1000 / 44100) = 0.99915 (a phase difference per sample averages the frequency over
    one sample), and the float32 model stays within a bound on its distance from the float64 evaluation:
      z: a chain of T fused steps on exact integers errs by at most T u sum|h| max|x| per component, u = 2^-24;
      re, im: two roundings each of values up to 2 |z|^2, so the angle of (re, im) moves by at most about
        (2 sqrt(2) T u sum|h| max|x| / |z| + 4 u) -- the relative error of z[n] and z[n - 1] plus the products';
      fm_atan2 adds 2^-19; times k; the product d k and the clip round once more (u).
    The worst fraction of the bound is printed."""
    nb = 12
    iq = FM.station(11 + W, nb, deviation, 1000.0, 8000.0, 3.0)
    m = FM.Fm(1, W, deviation, 0.0)
    y, lvl = m.run(iq[None])
    y64, lvl64 = FM.run64(iq, W, deviation, 0.0)
    skip = 16 * W
    amp = _tone_amplitude(y[0, skip:].astype(np.float64), 1000.0)
    sinc = np.sinc(1000.0 / 44100.0)
    print(f"NFM W = {W}, deviation {deviation:g}: recovered tone {amp:.5f}, sinc {sinc:.5f}")
    assert abs(amp / sinc - 1.0) <= 0.005 and abs(sinc - 0.99915) < 1e-5
    u, T = 2.0 ** -24, 16 * W
    sum_h = float(np.abs(FM.taps(W).astype(np.float64)).sum())
    zmag = (lvl64[skip:] * 32768.0).min()
    xmax = float(np.abs(iq.astype(np.float64)).max())
    k = float(m.k)
    bound = k * (2 * np.sqrt(2) * T * u * sum_h * xmax / zmag + 4 * u + ATAN_BOUND) + 2 * u
    err = float(np.abs(y[0, skip:].astype(np.float64) - y64[skip:]).max())
    print(f"NFM W = {W}: float32 model against float64 {err:.3e}, {err / bound:.3f} of the bound {bound:.3e}")
    assert err <= bound
    assert np.abs(lvl[0, skip:] / lvl64[skip:] - 1.0).max() < 1e-5


@pytest.mark.parametrize("W", [2, 3])
def test_fm_level_row_on_a_carrier(W):
    """an unmodulated carrier of A counts reads a level whose square is (A / 32768)^2 within the filter's ripple (0.001 dB); a
    full-scale one reads 1.0, mean square +3 dB on the ms_of_db scale"""
    from radiodsp_sdr_rx_amd.engine import db_of_ms
    for A, f in ((8000.0, 1500.0), (100.0, 0.0), (32767.0, -600.0)):
        t = np.arange(4 * 128)
        z = A * np.exp(2j * np.pi * f / 44100.0 * t + 0.3j)
        iq = np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16)
        lvl = FM.Fm(1, W).run(iq[None])[1][0, 16 * W:].astype(np.float64)
        want = (A / 32768.0) ** 2
        tol = 10 ** (0.001 / 10) - 1 + 2.0 / A                                          # the ripple, and the rounding to counts
        assert np.abs(lvl ** 2 / want - 1.0).max() <= tol, (A, f)
    assert abs(db_of_ms(float(np.mean(lvl[-128:] ** 2))) - 3.0103) < 0.01                 # the full-scale carrier


def _crafted_rows(nb=7):
    """int16 [rows, nb * 128, 2]: drawn stations, a row on the rails (+32767 / -32768 on both components), an all-zero row, a
    station that stops (the de-emphasis decays), full-range noise"""
    r = np.random.default_rng(17)
    rows = [FM.station(30, nb, 5000.0, 1000.0, 8000.0, 3.0), FM.station(31, nb, 2500.0, 2200.0, 300.0, 40.0, offset_hz=1500.0)]
    rows.append(r.choice(np.array([32767, -32768], np.int16), (nb * 128, 2)))
    rows.append(np.zeros((nb * 128, 2), np.int16))
    stop = FM.station(32, nb, 4000.0, 700.0, 20000.0, 0.0)
    stop[300:] = 0
    rows.append(stop)
    rows.append(r.integers(-32768, 32768, (nb * 128, 2)).astype(np.int16))
    return np.stack(rows)


@pytest.mark.parametrize("sanitize", [False, True])
def test_fm_host_program(tmp_path, sanitize):
    """tests/host/host_fm_check.cpp, plain and under ASan + UBSan, a program of its own run on the CPU: its arctangent sweep
    stays within 2^-19 and prints the worst value; on the crafted rows, for W = 2 and 3, with and without de-emphasis and calls
    of 1, 2 and 3 blocks (which it holds to one long call itself), its taps, constants, outputs, levels and final state words
    equal the model's"""
    exe = str(tmp_path / ("host_fm_check_san" if sanitize else "host_fm_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_fm_check.cpp"), "-o", exe])
    out = subprocess.run([exe, "atan2"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.endswith("host_fm_check OK\n"), out.stdout + out.stderr
    print(out.stdout.splitlines()[0])
    worst = float(out.stdout.split("worst fm_atan2 error ")[1].split()[0])
    assert 0 < worst <= ATAN_BOUND
    rows = _crafted_rows()
    n, t, _ = rows.shape
    fin, fout = str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")
    rows.tofile(fin)
    for W, dev, tau in ((2, 5000.0, 750.0), (3, 2500.0, 50.0), (3, 2500.0, 0.0)):
        m = FM.Fm(n, W, dev, tau)
        y, lvl = m.run(rows)
        T = 16 * W
        for call_blocks in (1, 2, 3):
            out = subprocess.run([exe, fin, fout, str(W), str(dev), str(tau), str(n), str(t // 128), str(call_blocks)], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0 and out.stdout.endswith("host_fm_check OK\n"), out.stdout + out.stderr
            assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
            w = np.fromfile(fout, np.uint32)
            assert np.array_equal(w[:T], bits(m.h)) and w[T] == bits(m.k) and w[T + 1] == bits(m.a)
            body = w[T + 2:].reshape(n, 2 * t + FM.STATE_WORDS)
            assert np.array_equal(body[:, :t], bits(y)) and np.array_equal(body[:, t:2 * t], bits(lvl)), (W, tau, call_blocks)
            assert np.array_equal(body[:, 2 * t:], m.words()), (W, tau, call_blocks)
    assert subprocess.run([exe, fin, fout, "4", "5000", "750", "1", "1", "1"], capture_output=True).returncode == 2
    assert np.abs(y[2]).max() == 1.0 and np.all(lvl[3] == 0) and np.all(y[3] == 0)            # the rails clip, silence stays silent


@functools.lru_cache(maxsize=None)
def _kat():
    return np.load(os.path.join(HERE, "golden", "engine_kat.npz"))


@pytest.mark.parametrize("name", ["lsb_sketch", "usb_fast", "cw_lsb_slow", "am", "als_notch", "wrap_agc_off", "mode6_agc_off", "agc_overdrive"])
def test_tail_model_is_the_images_tail(oracle, name):
    """tests/engine_tail_model.py from the "demod" tap on, bit for bit: the `filt`, `agc` and `als` taps and the int16 audio of
    tests/golden/engine_kat.npz -- an SSB setting (lsb_sketch: AGC medium; usb_fast: AGC fast; cw_lsb_slow: AGC slow), AM, the ALS
    notch adaptive, the AGC off with a wrapping store (wrap_agc_off, mode6_agc_off), an overdriven AGC.  The fixture holds the taps
    of a case's first blocks; where it holds none (wrap_agc_off) they are the restatement's (oracle/rdsp_engine_oracle.c, which
    tests/test_engine_kat.py holds to the image), the audio is the fixture's"""
    k = _kat()
    calls = json.loads(str(k[name + "_calls"]))
    stages = ("demod", "filt", "agc", "als")
    if name + "_tap_demod" in k.files:
        taps = {s: k[f"{name}_tap_{s}"][:, 0] for s in stages}
    else:
        e = oracle.OracleEngine(taps=True)
        e.run(k[name + "_iq"], calls)
        taps = {s: np.stack(e.taps[s])[:, 0] for s in stages}
    nb = len(taps["demod"])
    t = TM.Tail(1)
    for c in calls:
        assert c[0] == 0
        if hasattr(t, c[1]):
            getattr(t, c[1])(*c[2:])
    out = t.run(taps["demod"].reshape(1, -1))
    for s in stages[1:]:
        assert np.array_equal(bits(getattr(t, s))[0], bits(taps[s].reshape(-1))), (name, s)
    assert np.array_equal(out[0], k[name + "_out"][:nb * 128]), name
    if name == "wrap_agc_off":
        assert np.abs(np.diff(out[0].astype(np.int32))).max() > 40000                     # a wrapped store, not a saturated one


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _cuda(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _fm_engine(n, max_blocks, W=2, deviation=5000.0, tau=750.0, meter=False, nfm=True):
    from radiodsp_sdr_rx_amd.engine import Engine
    import oracle_lib
    e = Engine(n, max_blocks_per_call=max_blocks, tables=oracle_lib.engine_tables())
    e.sketch_setup()
    if meter:
        e.enable_meter()
    e.set_fm(W, deviation, tau)
    e.enable_fm()
    if nfm:
        assert e.setDemodMode(NFM) == 0.0
    return e


def _tail_settings(e, on):
    """audio filter 2700 on, AGC medium, ALS notch -- or all three off"""
    if on:
        e.enableAudioFilter(); e.setAudioFilter(6); e.setAGCmode(2); e.enableALSfilter(); e.setALSfilterNotch(); e.setALSfilterAdaptive()
    else:
        e.setAudioFilter(10); e.setAGCmode(0); e.disableALSfilter()


def _tail_model(n, on):
    t = TM.Tail(n)
    if on:
        t.enableALSfilter().setALSfilterNotch().setALSfilterAdaptive()
    else:
        t.setAudioFilter(10).setAGCmode(0)
    return t


@functools.lru_cache(maxsize=None)
def _stations(n, nb, seed=50):
    """int16 [n, nb * 128, 2]: a drawn FM station per channel (deviation, tone, offset, carrier and noise drawn); with three
    channels or more, channel 1 on the rails and channel 2 all zeros"""
    r = np.random.default_rng(seed + n)
    x = np.stack([FM.station(seed + 7 * c, nb, r.uniform(1500, 5000), r.uniform(300, 3000), r.uniform(200, 20000), r.uniform(1, 30), r.uniform(-2000, 2000))
                  for c in range(n)])
    if n >= 3:
        x[1] = r.choice(np.array([32767, -32768], np.int16), (nb * 128, 2))
        x[2] = 0
    return x


def _play(e, x, pattern):
    """the blocks of x in calls of pattern's sizes -> (audio int16 [n, t], demod, level float32 [n, t])"""
    audio, demod, level, a = [], [], [], 0
    for k in pattern:
        y = e.update(_cuda(x[:, a * 128:(a + k) * 128])).cpu().numpy()
        assert np.array_equal(y[..., 0], y[..., 1])
        audio.append(y[..., 0]); demod.append(e.read_demod(k).cpu().numpy()); level.append(e.read_fm_level(k).cpu().numpy())
        a += k
    return np.concatenate(audio, 1), np.concatenate(demod, 1), np.concatenate(level, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("tau", [0.0, 750.0])
@pytest.mark.parametrize("W", [2, 3])
@pytest.mark.parametrize("n", [1, 5, 97, 300])
def test_gpu_fm_rows_are_the_model(rdsp, n, W, tau):
    """1, 5, 97 and 300 receivers (a ragged last workgroup, more than one workgroup) in NFM, both channel filters, with and
    without de-emphasis: rdsp_engine_read_demod, rdsp_engine_read_fm_level and the int16 audio equal the models bit for bit --
    three blocks as one call, as 1 + 2 and as 1 + 1 + 1 (half trips and a carry between calls), nine blocks in one call (whole
    trips and a half), each from a reset, so also: a reset, then again.  The audio is engine_tail_model on the model's row, with
    the audio filter on, AGC medium and the ALS notch, and once more with all three off"""
    x = _stations(n, 9)
    m = FM.Fm(n, W, 5000.0 if W == 2 else 2500.0, tau)
    y, lvl = m.run(x)
    e = _fm_engine(n, 9, W, 5000.0 if W == 2 else 2500.0, tau)
    assert e.fm_enabled
    for on in (True, False):
        _tail_settings(e, on)
        want = _tail_model(n, on).run(y)
        for pattern in ([3], [1, 2], [1, 1, 1], [9]):
            e.reset()
            t = 128 * sum(pattern)
            audio, demod, level = _play(e, x, pattern)
            assert np.array_equal(bits(demod), bits(y[:, :t])), (on, pattern, np.argwhere(bits(demod) != bits(y[:, :t]))[:3])
            assert np.array_equal(bits(level), bits(lvl[:, :t])), (on, pattern)
            assert np.array_equal(audio, want[:, :t]), (on, pattern, np.argwhere(audio != want[:, :t])[:3])
    if n >= 3:
        assert (tau != 0.0 or np.abs(y[1]).max() == 1.0) and not y[2].any() and not lvl[2].any()   # the rails clip, silence stays silent
    e.close()


@pytest.mark.gpu
def test_gpu_fm_unaligned_rows(rdsp):
    """input rows that are not 16-byte aligned (the buffer begins one pair behind a boundary, the rows lie an odd number of pairs
    apart): the 4-byte loads give the rows of the aligned call"""
    import torch
    n, nb = 6, 3
    x = _stations(n, nb)
    m = FM.Fm(n, 3, 2500.0, 750.0)
    y, lvl = m.run(x)
    e = _fm_engine(n, 4, 3, 2500.0, 750.0)
    stride = nb * 128 + 3
    buf = torch.zeros(n * stride * 2 + 8, dtype=torch.int16, device="cuda")
    rows = buf[2:2 + n * stride * 2].view(n, stride, 2)
    rows[:, :nb * 128].copy_(_cuda(x))
    assert rows.data_ptr() % 16 == 4
    out = torch.empty((n, nb * 128, 2), dtype=torch.int16, device="cuda")
    assert e.lib.rdsp_engine_update(e.h, rows.data_ptr(), stride, nb, out.data_ptr(), nb * 128, None) == 0, e.lib.rdsp_last_error()
    assert np.array_equal(bits(e.read_demod(nb).cpu().numpy()), bits(y)) and np.array_equal(bits(e.read_fm_level(nb).cpu().numpy()), bits(lvl))
    e.close()


@pytest.mark.gpu
def test_gpu_fm_silence_decays_through_the_subnormals(rdsp):
    """a modulated burst of two blocks, then 34 blocks of zeros, de-emphasis 750 us: y decays by (1 - a) a sample, is below
    2^-126 after about 3000 samples and must match the model all the way down -- a build that flushes subnormals cannot"""
    nb = 36
    x = np.zeros((2, nb * 128, 2), np.int16)
    x[0, :256] = FM.station(70, 2, 5000.0, 400.0, 12000.0, 0.0)
    x[1, :256] = FM.station(71, 2, 3000.0, 900.0, 900.0, 0.0)
    m = FM.Fm(2, 2, 5000.0, 750.0)
    y, lvl = m.run(x)
    sub = (np.abs(y) > 0) & (np.abs(y) < 2.0 ** -126)
    assert sub[0].sum() > 100 and sub[1].sum() > 100, sub.sum(1)
    e = _fm_engine(2, nb)
    _tail_settings(e, False)
    audio, demod, level = _play(e, x, [nb])
    assert np.array_equal(bits(demod), bits(y)) and np.array_equal(bits(level), bits(lvl))
    assert np.array_equal(audio, _tail_model(2, False).run(y))
    e.close()


@pytest.mark.gpu
def test_gpu_fm_beside_lsb_and_am_groups(rdsp):
    """one engine with an LSB, an AM and an NFM group (3 + 4 + 5 receivers): the LSB and AM receivers equal, bit for bit, those of
    a second engine that never called rdsp_engine_enable_fm and has the same settings and input; the NFM receivers equal the
    model; the level rows of the receivers not in NFM read as zeros.  Nothing existing changes on the device"""
    from test_engine_meter import _bursts
    n, nb, first = 12, 6, [0, 3, 7]
    x = _bursts(81, n, nb)
    x[7:] = _stations(5, nb)
    engines = []
    for with_fm in (True, False):
        e = _fm_engine(n, 4, 2, 5000.0, 750.0, nfm=False) if with_fm else None
        if e is None:
            from test_engine_meter import _engine
            e = _engine(n, 4, meter=False)
            assert not e.fm_enabled
        e.set_groups(first)
        e.select_group(1); e.setDemodMode(4); e.setAudioFilter(0)
        e.select_group(2)
        if with_fm:
            assert e.setDemodMode(NFM) == 0.0
        e.select_group(-1)
        engines.append(e)
    a, b = engines
    fm_audio, fm_demod, fm_level = _play(a, x, [4, 2])
    plain = np.concatenate([b.update(_cuda(x[:, :512])).cpu().numpy(), b.update(_cuda(x[:, 512:])).cpu().numpy()], 1)[..., 0]
    assert np.array_equal(fm_audio[:7], plain[:7]) and plain[:7].any()
    m = FM.Fm(5, 2, 5000.0, 750.0)
    y, lvl = m.run(x[7:])
    assert np.array_equal(bits(fm_demod[7:]), bits(y)) and np.array_equal(bits(fm_level[7:]), bits(lvl)) and not fm_level[:7].any()
    assert np.array_equal(fm_audio[7:], TM.Tail(5).run(y))
    blob_a, blob_b = a.save_state(0, n), b.save_state(0, n)                               # a's blob carries the FM part, b's is as ever
    assert blob_a.view(np.uint32)[3] == 8 and blob_b.view(np.uint32)[3] == 0 and len(blob_b) + n * 50 * 4 == len(blob_a)
    assert np.array_equal(blob_a[16:16 + 7 * 2592 * 4], blob_b[16:16 + 7 * 2592 * 4])     # and the LSB and AM receivers' state is the same
    for e in engines:
        e.close()


def _keyed_carriers(n, nb, seed=90):
    """int16 [n, nb * 128, 2]: noise of a few counts everywhere; the odd channels carry an FM station keyed in drawn bursts of
    3 ... 6 blocks, the even ones stay idle"""
    r = np.random.default_rng(seed)
    x = np.rint(4.0 * r.standard_normal((n, nb * 128, 2))).astype(np.int16)
    for c in range(1, n, 2):
        st = FM.station(seed + c, nb, 4000.0, r.uniform(400, 2500), r.uniform(2000, 16000), 0.0).astype(np.int32)
        b = int(r.integers(0, 4))
        while b < nb:
            k = int(r.integers(3, 7))
            x[c, b * 128:(b + k) * 128] += st[b * 128:(b + k) * 128].astype(np.int16)
            b += k + int(r.integers(3, 8))
    return x


@pytest.mark.gpu
def test_gpu_fm_carrier_squelch(rdsp):
    """the meter of an NFM group measures the level rows: with thresholds between an idle channel's level and a carrier's, the idle
    receivers (noise only) stay closed and leave as zero words although their demodulated rows are full-scale noise, and carrier
    bursts open the gate.  rdsp_engine_read_meter's level, peak and open records equal engine_meter_model on the model's level
    rows; the active list, rdsp_engine_pack_active and rdsp_engine_pack_voice (R = 2) equal their models"""
    from radiodsp_sdr_rx_amd.engine import ms_of_db
    n, nb = 10, 24
    x = _keyed_carriers(n, nb)
    m = FM.Fm(n, 2, 5000.0, 0.0)                                                         # no de-emphasis: the idle noise stays on the rails
    y, lvl = m.run(x)
    s = Squelch(F32(ms_of_db(-40.0)), F32(ms_of_db(-46.0)), 2, attack=1.0, decay=1.0)    # a carrier of 2000 counts is -21 dB, the noise -75 dB
    e = _fm_engine(n, 16, tau=0.0, meter=True)
    e.set_meter(1.0, 1.0)                                                                # the level is the block's mean square
    e.set_squelch(float(s.open_ms), float(s.close_ms), s.hang_blocks)
    e.enable_voice(2)
    meter, voice, tail = Meter(n), V.Voice(n, 2), TM.Tail(n)
    for a, k in ((0, 16), (16, 8)):
        yd = e.update(_cuda(x[:, a * 128:(a + k) * 128]))
        audio = yd.cpu().numpy()
        level, peak, gate = (v.cpu().numpy() for v in e.read_meter(k))
        wl, wp, wg = meter.run(lvl[:, a * 128:(a + k) * 128], s)
        assert np.array_equal(bits(level), bits(wl)) and np.array_equal(bits(peak), bits(wp)) and np.array_equal(gate, wg)
        want = gated(tail.run(y[:, a * 128:(a + k) * 128]), wg)
        assert np.array_equal(audio[..., 0], want) and np.array_equal(audio[..., 1], want)
        lst, cnt = e.active()
        assert np.array_equal(lst.cpu().numpy(), np.flatnonzero(wg.any(1)))
        pa, pr, needed = e.pack_active(yd)
        wa, wr, wn = P.pack(want, wg)
        assert needed == wn and np.array_equal(pa.cpu().numpy(), wa) and np.array_equal(pr.cpu().numpy(), wr)
        vrows = voice.run(want)
        assert np.array_equal(e.read_voice(k).cpu().numpy(), vrows)
        va, vr, vneeded = e.pack_voice(k)
        wva, wvr, wvn = V.pack(vrows, wg, 2)
        assert vneeded == wvn and np.array_equal(va.cpu().numpy(), wva) and np.array_equal(vr.cpu().numpy(), wvr)
        if a == 0:
            assert not wg[0::2].any() and wg[1::2].any(1).all() and not wg[1::2].all()     # idle closed; every carrier opens and closes
            assert not audio[0::2].any() and np.abs(e.read_demod(k).cpu().numpy()[0::2]).max() > 0.9   # zero words over full-scale noise
    e.close()


def _fm_band(stations, fs, n, deviation, amp, seed):
    """a complex band at fs Hz: per station (Hz from the centre) a carrier of `amp`, frequency-modulated by a 1 kHz tone at the
    deviation, and weak noise"""
    r = np.random.default_rng(seed)
    t = np.arange(n)
    z = 0.002 * amp * (r.standard_normal(n) + 1j * r.standard_normal(n))
    for f in stations:
        z = z + amp * np.exp(1j * ((deviation / 1000.0) * np.sin(2 * np.pi * 1000.0 / fs * t + r.uniform(0, 6)) + 2 * np.pi * f / fs * t))
    return z


@pytest.mark.gpu
def test_gpu_fm_on_the_sources_path(rdsp):
    """three NFM receivers tuned with rdsp_engine_tune to stations inside one shared uint8 band at 44 100 x 160 / 147 = 48 000 Hz:
    setDemodMode(7) returned the offset 0.0, so the tuning pass puts each station at DC, and the audio, the demodulated rows and
    the level rows are bit for bit those of rdsp_engine_update on the tuned rows (the source pass restated in numpy by
    tests/engine_sources_model.py); the FM model on those rows gives the same bits"""
    import engine_sources_model as S
    from radiodsp_sdr_rx_amd.engine import SRC_U8
    P_, Q_, nb = 160, 147, 4
    stations = [-12000.0, 3000.0, 15500.0]
    n_in = (nb * 128 * P_) // Q_
    raw = S._to_u8(S._int16(_fm_band(stations, 48000.0, n_in, 2500.0, 6000.0, 5)))
    e = _fm_engine(3, nb, 3, 2500.0, 750.0, nfm=False)
    e.set_sources(1, [0, 0, 0])
    e.set_source_rate(P_, Q_)
    e.set_source_format(SRC_U8)
    assert e.setDemodMode(NFM) == 0.0
    e.tune(0, stations)
    y = e.update_sources(_cuda(raw[None]), n_blocks=nb).cpu().numpy()
    demod, level = e.read_demod(nb).cpu().numpy(), e.read_fm_level(nb).cpu().numpy()
    steps = np.array([[S.dphi_of(0.0, s, P_, Q_)] * nb for s in stations], np.uint64)
    tuned = S.stream(S.values(S.U8, raw), P_, Q_, S.taps_of(P_, Q_), steps, S.table(rdsp))[0]
    b = _fm_engine(3, nb, 3, 2500.0, 750.0)
    audio_b, demod_b, level_b = _play(b, tuned, [nb])
    assert np.array_equal(y[..., 0], audio_b) and np.array_equal(bits(demod), bits(demod_b)) and np.array_equal(bits(level), bits(level_b))
    m = FM.Fm(3, 3, 2500.0, 750.0)
    my, ml = m.run(tuned)
    assert np.array_equal(bits(demod), bits(my)) and np.array_equal(bits(level), bits(ml)) and np.array_equal(y[..., 0], TM.Tail(3).run(my))
    assert ml[:, 256:].min() > 0.1                                                      # every receiver sits on its carrier
    for e_ in (e, b):
        e_.close()


@pytest.mark.gpu
def test_gpu_fm_behind_the_channelizer(rdsp):
    """a station at 192 000 Hz (44 100 x 640 / 147) placed by rdsp_channelizer_place through a Channelizer at (640, 147, 16, 3):
    the receiver listens to the sub-band row it names, tuned to the residual it names, and the 1 kHz tone it recovers has the
    amplitude the CPU test holds the model to: within 0.5 % of sinc(1000 / 44100)"""
    import engine_sources_model as S
    from radiodsp_sdr_rx_amd.channelizer import Channelizer
    from radiodsp_sdr_rx_amd.engine import SRC_F32, SRC_S16
    nb, station = 10, 40700.0
    cz = Channelizer(1, 640, 147, 16, 3, fmt=SRC_S16, max_blocks_per_call=nb)
    n_in = cz.source_pairs(nb)
    src = S._int16(_fm_band([station, -30000.0], 192000.0, n_in, 2500.0, 5000.0, 6))
    k, residual = cz.place(station)
    assert k == 3 and abs(residual - 4700.0) < 1e-6
    rows = cz.update(_cuda(src[None]), nb)
    e = _fm_engine(1, nb, 3, 2500.0, 0.0, nfm=False)
    e.set_sources(16, [k])
    e.set_source_decimation(3)
    e.set_source_format(SRC_F32)
    assert e.setDemodMode(NFM) == 0.0
    e.tune(0, [residual])
    e.update_sources(rows.contiguous())
    demod = e.read_demod(nb).cpu().numpy()[0].astype(np.float64)
    amp, sinc = _tone_amplitude(demod[3 * 128:], 1000.0), np.sinc(1000.0 / 44100.0)
    print(f"NFM behind the channelizer: recovered tone {amp:.5f}, sinc {sinc:.5f}")
    assert abs(amp / sinc - 1.0) <= 0.005
    e.close()
    cz.close()


@pytest.mark.gpu
def test_gpu_fm_defaults(rdsp):
    """an engine that never called rdsp_engine_set_fm runs W = 2, 5000 Hz, 750 us; a group made later copies its group's settings"""
    from test_engine_meter import _engine
    x = _stations(5, 3, 75)
    e = _engine(5, 4, meter=False)
    e.enable_fm()
    assert e.setDemodMode(NFM) == 0.0
    y, lvl = FM.Fm(5).run(x)
    _, demod, level = _play(e, x, [3])
    assert np.array_equal(bits(demod), bits(y)) and np.array_equal(bits(level), bits(lvl))
    e.reset()
    e.set_groups([0, 2])
    e.select_group(1)
    e.set_fm(3, 2500.0, 0.0)
    e.select_group(-1)
    e.set_groups([0, 2, 4])                                                               # channel 4's new group copies group 1's settings
    _, demod, _ = _play(e, x, [3])
    assert np.array_equal(bits(demod[:2]), bits(y[:2])) and np.array_equal(bits(demod[2:]), bits(FM.Fm(3, 3, 2500.0, 0.0).run(x[2:])[0]))
    e.close()


def _blob_parts(blob, n, with_fm):
    """the words of a blob of n channels behind its channel words"""
    ch_words = 96 + 2 * 512 + 3 * 384 + 320
    return blob[16 + n * ch_words * 4:].view(np.uint32)


@pytest.mark.gpu
def test_gpu_fm_state(rdsp):
    """the detector's state is signal state (W = 3: all 47 history words matter): two FM receivers -- a station, whose 50 words
    are checked to be nonzero, and the all-zero row -- moved by blob to an engine with another channel count, another channel
    index and another max_blocks continues bit for bit; a regrouping in mid-stream keeps it; setDemodMode(7) in mid-stream starts
    from zero state at the next update; switching away and back resets; blob sizes and refusals are as specified; mode 7 is
    ignored before rdsp_engine_enable_fm; rdsp_engine_enable_fm twice is a no-op"""
    from test_engine_meter import _engine
    nb, cut = 8, 3
    x = _stations(4, nb, 60)
    W, DEV = 3, 2500.0
    m = FM.Fm(4, W, DEV, 750.0)
    y, lvl = m.run(x)
    tail = TM.Tail(4).run(y)
    a = _fm_engine(4, 4, W, DEV)
    a.enable_fm()                                                                            # again: a no-op
    first = _play(a, x[:, :cut * 128], [2, 1])
    assert np.array_equal(bits(first[1]), bits(y[:, :cut * 128]))
    blob = a.save_state(2, 2)                                                                # channel 2: the all-zero row; channel 3: a station
    plain = _engine(3, 8, meter=False)
    assert len(blob) == a.lib.rdsp_engine_state_bytes(a.h, 2) == plain.lib.rdsp_engine_state_bytes(plain.h, 2) + 2 * 50 * 4
    assert blob.view(np.uint32)[3] == 8
    mw = FM.Fm(4, W, DEV, 750.0)
    mw.run(x[:, :cut * 128])
    words = mw.words()
    assert words[3].all() and not words[2].any()                                             # every one of the 50 words is there to be lost
    assert np.array_equal(_blob_parts(blob, 2, True).reshape(2, 50), words[2:4])
    before = plain.save_state(0, 3)
    with pytest.raises(rdsp.RdspError) as ex:                                                # an engine without FM refuses the part
        plain.load_state(0, blob)
    assert ex.value.code == -4 and np.array_equal(plain.save_state(0, 3), before)
    assert plain.setDemodMode(NFM) == 8390.0 and not plain.fm_enabled                       # mode 7 before enable_fm: ignored as ever
    with pytest.raises(rdsp.RdspError) as ex:
        plain.read_fm_level(0)
    assert ex.value.code == -4
    # the receivers continue in another engine: 7 channels, indices 4 and 5, 16 blocks a call, a past of its own
    b = _fm_engine(7, 16, W, DEV)
    b.update(_cuda(_stations(7, 1, 61)))
    b.load_state(4, blob)
    assert np.array_equal(_blob_parts(b.save_state(4, 2), 2, True).reshape(2, 50), words[2:4])
    rest = np.zeros((7, (nb - cut) * 128, 2), np.int16)
    rest[4:6] = x[2:4, cut * 128:]
    audio, demod, level = _play(b, rest, [nb - cut])
    assert np.array_equal(bits(demod[4:6]), bits(y[2:4, cut * 128:])) and np.array_equal(bits(level[4:6]), bits(lvl[2:4, cut * 128:]))
    assert np.array_equal(audio[4:6], tail[2:4, cut * 128:]) and demod[5].any() and audio[5].any()
    # a blob without the part zeroes the detector words of the channel it lands on
    b.load_state(5, plain.save_state(0, 1))
    assert not _blob_parts(b.save_state(5, 1), 1, True).any()
    # regrouping in mid-stream keeps the state; the stream goes on in a's own engine
    a.set_groups([0, 1, 3])
    audio, demod, level = _play(a, x[:, cut * 128:], [4, 1])
    assert np.array_equal(bits(demod), bits(y[:, cut * 128:])) and np.array_equal(audio, tail[:, cut * 128:])
    # a group with a pending FM reset cannot join one without it; after the update it may
    a.select_group(1)
    a.setDemodMode(NFM)
    with pytest.raises(rdsp.RdspError) as ex:
        a.set_groups([0])
    assert ex.value.code == -5
    a.select_group(-1)
    # setDemodMode(7) in mid-stream: group 1 (channels 1, 2) starts from zero state at the next update, the others go on
    z = _stations(4, 2, 62)
    d = _play(a, z, [2])[1]
    fresh = FM.Fm(4, W, DEV, 750.0).run(z)[0]
    cont = m.run(z)[0]
    assert np.array_equal(bits(d[[0, 3]]), bits(cont[[0, 3]])) and np.array_equal(bits(d[[1, 2]]), bits(fresh[[1, 2]]))
    assert not np.array_equal(bits(cont[1]), bits(fresh[1]))
    a.set_groups([0])
    # switching away and back resets: a block in AM between two NFM calls (the state is not maintained outside NFM)
    a.setDemodMode(4)
    a.update(_cuda(z[:, :128]))
    a.setDemodMode(NFM)
    d = _play(a, z, [1, 1])[1]
    assert np.array_equal(bits(d), bits(fresh))
    # settings: refused values (a NaN among them) change nothing; rdsp_engine_reset keeps the settings
    nan = float("nan")
    for bad in ((1, 5000.0, 750.0), (4, 5000.0, 750.0), (2, 999.0, 750.0), (2, 7501.0, 750.0), (2, 5000.0, 24.0), (2, 5000.0, 1001.0), (2, 5000.0, -1.0),
                (2, nan, 750.0), (2, 5000.0, nan)):
        with pytest.raises(rdsp.RdspError) as ex:
            a.set_fm(*bad)
        assert ex.value.code == -1
    a.reset()
    assert np.array_equal(bits(_play(a, z, [2])[1]), bits(fresh))
    for e in (a, b, plain):
        e.close()
