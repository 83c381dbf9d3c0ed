"""The DTMF decoder of rdsp_engine_t without a GPU (include/rdsp.h "DTMF decoder"; csrc/rdsp_dtmf.h, csrc/rdsp_engine_dtmf_host.hip):
the exports, every refusal that needs no device, the steps and scales against float64, rdsp_engine_dtmf_gain against a float64
formula and against a sine pushed through the de-emphasis and the model, the key map, tests/host/host_dtmf_check.cpp --
csrc/rdsp_dtmf.h as a program of its own, plain and under ASan + UBSan, run directly -- against the model's bits at every cut of 1
to 3 blocks, and the decoder's figures on the float32 model, printed and asserted.  tests/test_engine_dtmf_gpu.py holds the kernel
to the same model."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import engine_dtmf_model as D
import engine_sources_model as S
import engine_tone_model as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_dtmf_exports(rdsp):
    from radiodsp_sdr_rx_amd import engine
    lib = rdsp.load()
    for name in ("enable_dtmf", "dtmf_enabled", "set_dtmf", "read_dtmf", "read_dtmf_digits", "dtmf_key", "dtmf_gain"):
        assert hasattr(lib, "rdsp_engine_" + name), name
    assert callable(engine.dtmf_key) and callable(engine.dtmf_gain)
    assert all(callable(getattr(engine.Engine, n)) for n in ("enable_dtmf", "set_dtmf", "read_dtmf", "read_dtmf_digits"))
    assert isinstance(engine.Engine.dtmf_enabled, property)


def test_dtmf_refusals_without_a_device(rdsp):
    """no object: every entry point refuses; rdsp_engine_dtmf_gain answers 0.0 to what rdsp_engine_tone_gain refuses.  The
    refusals that need an object are test_engine_dtmf_gpu's"""
    from radiodsp_sdr_rx_amd.engine import dtmf_gain
    lib = rdsp.load()
    assert lib.rdsp_engine_enable_dtmf(None) == -1 and lib.rdsp_engine_dtmf_enabled(None) == 0
    assert lib.rdsp_engine_set_dtmf(None, 4, 0.015, 4.0, 16.0, 0.5, 2, 2) == -1 and b"rdsp_engine_set_dtmf" in lib.rdsp_last_error()
    assert lib.rdsp_engine_read_dtmf(None, 0, None, 0, None, 0, None, 0, None, 0, None) == -1
    assert lib.rdsp_engine_read_dtmf_digits(None, 0, 1, None, None, None) == -1
    nan = float("nan")
    for f, tau in ((0.0, 750.0), (-697.0, 750.0), (22050.0, 750.0), (nan, 750.0), (697.0, 24.0), (697.0, 1001.0), (697.0, nan), (float("inf"), 0.0)):
        assert lib.rdsp_engine_dtmf_gain(f, tau) == 0.0 and b"rdsp_engine_dtmf_gain" in lib.rdsp_last_error(), (f, tau)
        with pytest.raises(rdsp.RdspError):
            dtmf_gain(f, tau)


def test_dtmf_key_map(rdsp):
    """rdsp_engine_dtmf_key is "123A456B789C*0#D"[sym], row by low tone and column by high tone, and 0 for anything else"""
    from radiodsp_sdr_rx_amd.engine import dtmf_key
    lib = rdsp.load()
    assert "".join(dtmf_key(s) for s in range(16)) == "123A456B789C*0#D" == D.KEYS
    for s in (16, 255, -1, 1 << 20):
        assert lib.rdsp_engine_dtmf_key(s) == b"\0" and dtmf_key(s) == ""
    pad = ("123A", "456B", "789C", "*0#D")
    for row in range(4):
        for col in range(4):
            assert dtmf_key(4 * row + col) == pad[row][col] and D.tones_of(4 * row + col) == (D.HZ[row], D.HZ[4 + col])
    assert D.tones_of(D.symbol_of("5")) == (770.0, 1336.0) and D.tones_of(D.symbol_of("D")) == (941.0, 1633.0)


def test_dtmf_steps_and_scales():
    """dphi_t = llround(f_t 2^32 4 / 44100) against the float64 quotient; every tone lies below the decimated Nyquist; scale and
    escale are the float32 nearest to 1 / (64 K)^2 and 1 / (256 K): a pair of sines of amplitudes A_L, A_H that fall on whole
    cycles reads A^2 and A_L^2 + A_H^2 in float64"""
    assert D.dphi_of(0) == round(697.0 * 4 * 2 ** 32 / 44100.0) == 271527638
    for t, f in enumerate(D.HZ):
        assert D.dphi_of(t) == round(f * 4 * 2 ** 32 / 44100.0) and abs(D.dphi_of(t) / 2 ** 32 * 11025.0 - f) < 2e-6 and D.dphi_of(t) < 2 ** 31
    for K in range(4, 33):
        assert D.scale_of(K) == F32(1.0 / (64.0 * K) ** 2) and D.escale_of(K) == F32(1.0 / (256.0 * K))
        assert abs(float(D.scale_of(K)) * (64.0 * K) ** 2 - 1.0) < 2.0 ** -24 and abs(float(D.escale_of(K)) * 256.0 * K - 1.0) < 2.0 ** -24
    K, A = 4, 0.25
    m = np.arange(32 * K)
    d = 4 * A * np.cos(2 * np.pi * 16 * m / (32 * K))                                        # 16 whole cycles a frame, the boxcar's gain taken as 4
    c = np.sum(d * np.exp(2j * np.pi * 16 * m / (32 * K)))
    assert abs(abs(c) ** 2 * float(D.scale_of(K)) - A * A) < 1e-7 and abs(np.sum(d * d) * float(D.escale_of(K)) - A * A) < 1e-7


def test_dtmf_gain_is_the_formula_and_the_filters(rdsp):
    """rdsp_engine_dtmf_gain equals |sin(4 pi f / 44100) / (4 sin(pi f / 44100))| x tone_gain in float64 within 4e-16 relative on
    the eight tones and five time constants, and is what the de-emphasis and the decimator do to a sine: a 770 Hz sine of 0.2
    behind the model's float32 de-emphasis reads sqrt(lo) = 0.2 x gain in the model's second frame of K = 32.  The bound: a frame
    of N = 1024 decimated samples correlates A cos(w n + p) into (A / 2)(N e^{jp} + e^{-jp} sum e^{-2 j w n}), and
    |sum| <= 1 / sin w = 2.36 at w = 2 pi 770 / 11025, so the reading is off by at most 2.36 / 1024 = 0.23 % (plus the table's
    2^-17)"""
    from radiodsp_sdr_rx_amd.engine import dtmf_gain, tone_gain
    for f in D.HZ:
        for tau in (0.0, 25.0, 75.0, 750.0, 1000.0):
            w = math.pi * float(F32(f)) / 44100.0
            want = abs(math.sin(4.0 * w) / (4.0 * math.sin(w))) * tone_gain(f, tau)
            g = dtmf_gain(f, tau)
            assert abs(g - want) <= 4e-16 * want and abs(g - D.gain(f, tau)) <= 4e-16 * want and 0.0 < g < 1.0, (f, tau, g, want)
    g = dtmf_gain(770.0, 750.0)
    print(f"dtmf_gain(770 Hz, 750 us) = {g:.5f}; (1633 Hz, 750 us) = {dtmf_gain(1633.0, 750.0):.5f}; boxcar alone at 1633 Hz {dtmf_gain(1633.0, 0.0):.5f}; "
          f"key A's twist behind 750 us: {20 * math.log10(dtmf_gain(697.0, 750.0) / dtmf_gain(1633.0, 750.0)):.2f} dB")
    y = T.deemph((0.2 * np.sin(2 * np.pi * 770.0 / 44100.0 * np.arange(64 * 128))).astype(F32), 750.0)
    m = D.Dtmf(1, S.table(rdsp), 32)
    key, new, lo, hi = m.run(y[None])
    amp = math.sqrt(float(lo[0, -1]))
    print(f"a 770 Hz sine of 0.2 reads {amp:.5f}; 0.2 x gain = {0.2 * g:.5f}")
    assert (key == 255).all() and (new == 255).all() and not lo[0, :31].any()                # one tone is no key
    assert abs(amp / (0.2 * g) - 1.0) < 1.0 / (1024 * math.sin(2 * math.pi * 770.0 / 11025.0)) + 2.0 ** -17


def _host_rows(nb):
    """float32 [6, nb * 128]: on the rails, all zeros, key 5 that stops in the middle of a block (and of a frame), keys 1 and 9
    back to back with no pause, a row whose only nonzero decimated sample is the first (every tone's phasor is (1, 0) there, so
    all eight powers are equal: both groups tie), the keyed pair under full-range noise"""
    r = np.random.default_rng(29)
    n = nb * 128
    stops = D.keyed("5", 22 * 128 + 64, 0, 0.3, 0.3, total=n)
    b2b = D.keyed("19", 16 * 128, 0, 0.3, 0.3, total=n)
    tie = np.zeros(n)
    tie[:4] = 1.0
    noisy = np.clip(D.keyed("#", 30 * 128, 0, 0.25, 0.2, total=n) + r.uniform(-1.0, 1.0, n), -1.0, 1.0)
    return np.stack([r.choice(np.array([1.0, -1.0]), n), np.zeros(n), stops, b2b, tie, noisy]).astype(F32)


@pytest.mark.parametrize("sanitize", [False, True])
def test_dtmf_host_program(rdsp, tmp_path, sanitize):
    """tests/host/host_dtmf_check.cpp, plain and under ASan + UBSan, a program of its own run on the CPU: on the rows of
    _host_rows, for K = 4 (ratio 1, share 0.01, one frame on and off) and K = 5 (the defaults) and calls of 1, 2 and 3 blocks
    (which it holds to one long call itself), its steps, scales, records and final words equal the model's.  The row of zeros
    and the rails never emit; the key that stops is emitted once and released; the two keys back to back are emitted as 1 and 9;
    the tied row reads key 1 (the lowest index of each group) in its first frame at ratio 1 and nothing at ratio 4"""
    exe = str(tmp_path / ("host_dtmf_check_san" if sanitize else "host_dtmf_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_dtmf_check.cpp"), "-o", exe])
    nb = 40
    rows = _host_rows(nb)
    n = len(rows)
    fin, fout = str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")
    rows.tofile(fin)
    tab = S.table(rdsp)
    for setting in ((4, 0.01, 1.0, 16.0, 0.01, 1, 1), (5, 0.015, 4.0, 16.0, 0.5, 2, 2)):
        K = setting[0]
        m = D.Dtmf(n, tab, *setting)
        key, new, lo, hi = m.run(rows)
        for call_blocks in (1, 2, 3):
            out = subprocess.run([exe, fin, fout] + [str(v) for v in setting] + [str(n), str(nb), str(call_blocks)], capture_output=True, text=True,
                                 timeout=120)
            assert out.returncode == 0 and out.stdout.endswith("host_dtmf_check OK\n"), out.stdout + out.stderr
            assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
            w = np.fromfile(fout, np.uint32)
            assert w[0] == bits(D.scale_of(K)) and w[1] == bits(D.escale_of(K)) and w[2] == bits(m.min2[0]), K
            assert np.array_equal(w[3:11], [D.dphi_of(t) for t in range(8)])
            body = w[11:].reshape(n, 4 * nb + D.WORDS)
            assert np.array_equal(body[:, :nb], key) and np.array_equal(body[:, nb:2 * nb], new), (K, call_blocks)
            assert np.array_equal(body[:, 2 * nb:3 * nb], bits(lo)) and np.array_equal(body[:, 3 * nb:4 * nb], bits(hi)), (K, call_blocks)
            assert np.array_equal(body[:, 4 * nb:], m.words()), (K, call_blocks)
        assert not m.keys(1) and (key[1] == 255).all() and not lo[1].any() and not hi[1].any()         # silence
        assert lo[0].any() and (not m.keys(0) or K == 4)                                              # the rails read something
        assert [k for k, _ in m.keys(2)] == ["5"] and key[2, -1] == 255 and (key[2] == D.symbol_of("5")).sum() >= 20 - K
        assert [k for k, _ in m.keys(3)] == ["1", "9"] and (new[3] != 255).sum() == 2 and key[3, -1] == 255
        assert (lo[:, :K - 1] == 0).all() and (key[:, :K - 1] == 255).all()                           # before the first frame
        first = new[4, K - 1]
        assert bits(lo[4, K - 1]) == bits(hi[4, K - 1]) and lo[4, K - 1] > 0 and first == (0 if K == 4 else 255) and (new[4, K:] == 255).all()
        assert m.words()[:, D.CNT].max() == nb % K and (m.words()[:, D.TBLOCKS] == nb).all() and not m.words()[:, 10:16].any()
    for bad in (["3", "0.015", "4", "16", "0.5", "2", "2"], ["0", "0.015", "4", "16", "0.5", "2", "2"], ["33", "0.015", "4", "16", "0.5", "2", "2"],
                ["4", "0", "4", "16", "0.5", "2", "2"], ["4", "0.015", "0.5", "16", "0.5", "2", "2"], ["4", "0.015", "4", "0.9", "0.5", "2", "2"],
                ["4", "0.015", "4", "16", "1.5", "2", "2"], ["4", "0.015", "4", "16", "0.5", "0", "2"], ["4", "0.015", "4", "16", "0.5", "2", "17"]):
        assert subprocess.run([exe, fin, fout] + bad + ["1", "1", "1"], capture_output=True).returncode == 2, bad


def _sequences():
    """36 keypad sequences: all 16 keys in a drawn order, 40 ms on and 40 ms off, each tone at 0.2 of the deviation under white
    noise of rms 0.03, the pair's frequencies off by -1.5, 0 and +1.5 %, six draws each flat at the tap and six behind the 750 us
    de-emphasis (no pre-emphasis at the transmitter: 7 dB of twist on key A), each after a drawn lead of silence"""
    on = off = 1764
    rows, orders, leads = [], [], []
    for k in range(36):
        r = np.random.default_rng(500 + k)
        order = "".join(r.permutation(list(D.KEYS)))
        leads.append(int(r.integers(0, 512)))
        u = D.keyed(order, on, off, 0.2, 0.2, offset=(-0.015, 0.0, 0.015)[k % 3], lead=leads[-1], phase=r.uniform(0, 6), total=444 * 128)
        rows.append(np.clip(u + 0.03 * r.standard_normal(len(u)), -1.0, 1.0))
        orders.append(order)
    rows = np.stack(rows).astype(F32)
    rows[18:] = D.deemph_rows(rows[18:], 750.0)
    return rows, orders, np.array(leads)


def _decoded(tab, rows, orders, **kw):
    m = D.Dtmf(len(rows), tab, **kw)
    frames = []
    m.run(rows, frames=frames)
    good = sum("".join(k for k, _ in m.keys(c)) == orders[c] and int(m.words()[c, D.NDIGITS]) == 16 for c in range(len(rows)))
    return good, m, frames


def test_dtmf_figures(rdsp):
    """the decoder's figures on the float32 model, printed and asserted, at the defaults K = 4, min_amp 0.015, ratio 4, twist 16,
    share 0.5, two frames on and two off.  The 36 sequences of _sequences are each read back exactly: the 16 keys once each, in
    order.  60 s of voice-band noise of rms 0.25 (engine_tone_model.voice_noise, clipped; 60 rows of a second, flat and behind
    the de-emphasis) emit nothing, and neither do 20 s of an idle discriminator (uniform +-1, flat and behind the de-emphasis).
    The largest share (P_L + P_H) / E of a frame of idle noise lies below the default share and the smallest share of a frame
    that lies wholly inside a key's 40 ms (every one of which reads that key) above it.  Printed only: K = 5 and twist 10 with min_amp 0.02, which the issue's float64 sketch saw fail"""
    tab = S.table(rdsp)
    rows, orders, leads = _sequences()
    good, m, frames = _decoded(tab, rows, orders, K=4)
    hit_share, hits = np.inf, 0
    for k, (P, E, sym, end) in enumerate(frames):                                            # frame k is samples 512 k ... 512 k + 511
        at = 512 * k - leads
        inside = (at >= 0) & (at % 3528 + 512 <= 1764) & (at // 3528 < 16)                    # wholly inside a key's 40 ms
        assert (sym[inside] == [D.symbol_of(orders[c][at[c] // 3528]) for c in np.flatnonzero(inside)]).all(), k
        if inside.any():
            hit_share, hits = min(hit_share, float(((P[:, :4].max(1) + P[:, 4:].max(1)) / E)[inside].min())), hits + int(inside.sum())
    print(f"defaults: {good} of 36 sequences read exactly; {hits} frames lie wholly inside a key and read it, their smallest share {hit_share:.3f}")
    assert good == 36 and hits >= 36 * 16 * 2
    for name, kw in (("K = 5", dict(K=5)), ("twist 10, min_amp 0.02", dict(K=4, twist=10.0, min_amp=0.02)), ("share 0.66", dict(K=4, share=0.66))):
        print(f"{name}: {_decoded(tab, rows, orders, **kw)[0]} of 36 sequences read exactly")
    sec = 345 * 128
    voice = np.clip(np.stack([T.voice_noise(900 + k, sec, 0.25) for k in range(60)]), -1.0, 1.0).astype(F32)
    r = np.random.default_rng(31)
    idle = r.uniform(-1.0, 1.0, (20, sec)).astype(F32)
    worst_idle = 0.0
    for name, x in (("voice-band noise, flat", voice), ("voice-band noise, de-emphasised", D.deemph_rows(voice)), ("idle, flat", idle),
                    ("idle, de-emphasised", D.deemph_rows(idle))):
        q = D.Dtmf(len(x), tab, 4)
        fr = []
        key, new, lo, hi = q.run(x, frames=fr)
        with np.errstate(divide="ignore", invalid="ignore"):
            share = max(float(np.nan_to_num((P[:, :4].max(1) + P[:, 4:].max(1)) / E).max()) for P, E, sym, end in fr)
        syms = sum(int((sym != 255).sum()) for P, E, sym, end in fr)
        print(f"{name}: {len(x) * sec / 44100.0:.0f} s, {int(q.words()[:, D.NDIGITS].sum())} digits, {syms} of {len(fr) * len(x)} frames read a symbol, "
              f"largest share {share:.3f}, largest sqrt(P) {math.sqrt(max(float(lo.max()), float(hi.max()))):.4f}")
        assert not q.words()[:, D.NDIGITS].any() and (new == 255).all() and (key == 255).all(), name
        if name.startswith("idle"):
            worst_idle = max(worst_idle, share)
    print(f"shares: idle noise at most {worst_idle:.3f} < {D.DEFAULT_SHARE} < {hit_share:.3f} on true hits")
    assert worst_idle < D.DEFAULT_SHARE < hit_share
