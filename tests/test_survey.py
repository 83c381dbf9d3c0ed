"""rdsp_survey_t (include/rdsp.h; kernel csrc/rdsp_survey.hip, host half csrc/rdsp_survey_host.c): Welch-averaged power spectra
of shared IQ source rows in the engine's four sample formats, and the station finder that turns a row into the station_hz of
rdsp_engine_tune.  tests/survey_model.py restates the definition in float64.

`-m "not gpu"`: the window (formula, sum, sidelobes of the float taps), the schedule and the axis, the finder on the model's row
of a band of three AM stations, tests/host/host_survey_check.c under the address and undefined-behaviour sanitizers, and the
noise floor of the float64 model and of the float32 reference (survey_model.survey_rows_f32) on survey_model.two_tone, with
the check the GPU floor test applies (survey_model.floor_within_margin) shown to refuse a floor of -130 dB.
`-m gpu` (3 sources, a few N pairs each): parity with the float64 model inside the float32 FFT bound, the call split and the
formats bit for bit, sign and scale, reset and refusals, and the way from a survey row to tuned receivers.
tests/test_survey_gpu.py goes on from here on the GPU: the kernel's floor against the float32 reference, and the schedule and
the launch shape at the settings these cases leave out (navg 1, 8 and 256, lead > 0 with a trailing row in one launch, 300
units, 67 and 4096 sources, drawn sessions with a reset in mid-row).

The bound (survey_model.survey_rows): per bin, summed over the row's frames, 2 |X_k| E + E^2 with
E = (12 log2 N + 2) 2^-24 sqrt(N) ||x_f||_2, plus navg 2^-24 sum P.  Worst observed fraction of it on an MI355X: 0.0037
(N = 1024) and 0.0019 (N = 4096), printed by test_gpu_parity_with_the_float64_model."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import survey_model as M
from engine_sources_model import FL, HERE, ROOT, S8, S16, U8, DTYPE, values, widened

NSRC = 3


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1024, 4096])
def test_window(rdsp, N):
    """rdsp_survey_window is the formula rounded to float32, sums to 1 within 2^-20, and the float taps keep the 4-term
    Blackman-Harris sidelobes: at most -92 dB outside +-4 bins (16x zero-padded float64 FFT; -92.03 dB at both sizes)"""
    from radiodsp_sdr_rx_amd import survey
    w = survey.window(N)
    assert w.dtype == np.float32 and np.array_equal(w, M.window_formula(N))
    assert abs(w.astype(np.float64).sum() - 1.0) <= 2.0 ** -20
    X = np.abs(np.fft.fft(w.astype(np.float64), 16 * N))
    k = np.arange(16 * N)
    away = np.minimum(k, 16 * N - k) / 16.0 > 4.0
    worst = 20.0 * np.log10(X[away].max() / X[0])
    print(f"N = {N}: highest sidelobe {worst:.2f} dB")
    assert worst <= -92.0
    with pytest.raises(rdsp.RdspError):
        survey.window(2048)


def test_schedule_and_axis(rdsp):
    """rows_between against rows(T + pairs) - rows(T) over ragged splits -- totals that cross N, 0-pair calls, pairs_before
    above 2^32 -- and bin_hz against (j - N / 2) 44100 P / (Q N)"""
    from radiodsp_sdr_rx_amd import survey
    r = np.random.default_rng(11)
    for N in (1024, 4096):
        for navg in (1, 2, 8, 256):
            for T0 in (0, N - 3, (1 << 32) + 12345, (1 << 40) + 1):
                T = T0
                cuts = [1, N // 2 - 1, 0, N // 2, N + 1, 777, 0] + [int(v) for v in r.integers(0, 3 * N * navg, 12)]
                for pairs in cuts:
                    assert survey.rows_between(N, navg, T, pairs) == M.rows_between(N, navg, T, pairs), (N, navg, T, pairs)
                    T += pairs
        assert survey.rows_between(N, 1, 0, N - 1) == 0 and survey.rows_between(N, 1, 0, N) == 1
        for P, Q in ((1, 1), (160, 147), (8000, 147)):
            for j in (0, 1, N // 2 - 1, N // 2, N // 2 + 1, N - 1):
                want = (j - N // 2) * 44100.0 * P / (Q * N)
                assert abs(survey.bin_hz(N, P, Q, j) - want) <= 1e-12 * max(abs(want), 1.0)
    for bad in ((512, 2), (1024, 3), (1024, 0), (1024, 512)):
        with pytest.raises(rdsp.RdspError):
            survey.rows_between(bad[0], bad[1], 0, 10)


@functools.lru_cache(maxsize=None)
def _band_rows():
    """the band of survey_model.band_u8, the model's rows of it (float64 [2, 1024]) and their bound"""
    from radiodsp_sdr_rx_amd import survey
    raw = M.band_u8()
    P, B = M.survey_rows(U8, raw, M.BAND["N"], M.BAND["navg"], survey.window(M.BAND["N"]))
    assert P.shape == (2, M.BAND["N"])
    return raw, P, B


def _check_stations(hz):
    half_bin = 0.5 * 44100.0 * M.BAND["P"] / (M.BAND["Q"] * M.BAND["N"])
    assert len(hz) == 3, hz
    for got, want in zip(hz, M.BAND["order"]):
        assert abs(got - want) <= half_bin, (hz, M.BAND["order"])


def test_find_stations_on_the_models_row(rdsp):
    """U8 at 160 / 147, N = 1024, navg = 4, carriers of 40, 12 and 25 codes at -17300, +2210.5 and +9050 Hz with 30 % AM at
    400 Hz in unit noise: min_db 20 and min_spacing 1000 Hz give exactly the three stations, strongest first, within half a
    bin (23.4 Hz) -- the +-400 Hz sidebands stand 28 - 39 dB over the floor and only the spacing rule drops them.  A flat row
    gives none, max_out = 2 the two strongest, bins 0 and N - 1 are never reported."""
    from radiodsp_sdr_rx_amd import survey
    _, P, _ = _band_rows()
    row = P[0].astype(np.float32)
    B = M.BAND
    hz, pw = survey.find_stations(row, B["P"], B["Q"], 20.0, 1000.0, 16)
    print("stations", hz, "off by", hz - np.array(B["order"]))
    _check_stations(hz)
    assert np.all(np.diff(pw) < 0) and abs(pw[0] / (40.0 * 256.0) ** 2 - 1.0) < 0.05
    assert np.allclose(hz, M.find_stations(row, B["N"], B["P"], B["Q"], 20.0, 1000.0, 16), rtol=0, atol=1e-6)
    every, _ = survey.find_stations(row, B["P"], B["Q"], 20.0, 0.0, 64)       # without the spacing rule: the six sidebands too
    assert len(every) == 9
    for f in B["order"]:
        assert np.abs(every - (f - 400.0)).min() < 24.0 and np.abs(every - (f + 400.0)).min() < 24.0
    two, _ = survey.find_stations(row, B["P"], B["Q"], 20.0, 1000.0, 2)
    assert np.array_equal(two, hz[:2])
    assert len(survey.find_stations(np.full(B["N"], 7.0, np.float32), B["P"], B["Q"], 20.0, 1000.0, 16)[0]) == 0
    edge = np.ones(B["N"], np.float32)
    edge[0] = edge[-1] = 1e9
    edge[300] = 1e6
    hz, _ = survey.find_stations(edge, B["P"], B["Q"], 20.0, 0.0, 16)
    assert len(hz) == 1 and hz[0] == survey.bin_hz(B["N"], B["P"], B["Q"], 300)
    with pytest.raises(rdsp.RdspError):
        survey.find_stations(np.ones(512, np.float32), 1, 1)


@functools.lru_cache(maxsize=None)
def _two_tone_rows(N, weak_db):
    """one row (navg = 2) of survey_model.two_tone in format F32: the float64 model's, its bound, the float32 reference's"""
    from radiodsp_sdr_rx_amd import survey
    raw = M.two_tone(N, weak_db, 2)
    assert raw.dtype == np.float32 and raw.shape == (N + N // 2, 2)
    P, B = M.survey_rows(FL, raw, N, 2, survey.window(N))
    R = M.survey_rows_f32(FL, raw, N, 2, survey.window(N))
    assert P.shape == B.shape == R.shape == (1, N) and R.dtype == np.float32
    for a in (P, B, R):
        a.setflags(write=False)
    return P[0], B[0], R[0]


@pytest.mark.parametrize("weak_db", [-100, -120])
@pytest.mark.parametrize("N", [1024, 4096])
def test_floor_of_the_model_and_of_the_float32_reference(rdsp, N, weak_db):
    """a float32 carrier of 0.5 on bin 37 and a tone weak_db below it on bin N / 4 + 3, F32, navg 2.  More than 8 bins from both,
    relative to the peak: the float64 model reads at most -160 dB; the float32 reference (survey_model.survey_rows_f32) at most
    -148 dB (N = 1024) and -153 dB (N = 4096); the bound of survey_rows admits at least -101 dB at every such bin, which is why
    the bound cannot hold a kernel to its floor.  The reference's weak bin is within 1 % of the model's in power."""
    P, B, R = _two_tone_rows(N, weak_db)
    strong, weak = M.tone_indices(N)
    far = M.far(N)
    assert far.sum() == N - 34 and not far[strong - 8] and far[strong - 9] and not far[weak + 8] and far[weak + 9]
    assert P.argmax() == strong and R.argmax() == strong and abs(P[strong] / 16384.0 ** 2 - 1.0) < 1e-3
    model, ref = M.floor_db(P, N), M.floor_db(R, N)
    bound = 10.0 * np.log10(B[far].min() / P.max())
    weak_off = abs(float(R[weak]) / P[weak] - 1.0)
    print(f"N = {N}, weak tone {weak_db} dB: far-bin maximum of the float64 model {model:.1f} dB, of the float32 reference {ref:.1f} dB; "
          f"the bound at the far bins {bound:.1f} dB; the reference's weak bin off the model's by {weak_off:.1e}")
    assert model <= -160.0
    assert ref <= (-148.0 if N == 1024 else -153.0)
    assert weak_off <= 0.01 and abs(10.0 * np.log10(P[weak] / P[strong]) - weak_db) < 0.01
    assert bound >= -101.0


@pytest.mark.parametrize("N", [1024, 4096])
def test_floor_check_has_teeth(N):
    """survey_model.floor_within_margin, the check the GPU floor test applies: the float32 reference's own row passes it; the
    same row with 10^-13 of its peak (-130 dB) added to every far bin fails it, while that row stays within a hundredth of
    the bound of survey_rows (-130 dB against a bound of about -99 dB is a factor 1e-3) -- the bound would not have noticed.
    The mirrored mask on the mirrored row likewise."""
    P, B, R = _two_tone_rows(N, -100)
    ok, got, ref = M.floor_within_margin(R, R, N)
    assert ok and got == ref
    bad = R.astype(np.float64)
    bad[M.far(N)] += 1e-13 * bad.max()
    ok, got, ref = M.floor_within_margin(bad, R, N)
    frac = (np.abs(bad - P) / B).max()
    print(f"N = {N}: a floor of {got:.1f} dB against the reference's {ref:.1f} dB fails; it sits at {frac:.4f} of the bound")
    assert not ok and got > ref + M.FLOOR_MARGIN_DB and -130.5 < got < -129.5
    assert frac <= 0.01
    assert M.floor_within_margin(R[::-1], R[::-1], N, mirror=True)[0] and not M.floor_within_margin(bad[::-1], R[::-1], N, mirror=True)[0]
    assert np.array_equal(M.far(N, mirror=True)[1:], M.far(N)[1:][::-1])


def test_float32_transform_without_scipy(monkeypatch):
    """survey_model._fft_c64 without scipy (the radix-2 numpy transform) stays complex64 and agrees with the float64 transform
    to float32 accuracy"""
    import sys
    r = np.random.default_rng(3)
    x = (r.standard_normal(1024) + 1j * r.standard_normal(1024)).astype(np.complex64)
    want = np.fft.fft(x.astype(np.complex128))
    with_scipy = M._fft_c64(x)
    monkeypatch.setitem(sys.modules, "scipy.fft", None)
    monkeypatch.setitem(sys.modules, "scipy", None)
    plain = M._fft_c64(x)
    for X in (with_scipy, plain):
        assert X.dtype == np.complex64 and np.abs(X - want).max() <= 1e-5 * np.abs(want).max()


def test_host_half_under_address_and_ub_sanitizers(tmp_path):
    """tests/host/host_survey_check.c, a program of its own, built with csrc/rdsp_survey_host.c under ASan + UBSan: the
    host-only functions on exactly sized buffers, and their refusals"""
    exe = str(tmp_path / "host_survey_check")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "host", "host_survey_check.c"),
                           os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc", "rdsp_survey_host.c"), "-lm", "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "host_survey_check OK" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _random_rows(fmt, n, seed):
    """[NSRC, n, 2] elements of format fmt over the whole range, the rail values mixed in"""
    r = np.random.default_rng(seed)
    if fmt == FL:
        x = r.uniform(-1.0, 1.0, (NSRC, n, 2)).astype(np.float32)
        rails = np.array([-1.0, 1.0, 1.5, -2.0, 0.0], np.float32)
    else:
        info = np.iinfo(DTYPE[fmt])
        x = r.integers(info.min, info.max + 1, (NSRC, n, 2)).astype(DTYPE[fmt])
        rails = np.array([info.min, info.max], DTYPE[fmt])
    at = r.random((NSRC, n, 2)) < 0.02
    x[at] = rails[r.integers(0, len(rails), int(at.sum()))]
    return x


def _odd_view(raw):
    """the rows on the device as a view at an odd pair offset into a longer buffer: src_stride > pairs, one-pair alignment"""
    import torch
    buf = torch.zeros((raw.shape[0], raw.shape[1] + 3, 2), dtype=torch.from_numpy(raw[:1, :1]).dtype, device="cuda")
    buf[:, 1:1 + raw.shape[1]].copy_(torch.from_numpy(raw))
    v = buf[:, 1:1 + raw.shape[1]]
    assert (v.data_ptr() // (2 * raw.itemsize)) % 2 == 1 and not v.is_contiguous()
    return v


def _survey(N, navg, fmt, max_pairs=1 << 20):
    from radiodsp_sdr_rx_amd.survey import Survey
    return Survey(NSRC, N, navg, fmt, max_pairs)


@functools.lru_cache(maxsize=None)
def _parity_case(N, fmt):
    """3 N + 77 + N / 2 pairs: the first 3 N + 77 complete two rows of navg = 2 and one frame of the third"""
    from radiodsp_sdr_rx_amd import survey
    raw = _random_rows(fmt, 3 * N + 77 + N // 2, 100 + fmt)
    model = [M.survey_rows(fmt, raw[s], N, 2, survey.window(N)) for s in range(NSRC)]
    return raw, np.stack([m[0] for m in model]), np.stack([m[1] for m in model])


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [S16, U8, S8, FL])
@pytest.mark.parametrize("N", [1024, 4096])
def test_gpu_parity_with_the_float64_model(rdsp, N, fmt):
    """navg = 2, one call of 3 N + 77 pairs: two rows, and a frame of the third, which a second call of N / 2 pairs completes
    from the partial sums and the history.  Every bin of every row within the bound of the module docstring."""
    raw, P, B = _parity_case(N, fmt)
    d = _odd_view(raw)
    sv = _survey(N, 2, fmt)
    n1 = 3 * N + 77
    assert sv.rows_for(n1) == 2
    a = sv.update(d[:, :n1])
    assert sv.rows_for(N // 2) == 1
    b = sv.update(d[:, n1:])
    got = np.concatenate([a.cpu().numpy(), b.cpu().numpy()], 1).astype(np.float64)
    assert got.shape == P.shape == (NSRC, 3, N) and np.isfinite(got).all() and P.min() >= 0 and got.max() > 0
    frac = np.abs(got - P) / B
    print(f"N = {N}, format {fmt}: worst |P^ - P| / bound = {frac.max():.4f}")
    assert frac.max() <= 1.0, (frac.max(), np.unravel_index(frac.argmax(), frac.shape))
    sv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", [S16, U8])
@pytest.mark.parametrize("N", [1024, 4096])
def test_gpu_call_split_bit_for_bit(rdsp, N, fmt):
    """navg = 4, 6 N + 91 pairs (11 frames: two rows and three frames of a third): one call against the same stream cut at
    1, H - 1, 0, H, N + 1, 777, rest -- row 0 straddles at least three calls, some complete no frame.  Rows are views at an odd
    pair offset into a longer buffer (src_stride > pairs).  rows_out is rows_for taken before the call and the model's
    schedule; the rows and, by a further call of N pairs on both objects, what the objects keep are the same bits."""
    import torch
    H = N // 2
    total = 6 * N + 91
    raw = _random_rows(fmt, total + N, 200 + fmt)
    d = _odd_view(raw)
    one, cut = _survey(N, 4, fmt), _survey(N, 4, fmt)
    whole = one.update(d[:, :total])
    assert whole.shape[1] == M.rows(N, 4, total) == 2
    parts, T = [], 0
    cuts = [1, H - 1, 0, H, N + 1, 777]
    cuts.append(total - sum(cuts))
    delivering = 0
    for pairs in cuts:
        want = cut.rows_for(pairs)
        assert want == M.rows_between(N, 4, T, pairs)
        rows = cut.update(d[:, T:T + pairs], pairs=pairs)
        assert rows.shape[1] == want
        delivering += want > 0
        parts.append(rows)
        T += pairs
    assert delivering >= 1 and M.frames(N, sum(cuts[:4])) == 1 and M.frames(N, sum(cuts[:6])) < 8
    assert torch.equal(torch.cat(parts, 1), whole)
    a, b = one.update(d[:, total:]), cut.update(d[:, total:])
    assert a.shape[1] == 1 and torch.equal(a, b)
    one.close()
    cut.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 4096])
def test_gpu_formats_bit_for_bit(rdsp, N):
    """U8 and S8 rows give the bits of S16 on the widened row, F32 rows of k / 32768 the bits of the S16 row k; F32 rows holding
    NaN, +-inf and 1e30 give finite rows within the bound of the model on src_value's values"""
    import torch
    from radiodsp_sdr_rx_amd import survey
    n = 3 * N + 5

    def run(fmt, raw, cut=N + 3):
        sv = _survey(N, 2, fmt)
        d = _odd_view(raw)
        out = torch.cat([sv.update(d[:, :cut]), sv.update(d[:, cut:])], 1)
        sv.close()
        assert out.shape[1] == 2
        return out

    for fmt in (U8, S8):
        raw = _random_rows(fmt, n, 300 + fmt)
        assert torch.equal(run(fmt, raw), run(S16, widened(fmt, raw)))
    k = _random_rows(S16, n, 310)
    assert torch.equal(run(FL, (k.astype(np.float32) / np.float32(32768.0))), run(S16, k))
    wild = _random_rows(FL, n, 311)
    at = np.random.default_rng(312).random(wild.shape) < 0.01
    wild[at] = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30], np.float32)[np.random.default_rng(313).integers(0, 5, int(at.sum()))]
    assert np.isnan(wild).any() and np.isinf(wild).any()
    got = run(FL, wild).cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    for s in range(NSRC):
        P, B = M.survey_rows(FL, wild[s], N, 2, survey.window(N))
        assert np.isfinite(P).all() and (np.abs(got[s] - P) <= B).all()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1024, 4096])
def test_gpu_sign_and_scale(rdsp, N):
    """int16 A e^{+j 2 pi k0 n / N}, A = 8000 counts, exactly on bin k0 = 37: out[N / 2 + k0] is A^2 -- within the bound of the
    model's value, which itself is within 2 A q + q^2 of A^2, q = 0.7072 (the window sums to 1 and a rounded pair is at most
    sqrt(0.5) from its value; the 0.0001 covers the float rounding of the window's sum) -- and the mirror bin N / 2 - k0 lies at
    most -90 dB below (quantisation puts about -113 dB there)"""
    from radiodsp_sdr_rx_amd import survey
    A, k0 = 8000.0, 37
    n = np.arange(2 * N)
    z = A * np.exp(2j * np.pi * k0 * n / N)
    raw = np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16)
    raw = np.stack([raw, raw[::-1].copy(), np.zeros_like(raw)])          # source 1 runs backwards: the tone at -k0
    sv = _survey(N, 2, S16)
    got = sv.update(_odd_view(raw)).cpu().numpy().astype(np.float64)
    sv.close()
    assert got.shape == (NSRC, 1, N) and not got[2].any()
    P, B = M.survey_rows(S16, raw[0], N, 2, survey.window(N))
    q = 0.7072
    assert abs(P[0, N // 2 + k0] - A * A) <= 2 * A * q + q * q
    assert abs(got[0, 0, N // 2 + k0] - P[0, N // 2 + k0]) <= B[0, N // 2 + k0]
    print(f"N = {N}: peak / A^2 - 1 = {got[0, 0, N // 2 + k0] / (A * A) - 1:.2e}, mirror {10 * np.log10(max(got[0, 0, N // 2 - k0], 1e-30) / (A * A)):.1f} dB")
    assert got[0, 0].argmax() == N // 2 + k0 and got[1, 0].argmax() == N // 2 - k0
    assert got[0, 0, N // 2 - k0] <= 1e-9 * A * A and got[1, 0, N // 2 + k0] <= 1e-9 * A * A


@pytest.mark.gpu
def test_gpu_reset_and_refusals(rdsp):
    """every refusal of create and update returns an error and leaves the object as it was: rows_for is unchanged, and the next
    valid call gives the bits of a twin that never saw the refused ones; after reset the stream reproduces a fresh object's
    bits"""
    import torch
    from radiodsp_sdr_rx_amd.survey import Survey
    lib = rdsp.load()
    N = 1024
    for args in ((0, 0, N, 2, S16, 100), (4097, 0, N, 2, S16, 100), (NSRC, 0, 2048, 2, S16, 100), (NSRC, 0, 256, 2, S16, 100),
                 (NSRC, 0, N, 3, S16, 100), (NSRC, 0, N, 0, S16, 100), (NSRC, 0, N, 512, S16, 100), (NSRC, 0, N, 2, 4, 100),
                 (NSRC, 0, N, 2, -1, 100), (NSRC, 0, N, 2, S16, 0)):
        h = C.c_void_p()
        assert lib.rdsp_survey_create(*args, C.byref(h)) == -1 and not h.value, args
        assert lib.rdsp_last_error()
    raw = _random_rows(S16, 5 * N, 400)
    d = _odd_view(raw)
    max_pairs = 3 * N
    a, b = Survey(NSRC, N, 2, S16, max_pairs), Survey(NSRC, N, 2, S16, max_pairs)
    assert (a.lib.rdsp_survey_sources(a.h), a.lib.rdsp_survey_fft_n(a.h), a.lib.rdsp_survey_navg(a.h), a.lib.rdsp_survey_format(a.h),
            a.lib.rdsp_survey_device(a.h)) == (NSRC, N, 2, S16, 0)
    first = [x.update(d[:, :N + 100]) for x in (a, b)]                  # one frame: a partial row and a history
    assert first[0].shape[1] == 0
    pairs = 2 * N                                                       # the next call completes rows
    want = a.rows_for(pairs)
    assert want == 2
    rows = torch.full((NSRC, want + 1, N), -1.0, dtype=torch.float32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = d[:, N + 100:]
    ptr, stride, out, ostride = src.data_ptr(), src.stride(0) // 2, rows.data_ptr(), rows.stride(0)
    got = C.c_int(-7)
    refused = [
        (ptr, stride, max_pairs + 1, out, 4 * N * 4, "pairs above max_pairs_per_call"),
        (ptr, pairs - 1, pairs, out, ostride, "src_stride below pairs"),
        (ptr + 2, stride, pairs, out, ostride, "source rows not aligned to a pair"),
        (0, stride, pairs, out, ostride, "no source rows"),
        (ptr, stride, pairs, out + 4, ostride, "d_rows not 16-byte aligned"),
        (ptr, stride, pairs, out, ostride + 2, "rows_stride no multiple of 4"),
        (ptr, stride, pairs, out, want * N - 4, "rows_stride below rows fft_n"),
        (ptr, stride, pairs, 0, ostride, "no d_rows for a call that completes rows"),
    ]
    for p_src, p_stride, p_pairs, p_out, p_ostride, what in refused:
        rc = a.lib.rdsp_survey_update(a.h, C.c_void_p(p_src), p_stride, p_pairs, C.c_void_p(p_out), p_ostride, C.byref(got), st)
        assert rc == -1 and got.value == -7 and a.lib.rdsp_last_error(), what
        assert a.rows_for(pairs) == want, what
    torch.cuda.synchronize()
    assert (rows == -1.0).all()
    ya, yb = a.update(src, pairs=pairs, out=rows), b.update(src, pairs=pairs)
    assert ya.shape[1] == want and ya.min() >= 0 and torch.equal(ya, yb) and (rows[:, want] == -1.0).all()
    # reset: T = 0, histories and partial rows zero
    fresh = Survey(NSRC, N, 2, S16, max_pairs)
    a.reset()
    assert a.rows_for(N) == 0 and a.rows_for(N + N // 2) == 1
    outs = [[x.update(d[:, :N + 7]), x.update(d[:, N + 7:3 * N]), x.update(d[:, 3 * N:])] for x in (a, fresh)]
    assert sum(o.shape[1] for o in outs[0]) == M.rows(N, 2, 5 * N) == 4
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    for x in (a, b, fresh):
        x.close()


@pytest.mark.gpu
def test_gpu_from_survey_to_receivers(rdsp):
    """the band of the CPU test on the GPU: find_stations on the survey's row 0 returns the three stations within half a bin,
    Engine.tune accepts them and one update_sources call on the same rows runs"""
    import oracle_lib
    import torch
    from radiodsp_sdr_rx_amd import survey
    from radiodsp_sdr_rx_amd.engine import Engine
    B = M.BAND
    raw, P, bound = _band_rows()
    d = torch.from_numpy(raw[None].copy()).cuda()
    sv = survey.Survey(1, B["N"], B["navg"], U8, len(raw))
    rows = sv.update(d)
    assert rows.shape == (1, 2, B["N"])
    row = rows[0, 0].cpu().numpy()
    assert (np.abs(row - P[0]) <= bound[0]).all()
    hz, pw = survey.find_stations(row, B["P"], B["Q"], 20.0, 1000.0, 16)
    print("stations", hz)
    _check_stations(hz)
    assert np.allclose(sv.axis_hz(B["P"], B["Q"])[[0, B["N"] // 2]], [-24000.0, 0.0])
    sv.close()
    e = Engine(3, max_blocks_per_call=8, tables=oracle_lib.engine_tables())
    e.sketch_setup()
    e.set_sources(1, [0, 0, 0])
    e.set_source_rate(B["P"], B["Q"], 1.0)
    e.set_source_format(U8)
    e.tune(0, hz)
    assert e.source_pairs(8) <= len(raw)
    y = e.update_sources(d, n_blocks=8)
    torch.cuda.synchronize()
    assert y.shape == (3, 8 * 128, 2) and y.cpu().numpy().any()
    e.close()
