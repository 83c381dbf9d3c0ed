"""rdsp_survey_t restated (include/rdsp.h has the definition): a float64 numpy evaluation that starts from the float32 values of
the source rows (engine_sources_model.values) and the library's float32 window, with the row schedule, the error bound of the
float32 kernel and the test band of the station finder; and, for the noise floor, the same definition in float32
(survey_rows_f32), a two-tone input and the rule that holds a row's floor to the float32 one's.  Plain numpy, and scipy's
complex64 transform where scipy is installed; the library is loaded where a function needs it."""
import numpy as np

from engine_sources_model import values

BH4 = (0.35875, 0.48829, 0.14128, 0.01168)


def window_formula(N):
    """the periodic 4-term Blackman-Harris window in double over its double sum (summed in tap order), rounded to float32"""
    a = 2.0 * np.pi * np.arange(N) / N
    w = BH4[0] - BH4[1] * np.cos(a) + BH4[2] * np.cos(2 * a) - BH4[3] * np.cos(3 * a)
    total = 0.0
    for v in w.tolist():
        total += v
    return (w / total).astype(np.float32)


def frames(N, T):
    return 0 if T < N else (T - N) // (N // 2) + 1


def rows(N, navg, T):
    return frames(N, T) // navg


def rows_between(N, navg, T, pairs):
    return rows(N, navg, T + pairs) - rows(N, navg, T)


def bound_E(N, x):
    """E of the bound: (12 log2 N + 2) 2^-24 sqrt(N) ||x_f||_2 -- the normwise bound of a float32 FFT whose twiddles are good to
    about 4 ulp (the plan's product chains), plus the window product's rounding"""
    return (12.0 * np.log2(N) + 2.0) * 2.0 ** -24 * np.sqrt(N) * np.sqrt(np.sum(np.abs(x) ** 2))


def survey_rows(fmt, raw, N, navg, w):
    """raw: [pairs, 2] elements of one source from a reset on; w: the library's float32 window -> (P float64 [rows, N], the
    bound [rows, N]): for every bin sum over the row's frames of 2 |X_k| E + E^2, plus navg 2^-24 sum of the frames' powers
    (the float32 adds)"""
    v = values(fmt, raw).astype(np.float64)
    x = v[:, 0] + 1j * v[:, 1]
    H = N // 2
    nrows = rows(N, navg, len(x))
    P = np.zeros((nrows, N))
    B = np.zeros((nrows, N))
    wd = w.astype(np.float64)
    for r in range(nrows):
        for f in range(r * navg, (r + 1) * navg):
            xf = wd * x[f * H:f * H + N]
            X = np.fft.fftshift(np.fft.fft(xf))
            E = bound_E(N, xf)
            P[r] += np.abs(X) ** 2
            B[r] += 2.0 * np.abs(X) * E + E * E
        B[r] += navg * 2.0 ** -24 * P[r]
        P[r] /= navg
        B[r] /= navg
    return P, B


# ---- the noise floor: a float32 reference and a two-tone input ------------------------------------------------------------------
K_STRONG = 37               # the carrier's bin; the weak tone sits on bin N / 4 + 3
FLOOR_MARGIN_DB = 12.0      # over the float32 reference's floor: the factor 4 in amplitude that twiddles good to about 4 ulp
                            # (the plan's product chains) can cost over exact ones


def two_tone(N, weak_db, frames):
    """float32 [(frames + 1) N / 2, 2] rows of format F32 (`frames` overlapping frames), no noise:
    0.5 e^{j 2 pi 37 n / N} + 0.5 10^(weak_db / 20) e^{j (2 pi (N / 4 + 3) n / N + 1)}, rounded to float32"""
    n = np.arange((frames + 1) * (N // 2), dtype=np.float64)
    z = 0.5 * np.exp(2j * np.pi * K_STRONG * n / N) + 0.5 * 10.0 ** (weak_db / 20.0) * np.exp(1j * (2.0 * np.pi * (N // 4 + 3) * n / N + 1.0))
    return np.stack([z.real, z.imag], 1).astype(np.float32)


def _fft_c64(x):
    """the forward transform of a complex64 vector in complex64: scipy's, or without scipy a radix-2 one with twiddles
    computed in float64"""
    try:
        import scipy.fft
    except ImportError:
        x = np.asarray(x, np.complex64)
        n = len(x)
        if n == 1:
            return x
        even, odd = _fft_c64(x[0::2]), _fft_c64(x[1::2])
        t = np.exp(-2j * np.pi * np.arange(n // 2) / n).astype(np.complex64) * odd
        return np.concatenate([even + t, even - t]).astype(np.complex64)
    X = scipy.fft.fft(np.asarray(x, np.complex64))
    assert X.dtype == np.complex64
    return X


def survey_rows_f32(fmt, raw, N, navg, w):
    """the definition evaluated in float32 -> float32 [rows, N]: one rounded window product per component, a complex64
    transform, |X|^2 as fmaf(re, re, im im), the frames added in ascending order from 0, times 1 / navg"""
    F = np.float32
    v = values(fmt, raw)
    w = np.asarray(w, F)
    assert v.dtype == F
    H = N // 2
    nrows = rows(N, navg, len(v))
    P = np.zeros((nrows, N), F)
    for r in range(nrows):
        acc = np.zeros(N, F)
        for f in range(r * navg, (r + 1) * navg):
            xf = np.empty(N, np.complex64)
            xf.real = w * v[f * H:f * H + N, 0]
            xf.imag = w * v[f * H:f * H + N, 1]
            X = np.fft.fftshift(_fft_c64(xf))
            re, im = X.real.astype(F), X.imag.astype(F)
            p = (re.astype(np.float64) * re + (im * im).astype(np.float64)).astype(F)     # fmaf(re, re, im * im)
            acc = (acc + p).astype(F)
        P[r] = acc * F(1.0 / navg)
    return P


def tone_indices(N, mirror=False):
    """the row indices of the carrier and the weak tone of two_tone; mirror: of the same rows run backwards"""
    s = -1 if mirror else 1
    return N // 2 + s * K_STRONG, N // 2 + s * (N // 4 + 3)


def far(N, mirror=False):
    """the mask of row indices more than 8 bins from both tones of two_tone"""
    j = np.arange(N)
    m = np.ones(N, bool)
    for c in tone_indices(N, mirror):
        d = np.abs(j - c)
        m &= np.minimum(d, N - d) > 8
    return m


def floor_db(row, N, mirror=False):
    """the largest far bin of a row of two_tone, in dB relative to the row's peak"""
    row = np.asarray(row, np.float64)
    return 10.0 * np.log10(max(row[far(N, mirror)].max(), 1e-300) / row.max())


def floor_within_margin(row, ref_row, N, mirror=False):
    """-> (ok, the row's floor, the reference row's floor): the floor of `row` is at most FLOOR_MARGIN_DB over that of the
    float32 reference's row of the same input"""
    got, ref = floor_db(row, N, mirror), floor_db(ref_row, N, mirror)
    return got <= ref + FLOOR_MARGIN_DB, got, ref


# ---- the station finder's band: U8 at 160 / 147 (48 000 Hz), three AM carriers in noise -------------------------------------
BAND = dict(P=160, Q=147, N=1024, navg=4, stations=(-17300.0, 2210.5, 9050.0), amps=(40.0, 12.0, 25.0), order=(-17300.0, 9050.0, 2210.5))


def band_u8():
    """H (2 navg + 1) pairs: carriers of 40, 12 and 25 codes with 30 % AM at 400 Hz, unit Gaussian noise per rail, rounded to
    uint8 about 127.5"""
    N, navg = BAND["N"], BAND["navg"]
    n = (N // 2) * (2 * navg + 1)
    fs = 44100.0 * BAND["P"] / BAND["Q"]
    r = np.random.default_rng(5)
    t = np.arange(n) / fs
    x = r.standard_normal(n) + 1j * r.standard_normal(n)
    for hz, a in zip(BAND["stations"], BAND["amps"]):
        x = x + a * (1.0 + 0.3 * np.cos(2 * np.pi * 400.0 * t)) * np.exp(2j * np.pi * hz * t)
    raw = np.stack([x.real, x.imag], 1)
    return np.clip(np.floor(raw + 127.5 + 0.5), 0, 255).astype(np.uint8)


def find_stations(row, N, P, Q, min_db, min_spacing_hz, max_out):
    """the finder restated in float64"""
    row = np.asarray(row, np.float32)
    db = 10.0 * np.log10(np.maximum(row.astype(np.float64), 1e-30))
    floor = np.median(db)
    bin_hz = 44100.0 * P / (Q * N)
    cand = [j for j in range(1, N - 1) if db[j] >= floor + min_db and row[j] >= row[j - 1] and row[j] > row[j + 1]]
    cand.sort(key=lambda j: (-float(row[j]), j))
    out = []
    for j in cand:
        a, b, d = db[j - 1], db[j], db[j + 1]
        den = a - 2.0 * b + d
        off = min(max(0.5 * (a - d) / den if den < 0 else 0.0, -0.5), 0.5)
        hz = (j - N // 2) * bin_hz + off * bin_hz
        if len(out) < max_out and all(abs(hz - o) >= min_spacing_hz for o in out):
            out.append(hz)
    return np.array(out)
