"""The engine's source front end restated once, for tests/test_engine_tuning.py, _ddc.py, _rate.py, _formats.py and
_sources.py: rows of any sample format at 44 100 P / Q Hz, every receiver tuned (and for P / Q > 1 low-passed and resampled by
Q / P), as csrc/rdsp_tune.h states it.  Plain numpy beside np_model.py and parity_util.py; torch and the library are imported
where a function needs them.

The product has one front end and one rate P / Q (D is P, Q = 1), and so has this module: one filter design taps_of(P, Q),
one history size keep(P, Q), one call call_rows() and one stream() for every rate.  The arithmetic of a call stays three
functions, as the header's is: the decimating pass multiplies the tap into the phasor, the polyphase pass into the sample, and
the two do not give the same bits at Q = 1 -- the engine routes Q = 1 to the decimating pass, and so does call_rows().
Below them the test signals, the library's side of the comparisons, the host program (tests/host/host_source_pass_check.cpp)
and the GPU drivers: Rx, which runs an engine through the Python wrapper and restates every receiver, and _setup / _c_call /
_stream, which make the raw C calls of the twin comparisons."""
import atexit
import ctypes as C
import functools
import math
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
M32 = (1 << 32) - 1
TUNING_OFFSET = {0: 8390.0, 1: 5390.0, 2: 7390.0, 3: 6390.0, 4: 6890.0, 5: 6890.0, 6: 5390.0}   # setDemodMode's answers
S16, U8, S8, FL = 0, 1, 2, 3
DTYPE = (np.int16, np.uint8, np.int8, np.float32)
HIST = 15          # a source at D x 44 100 Hz keeps its last 15 D pairs
BETA = 9.0


def _dc(P, Q):
    return -(-P // Q)


def _fs(P, Q):
    return (P * 44100.0) / Q                  # the operations of rate_dphi's divisor


def _pairs(P, Q, n_blocks):
    return (n_blocks * 128 * P) // Q


# ---- arithmetic -----------------------------------------------------------------------------------------------------------
def dphi_of(tuning_offset, station_hz, P=1, Q=1):
    """round((TuningOffset - station) 2^32 / (44 100 P / Q)), half away from zero, mod 2^32"""
    x = (float(F32(tuning_offset)) - float(station_hz)) * 4294967296.0 / _fs(P, Q)
    a = abs(x)
    r = math.floor(a)
    if a - r >= 0.5:
        r += 1
    return (r if x >= 0 else -r) & M32


def fmaf(a, b, c):
    """float32 fused multiply-add, exact: a b is exact in double; the double sum's rounding error (TwoSum) decides the
    one case where rounding that sum to float32 differs from rounding the exact value -- the sum landing on a midpoint"""
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    p = a.astype(np.float64) * b.astype(np.float64)
    cd = c.astype(np.float64)
    s = p + cd
    bv = s - p
    err = (p - (s - bv)) + (cd - bv)
    r = s.astype(F32)
    rd = r.astype(np.float64)
    other = np.where(s > rd, np.nextafter(r, F32(np.inf)), np.nextafter(r, F32(-np.inf)))
    od = other.astype(np.float64)
    tie = (s != rd) & ((rd + od) * 0.5 == s) & (err != 0)
    return np.where(tie & (np.sign(err) == np.sign(od - rd)), other, r)


def fma32(a, b, c):
    """fmaf, with a short cut: a b is exact in double, so rounding the double sum a b + c to float32 differs from rounding
    the exact sum only if the double sum sits on a midpoint between two float32 (the low 29 bits of its mantissa are
    1 << 28) -- no such element, no double rounding, and the 6-operation path is fmaf's answer.  That places the midpoints
    of normal float32 only: below 2^-126 float32's spacing stays 2^-149 and its midpoints sit at other bits of the double.
    So whenever a double sum is non-zero and below 2^-125 in magnitude the call is fmaf's as well, which is exact there too
    (tests/test_channelizer.py holds both to rational arithmetic).  A double sum of exactly 0 is exact -- a b + c of float32
    cannot underflow in double -- and takes the short cut: fresh histories are all zeros."""
    a, b, c = (np.asarray(v, F32) for v in (a, b, c))
    s = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    mag = np.abs(s)
    if np.any((s.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)) or np.any((mag < 2.0 ** -125) & (mag > 0.0)):
        return fmaf(a, b, c)
    return s.astype(F32)


def phasor(tab, ph):
    """(cos, sin) of 2 pi ph / 2^32 by the table, ph of any shape"""
    ph = np.asarray(ph, np.uint32)
    t = tab[(ph >> 22).astype(np.int64)]
    f = (ph & 0x3FFFFF).astype(F32) * F32(2.0 ** -22)
    return fmaf(f, t[..., 2], t[..., 0]), fmaf(f, t[..., 3], t[..., 1])


def values(fmt, raw):
    """the table of include/rdsp.h: what a row's elements are worth, float32 counts on the int16 scale"""
    raw = np.asarray(raw)
    assert raw.dtype == DTYPE[fmt]
    if fmt == U8:
        return (2 * raw.astype(np.int32) - 255).astype(F32) * F32(128.0)
    if fmt == S8:
        return raw.astype(F32) * F32(256.0)
    if fmt == FL:
        with np.errstate(invalid="ignore"):
            return np.where(np.isnan(raw), F32(0.0), np.minimum(np.maximum(raw, F32(-256.0)), F32(256.0)) * F32(32768.0)).astype(F32)
    return raw.astype(F32)


def widened(fmt, raw):
    """an 8-bit row as the int16 row of the same values (every one is an exact int16)"""
    v = values(fmt, raw)
    assert np.all(v == np.rint(v)) and v.min() >= -32768 and v.max() <= 32767
    return v.astype(np.int16)


def _sat16(v):
    return np.clip(np.rint(v), -32768, 32767).astype(np.int16)


# ---- filter design and schedule -------------------------------------------------------------------------------------------
def sin_halfpi(q, D):
    """sin(pi q / (2 D)), q >= 0 integers: rdsp_tune.h's ddc_sin_halfpi in numpy -- the same operations in the same order"""
    r = q % (4 * D)
    sign = np.where(r >= 2 * D, -1.0, 1.0)
    r = np.where(r >= 2 * D, r - 2 * D, r)
    r = np.where(r > D, 2 * D - r, r)
    a = (3.141592653589793 * r.astype(np.float64)) / (2.0 * float(D))
    a2 = a * a
    term, total = a.copy(), a.copy()
    for n in range(1, 15):
        term = -(term * a2) / float((2 * n) * (2 * n + 1))
        total = total + term
    return sign * total


def i0(x):
    y = np.asarray(x, np.float64) / 2.0
    term, total = np.ones_like(y), np.ones_like(y)
    for n in range(1, 41):
        t = y / float(n)
        term = term * (t * t)
        total = total + term
    return total


def taps_of(P, Q=1, gain=1.0):
    """the specified prototype: a sinc with its cutoff at 22 050 Hz under a Kaiser window (beta 9) at the rate 44 100 P,
    Tp = 16 ceil(P / Q) Q taps (16 D at an integer rate), sum 1 (summed in tap order), times Q gain, rounded to float32"""
    Tp = 16 * _dc(P, Q) * Q
    q = np.abs(2 * np.arange(Tp) - (Tp - 1))
    u = (3.141592653589793 * q.astype(np.float64)) / (2.0 * float(P))
    rho = q.astype(np.float64) / float(Tp - 1)
    h = (sin_halfpi(q, P) / u) * (i0(BETA * np.sqrt(1.0 - rho * rho)) / i0(BETA))
    total = 0.0
    for v in h.tolist():
        total += v
    return ((h / total) * (float(Q) * float(gain))).astype(F32)


def receiver_taps(h, dphi, tab):
    """the decimating pass's g[r][k] = (h_k c, h_k s), (c, s) the table's phasor at -k dphi[r]"""
    k = np.arange(len(h), dtype=np.uint64)
    ph = ((np.uint64(1 << 32) - ((k[None, :] * np.asarray(dphi, np.uint64)[:, None]) & np.uint64(M32))) & np.uint64(M32)).astype(np.uint32)
    c, s = phasor(tab, ph)
    return h[None, :] * c, h[None, :] * s


def schedule(P, Q, m0, n_out):
    """outputs m0 ... m0 + n_out - 1 since the reset: (frac, pairs, n local to the call, r)"""
    S = (m0 * P) // Q
    t = [(m0 * P) % Q + (i + 1) * P for i in range(n_out)]
    return (m0 * P) % Q, ((m0 + n_out) * P) // Q - S, np.array([v // Q - 1 for v in t], np.int64), np.array([v % Q for v in t], np.int64)


def keep(P, Q):
    """the pairs a source keeps between calls: rdsp_tune.h's rate_keep"""
    return 0 if (P, Q) == (1, 1) else HIST * P if Q == 1 else 16 * _dc(P, Q)


# ---- one call: the three passes -------------------------------------------------------------------------------------------
def tune_pairs(iq, ph, tab):
    """[n, 2] pairs (int16 or values) times e^{+j 2 pi ph / 2^32}: I' = fmaf(I, c, -(Q s)), Q' = fmaf(Q, c, I s), rne, saturate"""
    c, s = phasor(tab, ph)
    i, q = iq[:, 0].astype(F32), iq[:, 1].astype(F32)
    return np.stack([_sat16(fmaf(i, c, -(q * s))), _sat16(fmaf(q, c, i * s))], 1)


def ddc_rows(xh, D, h, dphi, ph0, tab):
    """one call of receivers that share a source at D x 44 100 Hz.  xh: [15 D + n_out D, 2], the row with the source's
    history in front; dphi, ph0: the receivers' steps and phases -> int16 [R, n_out, 2].  Per component ONE chain over k
    ascending: re = fmaf(gx, xi, re); re = fmaf(-gy, xq, re); im = fmaf(gx, xq, im); im = fmaf(gy, xi, im); then tune_pair's
    rotation"""
    T = 16 * D
    n_out = (len(xh) - HIST * D) // D
    dphi, ph0 = np.asarray(dphi, np.uint64), np.asarray(ph0, np.uint64)
    gx, gy = receiver_taps(h, dphi, tab)
    xi, xq = xh[:, 0].astype(F32), xh[:, 1].astype(F32)
    re = np.zeros((len(dphi), n_out), F32)
    im = np.zeros((len(dphi), n_out), F32)
    for k in range(T):
        a, b = xi[T - 1 - k::D][None, :n_out], xq[T - 1 - k::D][None, :n_out]
        re = fma32(gx[:, k:k + 1], a, re)
        re = fma32(-gy[:, k:k + 1], b, re)
        im = fma32(gx[:, k:k + 1], b, im)
        im = fma32(gy[:, k:k + 1], a, im)
    ph = ((ph0[:, None] + np.arange(n_out, dtype=np.uint64)[None, :] * ((dphi * np.uint64(D)) & np.uint64(M32))[:, None]) & np.uint64(M32)).astype(np.uint32)
    c, s = phasor(tab, ph)
    return np.stack([_sat16(fmaf(re, c, -(im * s))), _sat16(fmaf(im, c, re * s))], -1)


def rate_rows(xh, P, Q, frac, h, dphi, ph0, tab, n_out):
    """one call of receivers that share a source at 44 100 P / Q Hz.  xh: [Tb + pairs, 2], the row with the source's last Tb
    pairs in front; h: the prototype; dphi, ph0: the receivers' steps and phases -> int16 [R, n_out, 2].  u_j = h[j Q + r(i)]
    x[n(i) - j] (two rounded products), e_j the table's phasor at -j dphi; per component ONE chain over j ascending: re =
    fmaf(ex, ux, re); re = fmaf(-ey, uy, re); im = fmaf(ex, uy, im); im = fmaf(ey, ux, im); then tune_pair's rotation at ph0 +
    (n + 1 - Dc) dphi"""
    Dc = _dc(P, Q)
    Tb = 16 * Dc
    t = frac + (np.arange(n_out, dtype=np.int64) + 1) * P
    n, r = t // Q - 1, t % Q
    assert n[0] >= 0 and n[-1] + 1 + Tb == len(xh)
    dphi, ph0 = np.asarray(dphi, np.uint64), np.asarray(ph0, np.uint64)
    xi, xq = xh[:, 0].astype(F32), xh[:, 1].astype(F32)
    re = np.zeros((len(dphi), n_out), F32)
    im = np.zeros((len(dphi), n_out), F32)
    for j in range(Tb):
        ph = ((np.uint64(1 << 32) - ((np.uint64(j) * dphi) & np.uint64(M32))) & np.uint64(M32)).astype(np.uint32)
        ex, ey = phasor(tab, ph)
        ex, ey = ex[:, None], ey[:, None]
        hj = h[j * Q + r]
        ux, uy = (hj * xi[Tb + n - j])[None, :], (hj * xq[Tb + n - j])[None, :]
        re = fma32(ex, ux, re)
        re = fma32(-ey, uy, re)
        im = fma32(ex, uy, im)
        im = fma32(ey, ux, im)
    k = ((n + 1 - Dc) % (1 << 32)).astype(np.uint64)
    ph = ((ph0[:, None] + k[None, :] * dphi[:, None]) & np.uint64(M32)).astype(np.uint32)
    c, s = phasor(tab, ph)
    return np.stack([_sat16(fmaf(re, c, -(im * s))), _sat16(fmaf(im, c, re * s))], -1)


# ---- any rate -------------------------------------------------------------------------------------------------------------
def call_rows(xh, P, Q, frac, h, dphi, ph0, tab, n_out):
    """one call of receivers that share a source, by the pass the engine takes at P / Q: xh the VALUES (or int16) with the
    keep(P, Q) pairs before the call in front, h the prototype (none at 44 100 Hz) -> int16 [R, n_out, 2]"""
    if (P, Q) == (1, 1):
        t = np.arange(n_out, dtype=np.uint64)
        return np.stack([tune_pairs(xh, ((np.uint64(p) + t * np.uint64(d)) & np.uint64(M32)).astype(np.uint32), tab) for d, p in zip(dphi, ph0)])
    if Q == 1:
        return ddc_rows(xh, P, h, dphi, ph0, tab)
    return rate_rows(xh, P, Q, frac, h, dphi, ph0, tab, n_out)


def stream(src_row, P, Q, h, steps, tab, cuts=None):
    """receivers of one source over a stream from a reset: src_row int16 or values; steps uint32-valued [R, n_blocks], the
    step of each receiver in each block.  The stream is cut where a step changes and at `cuts` (blocks); frac, history and
    phases are carried -> (int16 [R, n, 2], phases after)"""
    steps = np.asarray(steps, np.uint64)
    R, nb = steps.shape
    marks = sorted({0, nb} | {b for b in range(1, nb) if np.any(steps[:, b] != steps[:, b - 1])} | set(cuts or ()))
    kp = keep(P, Q)
    x = np.concatenate([np.zeros((kp, 2), src_row.dtype), src_row])
    ph = np.zeros(R, np.uint64)
    out = []
    for a, b in zip(marks[:-1], marks[1:]):
        S = (a * 128 * P) // Q
        frac, pairs = (a * 128 * P) % Q, (b * 128 * P) // Q - S
        out.append(call_rows(x[S:S + kp + pairs], P, Q, frac, h, steps[:, a], ph, tab, (b - a) * 128))
        ph = (ph + np.uint64(pairs) * steps[:, a]) & np.uint64(M32)
    return np.concatenate(out, 1), ph


def tuned_row(src, dphi_blocks, tab):
    """a receiver's row at 44 100 Hz: block b of its source row at the step dphi_blocks[b], the phase continuous from 0"""
    return stream(src, 1, 1, None, [dphi_blocks], tab)[0][0]


# ---- test signals ---------------------------------------------------------------------------------------------------------
def _band(seed, n_sources, n_blocks):
    """int16 [n_sources, n, 2] at 44 100 Hz: in each, a dozen carriers and tones anywhere in the band, some keyed, and noise"""
    r = np.random.default_rng(seed)
    t = np.arange(n_blocks * 128)
    out = np.zeros((n_sources, len(t), 2), np.int16)
    for s in range(n_sources):
        z = np.zeros(len(t), np.complex128)
        for _ in range(12):
            f = r.uniform(-21000, 21000)
            env = 1 + 0.5 * np.sin(2 * np.pi * r.uniform(100, 800) / 44100.0 * t) if r.random() < 0.5 else (np.sin(2 * np.pi * r.uniform(2, 9) / 44100.0 * t) > 0)
            z += r.uniform(0.01, 0.12) * env * np.exp(2j * np.pi * f / 44100.0 * t + 1j * r.uniform(0, 6))
        z += 0.02 * (r.standard_normal(len(t)) + 1j * r.standard_normal(len(t)))
        out[s, :, 0] = np.clip(np.round(z.real * 32767), -32768, 32767)
        out[s, :, 1] = np.clip(np.round(z.imag * 32767), -32768, 32767)
    out[0, :64] = [[-32768, 32767], [32767, -32768]] * 32                               # full-scale pairs: saturation
    return out


def _tone(f, n, fs, amp, phase=0.0):
    return amp * np.exp(2j * np.pi * (f / fs) * np.arange(n) + 1j * phase)


def _int16(z):
    return np.stack([np.clip(np.round(z.real), -32768, 32767), np.clip(np.round(z.imag), -32768, 32767)], -1).astype(np.int16)


def wide(seed, n_sources, n_blocks, P, Q=1, level=0.05):
    """int16 [n_sources, floor(n_blocks 128 P / Q), 2] at 44 100 P / Q Hz: in each, twenty carriers anywhere in the band, half
    of them modulated or keyed, and noise; source 0 starts with full-scale pairs (saturation behind a gain above 1)"""
    r = np.random.default_rng(seed)
    fs, n, Dc = _fs(P, Q), _pairs(P, Q, n_blocks), _dc(P, Q)
    t = np.arange(n)
    out = np.zeros((n_sources, n, 2), np.int16)
    for s in range(n_sources):
        z = np.zeros(n, np.complex128)
        for _ in range(20):
            f = r.uniform(-0.49, 0.49) * fs
            env = 1 + 0.5 * np.sin(2 * np.pi * r.uniform(100, 800) / fs * t) if r.random() < 0.5 else (np.sin(2 * np.pi * r.uniform(2, 9) / fs * t) > 0)
            z += r.uniform(0.2, 1.0) * level * env * np.exp(2j * np.pi * f / fs * t + 1j * r.uniform(0, 6))
        z += 0.3 * level * (r.standard_normal(n) + 1j * r.standard_normal(n))
        out[s] = _int16(z * 32767)
    out[0, :32 * Dc] = np.repeat(np.array([[-32768, 32767], [32767, -32768], [32767, 32767], [-32768, -32768]], np.int16), 8 * Dc, 0)
    return out


def _to_u8(x):
    return np.clip(np.rint(x.astype(np.float64) / 256.0 + 127.5), 0, 255).astype(np.uint8)


def _to_s8(x):
    return np.clip(np.rint(x.astype(np.float64) / 256.0), -128, 127).astype(np.int8)


def _raw_of(fmt, x, seed=0):
    """a row of format fmt from an int16 band x: 8-bit by its high byte; float as k / 32768 (seed 0) or with a drawn fraction
    of a count added (random non-integer values)"""
    if fmt == U8:
        return _to_u8(x)
    if fmt == S8:
        return _to_s8(x)
    if fmt == FL:
        j = np.random.default_rng(seed).uniform(-0.5, 0.5, x.shape) if seed else 0.0
        return ((x.astype(np.float64) + j) / 32768.0).astype(F32)
    return x


def _stations(seed, n, P, Q):
    lim = (22050.0 * P) / Q
    st = np.random.default_rng(seed).uniform(-lim + 1, lim - 1, n)
    st[:2] = [lim - 0.5, 0.0]
    return st


def _dphis(stations, P, Q):
    return np.array([dphi_of(TUNING_OFFSET[0], s, P, Q) for s in stations], np.uint64)


def _phasor_modulus_error(tab):
    """what the exact-arithmetic bounds stand on: |table phasor - e^{j phi}| as a complex MODULUS (the chord's error is
    radial, (2 pi / 1024)^2 / 8 = 4.7e-6, plus the roundings of the table and of the fmaf): the worst of a million drawn
    phases, the neighbours of every table entry and every entry's midpoint"""
    r = np.random.default_rng(1)
    k = np.arange(1024, dtype=np.uint64) << np.uint64(22)
    ph = np.concatenate([r.integers(0, 1 << 32, 1000000, dtype=np.uint64), k, (k + np.uint64(1)) & np.uint64(M32), (k - np.uint64(1)) & np.uint64(M32), k + np.uint64(1 << 21)]).astype(np.uint32)
    c, s = phasor(tab, ph)
    a = 2 * np.pi * ph.astype(np.float64) / 4294967296.0
    return np.hypot(c - np.cos(a), s - np.sin(a)).max()


# ---- the library's side ---------------------------------------------------------------------------------------------------
def engine(n_channels, max_blocks):
    from radiodsp_sdr_rx_amd.engine import Engine
    import oracle_lib
    return Engine(n_channels, max_blocks_per_call=max_blocks, tables=oracle_lib.engine_tables())


def lib_taps(P, Q=1, gain=1.0):
    """the library's prototype: rdsp_engine_ddc_taps at an integer rate, rdsp_engine_rate_taps at a rational one, none at
    44 100 Hz"""
    from radiodsp_sdr_rx_amd.engine import ddc_taps, rate_taps
    return None if (P, Q) == (1, 1) else ddc_taps(P, gain) if Q == 1 else rate_taps(P, Q, gain)


def table(rdsp):
    return np.ctypeslib.as_array(rdsp.load().rdsp_engine_tune_table(), (1024, 4)).copy()


# ---- rdsp_tune.h on the host ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def host_program():
    """tests/host/host_source_pass_check.cpp compiled as the kernels are (-ffp-contract=off), once per process -> its path"""
    d = tempfile.mkdtemp(prefix="host_source_pass_check")
    atexit.register(shutil.rmtree, d, ignore_errors=True)
    exe = os.path.join(d, "host_source_pass_check")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-I",
                           os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"), os.path.join(HERE, "host", "host_source_pass_check.cpp"),
                           "-o", exe])
    return exe


def host_rows(exe, d, fmt, raw, hist_vals, P, Q, frac, gain, dphi, ph0, n_out, to=(), stations=()):
    """`exe rows` (exe: host_program()) in the directory d: the call's pairs `raw` in their own format, the VALUES of the
    keep(P, Q) pairs before it, the receivers' steps and phases -> words [R, n_out] of tune_pair, ddc_output or rate_output.
    The program leaves taps.bin, g.bin (decimating pass), sched.bin (polyphase pass) and dphi.bin (the steps of the tuning
    offsets `to` at `stations`) in d"""
    kind = 0 if (P, Q) == (1, 1) else 1 if Q == 1 else 2
    np.concatenate([[fmt, kind, P, Q, frac, n_out, len(dphi)], np.stack([dphi, ph0], 1).reshape(-1)]).astype(np.uint32).tofile(d / "params.bin")
    np.array([gain], F32).tofile(d / "gain.bin")
    np.ascontiguousarray(hist_vals, F32).tofile(d / "hist.bin")
    np.ascontiguousarray(raw, DTYPE[fmt]).tofile(d / "src.bin")
    np.asarray(to, F32).tofile(d / "to.bin")
    np.asarray(stations, np.float64).tofile(d / "station.bin")
    out = subprocess.run([exe, "rows", str(d)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return np.fromfile(d / "out.bin", np.uint32).reshape(len(dphi), n_out)


# ---- GPU: an engine through the Python wrapper, every receiver restated ---------------------------------------------------
class Rx:
    """an engine on shared sources at 44 100 P / Q Hz, and what the CPU needs to restate each receiver: per block the step
    its group's mode and its station gave it (per source sample), and the setter calls that reached it (as OracleEngine.run
    takes them).  The engine has had sketch_setup(): every group starts in LSB.  The rate is set between set_sources and the
    first tune: by set_source_decimation at an integer rate, by set_source_rate at a rational one, by nothing at 44 100 Hz
    (the default configuration).  At an integer rate a call takes a contiguous copy of its pairs; at a rational one
    source_pairs(n_blocks) pairs of every row from where the last call stopped -- a view into the one long device buffer, no
    copy; with odd, every call's rows start at an odd pair offset of a second long buffer (4-byte alignment only)."""

    def __init__(self, eng, src, source_of, firsts, stations, P=1, Q=1, gain=None, odd=False):
        import torch
        self.eng, self.src, self.n, self.P, self.Q, self.gain, self.odd = eng, src, eng.n_channels, P, Q, gain, odd
        self.source_of = [int(s) for s in source_of]
        eng.set_sources(src.shape[0], self.source_of)
        if Q > 1:
            eng.set_source_rate(P, Q, gain)
            assert eng.source_rate() == (P, Q) and eng.source_decimation() == 0
        elif P > 1:
            eng.set_source_decimation(P, gain)
            assert eng.source_decimation() == P
        else:
            assert gain is None
        self.firsts, self.modes = [0], [0]
        self.set_groups(firsts)
        self.station = np.zeros(self.n)
        self.tune(0, stations)
        self.calls = [[] for _ in range(self.n)]
        self.steps = [[] for _ in range(self.n)]
        self.d = torch.from_numpy(src).cuda()
        self.long = torch.zeros((src.shape[0], src.shape[1] + 2 * 128 + 64, 2), dtype=torch.int16, device="cuda") if odd else None
        self.at = 1                                          # where the next call's rows start in self.long
        self.nb = (src.shape[1] * Q + Q - 1) // (128 * P)    # whole blocks the source rows hold
        self.outs = []
        self.tab = eng.tune_table()
        self.h = lib_taps(P, Q, gain)
        self.rows = {}

    def group_of(self, c):
        return max(g for g, f in enumerate(self.firsts) if f <= c)

    def set_groups(self, firsts):
        self.modes = [self.modes[self.group_of(f)] for f in firsts]
        self.eng.set_groups(firsts)
        self.firsts = list(firsts)

    def tune(self, first, stations):
        self.eng.tune(first, stations)
        self.station[first:first + len(stations)] = stations

    def call(self, block, group, name, *args):
        self.eng.select_group(group)
        getattr(self.eng, name)(*args)
        self.eng.select_group(-1)
        groups = range(len(self.firsts)) if group < 0 else [group]
        for g in groups:
            if name == "setDemodMode" and args[0] in TUNING_OFFSET:
                self.modes[g] = args[0]
            for c in range(self.firsts[g], (self.firsts + [self.n])[g + 1]):
                self.calls[c].append([block, name] + list(args))

    def run(self, a, b, split):
        P, Q = self.P, self.Q
        a, b = min(a, self.nb), min(b, self.nb)              # a script written for more blocks than the source has
        for u in range(a, b, split):
            v = min(b, u + split)
            for c in range(self.n):
                self.steps[c] += [dphi_of(TUNING_OFFSET[self.modes[self.group_of(c)]], self.station[c], P, Q)] * (v - u)
            S, pairs = _pairs(P, Q, u), _pairs(P, Q, v) - _pairs(P, Q, u)
            rows = self.d[:, S:S + pairs]
            if Q == 1:
                self.outs.append(self.eng.update_sources(rows.contiguous()))
                continue
            assert self.eng.source_pairs(v - u) == pairs
            if self.odd:
                self.long[:, self.at:self.at + pairs].copy_(rows)
                rows = self.long[:, self.at:self.at + pairs]
                assert (rows.data_ptr() // 4) % 2 == 1 and not rows.is_contiguous()
                self.at += pairs
                self.at += (self.at + 1) % 2               # odd again
            self.outs.append(self.eng.update_sources(rows, n_blocks=v - u))

    def result(self):
        import torch
        y = torch.cat(self.outs, 1).cpu().numpy()
        assert np.array_equal(y[..., 0], y[..., 1])
        return y[..., 0]

    def restate(self, channels):
        """the tuned rows of `channels`, all receivers of a source at once; a row restated once stays"""
        for s in sorted({self.source_of[c] for c in channels}):
            cs = [c for c in channels if self.source_of[c] == s and c not in self.rows]
            if cs:
                y, _ = stream(self.src[s], self.P, self.Q, self.h, np.array([self.steps[c] for c in cs], np.uint64), self.tab)
                self.rows.update(zip(cs, y))

    def want(self, c):
        import oracle_lib
        self.restate([c])
        return oracle_lib.OracleEngine().run(self.rows[c], self.calls[c])

    def check(self, y, channels=None):
        channels = list(range(self.n) if channels is None else channels)
        self.restate(channels)
        for c in channels:
            w = self.want(c)
            assert np.array_equal(y[c], w), (c, int(np.argmax(y[c] != w)))


def _script_97(R, split, nb):
    """five groups in LSB, USB, CW, AM, SAM; at block 13 a third of the receivers retune; at block 20 the groups are cut
    anew into six and every group's mode is set again; at block 27 two groups change mode and one its audio filter"""
    r = np.random.default_rng(77)
    lim = (float(R.P) / R.Q) * 22050.0
    for g, m in enumerate([0, 1, 2, 4, 5]):
        R.call(0, g, "setDemodMode", m)
    R.run(0, 13, split)
    R.tune(5, r.uniform(-lim + 1, lim - 1, 32))
    R.run(13, 20, split)
    R.set_groups([0, 11, 40, 58, 70, 90])
    for g, m in enumerate([0, 1, 2, 4, 5, 3]):              # channels 11-18 go from LSB to USB, 70-76 from AM to SAM, 90-96 to CW
        R.call(20, g, "setDemodMode", m)
    R.run(20, 27, split)
    R.call(27, 2, "setDemodMode", 3)
    R.call(27, 4, "setDemodMode", 1)
    R.call(27, 1, "setAudioFilter", 3)
    R.run(27, nb, split)


# ---- GPU: the C entries themselves, for the twin comparisons --------------------------------------------------------------
def _setup(nch, n_sources, source_of, P, Q, gain, stations, fmt, max_blocks=8):
    e = engine(nch, max_blocks)
    e.sketch_setup()
    e.set_sources(n_sources, source_of)
    if (P, Q) != (1, 1):
        e.set_source_rate(P, Q, gain)
    if fmt != S16:
        e.set_source_format(fmt)
    assert e.source_format() == fmt
    e.tune(0, stations)
    return e


def _c_call(e, rows, nb, out, entry="rdsp_engine_update_source_samples", stride=None, ptr=None):
    """the C entry itself: rows a device tensor [n_sources, pairs, 2], contiguous or a view into a longer buffer"""
    import torch
    if stride is None:
        stride = rows.stride(0) // 2 if rows.shape[0] > 1 else rows.shape[1]
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    return getattr(e.lib, entry)(e.h, rows.data_ptr() if ptr is None else ptr, stride, nb, out.data_ptr(), out.shape[1], s)


def _stream(e, d, P, Q, a, b, split, entry="rdsp_engine_update_source_samples", odd=False):
    """blocks a ... b of the device rows d in calls of `split`: the calls walk through d from pair e.pos_pairs on; integer
    rates take contiguous 16-byte aligned copies, rational ones views -- with `odd`, views at odd pair offsets of a second
    long buffer.  -> the audio of every call, on the host"""
    import torch
    outs = []
    long = torch.zeros((d.shape[0], d.shape[1] + 4 * (b - a) + 8, 2), dtype=d.dtype, device="cuda") if odd else None
    at = 1
    S = e.pos_pairs
    for u in range(a, b, split):
        v = min(b, u + split)
        pairs = e.source_pairs(v - u)
        rows = d[:, S:S + pairs]
        assert rows.shape[1] == pairs
        if Q == 1:
            rows = rows.contiguous()
        elif odd:
            long[:, at:at + pairs].copy_(rows)
            rows = long[:, at:at + pairs]
            assert (rows.data_ptr() // (2 * d.element_size())) % 2 == 1 and not rows.is_contiguous()
            at += pairs
            at += (at + 1) % 2
        out = torch.empty((e.n_channels, (v - u) * 128, 2), dtype=torch.int16, device="cuda")
        assert _c_call(e, rows, v - u, out, entry) == 0, e.lib.rdsp_last_error()
        outs.append(out.cpu().numpy())
        S += pairs
    e.pos_pairs = S
    return outs
