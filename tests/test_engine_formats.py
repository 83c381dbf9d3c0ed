"""rdsp_engine_t on source rows of uint8, int8 and float32 IQ, read in place (rdsp_engine_set_source_format /
rdsp_engine_update_source_samples, include/rdsp.h; the value of a sample is csrc/rdsp_tune.h's src_value, everything after it
the arithmetic of the three passes as it was), and rdsp_iq_reader_t on recordings in those formats (csrc/rdsp_io.c).

`-m "not gpu"`: the value table, exactly; each pass under the header's arithmetic compiled on the host
(tests/host/host_source_pass_check.cpp): an 8-bit row gives the bits of the int16 pass on the widened row, a float row of
k / 32768 the bits of the int16 row k, a random float row the bits of the numpy restatement (tests/engine_sources_model.py:
values(), then the chains of the three passes, which take values as they take int16) and stays within the project's bound of a
float64 evaluation of the definition; the readers.
`-m gpu`: 8-bit and k / 32768 rows against an int16 twin bit for bit, call by call, state blobs included; random float rows
against rdsp_engine_update on the restated rows; the format as a setting; the refusals; the Python wrapper."""
import os
import struct
import subprocess

import numpy as np
import pytest

import engine_sources_model as model
from engine_sources_model import (DTYPE, F32, FL, HERE, M32, ROOT, S8, S16, U8, _c_call, _dc, _dphis, _pairs, _phasor_modulus_error, _raw_of,
                                  _setup, _stations, _stream, _to_u8, call_rows, engine, host_program, host_rows, lib_taps, schedule, stream,
                                  table, values, wide, widened)
S16, U8, S8, FL = 0, 1, 2, 3
DTYPE = (np.int16, np.uint8, np.int8, np.float32)
CPU_RATES = [(1, 1), (3, 1), (3, 2), (160, 147)]
GPU_RATES = [(1, 1), (2, 1), (30, 1), (48, 1), (3, 2), (160, 147), (17, 2)]


def _restate(vals, P, Q, gain, dphi, nb, tab, cuts=None):
    """receivers of one source over a stream of nb blocks from a reset, at constant steps: the tuned rows [R, nb 128, 2]"""
    return stream(vals, P, Q, lib_taps(P, Q, gain), np.repeat(np.asarray(dphi, np.uint64)[:, None], nb, 1), tab, cuts)[0]


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check():
    return host_program()


def _words(rows):
    return np.ascontiguousarray(rows).view(np.uint32)[..., 0]


def _case(P, Q, seed, n_out=256, n_rx=6):
    """a call 37 outputs into a stream (frac not 0 at a rational rate): int16 band with the history in front, steps, phases"""
    r = np.random.default_rng(seed)
    frac, pairs, _, _ = schedule(P, Q, 37, n_out)
    keep = model.keep(P, Q)
    x = r.integers(-9000, 9000, (keep + pairs, 2)).astype(np.int16)
    x[r.integers(0, len(x), 24)] = r.choice(np.array([-32768, -32767, -1, 0, 1, 32767], np.int16), (24, 2))
    dphi = _dphis(_stations(seed + 1, n_rx, P, Q), P, Q)
    ph0 = r.integers(0, 1 << 32, n_rx, dtype=np.uint64)
    ph0[0] = 0
    return frac, keep, x, dphi, ph0


def test_format_sample_value_table(host_check):
    """src_value compiled on the host: all 256 bytes under U8 ((2 u - 255) x 128) and S8 (s x 256), and the floats 0, +-1,
    +-2^-15, a denormal, 0.999 999 94, +-256, +-256.5, +-3e38, +-inf, NaN: the table's values exactly (NaN -> 0, +-2^23 beyond
    +-256), and the numpy statement of the table (engine_sources_model.values) agrees"""
    out = subprocess.run([host_check, "values"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    got = {"u8": {}, "s8": {}, "f32": {}}
    for line in out.stdout.split("\n"):
        if line:
            k, a, b = line.split()
            got[k][int(a, 16) if k == "f32" else int(a)] = struct.unpack("<f", struct.pack("<I", int(b, 16)))[0]
    assert len(got["u8"]) == 256 and len(got["s8"]) == 256 and len(got["f32"]) == 16
    for u in range(256):
        assert got["u8"][u] == (2 * u - 255) * 128.0 and got["s8"][u] == (u - 256 if u > 127 else u) * 256.0, u
    assert got["u8"][0] == -32640.0 and got["u8"][255] == 32640.0 and got["u8"][127] == -got["u8"][128] == -128.0
    bits = lambda v: struct.unpack("<I", struct.pack("<f", v))[0]
    inf = float("inf")
    want = {0.0: 0.0, 1.0: 32768.0, -1.0: -32768.0, 2.0 ** -15: 1.0, -2.0 ** -15: -1.0, 2.0 ** -140: 2.0 ** -125, 0.99999994: 32767.998046875,
            256.0: 2.0 ** 23, -256.0: -2.0 ** 23, 256.5: 2.0 ** 23, -256.5: -2.0 ** 23, 3e38: 2.0 ** 23, -3e38: -2.0 ** 23, inf: 2.0 ** 23,
            -inf: -2.0 ** 23}
    for x, v in want.items():
        assert got["f32"][bits(x)] == v and bits(got["f32"][bits(x)]) == bits(v), (x, got["f32"][bits(x)])
    assert got["f32"][0x7FC00000] == 0.0
    assert np.array_equal(values(U8, np.arange(256, dtype=np.uint8)), np.array([got["u8"][u] for u in range(256)], F32))
    assert np.array_equal(values(S8, np.arange(256, dtype=np.uint8).view(np.int8)), np.array([got["s8"][u] for u in range(256)], F32))
    fl = np.array(list(want) + [float("nan")], F32)
    assert np.array_equal(values(FL, fl), np.array([got["f32"][int(b)] for b in fl.view(np.uint32)], F32))


@pytest.mark.parametrize("P,Q", CPU_RATES)
@pytest.mark.parametrize("fmt", [U8, S8])
def test_format_8bit_row_is_the_int16_pass_on_the_widened_row(host_check, tmp_path, rdsp, fmt, P, Q):
    """the header's arithmetic on the host, 256 outputs of 6 receivers from drawn phases, 37 outputs into a stream, with a
    history: the 8-bit row's words are the int16 pass's words on the widened row, and the numpy restatement's on the values"""
    frac, keep, x, dphi, ph0 = _case(P, Q, 10 * fmt + P)
    raw = _raw_of(fmt, x * 3)
    raw[:4] = [[0, 255], [255, 0], [128, 127], [1, 254]] if fmt == U8 else [[-128, 127], [127, -128], [0, -1], [1, -127]]
    v, w = values(fmt, raw), widened(fmt, raw)
    tab = table(rdsp)
    got = host_rows(host_check, tmp_path, fmt, raw[keep:], v[:keep], P, Q, frac, 2.0, dphi, ph0, 256)
    twin = host_rows(host_check, tmp_path, S16, w[keep:], v[:keep], P, Q, frac, 2.0, dphi, ph0, 256)
    assert got.any() and np.array_equal(got, twin)
    assert np.array_equal(got, _words(call_rows(v, P, Q, frac, lib_taps(P, Q, 2.0), dphi, ph0, tab, 256)))
    assert np.array_equal(got, _words(call_rows(w, P, Q, frac, lib_taps(P, Q, 2.0), dphi, ph0, tab, 256)))


@pytest.mark.parametrize("P,Q", CPU_RATES)
def test_format_float_rows_of_integers_are_the_int16_rows(host_check, tmp_path, P, Q):
    """a float row of k / 32768 gives the bits of the int16 row k (+-32767, -32768, 0, +-1 among them)"""
    frac, keep, x, dphi, ph0 = _case(P, Q, 50 + P)
    raw = _raw_of(FL, x)
    assert np.array_equal(values(FL, raw), x.astype(F32))
    got = host_rows(host_check, tmp_path, FL, raw[keep:], x[:keep], P, Q, frac, 2.0, dphi, ph0, 256)
    twin = host_rows(host_check, tmp_path, S16, x[keep:], x[:keep], P, Q, frac, 2.0, dphi, ph0, 256)
    assert got.any() and np.array_equal(got, twin)


@pytest.mark.parametrize("P,Q", CPU_RATES)
def test_format_random_float_rows_against_the_restatement_and_exact_arithmetic(host_check, tmp_path, rdsp, P, Q):
    """rows of random non-integer values at +-0.05 of full scale.  (a) the header's arithmetic on the host is the numpy
    restatement bit for bit.  (b) the restated rows against a float64 evaluation of the definition, every sample of both
    components, within the project's bound |diff| <= 0.5 + A (2 x 2^-17 + (2 T + 4) 2^-24) counts, A[i] = sum_j |h| |x| in
    counts, T the taps of an output (0 for the plain tuning pass): tests/test_engine_rate.py and test_engine_ddc.py derive
    it for int16 rows, and it carries over unchanged because the scale 32768 is a power of two: the value of a float
    element is exact, so the arithmetic starts from exact inputs as it does from int16.  The worst ratio is printed."""
    tab = table(rdsp)
    assert _phasor_modulus_error(tab) < 2.0 ** -17
    r = np.random.default_rng(70 + P)
    n_out, gain = 256, 2.0
    frac, pairs, n, br = schedule(P, Q, 37, n_out)
    keep = model.keep(P, Q)
    raw = r.uniform(-0.05, 0.05, (keep + pairs, 2)).astype(F32)
    v = values(FL, raw)
    assert np.any(v != np.rint(v)) and np.array_equal(v, raw * F32(32768.0))
    dphi = _dphis(_stations(71 + P, 6, P, Q), P, Q)
    ph0 = r.integers(0, 1 << 32, 6, dtype=np.uint64)
    got = call_rows(v, P, Q, frac, lib_taps(P, Q, gain), dphi, ph0, tab, n_out)
    host = host_rows(host_check, tmp_path, FL, raw[keep:], v[:keep], P, Q, frac, gain, dphi, ph0, n_out)
    assert np.array_equal(_words(got), host)
    Dc = _dc(P, Q)
    Tb = 1 if (P, Q) == (1, 1) else 16 * Dc
    h = np.ones(1) if (P, Q) == (1, 1) else lib_taps(P, Q, gain).astype(np.float64)
    x = np.concatenate([np.zeros(Tb - keep), v[:, 0].astype(np.float64) + 1j * v[:, 1].astype(np.float64)])   # index Tb + n is pair n
    j = np.arange(Tb)
    X = x[Tb + n[:, None] - j[None, :]]
    H = h[j[None, :] * Q + br[:, None]]
    A = (np.abs(H) * np.abs(X)).sum(1)
    T = 0 if (P, Q) == (1, 1) else Tb
    bound = 0.5 + A * (2 * 2.0 ** -17 + (2 * T + 4) * 2.0 ** -24)
    worst = 0.0
    for i, d in enumerate(dphi):
        e = np.exp(-2j * np.pi * ((j * int(d)) % (1 << 32)) / 4294967296.0)
        k = np.array([(int(ph0[i]) + (int(m) + 1 - Dc) * int(d)) & M32 for m in n], np.float64)
        z = (H * X * e[None, :]).sum(1) * np.exp(2j * np.pi * k / 4294967296.0)
        for comp, want in ((0, z.real), (1, z.imag)):
            diff = np.abs(got[i, :, comp].astype(np.float64) - np.clip(want, -32768, 32767))
            worst = max(worst, float((diff / bound).max()))
            assert np.all(diff <= bound), (P, Q, i, comp, int(np.argmax(diff - bound)), float(diff.max()))
    print(f"float rows at {P} / {Q}: worst |diff| / bound = {worst:.3f}")


def test_format_phase_zero_is_the_value(host_check, tmp_path, rdsp):
    """at 44 100 Hz a receiver whose shift is 0 from phase 0 gets its source's values: a U8 row comes out as its widened int16,
    an F32 row as sat16(rne(32768 x)) (rails, halves that round to even, NaN, +-inf among them)"""
    r = np.random.default_rng(3)
    z = np.zeros(1, np.uint64)
    u = r.integers(0, 256, (128, 2)).astype(np.uint8)
    u[:2] = [[0, 255], [127, 128]]
    got = host_rows(host_check, tmp_path, U8, u, np.zeros((0, 2)), 1, 1, 0, 1.0, z, z, 128)
    assert np.array_equal(got[0], _words(widened(U8, u)))
    f = r.uniform(-1.2, 1.2, (128, 2)).astype(F32)
    f[:6] = [[1.0, -1.0], [0.5 / 32768, 1.5 / 32768], [2.5 / 32768, -0.5 / 32768], [np.nan, np.inf], [-np.inf, 3e38], [-3e38, 0.99999994]]
    got = host_rows(host_check, tmp_path, FL, f, np.zeros((0, 2)), 1, 1, 0, 1.0, z, z, 128)
    with np.errstate(invalid="ignore"):
        want = np.clip(np.rint(np.where(np.isnan(f), 0.0, f.astype(np.float64) * 32768.0)), -32768, 32767).astype(np.int16)
    assert np.array_equal(got[0], _words(want))
    assert list(want[1]) == [0, 2] and list(want[2]) == [2, 0] and list(want[3]) == [0, 32767] and list(want[4]) == [-32768, 32767]
    tab = table(rdsp)
    assert np.array_equal(_words(call_rows(values(FL, f), 1, 1, 0, None, z, z, tab, 128)), got)


@pytest.mark.parametrize("P,Q", CPU_RATES)
@pytest.mark.parametrize("fmt", [U8, FL])
def test_format_restatement_does_not_depend_on_the_call_split(rdsp, fmt, P, Q):
    """8 blocks of a U8 and of a random float row in one call, against calls of 1 and 7 blocks with the history (kept as values),
    frac and the phases carried: sample for sample"""
    tab = table(rdsp)
    nb = 8
    v = values(fmt, _raw_of(fmt, wide(5 + P, 1, nb, P, Q, level=0.3)[0], seed=9))
    dphi = _dphis(_stations(6, 3, P, Q), P, Q)
    whole = _restate(v, P, Q, 1.5, dphi, nb, tab)
    assert whole.any()
    for split in (1, 7):
        assert np.array_equal(_restate(v, P, Q, 1.5, dphi, nb, tab, cuts=range(0, nb, split)), whole), split


# ---- readers --------------------------------------------------------------------------------------------------------------
def _wav(path, tag, nch, bits, rate, data, extensible=False):
    fmt = struct.pack("<HHIIHH", 0xFFFE if extensible else tag, nch, rate, rate * nch * bits // 8, nch * bits // 8, bits)
    if extensible:
        fmt += struct.pack("<HHIH", 22, bits, 3, tag) + bytes(14)
    body = b"WAVEfmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def test_format_readers(rdsp, tmp_path):
    """numpy writes RAW .cu8 / .cs8 / .cf32 and WAV 8-bit / float32 (plain and extensible): format, rate, frame count and
    contents come back exactly; refused: WAV 24-bit, mono, a sample_format that contradicts the header, read() on a U8 reader"""
    from radiodsp_sdr_rx_amd._lib import RdspError
    from radiodsp_sdr_rx_amd.io import IO_AUTO, IO_RAW, IO_WAV, IqReader
    r = np.random.default_rng(1)
    n = 1001
    rec = {U8: r.integers(0, 256, (n, 2)).astype(np.uint8), S8: r.integers(-128, 128, (n, 2)).astype(np.int8),
           FL: r.uniform(-1, 1, (n, 2)).astype(F32)}
    rec[FL][0] = [np.inf, -0.0]
    files = []
    for fmt, ext in ((U8, "cu8"), (S8, "cs8"), (FL, "cf32")):
        p = tmp_path / ("rec." + ext)
        rec[fmt].tofile(p)
        files.append((p, IO_RAW, fmt, fmt, 0.0))
    _wav(tmp_path / "u8.wav", 1, 2, 8, 2400000, rec[U8].tobytes())
    _wav(tmp_path / "f32.wav", 3, 2, 32, 250000, rec[FL].tobytes())
    _wav(tmp_path / "f32x.wav", 3, 2, 32, 2048000, rec[FL].tobytes(), extensible=True)
    files += [(tmp_path / "u8.wav", IO_AUTO, -1, U8, 2400000.0), (tmp_path / "f32.wav", IO_WAV, -1, FL, 250000.0),
              (tmp_path / "f32x.wav", IO_AUTO, FL, FL, 2048000.0)]
    for p, container, ask, fmt, rate in files:
        rd = IqReader(p, container, sample_format=ask)
        assert (rd.sample_format, rd.sample_rate, rd.frames) == (fmt, rate, n), p
        a, b, c = rd.read_samples(400), rd.read_samples(400), rd.read_samples(400)
        assert len(c) == 201 and a.dtype == DTYPE[fmt] and len(rd.read_samples(5)) == 0
        assert np.array_equal(np.concatenate([a, b, c]).view(np.uint8), rec[fmt].view(np.uint8)), p
        rd.close()
    _wav(tmp_path / "p24.wav", 1, 2, 24, 48000, bytes(48))
    _wav(tmp_path / "mono.wav", 1, 1, 8, 48000, bytes(48))
    for p, ask in ((tmp_path / "p24.wav", -1), (tmp_path / "mono.wav", -1), (tmp_path / "mono.wav", U8), (tmp_path / "u8.wav", FL),
                   (tmp_path / "u8.wav", S16), (tmp_path / "u8.wav", S8), (tmp_path / "f32.wav", U8), (tmp_path / "f32x.wav", S16)):
        with pytest.raises(RdspError) as ex:
            IqReader(p, IO_WAV, sample_format=ask)
        assert ex.value.code == -5, (p, ask)
    with pytest.raises(RdspError):
        IqReader(tmp_path / "u8.wav")                          # the int16 entry point keeps its behaviour
    rd = IqReader(tmp_path / "rec.cu8", IO_RAW, sample_format=U8)
    assert len(rd.read(10)) == 0 and b"not int16" in rd.lib.rdsp_last_error()
    assert np.array_equal(rd.read_samples(10), rec[U8][:10])  # and consumed nothing
    rd.close()
    x = r.integers(-30000, 30000, (64, 2)).astype(np.int16)
    x.tofile(tmp_path / "x.raw")
    for rd in (IqReader(tmp_path / "x.raw"), IqReader(tmp_path / "x.raw", IO_RAW, sample_format=-1)):
        assert rd.sample_format == S16 and rd.frames == 64 and np.array_equal(rd.read(64), x)
        rd.close()


def test_format_readers_under_address_and_ub_sanitizers(tmp_path):
    """tests/host/host_reader_formats.c, a program of its own, built with rdsp_io.c under ASan + UBSan: the same files and
    refusals with exactly sized buffers"""
    exe = str(tmp_path / "host_reader_formats")
    csrc = os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc")
    subprocess.check_call(["gcc", "-std=c11", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fopenmp", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"), os.path.join(HERE, "host", "host_reader_formats.c")]
                          + [os.path.join(csrc, f) for f in ("rdsp_graph.c", "rdsp_io.c", "rdsp_design.c", "rdsp_q15_tables.c")] + ["-lm", "-o", exe])
    out = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "host_reader_formats OK" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _shape(P, Q, seed, level=0.3):
    """the shape of the GPU cases: 2 sources, 5 receivers (17 under an integer D > 1: one full 16-receiver workgroup of the
    decimating kernel and a ragged one), 8 blocks"""
    nch = 17 if Q == 1 and P > 1 else 5
    source_of = [int(s) for s in np.random.default_rng(seed).integers(0, 2, nch)]
    if Q == 1 and P > 1:
        source_of = [0] * 16 + [1]
    return nch, source_of, _stations(seed + 1, nch, P, Q), wide(seed + 2, 2, 8, P, Q, level=level)


def _twin_runs(fmt, P, Q, raw, x16, nch, source_of, stations, gain=2.0):
    """an engine on `raw` rows of format fmt through update_source_samples and its twin on the int16 rows x16 through
    update_sources: 8 blocks in calls of 1, 2 and 5, the first call on a zero history: equal audio call by call, equal blobs"""
    import torch
    d, d16 = torch.from_numpy(raw).cuda(), torch.from_numpy(x16).cuda()
    for split in (1, 2, 5):
        e, t = (_setup(nch, 2, source_of, P, Q, gain, stations, f) for f in (fmt, S16))
        e.pos_pairs = t.pos_pairs = 0
        ya = _stream(e, d, P, Q, 0, 8, split, odd=split == 5 and Q > 1)
        yb = _stream(t, d16, P, Q, 0, 8, split, entry="rdsp_engine_update_sources")
        assert np.concatenate(yb, 1).any()
        for k, (a, b) in enumerate(zip(ya, yb)):
            assert np.array_equal(a, b), (split, k, np.argwhere(a != b)[:3])
        assert np.array_equal(e.save_state(0, nch), t.save_state(0, nch))
        assert e.source_format() == fmt and t.source_format() == S16
        e.close()
        t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("P,Q", GPU_RATES)
@pytest.mark.parametrize("fmt", [U8, S8])
def test_gpu_format_8bit_against_an_int16_twin(rdsp, fmt, P, Q):
    """D = 1; D = 2, 30 and 48 (the decimating kernel's 4, 2 and 1 outputs a lane with calls of 2 blocks); 3 / 2, 160 / 147 and
    17 / 2 (Tb = 144: across the 128-tap LDS chunk).  In the 5-block runs of a rational rate every call's rows start at an odd
    pair offset into one long device buffer (2-byte alignment only)."""
    nch, source_of, stations, x = _shape(P, Q, 100 + P + fmt)
    raw = _raw_of(fmt, x)
    _twin_runs(fmt, P, Q, raw, widened(fmt, raw), nch, source_of, stations)


@pytest.mark.gpu
@pytest.mark.parametrize("P,Q", GPU_RATES)
def test_gpu_format_float_rows_of_integers_against_an_int16_twin(rdsp, P, Q):
    """float rows k / 32768 against the twin on the int16 rows k (the full-scale pairs of wide() among them); odd pair
    offsets (8-byte alignment only) in the 5-block runs of a rational rate"""
    nch, source_of, stations, x = _shape(P, Q, 200 + P, level=0.05)
    _twin_runs(FL, P, Q, _raw_of(FL, x), x, nch, source_of, stations)


@pytest.mark.gpu
@pytest.mark.parametrize("P,Q", GPU_RATES)
def test_gpu_format_random_float_rows_against_the_restatement(rdsp, P, Q):
    """random non-integer float rows at +-0.05 of full scale, row 1 salted with NaN, +-inf and +-3e38: the numpy restatement's
    tuned rows, fed to rdsp_engine_update of a twin without sources, give the audio of update_source_samples bit for bit, in
    calls of 1, 2 and 5 blocks (as tests/test_engine_rate.py compares)"""
    import torch
    nch, source_of, stations, x = _shape(P, Q, 300 + P, level=0.05)
    raw = _raw_of(FL, x, seed=301 + P)
    r = np.random.default_rng(302 + P)
    at = r.integers(0, raw.shape[1], 40)
    raw[1, at, r.integers(0, 2, 40)] = r.choice(np.array([np.nan, np.inf, -np.inf, 3e38, -3e38], F32), 40)
    raw[1, :3] = [[np.nan, np.inf], [-np.inf, 3e38], [-3e38, np.nan]]
    gain = 2.0
    tab = table(rdsp)
    tuned = np.zeros((nch, 8 * 128, 2), np.int16)
    for s in (0, 1):
        cs = [c for c in range(nch) if source_of[c] == s]
        if cs:
            tuned[cs] = _restate(values(FL, raw[s]), P, Q, gain, _dphis(stations[cs], P, Q), 8, tab)
    d, dt = torch.from_numpy(raw).cuda(), torch.from_numpy(tuned).cuda()
    for split in (1, 2, 5):
        e = _setup(nch, 2, source_of, P, Q, gain, stations, FL)
        t = engine(nch, 8)
        t.sketch_setup()
        e.pos_pairs = 0
        ya = _stream(e, d, P, Q, 0, 8, split, odd=split == 5 and Q > 1)
        yb = [t.update(dt[:, u * 128:min(8, u + split) * 128].contiguous()).cpu().numpy() for u in range(0, 8, split)]
        assert np.concatenate(yb, 1).any()
        for k, (a, b) in enumerate(zip(ya, yb)):
            assert np.array_equal(a, b), (split, k, np.argwhere(a != b)[:3])
        e.close()
        t.close()


@pytest.mark.gpu
def test_gpu_format_more_than_a_workgroup_of_receivers_on_one_source(rdsp):
    """U8, one source at 160 / 147, 4 blocks, 256 + 44 receivers (one full workgroup of the polyphase kernel and a ragged one):
    the receivers test_gpu_rate_more_than_a_workgroup_of_receivers_on_one_source lists, against the int16 twin"""
    import torch
    P, Q, nch, nb = 160, 147, 300, 4
    raw = _to_u8(wide(11, 1, nb, P, Q, level=0.3))
    stations = _stations(12, nch, P, Q)
    outs = []
    for fmt, rows in ((U8, raw), (S16, widened(U8, raw))):
        e = _setup(nch, 1, [0] * nch, P, Q, 2.0, stations, fmt, max_blocks=nb)
        e.pos_pairs = 0
        outs.append(_stream(e, torch.from_numpy(rows).cuda(), P, Q, 0, nb, nb)[0])
        e.close()
    for c in [0, 1, 63, 64, 127, 128, 191, 192, 254, 255, 256, 257, 298, 299]:
        assert outs[1][c].any() and np.array_equal(outs[0][c], outs[1][c]), c


@pytest.mark.gpu
def test_gpu_format_is_a_setting(rdsp):
    """160 / 147, 2 sources, 5 receivers.  The format survives reset, set_sources and the rate setters; after a reset (made where
    frac is not 0) the next call equals a fresh engine's first call.  U8 -> F32 -> U8 in mid-stream: each switch starts from
    zero histories and frac = 0 with the phases kept -- against an int16 twin that begins a new stream the same way (its rate
    set to 88 200 Hz and back: histories and frac zeroed, phases kept).  Setting the format the engine has, in mid-stream,
    changes no bit."""
    import torch
    P, Q, gain = 160, 147, 2.0
    nch, source_of, stations, x = _shape(P, Q, 400)
    x = np.concatenate([x, wide(403, 2, 8, P, Q, level=0.3)], 1)          # 16 blocks and a few pairs
    u8 = _to_u8(x)
    w = widened(U8, u8)
    fl = _raw_of(FL, w)                                                          # k / 32768 of the same values
    du, dw, df = (torch.from_numpy(a).cuda() for a in (u8, w, fl))
    e, t = (_setup(nch, 2, source_of, P, Q, gain, stations, f) for f in (U8, S16))
    e.pos_pairs = t.pos_pairs = 0
    first = _stream(e, du, P, Q, 0, 3, 3)[0]
    assert (3 * 128 * P) % Q != 0
    e.reset()
    e.set_sources(2, source_of)
    e.set_source_rate(P, Q, gain)
    assert e.source_format() == U8 and e.source_pairs(3) == _pairs(P, Q, 3)
    e.pos_pairs = 0
    assert np.array_equal(_stream(e, du, P, Q, 0, 3, 3)[0], first)               # the format kept, histories and frac zero
    assert np.array_equal(_stream(t, dw, P, Q, 0, 3, 3)[0], first)
    # from here e and t are 3 blocks into the same stream; e sets U8 again between calls
    e.set_source_format(U8)
    ya, yb = _stream(e, du, P, Q, 3, 5, 1), _stream(t, dw, P, Q, 3, 5, 1)
    e.set_source_format(U8)
    ya += _stream(e, du, P, Q, 5, 6, 1)
    yb += _stream(t, dw, P, Q, 5, 6, 1)
    assert e.source_pairs(2) == t.source_pairs(2)
    for fmt, dev in ((FL, df), (U8, du)):                                        # another format: another stream, phases kept
        e.set_source_format(fmt)
        t.set_source_decimation(2)
        t.set_source_rate(P, Q, gain)
        assert e.source_format() == fmt and e.source_pairs(2) == _pairs(P, Q, 2) == t.source_pairs(2)
        s0 = e.pos_pairs
        ya += _stream(e, dev, P, Q, 0, 4, 2)
        e.pos_pairs = t.pos_pairs = s0
        yb += _stream(t, dw, P, Q, 0, 4, 2)
        e.pos_pairs = t.pos_pairs
    for k, (a, b) in enumerate(zip(ya, yb)):
        assert a.any() and np.array_equal(a, b), (k, np.argwhere(a != b)[:3])
    assert np.array_equal(e.save_state(0, nch), t.save_state(0, nch))
    assert e.save_state(0, 2).size == 16 + 2 * (10368 + 4)                       # the format is in no blob
    e.close()
    t.close()


@pytest.mark.gpu
def test_gpu_format_refusals(rdsp):
    """refused with nothing changed: set_source_format before set_sources (NOT_READY); format 4 and -1; update_sources under U8;
    at an integer rate a row that is not 16-byte aligned and a stride whose bytes are no multiple of 16; at a rational rate a
    row that is not aligned to a pair (U8: 2 bytes, F32: 8 bytes); a stride shorter than source_pairs -- the object then runs
    on exactly as a twin that never saw those calls"""
    import torch
    from radiodsp_sdr_rx_amd._lib import RdspError
    fresh = engine(2, 4)
    with pytest.raises(RdspError) as ex:
        fresh.set_source_format(U8)
    assert ex.value.code == -4 and b"set_sources" in fresh.lib.rdsp_last_error() and fresh.source_format() == S16
    fresh.close()
    nch, source_of, _, x = _shape(2, 1, 500)
    stations = _stations(502, nch, 3, 2)                                         # inside both rates' bands
    u8 = _to_u8(x)
    d = torch.from_numpy(u8).cuda()
    out = torch.empty((nch, 4 * 128, 2), dtype=torch.int16, device="cuda")
    eng, twin = (_setup(nch, 2, source_of, 2, 1, 2.0, stations, U8) for _ in range(2))
    eng.pos_pairs = twin.pos_pairs = 0
    for f in (4, -1, 1000):
        with pytest.raises(RdspError) as ex:
            eng.set_source_format(f)
        assert ex.value.code == -1 and eng.source_format() == U8
    rows = d[:, :4 * 128 * 2].contiguous()
    n = rows.shape[1]
    assert _c_call(eng, rows, 4, out, "rdsp_engine_update_sources") == -1 and b"format" in eng.lib.rdsp_last_error()
    assert _c_call(eng, rows, 4, out, ptr=rows.data_ptr() + 2) == -1             # on a pair, not on 16 bytes
    assert _c_call(eng, rows, 4, out, stride=n + 4) == -1                        # 2 (n + 4) bytes: no multiple of 16
    assert _c_call(eng, rows, 4, out, stride=n - 8) == -1                        # shorter than source_pairs
    assert _c_call(eng, rows, 5, out) == -1
    y = [_stream(e, d, 2, 1, 0, 4, 4)[0] for e in (eng, twin)]
    assert y[0].any() and np.array_equal(y[0], y[1])
    # a rational rate: rows aligned to one pair
    raw = {U8: _to_u8(wide(501, 2, 8, 3, 2, level=0.3))}
    raw[FL] = _raw_of(FL, widened(U8, raw[U8]), seed=5)
    for fmt in (U8, FL):
        dev = torch.from_numpy(raw[fmt]).cuda()
        for e in (eng, twin):
            e.set_source_rate(3, 2, 2.0)
            e.set_source_format(fmt)
            e.pos_pairs = 0
        need = eng.source_pairs(4)
        rows = dev[:, 1:1 + need]
        assert _c_call(eng, rows, 4, out, ptr=rows.data_ptr() + (1 if fmt == U8 else 4)) == -1
        assert _c_call(eng, rows, 4, out, stride=need - 1) == -1
        assert _c_call(eng, rows, 4, out, "rdsp_engine_update_sources") == -1
        assert eng.source_pairs(4) == need and eng.source_format() == fmt
        y = [_stream(e, dev, 3, 2, 0, 8, 4) for e in (eng, twin)]
        assert y[0][1].any() and all(np.array_equal(a, b) for a, b in zip(*y))
    eng.close()
    twin.close()


@pytest.mark.gpu
def test_gpu_format_python_wrapper(rdsp):
    """Engine.update_sources takes torch.uint8 and torch.float32 rows under the matching format (an integer rate without
    n_blocks, a rational one with n_blocks on a view): the audio of the C entry; an int16 tensor under U8 is refused"""
    import torch
    from radiodsp_sdr_rx_amd.engine import SRC_F32, SRC_U8
    assert (SRC_U8, SRC_F32) == (U8, FL)
    for P, Q in ((2, 1), (160, 147)):
        nch, source_of, stations, x = _shape(P, Q, 600 + P)
        u8 = _to_u8(x)
        for fmt, raw in ((U8, u8), (FL, _raw_of(FL, widened(U8, u8)))):
            d = torch.from_numpy(raw).cuda()
            e, t = (_setup(nch, 2, source_of, P, Q, 2.0, stations, fmt) for _ in range(2))
            t.pos_pairs = 0
            need = e.source_pairs(8)
            y = e.update_sources(d[:, :need].contiguous()) if Q == 1 else e.update_sources(d[:, :need], n_blocks=8)
            assert y.dtype == torch.int16 and np.array_equal(y.cpu().numpy(), _stream(t, d, P, Q, 0, 8, 8)[0])
            with pytest.raises(AssertionError):
                e.update_sources(torch.zeros((2, need, 2), dtype=torch.int16, device="cuda"), n_blocks=8)
            e.close()
            t.close()
