"""The AFSK 1200 packet decoder of rdsp_engine_t without a GPU (include/rdsp.h "AFSK 1200 packet decoder"; csrc/rdsp_afsk.h,
csrc/rdsp_engine_afsk_host.hip): the exports, every refusal that needs no device, the steps against float64, the frame check
sequence, rdsp_engine_afsk_space_gain against its formula, ax25.parse, tests/host/host_afsk_check.cpp -- csrc/rdsp_afsk.h as a
program of its own, plain and under ASan + UBSan, run directly -- against the model's bits under every cut of 1 to 3 blocks, and
the decoder's figures on the float32 model, printed and asserted.  tests/test_engine_afsk_gpu.py holds the kernel to the same
model."""
import math
import os
import subprocess

import numpy as np
import pytest

import engine_afsk_model as A
import engine_dtmf_model as D
import engine_sources_model as S
import engine_tone_model as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def test_afsk_exports(rdsp):
    from radiodsp_sdr_rx_amd import ax25, engine
    lib = rdsp.load()
    for name in ("enable_afsk", "afsk_enabled", "set_afsk", "read_afsk", "read_afsk_frames", "afsk_space_gain", "afsk_fcs"):
        assert hasattr(lib, "rdsp_engine_" + name), name
    assert callable(engine.afsk_space_gain) and callable(engine.afsk_fcs) and callable(ax25.parse)
    assert all(callable(getattr(engine.Engine, n)) for n in ("enable_afsk", "set_afsk", "read_afsk", "read_afsk_ring", "read_afsk_frames"))
    assert isinstance(engine.Engine.afsk_enabled, property)


def test_afsk_refusals_without_a_device(rdsp):
    """no object: every entry point refuses; rdsp_engine_afsk_space_gain answers 0.0 to a time constant rdsp_engine_tone_gain
    refuses.  The refusals that need an object are test_engine_afsk_gpu's"""
    from radiodsp_sdr_rx_amd.engine import afsk_space_gain
    lib = rdsp.load()
    assert lib.rdsp_engine_enable_afsk(None) == -1 and lib.rdsp_engine_afsk_enabled(None) == 0
    assert lib.rdsp_engine_set_afsk(None, 1, 1.0, 2, 17) == -1 and b"rdsp_engine_set_afsk" in lib.rdsp_last_error()
    assert lib.rdsp_engine_read_afsk(None, 0, None, 0, None, 0, None, 0, None, 0, None) == -1
    assert lib.rdsp_engine_read_afsk_frames(None, 0, 1, None, None, None) == -1
    for tau in (24.0, 1001.0, -1.0, float("nan"), float("inf")):
        assert lib.rdsp_engine_afsk_space_gain(tau) == 0.0 and b"rdsp_engine_afsk_space_gain" in lib.rdsp_last_error(), tau
        with pytest.raises(rdsp.RdspError):
            afsk_space_gain(tau)


def test_afsk_fcs_and_residue(rdsp):
    """the X-25 check value, the library's against the model's on drawn bytes, and the residue: the running register over a
    frame with its FCS, low byte first, ends at 0xF0B8 whatever the frame"""
    from radiodsp_sdr_rx_amd.engine import afsk_fcs
    assert afsk_fcs(b"123456789") == 0x906E == A.fcs(b"123456789") and afsk_fcs(b"") == 0 == A.fcs(b"")
    r = np.random.default_rng(3)
    for n in (1, 2, 15, 17, 80, 328):
        data = bytes(r.integers(0, 256, n, dtype=np.uint8))
        assert afsk_fcs(data) == A.fcs(data)
        crc = 0xFFFF
        for b in A.with_fcs(data):
            crc = A.crc_byte(crc, b)
        assert crc == 0xF0B8 == A.RESIDUE


def test_afsk_steps_against_float64():
    """the three steps are llround(f 2^32 4 / 44100); a bit is 9.1875 decimated samples; lscale is the float32 nearest to
    1 / (32 24^2); a sine of amplitude A at 1200 Hz, taken as 4 A at the decimated rate (the boxcar's gain left out), reads
    P_mark = (24 A)^2 within the double-frequency ripple sum |e^{2 j w n}| <= 1 / sin w over 12, and next to nothing at 2200 Hz"""
    for f, d in ((1200.0, A.STEP), (1200.0, A.DPHI_MARK), (2200.0, A.DPHI_SPACE)):
        assert d == round(f * 4 * 2 ** 32 / 44100.0) and abs(d / 2 ** 32 * 11025.0 - f) < 2e-6 and d < 2 ** 31
    assert A.STEP == 467479434 and abs(2 ** 32 / A.STEP - 9.1875) < 1e-7
    assert A.LSCALE == F32(1.0 / 18432.0) and abs(float(A.LSCALE) * 18432.0 - 1.0) < 2.0 ** -24
    amp = 0.25
    m = np.arange(400)
    w = 2 * np.pi * 1200.0 / 11025.0
    d = 4 * amp * np.cos(w * m + 0.4)
    for f, want in ((1200.0, (24 * amp) ** 2), (2200.0, 0.0)):
        c = np.array([np.sum(d[k - 11:k + 1] * np.exp(2j * np.pi * f / 11025.0 * m[k - 11:k + 1])) for k in range(11, 400)])
        P = np.abs(c) ** 2
        if want:
            ripple = 1.0 / (12 * math.sin(w))
            assert np.all(np.abs(np.sqrt(P / want) - 1.0) < ripple), (f, P.min(), P.max())
        else:
            assert P.max() < 0.12 * (24 * amp) ** 2, P.max()                  # 12 samples hold 1.3 and 2.4 cycles: not orthogonal, but 9 dB down


def test_afsk_stage2_is_float64(rdsp):
    """the float32 correlators against float64 on drawn rows: P_mark, g P_space (through lvl) within 12 roundings and the table's
    2^-17, and every raw decision whose float64 margin exceeds that is the float64 one"""
    tab = S.table(rdsp)
    r = np.random.default_rng(11)
    rows = r.uniform(-1.0, 1.0, (3, 9 * 128)).astype(F32)
    raw, lvl, hist = A.stage12(tab, rows, np.zeros((3, 11), F32), np.zeros(3, np.uint32), np.full(3, 3.27, F32))
    d = np.concatenate([np.zeros((3, 11)), rows.astype(np.float64).reshape(3, -1, 4).sum(2)], 1)
    m = np.arange(-11, 9 * 32)
    P = []
    for f in (1200.0, 2200.0):
        p = d * np.exp(2j * np.pi * f * 4 / 44100.0 * m)[None]
        P.append(np.abs(np.stack([p[:, k:k + 12].sum(1) for k in range(9 * 32)], 1)) ** 2)
    g = float(F32(3.27))
    v = P[0] - g * P[1]
    tol = 1e-4 * (P[0] + g * P[1]) + 1e-9
    sure = np.abs(v) > tol
    assert sure.mean() > 0.99 and np.array_equal(raw[sure], (v > 0)[sure])
    want = (P[0] + g * P[1]).reshape(3, 9, 32).sum(2) / 18432.0
    assert np.allclose(lvl, want, rtol=1e-4) and np.array_equal(bits(hist), bits(D.quad(rows)[:, -11:]))


def test_afsk_space_gain_is_the_formula(rdsp):
    """rdsp_engine_afsk_space_gain is (dtmf_gain(1200) / dtmf_gain(2200))^2 in double: 1.09 without a de-emphasis (the boxcar of
    4 alone) and 3.57 behind 750 us, of which the de-emphasis is 3.27"""
    from radiodsp_sdr_rx_amd.engine import afsk_space_gain, dtmf_gain
    for tau in (0.0, 25.0, 75.0, 530.0, 750.0, 1000.0):
        want = (dtmf_gain(1200.0, tau) / dtmf_gain(2200.0, tau)) ** 2
        g = afsk_space_gain(tau)
        assert abs(g - want) <= 4e-16 * want and abs(g - A.space_gain(tau)) <= 1e-15 * want and 1.0 < g < 16.0, (tau, g, want)
    print(f"space_gain: {afsk_space_gain(0.0):.4f} flat, {afsk_space_gain(75.0):.4f} at 75 us, {afsk_space_gain(750.0):.4f} at 750 us")
    assert abs(afsk_space_gain(750.0) / afsk_space_gain(0.0) - 3.27) < 0.01 and abs(afsk_space_gain(0.0) - 1.09) < 0.01


def _addr(call, ssid, last=False, h=False):
    return bytes(ord(c) << 1 for c in call.ljust(6)) + bytes([0x60 | ssid << 1 | (0x80 if h else 0) | (1 if last else 0)])


def test_ax25_parse():
    """a hand-built APRS UI frame through two repeaters, the first of which has repeated it; an I frame; a frame without a PID;
    the malformed ones: too short, an address list that never ends or ends inside a callsign or behind the destination, a
    callsign with a character AX.25 has not"""
    from radiodsp_sdr_rx_amd import ax25
    info = b"!4903.50N/07201.75W-Test 001234"
    frame = _addr("APRS", 0) + _addr("N0CALL", 7) + _addr("WIDE1", 1, h=True) + _addr("WIDE2", 2, last=True) + b"\x03\xf0" + info
    f = ax25.parse(frame)
    assert f == ("APRS", "N0CALL-7", ("WIDE1-1*", "WIDE2-2"), 0x03, 0xF0, info) and f.source == "N0CALL-7" and f.info == info
    f = ax25.parse(_addr("CQ", 0) + _addr("DL1ABC", 15, last=True) + b"\x00\xcf" + b"hello")
    assert f == ("CQ", "DL1ABC-15", (), 0x00, 0xCF, b"hello")
    f = ax25.parse(_addr("CQ", 0) + _addr("DL1ABC", 0, last=True) + b"\x3f")              # SABM: no PID, no info
    assert f == ("CQ", "DL1ABC", (), 0x3F, None, b"")
    bad = [b"", frame[:14],
           _addr("APRS", 0) + _addr("N0CALL", 7) + _addr("WIDE1", 1) + b"\x03\xf0",      # the list does not end
           _addr("APRS", 0, last=True) + _addr("N0CALL", 7, last=True) + b"\x03\xf0",    # ends behind the destination
           bytes([frame[0] | 1]) + frame[1:],                                             # ends inside a callsign
           _addr("ap rs", 0) + _addr("N0CALL", 7, last=True) + b"\x03\xf0",              # no callsign
           _addr("", 0) + _addr("N0CALL", 7, last=True) + b"\x03\xf0",
           _addr("APRS", 0) + _addr("N0CALL", 7) + b"".join(_addr("R%d" % k, 0) for k in range(9)) + _addr("LAST", 0, last=True) + b"\x03\xf0",
           _addr("APRS", 0) + _addr("N0CALL", 7, last=True) + b"\x03"]                    # a UI frame without its PID
    for b in bad:
        with pytest.raises(ValueError):
            ax25.parse(b)


def _from_bits(hdlc_bits, total, **kw):
    return A.audio(A.nrzi(hdlc_bits), total=total, **kw)


def _host_rows():
    """-> (short rows float32 [8, 400 * 128], what each must read, the long row [1, 1700 * 128]).  On the rails; all zeros; a frame
    aborted by seven ones in front of a whole one; two frames sharing one flag; a byte that ends in five ones, so that the
    stuffed bit falls on a byte boundary; a payload of 0xFF bytes, the most stuffing; six frames through the ring of four; the
    model's own noise.  The long row: a frame of 331 bytes (FCS included), which is dropped, and one of 330, which is kept"""
    r = np.random.default_rng(41)
    nb = 400
    n = nb * 128
    pay = lambda k: bytes(r.integers(0, 256, k, dtype=np.uint8))
    a1, a2 = pay(24), pay(20)
    aborted = A.FLAG * 6 + A.stuffed(a1)[:100] + [1] * 7 + A.FLAG * 3 + A.stuffed(A.with_fcs(a2)) + A.FLAG * 2
    s1, s2 = pay(18), pay(31)
    shared = A.FLAG * 6 + A.stuffed(A.with_fcs(s1)) + A.FLAG + A.stuffed(A.with_fcs(s2)) + A.FLAG * 2
    edge = bytes([0xF8, 0x1F, 0x3E]) * 6 + pay(4)                                        # five ones end on a byte's last bit
    ff = b"\xff" * 40
    six = [pay(15 + k) for k in range(6)]
    many = []
    for p in six:
        many += A.frame_bits(p, flags_before=3, flags_after=1)
    rows = np.stack([r.choice(np.array([1.0, -1.0]), n), np.zeros(n), _from_bits(aborted, n), _from_bits(shared, n, lead=77),
                     _from_bits(A.frame_bits(edge, 6, 2), n, lead=5), _from_bits(A.frame_bits(ff, 6, 2), n), _from_bits(many, n, lead=130, amp=0.2),
                     r.uniform(-1.0, 1.0, n)]).astype(F32)
    want = [None, [], [a2], [s1, s2], [edge], [ff], six[2:], None]
    big_no, big_yes = pay(329), pay(328)
    long_bits = A.frame_bits(big_no, 6, 2) + A.frame_bits(big_yes, 4, 2)
    assert len(long_bits) * 36.75 < 1700 * 128
    long_row = _from_bits(long_bits, 1700 * 128, lead=9)[None].astype(F32)
    return rows, want, long_row, big_yes


@pytest.mark.parametrize("sanitize", [False, True])
def test_afsk_host_program(rdsp, tmp_path, sanitize):
    """tests/host/host_afsk_check.cpp, plain and under ASan + UBSan, a program of its own run on the CPU: on the rows of
    _host_rows, for the defaults and for pull 1 with the de-emphasis value of space_gain, under 27 cuts into calls of 1 to 3
    blocks (which it holds to one long call itself), its steps, records and final words equal the model's.  At the defaults the
    rows read what their construction says; the row of zeros saturates `ones` at 7; six frames leave frames 2 ... 5 in the ring
    with n_frames 6; the frame of 331 bytes is dropped and the one of 330 kept"""
    exe = str(tmp_path / ("host_afsk_check_san" if sanitize else "host_afsk_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_afsk_check.cpp"), "-o", exe])
    rows, want, long_row, big_yes = _host_rows()
    tab = S.table(rdsp)
    fin, fout = str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")
    for x, settings in ((rows, ((1.0, 2, 17), (A.space_gain(750.0), 1, 9))), (long_row, ((1.0, 2, 17),))):
        n, nb = x.shape[0], x.shape[1] // 128
        x.tofile(fin)
        for g, pull, min_bytes in settings:
            m = A.Afsk(n, tab, 1, g, pull, min_bytes)
            sync, new, bad, lvl = m.run(x)
            out = subprocess.run([exe, fin, fout, repr(float(F32(g))), str(pull), str(min_bytes), str(n), str(nb)], capture_output=True, text=True, timeout=600)
            assert out.returncode == 0 and out.stdout.endswith("host_afsk_check OK\n"), out.stdout + out.stderr
            assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
            w = np.fromfile(fout, np.uint32)
            assert w[0] == bits(A.LSCALE) and list(w[1:4]) == [A.STEP, A.DPHI_MARK, A.DPHI_SPACE]
            body = w[4:].reshape(n, 4 * nb + A.WORDS)
            assert np.array_equal(body[:, :nb], sync) and np.array_equal(body[:, nb:2 * nb], new) and np.array_equal(body[:, 2 * nb:3 * nb], bad), (g, pull)
            assert np.array_equal(body[:, 3 * nb:4 * nb], bits(lvl)), (g, pull)
            assert np.array_equal(body[:, 4 * nb:], m.words()), (g, pull)
            wd = m.words()
            assert (wd[:, A.TBLOCKS] == nb).all() and not wd[:, 13:16].any() and not wd[:, A.HIST_ + 11].any()
            if (g, pull, min_bytes) != (1.0, 2, 17):
                continue
            if n == 1:
                assert [f for _, f in m.frames(0)] == [big_yes] and wd[0, A.NFRAMES] == 1 and wd[0, A.NBAD] == 0 and new.sum() == 1
                continue
            for c, frames in enumerate(want):
                if frames is not None:
                    assert [f for _, f in m.frames(c)] == frames, c
            assert wd[1, A.ONES] == 7 and wd[1, A.INFRAME] == 0 and not lvl[1].any() and not sync[1].any()           # silence: ones saturate
            assert wd[2, A.NFRAMES] == 1 and wd[2, A.NBAD] == 0                                                       # the abort is no bad frame
            assert wd[6, A.NFRAMES] == 6 and new[6].sum() == 6 and sorted(t for t, _ in m.frames(6)) == [t for t, _ in m.frames(6)]
            assert [int(b) + 1 for b in np.flatnonzero(new[6])][2:] == [t for t, _ in m.frames(6)]
            assert wd[0, A.NFRAMES] == 0 and wd[7, A.NFRAMES] == 0 and lvl[0].all()
    for bad_args in (["0.01", "2", "17"], ["17", "2", "17"], ["nan", "2", "17"], ["1", "0", "17"], ["1", "5", "17"], ["1", "2", "8"], ["1", "2", "331"]):
        assert subprocess.run([exe, fin, fout] + bad_args + ["1", "1"], capture_output=True).returncode == 2, bad_args


def _points():
    """the sketch's conditions: tones at 0.3 of the deviation, white noise of rms sigma at the 44.1 kHz tap, the baud rate off by
    a drawn +-300 ppm and the tones by a drawn +-1 %, payloads of 20 to 80 drawn bytes; 20 frames a point, every frame a row of
    its own behind 12 flags and a drawn lead -> (rows float64 [20, t] without noise, the payloads)"""
    r = np.random.default_rng(77)
    t = 260 * 128
    rows, sent = [], []
    for k in range(20):
        p = bytes(r.integers(0, 256, int(r.integers(20, 81)), dtype=np.uint8))
        rows.append(A.audio(A.nrzi(A.frame_bits(p, 12, 2)), 0.3, ppm=r.uniform(-300, 300), tone_off=r.uniform(-0.01, 0.01), phase=r.uniform(0, 6),
                            lead=int(r.integers(0, 700)), total=t))
        sent.append(p)
    return np.stack(rows), sent


def _read(tab, x, sent, **kw):
    """-> (rows that read exactly their payload, once; frames emitted that are not the row's payload or are a second copy of it)"""
    m = A.Afsk(len(x), tab, 1, **kw)
    m.run(x)
    assert (m.words()[:, A.NFRAMES] <= A.RING).all()                                # frames() shows every frame emitted
    got = [[f for _, f in m.frames(c)] for c in range(len(x))]
    good = sum(1 for c in range(len(x)) if got[c] == [sent[c]])
    extras = sum(len(got[c]) - (1 if sent[c] in got[c] else 0) for c in range(len(x)))
    return good, extras


def test_afsk_figures(rdsp):
    """the decoder's figures on the float32 model, printed and asserted.  The table of the issue's float64 sketch: W = 12 flat with
    g = 1 and behind the 750 us de-emphasis with g = 3.27 (pull 1 and 3 beside the default 2, printed only), and the points of
    W = 9 and W = 8 that the choice of W = 12 rests on, through the model's window argument (every row starts from a fresh
    detector, so a shorter window needs nothing of the state layout); every point of one condition sees the same noise whatever
    W and pull.  The de-emphasised points again at g = afsk_space_gain(750) = 3.57, the helper's own value.  Asserted: at the
    defaults every frame is read at sigma <= 0.1, flat and de-emphasised, at both values of g; whatever W, pull and sigma, a row
    emits nothing but its payload, once.  Then 20 rows of one second of an idle discriminator (uniform +-1) and 60 rows of one
    second of voice-band noise of rms 0.25, flat and de-emphasised, emit nothing: each row is a detector of its own that starts
    from zeros, so these are 20 and 60 s of noise but not one stream of that length -- clock and HDLC state do not carry from one
    second into the next"""
    tab = S.table(rdsp)
    clean, sent = _points()
    g_sketch, g_helper = 3.27, A.space_gain(750.0)                                  # the sketch's leaves out the boxcar's 1.09
    noisy = {}

    def rows(sigma, de):
        if (sigma, de) not in noisy:
            x = (clean + sigma * np.random.default_rng(int(1000 * sigma) + (7 if de else 0)).standard_normal(clean.shape)).astype(F32)
            noisy[sigma, de] = D.deemph_rows(x, 750.0) if de else x
        return noisy[sigma, de]

    def point(name, sigma, de, **kw):
        good, extras = _read(tab, rows(sigma, de), sent, **kw)
        assert extras == 0, (name, sigma, kw)
        return good

    for name, sigmas, g, de in (("flat, g = 1", (0.05, 0.1, 0.2, 0.3, 0.4), 1.0, False),
                                (f"750 us, g = {g_sketch:.2f}", (0.05, 0.1, 0.12, 0.15, 0.16, 0.2), g_sketch, True)):
        for sigma in sigmas:
            res = {pull: point(name, sigma, de, space_gain=g, pull=pull) for pull in (1, 2, 3)}
            print(f"W = 12, {name}, sigma {sigma}: " + ", ".join(f"pull {p}: {res[p]}/20" for p in (1, 2, 3)))
            if sigma <= 0.1:
                assert res[2] == 20, (name, sigma)
    for W, name, sigmas, g, de in ((9, "flat, g = 1", (0.05, 0.1, 0.2, 0.3), 1.0, False), (9, f"750 us, g = {g_sketch:.2f}", (0.15,), g_sketch, True),
                                   (8, f"750 us, g = {g_sketch:.2f}", (0.12,), g_sketch, True), (8, "flat, g = 1", (0.05, 0.2), 1.0, False)):
        for sigma in sigmas:
            print(f"W = {W}, {name}, sigma {sigma}: pull 2: {point(name, sigma, de, space_gain=g, window=W)}/20")
    for sigma in (0.05, 0.1, 0.12, 0.15, 0.16, 0.2):
        good = point("helper", sigma, True, space_gain=g_helper)
        print(f"W = 12, 750 us, g = afsk_space_gain(750) = {g_helper:.2f}, sigma {sigma}: pull 2: {good}/20")
        if sigma <= 0.1:
            assert good == 20, sigma
    sec = 345 * 128
    idle = np.random.default_rng(5).uniform(-1.0, 1.0, (20, sec)).astype(F32)
    voice = np.clip(np.stack([T.voice_noise(900 + k, sec, 0.25) for k in range(60)]), -1.0, 1.0).astype(F32)
    for name, x, g in (("idle, flat", idle, 1.0), ("idle, de-emphasised", D.deemph_rows(idle), g_sketch), ("voice-band noise, flat", voice, 1.0),
                       ("voice-band noise, de-emphasised", D.deemph_rows(voice), g_sketch)):
        m = A.Afsk(len(x), tab, 1, space_gain=g)
        sync, new, bad, lvl = m.run(x)
        print(f"{name}: {len(x)} rows of {sec / 44100.0:.2f} s, {int(m.words()[:, A.NFRAMES].sum())} frames, {int(m.words()[:, A.NBAD].sum())} bad FCS, "
              f"in sync {sync.mean():.3f} of the blocks, sqrt(lvl) {math.sqrt(float(lvl.mean())):.3f}")
        assert not m.words()[:, A.NFRAMES].any() and not new.any(), name
