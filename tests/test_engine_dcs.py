"""The DCS code squelch of rdsp_engine_t without a GPU (include/rdsp.h "code squelch"; csrc/rdsp_dcs.h,
csrc/rdsp_engine_dcs_host.hip): the exports, every refusal that needs no device, the code words and the facts about their
rotation classes, rdsp_dcs_code_of_word on every rotation of every standard word and its inverse, the bit clock's step and the
bound on on_hits, tests/host/host_dcs_check.cpp -- csrc/rdsp_dcs.h as a program of its own, plain and under ASan + UBSan, run
directly -- against tests/engine_dcs_model.py's bits at every cut of 1 to 3 blocks, and the detector's figures on synthetic
demodulated rows, printed and asserted on the float32 model.  tests/test_engine_dcs_gpu.py holds the kernel to the same model."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import engine_dcs_model as D
import engine_tone_model as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32
W023, W754 = D.codeword(0o023), D.codeword(0o754)


def test_dcs_exports(rdsp):
    from radiodsp_sdr_rx_amd import engine
    lib = rdsp.load()
    for name in ("engine_enable_dcs", "engine_dcs_enabled", "engine_set_dcs_codes", "engine_set_dcs_squelch", "engine_read_dcs", "dcs_codeword",
                 "dcs_standard", "dcs_code_of_word"):
        assert hasattr(lib, "rdsp_" + name), name
    assert all(callable(getattr(engine, n)) for n in ("dcs_codeword", "standard_dcs_codes", "dcs_code_of_word"))
    assert all(callable(getattr(engine.Engine, n)) for n in ("enable_dcs", "set_dcs_codes", "set_dcs_squelch", "read_dcs"))
    assert isinstance(engine.Engine.dcs_enabled, property)
    assert engine.DCS_ANY == D.ANY == 0xFFFF and engine.DCS_INVERTED == D.INVERTED == 0x8000


def test_dcs_refusals_without_a_device(rdsp):
    """no object: every entry point refuses; the host functions refuse a code outside 0 ... 511, NULL pointers, a word that is 0,
    wider than 23 bits or in no standard code's class.  The refusals that need an object are test_engine_dcs_gpu's"""
    from radiodsp_sdr_rx_amd.engine import dcs_code_of_word, dcs_codeword
    lib = rdsp.load()
    codes = (C.c_uint16 * 2)(0o023, 0)
    assert lib.rdsp_engine_enable_dcs(None) == -1 and lib.rdsp_engine_dcs_enabled(None) == 0
    assert lib.rdsp_engine_set_dcs_codes(None, 0, 2, codes) == -1 and b"rdsp_engine_set_dcs_codes" in lib.rdsp_last_error()
    assert lib.rdsp_engine_set_dcs_squelch(None, 64, 1, 12, 6) == -1 and b"rdsp_engine_set_dcs_squelch" in lib.rdsp_last_error()
    assert lib.rdsp_engine_read_dcs(None, 0, None, 0, None, 0, None, 0, None) == -1
    for bad in (-1, 512, 1 << 20):
        assert lib.rdsp_dcs_codeword(bad) == 0 and b"rdsp_dcs_codeword" in lib.rdsp_last_error()
        with pytest.raises(rdsp.RdspError):
            dcs_codeword(bad)
    assert lib.rdsp_dcs_standard(None) == -1
    code, inv = C.c_int(-7), C.c_int(-7)
    assert lib.rdsp_dcs_code_of_word(W023, None, C.byref(inv)) == -1 and lib.rdsp_dcs_code_of_word(W023, C.byref(code), None) == -1
    for bad in (0, 0x800000, 0xFFFFFFFF, D.codeword(0o001), W023 ^ 1, 0x7FFFFF):
        assert D.code_of_word(bad & D.MASK) is None or bad > D.MASK
        assert lib.rdsp_dcs_code_of_word(bad, C.byref(code), C.byref(inv)) == -1 and b"rdsp_dcs_code_of_word" in lib.rdsp_last_error(), hex(bad)
        assert code.value == -7 and inv.value == -7
    with pytest.raises(rdsp.RdspError):
        dcs_code_of_word(W023 ^ 1)


def test_dcs_codewords_and_classes(rdsp):
    """rdsp_dcs_codeword(023) == 0x763813 and every code's word is the model's; the 104 standard codes are the model's list,
    ascending; their words lie in 104 distinct rotation classes, any two at least 7 bits apart over all rotations; the 512 codes
    fall into 177 classes, each with at most one standard code; the inverted word of every standard code is a rotation of
    another standard code's word (inverted 023 is normal 047).  rdsp_dcs_code_of_word, on every rotation of every standard word
    and of its inverse, names the code of the normal-polarity reading, as the model does"""
    from radiodsp_sdr_rx_amd.engine import dcs_code_of_word, dcs_codeword, standard_dcs_codes
    assert dcs_codeword(0o023) == 0x763813 == W023
    words = [dcs_codeword(c) for c in range(512)]
    assert words == [D.codeword(c) for c in range(512)]
    assert all(w & 0xFFF == 0x800 | c and w >> 12 == D.parity(0x800 | c) for c, w in enumerate(words))
    std = standard_dcs_codes()
    assert std.dtype == np.uint16 and tuple(int(c) for c in std) == D.STANDARD and len(std) == 104 and np.all(np.diff(std.astype(int)) > 0)
    assert std[0] == 0o023 and std[-1] == 0o754
    classes = {}
    for c, w in enumerate(words):
        classes.setdefault(D.canon(w), []).append(c)
    assert len(classes) == 177 and max(sum(c in D.STANDARD for c in v) for v in classes.values()) == 1
    std_class = {D.canon(words[c]): c for c in D.STANDARD}
    assert len(std_class) == 104
    sw = np.array([words[c] for c in D.STANDARD], np.uint32)
    rots = D.rotations(sw)                                                                   # [104, 23]
    dist = D.popcount(sw[:, None, None] ^ rots[None])                                        # [104, 104, 23]
    dist[np.arange(104), np.arange(104)] = 99
    assert dist.min() == 7
    for c in D.STANDARD:
        other = std_class.get(D.canon(words[c] ^ D.MASK))
        assert other is not None and other != c, oct(c)
    assert std_class[D.canon(W023 ^ D.MASK)] == 0o047
    for c in D.STANDARD:
        inv_reads = std_class[D.canon(words[c] ^ D.MASK)]
        for r in range(23):
            assert dcs_code_of_word(D.rot(words[c], r)) == (c, False) == D.code_of_word(D.rot(words[c], r)), (oct(c), r)
            assert dcs_code_of_word(D.rot(words[c] ^ D.MASK, r)) == (inv_reads, False), (oct(c), r)


def test_dcs_step_and_hit_bound(rdsp):
    """step = llround(134.4 32 2^32 / 44100) = 418861572, below 2^29 (at most one hypothesis ticks per decimated value), 10.254
    values a bit; on_hits is bounded by the bits of a window, K 128 134.4 / 44100 rounded down = K 1024 / 2625: 3 at K = 8, 24 at
    the default K = 64, 199 at K = 512, so the hits of a window fit the uint8 record; the defaults are within their bound"""
    assert D.STEP == 418861572 == round(134.4 * 32 * 2 ** 32 / 44100) < 2 ** 29
    assert abs(2 ** 32 / D.STEP - 10.254) < 1e-3
    for K in range(8, 513):
        assert D.max_hits(K) == int(np.floor(K * 128 * 134.4 / 44100.0 + 1e-9)), K
    assert (D.max_hits(8), D.max_hits(64), D.max_hits(512)) == (3, 24, 199)
    assert 1 <= D.DEFAULT_OFF <= D.DEFAULT_ON <= D.max_hits(D.DEFAULT_K)


def _crafted_rows(nb):
    """float32 [rows, nb * 128] with their codes: coded rows under voice noise (normal, inverted, read by ANY, no code set), rows
    of zeros, rows on the rails (+-1 drawn, and +1 throughout), a code that stops after 70 blocks, a code that changes there"""
    r = np.random.default_rng(29)
    z, n = np.zeros(nb * 128, F32), nb * 128
    rows = [D.demod_row(1, nb, W023, phase=3.3), D.demod_row(2, nb, W754 ^ D.MASK, 0.15, -0.1, phase=17.8), D.demod_row(3, nb, W023, phase=0.5),
            D.demod_row(4, nb, W023), z, z, r.choice(np.array([1.0, -1.0], F32), n), np.ones(n, F32),
            D.demod_row(5, nb, W023, 0.3, 0.0, 0.0, 0.0, 7.1, until=70 * 128), D.demod_row(6, nb, W023, 0.3, 0.05, 0.1, 750.0, 2.2, until=70 * 128, then=W754)]
    return np.stack(rows).astype(F32), [0o023, 0o754 | D.INVERTED, D.ANY, 0, 0o023, D.ANY, D.ANY, 0o023, D.ANY, 0o754]


@pytest.mark.parametrize("sanitize", [False, True])
def test_dcs_host_program(rdsp, tmp_path, sanitize):
    """tests/host/host_dcs_check.cpp, plain and under ASan + UBSan, a program of its own run on the CPU: on the crafted rows (a
    coded row, rows of zeros, rows on the rails, a code that stops, a code that changes), at K = 8 with max_err 1 and 0 and calls
    of 1, 2 and 3 blocks (which it holds to one long call itself), its step, settings, records and all 232 final words equal the
    model's.  The coded rows are found after 59 blocks and read back as 023 through code_of_word; the code that stops is found
    and then lost; the changed code is found after the change; zeros and rails never match; no code leaves zero words"""
    exe = str(tmp_path / ("host_dcs_check_san" if sanitize else "host_dcs_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_dcs_check.cpp"), "-o", exe])
    nb = 149
    rows, codes = _crafted_rows(nb)
    n = len(rows)
    fin, fout = str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")
    rows.tofile(fin)
    for K, err, on, off in ((8, 1, 2, 1), (8, 0, 3, 2)):
        m = D.Dcs(n, codes, K, err, on, off)
        dcs, hits, word = m.run(rows)
        for call_blocks in (1, 2, 3):
            out = subprocess.run([exe, fin, fout, str(K), str(err), str(on), str(off), str(n), str(nb), str(call_blocks)] + [str(v) for v in codes],
                                 capture_output=True, text=True, timeout=120)
            assert out.returncode == 0 and out.stdout.endswith("host_dcs_check OK\n"), out.stdout + out.stderr
            assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
            w = np.fromfile(fout, np.uint32)
            assert w[0] == D.STEP
            body = w[1:].reshape(n, 1 + 3 * nb + D.WORDS)
            assert np.array_equal(body[:, 0], m.sel), (K, call_blocks)
            assert np.array_equal(body[:, 1:1 + nb], dcs) and np.array_equal(body[:, 1 + nb:1 + 2 * nb], hits), (K, err, call_blocks)
            assert np.array_equal(body[:, 1 + 2 * nb:1 + 3 * nb], word), (K, err, call_blocks)
            assert np.array_equal(body[:, 1 + 3 * nb:], m.words()), (K, err, call_blocks, np.argwhere(body[:, 1 + 3 * nb:] != m.words())[:4])
        if err == 1:
            assert not dcs[:, :63].any() and dcs[0, 71:].all() and dcs[1, 71:].all() and dcs[2, 71:].all()     # 23 bits take 59 blocks
            assert word[0, -1] == D.canon(W023) and word[1, -1] == D.canon(W754 ^ D.MASK) and D.code_of_word(int(word[2, -1])) == (0o023, False)
            assert not m.words()[3].any() and not dcs[3].any()
            assert not hits[4:8].any() and not dcs[4:8].any() and m.words()[4:8].any(1).all()
            assert dcs[8, 64:72].all() and not dcs[8, -8:].any() and D.code_of_word(int(word[8, 71])) == (0o023, False)
            assert not dcs[9, :72].any() and dcs[9, -8:].all() and word[9, -1] == D.canon(W754)
    assert subprocess.run([exe, fin, fout, "7", "1", "2", "1", "1", "1", "1", "19"], capture_output=True).returncode == 2
    assert subprocess.run([exe, fin, fout, "8", "4", "2", "1", "1", "1", "1", "19"], capture_output=True).returncode == 2
    assert subprocess.run([exe, fin, fout, "8", "1", "4", "1", "1", "1", "1", "19"], capture_output=True).returncode == 2
    assert subprocess.run([exe, fin, fout, "8", "1", "2", "1", "1", "1", "1", "512"], capture_output=True).returncode == 2
    assert subprocess.run([exe, fin, fout, "8", "1", "2", "1", "1", "1", "1", "32768"], capture_output=True).returncode == 2


WINDOWS = 40


@functools.lru_cache(maxsize=None)
def _figure_rows():
    """the rows of the figures, 40 windows of 64 blocks each, built as engine_tone_model.demod_row builds its own: NRZ of a code at
    amplitude A, a DC offset of +-0.1, voice-band noise of rms 0.25, clipped to +-1, the 750 us de-emphasis"""
    nb = WINDOWS * 64
    r = np.random.default_rng(13)
    return {"023 A 0.15": D.demod_row(1, nb, W023, 0.15, 0.1, phase=5.4), "023 A 0.10": D.demod_row(1, nb, W023, 0.10, 0.1, phase=5.4),
            "754 DC -0.1": D.demod_row(1, nb, W754, 0.15, -0.1, phase=11.7), "voice": D.demod_row(1, nb, None, 0.0, 0.1),
            "023 clock +0.2 %": D.demod_row(1, nb, W023, 0.15, 0.1, phase=5.4, rate=D.BIT_RATE * 1.002),
            "idle": T.deemph(r.uniform(-1.0, 1.0, nb * 128).astype(F32), 750.0)}


def _windows(row, codes, K, max_err=D.DEFAULT_ERR, on_hits=D.DEFAULT_ON, off_hits=D.DEFAULT_OFF):
    """one detector per code on the same row -> (dcs, hits, word) at the end of every window, [len(codes), windows]"""
    m = D.Dcs(len(codes), list(codes), K, max_err, min(on_hits, D.max_hits(K)), min(off_hits, D.max_hits(K)))
    return tuple(v[:, K - 1::K] for v in m.run(np.broadcast_to(row, (len(codes), len(row)))))


def test_dcs_figures(rdsp):
    """the detector's figures on the float32 model, printed, over 40 windows of K = 64 (and 80 of K = 32, printed only).  Asserted
    at the defaults (K = 64, max_err 1, on_hits 16, off_hits 12): a detector set to the station's code (023 at A = 0.15 and 0.10
    with DC +0.1, 754 with DC -0.1) is open in every window from the second on; detectors set to 025 and to inverted 023 on the
    023 station, a detector set to 023 on voice without a code and on an idle discriminator (uniform +-1 behind the
    de-emphasis) never open; a station whose bit clock is 0.2 % fast stays open; RDSP_DCS_ANY reads 023 back through
    code_of_word in every window from the second on.

    Observed (seed 1): 25 hits a window from the second on for every matching detector and for ANY at K = 64 (the first window
    holds the 59 blocks the first 23 bits take: 3 hits), 0, 3, then 13 at K = 32; 0 always for the wrong code, the wrong polarity,
    voice without a code and the idle discriminator, at max_err 1 and 0 -- the figures of the float64 prototype, which allowed
    the idle row one hit a window at max_err 1"""
    rows = _figure_rows()
    own = {"023 A 0.15": 0o023, "023 A 0.10": 0o023, "754 DC -0.1": 0o754, "023 clock +0.2 %": 0o023}
    for name, code in own.items():
        dcs, hits, word = _windows(rows[name], (code, D.ANY), 64)
        d32, h32, _ = _windows(rows[name], (code,), 32)
        print(f"{name}: detector {code:03o}, K = 64: hits {hits[0, :4].tolist()} ... min {hits[0, 1:].min()} max {hits[0, 1:].max()} from the second window on; "
              f"ANY: {hits[1, :4].tolist()} ... min {hits[1, 1:].min()}; K = 32: {h32[0, :5].tolist()} ... min {h32[0, 2:].min()} from the third on")
        assert dcs[0, 1:].all() and dcs[1, 1:].all(), name
        assert all(D.code_of_word(int(w)) == (code, False) for w in word[1, 1:]) and np.all(word[0, 1:] == D.canon(D.codeword(code))), name
    for name, codes in (("023 A 0.15", (0o025, 0o023 | D.INVERTED)), ("voice", (0o023,)), ("idle", (0o023,))):
        for K in (64, 32):
            dcs, hits, word = _windows(rows[name], codes, K)
            print(f"{name}: detectors {[oct(c) for c in codes]}, K = {K}: at most {hits.max(1).tolist()} hits over {hits.shape[1]} windows")
            assert not dcs.any() and hits.shape[1] >= WINDOWS, (name, K)
            if name != "idle":
                assert not hits.any(), (name, K)
    for err in (1, 0):
        dcs, hits, word = _windows(rows["idle"], (0o023,), 64, err)
        print(f"idle, detector 023, K = 64, max_err {err}: at most {hits.max()} hits a window over {hits.shape[1]} windows")
        assert hits.max() <= (1 if err else 0)
