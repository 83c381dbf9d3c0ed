"""The POCSAG pager decoder of rdsp_engine_t without a GPU (include/rdsp.h "POCSAG pager decoder"; csrc/rdsp_pocsag.h,
csrc/rdsp_engine_pocsag_host.hip): the exports, every refusal that needs no device, the sync and idle words as codewords, the
syndrome table, every error pattern of weight <= 2 corrected and none of weight 3 accepted at fix <= 1, pocsag.py's round trips
(a message of exactly 80 codewords and one of 81 among them), tests/host/host_pocsag_check.cpp -- csrc/rdsp_pocsag.h as a
program of its own, plain and under ASan + UBSan, run directly -- against the model's words under every cut of 1 to 3 blocks,
and the decoder's figures on the float32 model, printed and asserted.  tests/test_engine_pocsag_gpu.py holds the kernel to the
same model."""
import itertools
import os
import subprocess

import numpy as np
import pytest

import engine_pocsag_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _P():
    from radiodsp_sdr_rx_amd import pocsag
    return pocsag


def test_pocsag_exports(rdsp):
    from radiodsp_sdr_rx_amd import engine, pocsag
    lib = rdsp.load()
    for name in ("enable_pocsag", "pocsag_enabled", "set_pocsag", "read_pocsag", "read_pocsag_messages", "pocsag_bch_table", "pocsag_codeword"):
        assert hasattr(lib, "rdsp_engine_" + name), name
    assert callable(engine.pocsag_bch_table) and callable(engine.pocsag_codeword)
    assert all(callable(getattr(pocsag, n)) for n in ("codeword", "address_word", "message_word", "batches", "bits", "numeric", "alpha", "transmit", "from_slot"))
    assert all(callable(getattr(engine.Engine, n)) for n in ("enable_pocsag", "set_pocsag", "read_pocsag", "read_pocsag_ring", "read_pocsag_messages"))
    assert isinstance(engine.Engine.pocsag_enabled, property)


def test_pocsag_refusals_without_a_device(rdsp):
    """no object: every entry point refuses.  The refusals that need an object are test_engine_pocsag_gpu's"""
    lib = rdsp.load()
    assert lib.rdsp_engine_enable_pocsag(None) == -1 and lib.rdsp_engine_pocsag_enabled(None) == 0
    assert lib.rdsp_engine_set_pocsag(None, 1200, 2, 3, 2, 1, 2) == -1 and b"rdsp_engine_set_pocsag" in lib.rdsp_last_error()
    assert lib.rdsp_engine_read_pocsag(None, 0, None, 0, None, 0, None, 0, None, 0, None, 0, None) == -1
    assert lib.rdsp_engine_read_pocsag_messages(None, 0, 1, None, None, None) == -1


def test_pocsag_codewords(rdsp):
    """the sync word and the idle word are the codewords of their own upper 21 bits; the library's, the model's and pocsag.py's
    codeword agree on drawn data, every codeword has syndrome 0 and even parity; the steps are llround(baud 2^32 4 / 44100) and
    below 2^31, which afsk_clock asks for"""
    from radiodsp_sdr_rx_amd.engine import pocsag_codeword
    P = _P()
    for w in (M.SYNC, M.IDLE):
        assert pocsag_codeword(w >> 11) == w == M.codeword(w >> 11) == P.codeword(w >> 11)
    assert P.SYNC == M.SYNC == 0x7CD215D8 and P.IDLE == M.IDLE == 0x7A89C197
    r = np.random.default_rng(1)
    for d in [0, 0x1FFFFF] + [int(v) for v in r.integers(0, 1 << 21, 200)]:
        w = pocsag_codeword(d)
        assert w == M.codeword(d) == P.codeword(d) and w >> 11 == d and M.syndrome(w) == 0 and M.popcount(w) % 2 == 0
    for baud, per in ((512, 21.533), (1200, 9.1875), (2400, 4.59375)):
        assert M.step_of(baud) == round(baud * 4 * 2 ** 32 / 44100.0) < 2 ** 31 and abs(2 ** 32 / M.step_of(baud) - per) < 1e-3
        assert M.WINDOWS[baud] <= per


def test_pocsag_syndrome_table(rdsp):
    """the 1024 entries: syndrome 0 is no error, 496 other syndromes have their pattern of weight 1 or 2 -- distinct patterns, each
    with the syndrome it stands under -- and the rest have none; the library's table is the model's"""
    from radiodsp_sdr_rx_amd.engine import pocsag_bch_table
    t = pocsag_bch_table()
    assert t.shape == (1024,) and np.array_equal(t, M.bch_table()) and t[0] == 0
    has = np.flatnonzero(t[1:] != 0xFFFF) + 1
    assert len(has) == 496 and len(set(int(t[s]) for s in has)) == 496
    for s in has:
        e = int(t[s])
        b1, b2, ne = e & 31, e >> 5 & 31, e >> 10
        assert 1 <= b1 <= 31 and ne == (2 if b2 else 1) and (b2 == 0 or b1 < b2 <= 31)
        assert M.syndrome(1 << b1 | (1 << b2 if b2 else 0)) == s


def test_pocsag_corrects_two_errors_and_accepts_no_three(rdsp):
    """on drawn codewords, address and message words, through the library's table: every pattern of weight <= 2 over the 32 bits
    (529 of them) is corrected to the codeword with ne = the weight; accepted iff ne <= fix of its kind.  No pattern of weight 3
    (4960) is accepted at fix <= 1: the extended code's distance is 6, so a word three bits from one codeword is at least three
    from every other"""
    from radiodsp_sdr_rx_amd.engine import pocsag_bch_table
    M.TABLE[:] = [int(v) for v in pocsag_bch_table()]
    r = np.random.default_rng(2)
    cws = [M.codeword(int(d)) for d in r.integers(0, 1 << 21, 6)] + [M.SYNC, M.IDLE]
    assert any(c >> 31 for c in cws) and any(not c >> 31 for c in cws)
    patterns = [0] + [1 << a for a in range(32)] + [1 << a | 1 << b for a, b in itertools.combinations(range(32), 2)]
    assert len(patterns) == 529
    for c in cws:
        for e in patterns:
            ok, fixed, ne = M.correct(c ^ e, 2, 2)
            assert ok and fixed == c and ne == M.popcount(e), (hex(c), hex(e))
            for fix in (0, 1):
                assert M.correct(c ^ e, fix, fix)[0] == (M.popcount(e) <= fix)
            assert M.correct(c ^ e, 0, 2)[0] == (M.popcount(e) <= (2 if c >> 31 else 0))
    for c in cws[:2]:
        for a, b, d in itertools.combinations(range(32), 3):
            assert not M.correct(c ^ (1 << a | 1 << b | 1 << d), 1, 1)[0]


def _row(words, baud, nb, preamble=64, **kw):
    """a transmission as a tap row of nb blocks: float64"""
    P = _P()
    kw.setdefault("lead", 100)
    x = P.transmit(P.bits(words, preamble), baud, total=nb * 128, **kw)
    return x


def _blocks(words, baud, preamble=64, lead=100, tail=4):
    return int(np.ceil((lead + (preamble + 32 * len(words)) * 44100.0 / baud) / 128.0)) + tail


def _read(m, c=0):
    """channel c's messages as (address, function, words) with their flags"""
    return [((a, f, w), fl) for _, a, f, w, fl, _ in m.messages(c)]


def test_pocsag_round_trips():
    """pocsag.py: numeric and alphanumeric text through words and back; a batch puts every address word into its frame and fills
    with idle words; and through transmit() and the model at 2400 baud: a numeric page, a tone-only page and alphanumeric
    messages of exactly 80 codewords, read whole, and of 81, read as its first 80 and flagged truncated"""
    P = _P()
    assert P.numeric(P.numeric_words("0123456789*U -)(")) == "0123456789*U -)(" + " " * 4
    assert P.numeric_words("12345") == [int("1000" "0100" "1100" "0010" "1010", 2)]
    text = "The quick brown fox @ 12:45 ~{}"
    assert P.alpha(P.alpha_words(text)) == text and len(P.alpha_words("abc")) == 2
    assert P.alpha_words("a") == [int("1000011" + "0" * 13, 2)]
    for address in (0, 5, 1234567, (1 << 21) - 1):
        words = P.batches([(address, 2, [1, 2, 3])])
        assert words[0] == P.SYNC and len(words) % 17 == 0
        at = words.index(P.address_word(address, 2))
        assert (at - 1) % 17 == 2 * (address & 7) and all(w == P.IDLE for w in words[1:at])
    with pytest.raises(ValueError):
        P.address_word(1 << 21)
    t80, t81 = "x" * 227 + "Z", "y" * 228 + "Z"
    assert len(P.alpha_words(t80)) == 80 and len(P.alpha_words(t81)) == 81
    sent = [(1000, 0, P.numeric_words("555 0199")), (1003, 1, []), (2004, 3, P.alpha_words(t80)), (77, 3, P.alpha_words(t81))]
    words = P.batches(sent)
    nb = _blocks(words, 2400)
    m = M.Pocsag(1, 2400)
    sync, new, bad, lvl, dc = m.run(_row(words, 2400, nb).astype(F32)[None])
    got = _read(m)
    assert [g for g, _ in got[:3]] == sent[:3] and [fl for _, fl in got] == [0, 0, 0, M.FLAG_TRUNCATED]
    assert got[3][0] == (77, 3, P.alpha_words(t81)[:80]) and new.sum() == 4 and not bad.any()
    assert P.numeric(got[0][0][2]) == "555 0199  " and P.alpha(got[2][0][2]) == t80 and P.alpha(got[3][0][2]) == t81[:228]
    msg = P.from_slot(m.ring()[1][0, 3])
    assert msg.address == 77 and msg.function == 3 and msg.flags == 2 and len(msg.words) == 80 and msg.errors == [0] * 80 and msg.corrected == 0


def _flip(word, *at):
    for b in at:
        word ^= 1 << b
    return word


def host_rows(baud):
    """-> (rows float32 [11, nb 128], what each reads under invert 2 / 0 / 1 at the defaults else: a list of ((address, function,
    words), flags) or None for "whatever the model says").  On the rails; all zeros; one message, inverted; the same as sent; a
    sync word with 2 errors; with 3 errors (not found: nothing is read); a message across two batches whose second sync word is
    lost (cut); six messages through the four slots; a tone-only page; a message across two batches; a message with a corrected
    and an uncorrectable word inside"""
    P = _P()
    r = np.random.default_rng(baud)
    one = [(1234561, 1, [int(v) for v in r.integers(0, 1 << 20, 3)])]
    w1 = P.batches(one)
    two = [(4007, 3, [int(v) for v in r.integers(0, 1 << 20, 6)])]                          # frame 7: five words fall into the second batch
    w2 = P.batches(two)
    assert len(w2) == 34
    six = [(800 + 9 * k, k % 4, [int(r.integers(0, 1 << 20))] if k % 2 else []) for k in range(6)]
    assert sorted((a & 7) for a, _, _ in six) == [0, 1, 2, 3, 4, 5]
    six.sort(key=lambda m: m[0] & 7)
    w6 = P.batches(six)
    assert len(w6) == 17
    tone = [(93, 2, [])]
    s2, s3, lost = list(w1), list(w1), list(w2)
    s2[0], s3[0] = _flip(P.SYNC, 3, 30), _flip(P.SYNC, 0, 17, 25)
    lost[17] = 0x12345678
    hurt = [(52, 0, [int(v) for v in r.integers(0, 1 << 20, 4)])]
    wh = P.batches(hurt)
    at = wh.index(P.address_word(52, 0))
    wh[at + 2] = _flip(wh[at + 2], 5, 20)                                                     # two errors: corrected (fix_data 2)
    wh[at + 3] = _flip(wh[at + 3], 1, 12, 25)                                                 # three errors: never accepted
    nb = _blocks(w2, baud)
    n = nb * 128
    rows = np.stack([r.choice(np.array([1.0, -1.0]), n), np.zeros(n), _row(w1, baud, nb, invert=True), _row(w1, baud, nb, ppm=80.0), _row(s2, baud, nb, lead=7),
                     _row(s3, baud, nb), _row(lost, baud, nb, ppm=-60.0), _row(w6, baud, nb, lead=133, amp=0.3), _row(P.batches(tone), baud, nb, dc=0.05), _row(w2, baud, nb, lead=61), _row(wh, baud, nb)]).astype(F32)
    cut_words = two[0][2][:1]                                                                 # frame 7: address, one word, then the lost sync
    both = {"inv": [(one[0], 0)], "plain": [(one[0], 0)], "s2": [(one[0], 0)], "s3": [], "lost": [((4007, 3, cut_words), M.FLAG_CUT)],
            "six": [(m, 0) for m in six[2:]], "tone": [(tone[0], 0)], "two": [(two[0], 0)]}
    want = {2: [None, [], both["inv"], both["plain"], both["s2"], both["s3"], both["lost"], both["six"], both["tone"], both["two"], None],
            0: [None, [], [], both["plain"], both["s2"], both["s3"], both["lost"], both["six"], both["tone"], both["two"], None],
            1: [None, [], both["inv"], [], [], [], [], [], [], [], None]}
    return rows, want, hurt[0]


@pytest.mark.parametrize("sanitize", [False, True])
def test_pocsag_host_program(rdsp, tmp_path, sanitize):
    """tests/host/host_pocsag_check.cpp, plain and under ASan + UBSan, a program of its own run on the CPU: on the rows of
    host_rows at 2400 baud under invert 2, 0 and 1 and a setting away from the defaults, and at 1200 and 512 baud at the
    defaults, each under 27 cuts into calls of 1 to 3 blocks (which it holds to one long call itself), its steps, records and
    final words equal the model's.  The rows read what their construction says: the inverted transmission is read under
    invert 1 and 2 only (polarity 1), the others under 0 and 2 only; two errors in the sync word are found, three are not; the
    lost second sync word closes the message with `cut`; six messages leave the last four with n_msgs 6; the message with a
    hurt word holds a corrected one (ne 2) and flags its uncorrectable one"""
    exe = str(tmp_path / ("host_pocsag_check_san" if sanitize else "host_pocsag_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_pocsag_check.cpp"), "-o", exe])
    fin, fout = str(tmp_path / "rows.bin"), str(tmp_path / "out.bin")
    default = (2, 3, 2, 1, 2)
    for baud, settings in ((2400, (default, (0, 3, 2, 1, 2), (1, 3, 2, 1, 2), (2, 1, 3, 2, 0))), (1200, (default,)), (512, (default,))):
        x, want, hurt = host_rows(baud)
        n, nb = x.shape[0], x.shape[1] // 128
        x.tofile(fin)
        for st in settings:
            m = M.Pocsag(n, baud, **dict(zip(("invert", "pull", "sync_errs", "fix_addr", "fix_data"), st)))
            sync, new, bad, lvl, dc = m.run(x)
            out = subprocess.run([exe, fin, fout, str(baud)] + [str(v) for v in st] + [str(n), str(nb)], capture_output=True, text=True, timeout=600)
            assert out.returncode == 0 and out.stdout.endswith("host_pocsag_check OK\n"), out.stdout + out.stderr
            assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
            w = np.fromfile(fout, np.uint32)
            assert w[0] == bits(M.lscale_of(M.WINDOWS[baud])) and w[1] == M.step_of(baud)
            body = w[2:].reshape(n, 5 * nb + M.WORDS)
            assert np.array_equal(body[:, :nb], sync) and np.array_equal(body[:, nb:2 * nb], new) and np.array_equal(body[:, 2 * nb:3 * nb], bad), (baud, st)
            assert np.array_equal(body[:, 3 * nb:4 * nb], bits(lvl)) and np.array_equal(body[:, 4 * nb:5 * nb], bits(dc)), (baud, st)
            assert np.array_equal(body[:, 5 * nb:], m.words()), (baud, st)
            wd = m.words()
            assert (wd[:, M.TBLOCKS] == nb).all() and (wd[:, M.BAUD] == baud).all() and not wd[:, M.HIST_ + 19].any() and not wd[:, M.MSG:M.MSG + 4].any()
            if st[1:] != default[1:]:
                continue
            for c, msgs in enumerate(want[st[0]]):
                if msgs is not None:
                    assert _read(m, c) == msgs, (baud, st, c)
            assert not lvl[1].any() and not sync[1].any() and lvl[0].all() and np.abs(dc[8, -20:] - F32(0.05)).max() < 1e-6
            if st[0] != 1:
                assert wd[7, M.NMSGS] == 6 and new[7].sum() == 6 and wd[6, M.NMSGS] == 1 and wd[5, M.NMSGS] == 0 and not sync[5].any()
                assert [p for *_, p in m.messages(3)] == [0]
                (t, a, f, words, fl, pol), = m.messages(10)
                slot = m.ring()[1][10, 0]
                assert (a, f) == hurt[:2] and words[:2] == hurt[2][:2] and len(words) == 4 and slot[4 + 1] >> 24 == 2
                assert fl == M.FLAG_UNCORRECTABLE and slot[4 + 2] >> 31 and slot[3] == 2 | 1 << 16 and wd[10, M.NBAD] == 1 and bad[10].sum() == 1
            if st[0] != 0:
                assert [p for *_, p in m.messages(2)] == [1]
    for bad_args in (["0", "2", "3", "2", "1", "2"], ["600", "2", "3", "2", "1", "2"], ["1200", "3", "3", "2", "1", "2"], ["1200", "2", "0", "2", "1", "2"],
                     ["1200", "2", "5", "2", "1", "2"], ["1200", "2", "3", "4", "1", "2"], ["1200", "2", "3", "2", "3", "2"], ["1200", "2", "3", "2", "1", "-1"]):
        assert subprocess.run([exe, fin, fout] + bad_args + ["1", "1"], capture_output=True).returncode == 2, bad_args


# ---- the figures ----

def _transmissions(baud, seed):
    """the sketch's set-up: 10 transmissions, each a preamble of 576 bits, one alphanumeric message of 5 to 39 characters and one
    tone-only page, the baud rate off by a drawn +-100 ppm, DC of 0.05, amplitude 0.6, a batch's length of nothing (noise, once
    it is added) behind -> (rows float64 [10, t] without noise, per row the two messages sent)"""
    P = _P()
    r = np.random.default_rng(seed)
    rows, sent = [], []
    for k in range(10):
        text = "".join(chr(int(c)) for c in r.integers(32, 127, int(r.integers(5, 40))))
        msgs = [(int(r.integers(0, 1 << 21)), 3, P.alpha_words(text)), (int(r.integers(0, 1 << 21)), int(r.integers(0, 4)), [])]
        rows.append((P.bits(P.batches(msgs), 576), float(r.uniform(-100, 100)), int(r.integers(0, 400))))
        sent.append(msgs)
    t = 128 * int(np.ceil(max(lead + (len(b) + 17 * 32) * 44100.0 / baud for b, _, lead in rows) / 128.0))
    return np.stack([P.transmit(b, baud, 0.6, ppm, lead, t, dc=0.05) for b, ppm, lead in rows]), sent


def _count(m, sent):
    """-> (sent messages read right, messages emitted that were not sent, sent messages emitted more than once)"""
    good = wrong = twice = 0
    for c, msgs in enumerate(sent):
        got = [(a, f, w) for _, a, f, w, _, _ in m.log[c]]
        assert len(got) == m.words()[c, M.NMSGS]
        good += sum(1 for s in msgs if s in got)
        wrong += sum(1 for g in got if g not in msgs)
        twice += sum(1 for s in msgs if got.count(s) > 1)
    return good, wrong, twice


def test_pocsag_figures():
    """the decoder's figures on the float32 model, printed and asserted.  The table of the issue's float64 sketch -- white noise of
    rms sigma on a tap of amplitude 0.6, clipped at +-1, DC 0.05, 20 messages a point, "read right + emitted wrong" -- for pull 2
    and 3 and fix_addr 1 and 2 at W = 20, 8 and 4, and W = 9 / 6 at 1200 baud and 5 / 3 at 2400 baud beside them, through the
    model's window argument; every point of one baud and sigma sees the same noise.  Asserted: every message is read at sigma <=
    0.5 at each baud at the defaults; no row of any point emits a sent message twice; 60 rows of one second of clipped noise of
    rms 1.0 emit nothing at any baud (each row is a detector of its own that starts from zeros).  White noise on the tap is not
    a discriminator's noise, whose spectrum rises with frequency: the figures compare settings, they are no sensitivity"""
    table = {512: ((0.8, 1.2, 1.6, 2.0), ((20, 2, 1), (20, 3, 1), (20, 2, 2))),
             1200: ((0.8, 1.2, 1.6), ((8, 2, 1), (8, 3, 1), (8, 2, 2), (9, 3, 1), (6, 3, 1))),
             2400: ((0.8, 1.2), ((4, 2, 1), (4, 3, 1), (4, 2, 2), (5, 3, 1), (3, 3, 1)))}
    for baud, (sigmas, settings) in table.items():
        clean, sent = _transmissions(baud, 100 + baud)
        noisy = lambda sigma: np.clip(clean + sigma * np.random.default_rng(int(100 * sigma) + baud).standard_normal(clean.shape), -1.0, 1.0).astype(F32)
        for sigma in (0.3, 0.5):
            m = M.Pocsag(10, baud)
            m.run(noisy(sigma))
            good, wrong, twice = _count(m, sent)
            print(f"{baud}: defaults, sigma {sigma}: {good}+{wrong}")
            assert good == 20 and twice == 0, (baud, sigma, good)
        xs = {sigma: noisy(sigma) for sigma in sigmas}
        for W, pull, fix_addr in settings:
            cells = []
            for sigma in sigmas:
                m = M.Pocsag(10, baud, W, pull=pull, fix_addr=fix_addr)
                m.run(xs[sigma])
                good, wrong, twice = _count(m, sent)
                assert twice == 0, (baud, W, pull, fix_addr, sigma)
                cells.append(f"sigma {sigma}: {good}+{wrong}")
            print(f"{baud}: W {W}, pull {pull}, fix_addr {fix_addr}: " + ", ".join(cells))
    sec = 345 * 128
    noise = np.clip(np.random.default_rng(9).standard_normal((60, sec)), -1.0, 1.0).astype(F32)
    for baud in (512, 1200, 2400):
        m = M.Pocsag(60, baud)
        sync, new, bad, lvl, dc = m.run(noise)
        print(f"{baud}: 60 rows of {sec / 44100.0:.2f} s of clipped noise: {int(m.words()[:, M.NMSGS].sum())} messages, in sync {sync.mean():.4f} of the blocks, "
              f"{int(m.words()[:, M.NBAD].sum())} uncorrectable words, lvl {float(lvl.mean()):.3f}")
        assert not m.words()[:, M.NMSGS].any() and not new.any(), baud
