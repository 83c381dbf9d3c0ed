"""The signal meter, squelch and active-receiver list of rdsp_engine_t (include/rdsp.h "signal meter and squelch";
csrc/rdsp_meter.h, csrc/rdsp_engine_meter.hip).

`-m "not gpu"`: tests/engine_meter_model.py, the numpy restatement, against tests/host/host_meter_check.cpp, which compiles
csrc/rdsp_meter.h as the kernel is compiled (-ffp-contract=off) -- plain and under ASan + UBSan, a program of its own run
directly -- bit for bit; and the gate model through every transition.
`-m gpu`: the engine against the restatement applied to the rows rdsp_engine_read_demod returns, bit for bit: levels, peaks,
gates, the gated audio, the active list; independent of the call split, of groups and regroupings, of the path the rows came
by, and carried by a state blob -- also one with both optional parts, tuning phases and meter words, between engines on two
sources at D = 2.  Engines of 97 channels (a ragged last workgroup of the meter's four channels) and max_blocks 64 unless a
test says otherwise."""
import functools
import os
import subprocess

import numpy as np
import pytest

import engine_meter_model as M
from engine_meter_model import F32, Meter, Squelch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NCH, MAXB = 97, 64
STATE_CH_BYTES = (96 + 512 + 512 + 3 * 384 + 256 + 64) * 4    # a channel's words in a blob, as before the meter existed


def same_bits(a, b):
    """bit for bit, but any NaN equals any NaN (a NaN's payload is no part of the definition)"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


# ---- CPU: the restatement against the header ------------------------------------------------------------------------------
def _host_exe(tmp_path, sanitize):
    exe = str(tmp_path / ("host_meter_check_san" if sanitize else "host_meter_check"))
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_meter_check.cpp"), "-o", exe])
    return exe


def _host_run(exe, tmp_path, rows, s):
    """rows float32 [n, n_blocks * 128] through the header, every row from a fresh state -> ms, pk, level, open, hang [n, n_blocks]"""
    rows = np.ascontiguousarray(rows, F32)
    n, nb = rows.shape[0], rows.shape[1] // 128
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    rows.tofile(fin)
    args = [exe, fin, fout, str(n), str(nb), repr(float(s.attack)), repr(float(s.decay)), str(int(s.on)), repr(float(s.open_ms)),
            repr(float(s.close_ms)), str(s.hang_blocks)]
    out = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "host_meter_check OK" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
    w = np.fromfile(fout, np.uint32).reshape(n, nb, 5)
    return w[..., 0].view(F32), w[..., 1].view(F32), w[..., 2].view(F32), w[..., 3].astype(np.int32), w[..., 4].astype(np.int32)


def _drawn_rows(nb=12):
    """rows of nb blocks: zeros; denormals, and values whose squares are denormal; +-1; values near 1e19, whose squares
    overflow; noise over six decades, where a reordered sum rounds differently; a quiet row with one loud sample per block"""
    r = np.random.default_rng(11)
    n = nb * 128
    rows = [np.zeros(n), r.standard_normal(n) * 1e-40, r.standard_normal(n) * 3e-20, r.standard_normal(n) * 3e-21, r.choice([-1.0, 1.0], n),
            r.standard_normal(n) * 1e19, np.where(r.random(n) < 0.05, 3e19, 1e-3) * r.choice([-1.0, 1.0], n)]
    rows += [r.standard_normal(n) * 10.0 ** r.uniform(-3, 3, n) for _ in range(6)]
    rows += [r.standard_normal(n) * 0.1 * np.repeat(r.choice([1e-3, 1.0], nb), 128) for _ in range(4)]
    spike = r.standard_normal(n) * 1e-4
    spike[r.integers(0, 128, nb) + 128 * np.arange(nb)] = 0.9
    return np.stack(rows + [spike]).astype(F32)


@pytest.mark.parametrize("sanitize", [False, True])
def test_meter_model_is_the_header(tmp_path, sanitize):
    """drawn rows through csrc/rdsp_meter.h (the host program) and through the numpy restatement: mean squares, peaks, levels,
    gates and hang counters bit for bit, with the squelch off, with the default coefficients and with others.  The rows
    include some on which a plain left-to-right sum rounds differently from the tree: the tree is what is compared."""
    rows = _drawn_rows()
    with np.errstate(all="ignore"):
        sq = rows.reshape(len(rows), -1, 128) ** 2
        tree, plain = M.tree_sum(sq), M.left_to_right_sum(sq)
    finite = np.isfinite(tree) & np.isfinite(plain)
    assert np.any(tree[finite] != plain[finite])                                       # the order matters on these rows
    tiny = lambda v: np.any((v != 0) & (np.abs(v) < 1.17e-38))
    assert np.any(np.isinf(tree)) and tiny(rows) and tiny(sq) and tiny(tree) and np.any(tree == 128.0)   # overflow, denormals at every step, +-1
    exe = _host_exe(tmp_path, sanitize)
    for s in (Squelch(), Squelch(1e-4, 1e-6, 2), Squelch(0.3, 0.0, 0, attack=1.0, decay=0.3), Squelch(1e-7, 1e-7, 65535, attack=0.01, decay=1.0)):
        ms, pk, level, gate, hang = _host_run(exe, tmp_path, rows, s)
        m = Meter(len(rows))
        want_level, want_pk, want_gate = m.run(rows, s)
        want_ms = M.measure(rows)[0]
        assert same_bits(ms, want_ms) and same_bits(pk, want_pk) and same_bits(level, want_level)
        assert np.array_equal(gate, want_gate) and np.array_equal(hang, m.hangs)
        assert same_bits(M.level_step(np.zeros(len(rows), F32), want_ms[:, 0], s.attack, s.decay), level[:, 0])


def test_meter_setters_limits_refuse(tmp_path):
    """the host program runs the header's limit checks on start (it fails if one is wrong) and exits with 2 on a refused setting"""
    exe = _host_exe(tmp_path, False)
    np.zeros(128, F32).tofile(str(tmp_path / "in.bin"))
    for bad in (["0", "0.5", "0", "0", "0", "0"], ["0.5", "nan", "0", "0", "0", "0"], ["0.5", "0.5", "1", "0.1", "0.2", "0"],
                ["0.5", "0.5", "1", "inf", "0.2", "0"], ["0.5", "0.5", "1", "0.2", "0.1", "65536"], ["0.5", "0.5", "1", "0.2", "-0.1", "3"]):
        rc = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), "1", "1"] + bad, capture_output=True, timeout=60).returncode
        assert rc == 2, bad


def test_gate_model_walks_every_transition(tmp_path):
    """blocks of constant magnitude (their mean square is exactly the magnitude's square) in drawn bursts and silences: the
    restatement's gate against the header's, and the sequence holds every transition: the gate opening from closed, a hang
    re-armed while it ran, a hang that ran out, and the gate closing"""
    r = np.random.default_rng(5)
    nb, n = 96, 6
    amp = np.zeros((n, nb))
    for c in range(n):
        b = int(r.integers(1, 4))
        while b < nb:
            loud, quiet = int(r.integers(2, 6)), int(r.choice([3, 5, 6, 7, 14, 18]))
            amp[c, b:b + loud] = r.uniform(0.3, 0.6)
            b += loud + quiet
    rows = (np.repeat(amp, 128, 1) * r.choice([-1.0, 1.0], (n, nb * 128))).astype(F32)
    ms = M.measure(rows)[0]
    assert np.array_equal(ms, (amp.astype(F32) ** 2).astype(F32))
    s = Squelch(0.05, 0.01, 4, attack=0.5, decay=0.5)
    m = Meter(n)
    level, _, gate = m.run(rows, s)
    seen = M.transitions(gate, m.cases, m.hangs)
    assert all(seen.values()), seen
    assert set(np.unique(m.cases)) == {1, 2, 3, 4}
    _, _, host_level, host_gate, host_hang = _host_run(_host_exe(tmp_path, False), tmp_path, rows, s)
    assert same_bits(host_level, level) and np.array_equal(host_gate, gate) and np.array_equal(host_hang, m.hangs)


def test_db_helpers():
    from radiodsp_sdr_rx_amd.engine import db_of_ms, ms_of_db
    assert ms_of_db(0.0) == 0.5 and abs(ms_of_db(-20.0) - 0.005) < 1e-15 and db_of_ms(0.5) == 0.0
    for db in (-90.0, -37.5, -3.0, 6.0):
        assert abs(db_of_ms(ms_of_db(db)) - db) < 1e-9
    assert db_of_ms(0.0) == -np.inf


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def _engine(n=NCH, max_blocks=MAXB, meter=True):
    from radiodsp_sdr_rx_amd.engine import Engine
    import oracle_lib
    e = Engine(n, max_blocks_per_call=max_blocks, tables=oracle_lib.engine_tables())
    e.sketch_setup()
    if meter:
        e.enable_meter()
    return e


def _bursts(seed, n, nb, quiet=(2, 3, 9, 10, 12), silent=()):
    """int16 [n, nb * 128, 2]: per channel a tone inside the LSB passband keyed in drawn bursts (2 ... 5 blocks loud, then a
    drawn count of quiet blocks) over weak noise; the channels of `silent` are all zero"""
    r = np.random.default_rng(seed)
    t = np.arange(nb * 128)
    x = np.zeros((n, nb * 128, 2), np.int16)
    for c in range(n):
        if c in silent:
            continue
        amp = np.full(nb, 0.0005)
        b = int(r.integers(0, 4))
        while b < nb:
            loud = int(r.integers(2, 6))
            amp[b:b + loud] = r.uniform(0.1, 0.4)
            b += loud + int(r.choice(quiet))
        z = np.repeat(amp, 128) * np.exp(2j * np.pi * r.uniform(6200, 7800) / 44100.0 * t + 1j * r.uniform(0, 6))
        z += 0.0003 * (r.standard_normal(len(t)) + 1j * r.standard_normal(len(t)))
        x[c, :, 0], x[c, :, 1] = np.round(z.real * 32767), np.round(z.imag * 32767)
    return x


class _Run:
    """a stream through an engine in calls of `split` blocks; after every call the audio and -- of an engine with the meter --
    the records, the demodulated rows and the active list are read back"""

    def __init__(self, eng, meter=True):
        self.eng, self.meter = eng, meter
        self.audio, self.level, self.peak, self.gate, self.demod, self.active = [], [], [], [], [], []

    def play(self, x, split, before=None):
        """x int16 [n, nb * 128, 2]; before(block): called in front of the call that starts at `block`"""
        import torch
        nb = x.shape[1] // 128
        for a in range(0, nb, split):
            b = min(nb, a + split)
            if before is not None:
                before(a)
            y = self.eng.update(torch.from_numpy(np.ascontiguousarray(x[:, a * 128:b * 128])).cuda()).cpu().numpy()
            assert np.array_equal(y[..., 0], y[..., 1])
            self.audio.append(y[..., 0])
            self.demod.append(self.eng.read_demod(b - a).cpu().numpy())
            if self.meter:
                lv, pk, g = (v.cpu().numpy() for v in self.eng.read_meter(b - a))
                self.level.append(lv); self.peak.append(pk); self.gate.append(g)
                lst, cnt = self.eng.active()
                lst = lst.cpu().numpy()
                assert cnt == len(lst) and np.array_equal(lst, np.flatnonzero(g.any(1)))   # ascending, the call's open channels
                self.active.append(lst)
        return self

    def cat(self):
        """-> audio [n, t], demod [n, t], level, peak, gate [n, nb]"""
        c = lambda v: np.concatenate(v, 1) if v else None
        return c(self.audio), c(self.demod), c(self.level), c(self.peak), c(self.gate)


def _thresholds(level):
    """open and close thresholds from the model's levels of a bursty stream: between the loud and the quiet levels"""
    top = float(np.median(level.max(1)))
    return F32(0.2 * top), F32(0.02 * top)


@pytest.mark.gpu
def test_gpu_meter_arithmetic(rdsp):
    """three cases of tests/golden/engine_kat.npz -- lsb_sketch (SSB: the Hilbert kernel writes the rows), am and sam (the front
    kernel does) -- as three groups of one 97-channel engine, 32 blocks in calls of 16: levels, peaks and get_meter equal the
    restatement applied to read_demod's rows, bit for bit, and the squelch being off the audio is the fixture's"""
    import json
    kat = np.load(os.path.join(HERE, "golden", "engine_kat.npz"))
    names, first, nb = ["lsb_sketch", "am", "sam"], [0, 31, 66], 32
    ends = first[1:] + [NCH]
    x = np.concatenate([np.repeat(kat[n + "_iq"][None, :nb * 128], e - f, 0) for n, f, e in zip(names, first, ends)])
    eng = _engine()
    eng.set_groups(first)
    for g, n in enumerate(names):
        eng.select_group(g)
        for c in json.loads(str(kat[n + "_calls"])):
            assert c[0] == 0
            getattr(eng, c[1])(*c[2:])
    eng.select_group(-1)
    assert eng.meter_enabled() and not np.any(eng.meter())
    run = _Run(eng).play(x, 16)
    audio, demod, level, peak, gate = run.cat()
    m = Meter(NCH)
    want_level, want_peak, want_gate = m.run(demod, Squelch())
    assert np.all(want_level[:, -1] > 0) and len({want_level[f, -1] for f in first}) == 3
    assert same_bits(level, want_level) and same_bits(peak, want_peak) and np.array_equal(gate, want_gate) and np.all(gate == 1)
    assert same_bits(eng.meter(), m.scalars())
    for n, f, e in zip(names, first, ends):
        for c in range(f, e):
            assert np.array_equal(audio[c], kat[n + "_out"][:nb * 128]), (n, c)
    assert all(np.array_equal(a, np.arange(NCH)) for a in run.active)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lsb_sketch", "am", "sam"])
def test_gpu_read_demod_is_the_demod_tap(rdsp, name):
    """read_demod's rows against tap "demod" of the CPU restatement of the image's engine on the same input, bit for bit"""
    import json
    import oracle_lib
    kat = np.load(os.path.join(HERE, "golden", "engine_kat.npz"))
    nb = 32
    iq, calls = kat[name + "_iq"][:nb * 128], json.loads(str(kat[name + "_calls"]))
    o = oracle_lib.OracleEngine(taps=True)
    o.run(iq, calls)
    want = np.concatenate([t[0] for t in o.taps["demod"]])
    eng = _engine(3, 16, meter=False)
    for c in calls:
        getattr(eng, c[1])(*c[2:])
    got = _Run(eng, meter=False).play(np.stack([iq, iq[::-1].copy(), iq]), 16).cat()[1]
    assert same_bits(got[0], want) and same_bits(got[2], want), (name, int(np.argmax(got[0].view(np.uint32) != want.view(np.uint32))))


@pytest.mark.gpu
def test_gpu_meter_call_split(rdsp):
    """a 64-block stream of keyed tones as one call, as calls of 7 blocks and as calls of 1 block, the squelch on: levels, peaks,
    gates, audio and the union of the calls' active lists are identical (and the restatement's); with the squelch off the audio
    is that of an engine that never enabled the meter, bit for bit"""
    x = _bursts(21, NCH, 64)
    plain = _Run(_engine(meter=False), meter=False).play(x, 64).cat()
    free = _engine()
    free.set_meter(0.5, 0.5)
    off = _Run(free).play(x, 64).cat()
    assert np.array_equal(off[0], plain[0]) and same_bits(off[1], plain[1]) and np.all(off[4] == 1)
    m = Meter(NCH)
    open_ms, close_ms = _thresholds(m.run(plain[1], Squelch(attack=0.5, decay=0.5))[0])
    s = Squelch(open_ms, close_ms, 2, attack=0.5, decay=0.5)
    m = Meter(NCH)
    want_level, want_peak, want_gate = m.run(plain[1], s)
    assert all(M.transitions(want_gate, m.cases, m.hangs).values())
    for split in (64, 7, 1):
        eng = _engine()
        eng.set_meter(0.5, 0.5)
        eng.set_squelch(open_ms, close_ms, 2)
        run = _Run(eng).play(x, split)
        audio, demod, level, peak, gate = run.cat()
        assert same_bits(demod, plain[1]), split
        assert same_bits(level, want_level) and same_bits(peak, want_peak) and np.array_equal(gate, want_gate), split
        assert np.array_equal(audio, M.gated(plain[0], want_gate)), split
        assert np.array_equal(np.unique(np.concatenate(run.active)), np.flatnonzero(want_gate.any(1))), split
        assert same_bits(eng.meter(), m.scalars()), split
        eng.close()


@pytest.mark.gpu
def test_gpu_squelch(rdsp):
    """keyed tones and silences, thresholds between the model's loud and quiet levels, a hang of 3 blocks: the gates equal the
    model's, which contain the gate opening, closing, a hang running out and a hang re-armed; a closed block is 128 zero words
    on both outputs, an open block is the meterless engine's; rows of the output further apart than the call is long and not
    16-byte aligned take the word stores"""
    import torch
    x = _bursts(22, NCH, 64, silent=(3, 50))
    plain = _Run(_engine(meter=False), meter=False).play(x, 64).cat()
    m = Meter(NCH)
    open_ms, close_ms = _thresholds(m.run(plain[1], Squelch(attack=0.5, decay=0.5))[0])
    s = Squelch(open_ms, close_ms, 3, attack=0.5, decay=0.5)
    m = Meter(NCH)
    want_level, _, want_gate = m.run(plain[1], s)
    seen = M.transitions(want_gate, m.cases, m.hangs)
    assert all(seen.values()), seen
    assert not want_gate[3].any() and not want_gate[50].any() and 0.2 < want_gate.mean() < 0.9
    eng = _engine()
    eng.set_meter(0.5, 0.5)
    eng.set_squelch(open_ms, close_ms, 3)
    audio, _, level, _, gate = _Run(eng).play(x, 64).cat()
    assert np.array_equal(gate, want_gate) and same_bits(level, want_level)
    a3, p3 = audio.reshape(NCH, 64, 128), plain[0].reshape(NCH, 64, 128)
    assert not a3[gate == 0].any() and np.array_equal(a3[gate == 1], p3[gate == 1]) and p3[gate == 0].any()
    # the same stream again from a reset (settings kept, meter state zeroed) into rows 130 words apart starting at an odd word
    eng.reset()
    assert not np.any(eng.meter())
    buf = torch.full((NCH * (64 * 128 + 2) + 1, 2), 7, dtype=torch.int16, device="cuda")
    d = torch.from_numpy(x).cuda()
    rc = eng.lib.rdsp_engine_update(eng.h, d.data_ptr(), 64 * 128, 64, buf.data_ptr() + 4, 64 * 128 + 2, None)
    assert rc == 0
    got = buf[1:].reshape(NCH, 64 * 128 + 2, 2).cpu().numpy()
    assert np.array_equal(got[:, :64 * 128, 0], audio) and np.array_equal(got[:, :64 * 128, 1], audio) and np.all(got[:, 64 * 128:] == 7)


@pytest.mark.gpu
def test_gpu_meter_groups(rdsp):
    """three groups (channels 0-19 squelch off, 20-69 a low threshold, 70-96 a high one with other coefficients) for 32 blocks in
    calls of 8, then a regrouping into two (0-49, which takes group 0's settings; 50-96, which takes those of channel 50's old
    group) and 32 more: every channel equals the model run on its own history of settings -- its level, gate and hang went with
    it -- and its audio is the meterless engine's, gated"""
    x = _bursts(23, NCH, 64)
    plain = _Run(_engine(meter=False), meter=False).play(x, 64).cat()
    m = Meter(NCH)
    lo_open, lo_close = _thresholds(m.run(plain[1], Squelch(attack=0.5, decay=0.5))[0])
    off, low, high = Squelch(), Squelch(lo_open, lo_close, 2, attack=0.5, decay=0.5), Squelch(4 * lo_open, 2 * lo_open, 0, attack=0.25, decay=0.75)
    eng = _engine()
    eng.set_groups([0, 20, 70])
    for g, s in ((1, low), (2, high)):
        eng.select_group(g)
        eng.set_meter(float(s.attack), float(s.decay))
        eng.set_squelch(s.open_ms, s.close_ms, s.hang_blocks)
    run = _Run(eng).play(x[:, :32 * 128], 8)
    eng.set_groups([0, 50])
    run.play(x[:, 32 * 128:], 8)
    audio, demod, level, peak, gate = run.cat()
    assert same_bits(demod, plain[1])
    m = Meter(NCH)
    a = m.run(plain[1][:, :32 * 128], [off] * 20 + [low] * 50 + [high] * 27)
    b = m.run(plain[1][:, 32 * 128:], [off] * 50 + [low] * 47)
    want_level, want_gate = np.concatenate([a[0], b[0]], 1), np.concatenate([a[2], b[2]], 1)
    assert same_bits(level, want_level) and np.array_equal(gate, want_gate)
    assert np.array_equal(audio, M.gated(plain[0], want_gate))
    assert np.all(gate[:20] == 1) and np.all(gate[20:50, 32:] == 1) and not np.all(gate[20:70, :32] == 1) and not np.all(gate[70:, 32:] == 1)
    assert want_gate[70:, :32].mean() < want_gate[20:70, :32].mean()


@pytest.mark.gpu
def test_gpu_meter_state_as_data(rdsp):
    """channels 5 ... 9 hear a tone for 10 blocks and weak noise after it; with a hang of 12 blocks they are saved at block 20, in
    the middle of the running hang, and loaded into an engine of 40 channels and max_blocks 16 at channel 21: level, gate and
    audio continue bit for bit.  Sizes and flags: the meter adds three words per channel and flag 2, behind the phase word of
    an engine with sources; an engine without the meter writes the blob it always wrote; a blob with meter words needs the
    meter (NOT_READY); a blob without them zeroes the meter state of the channels it lands on"""
    import torch
    from radiodsp_sdr_rx_amd._lib import RdspError
    x = _bursts(24, NCH, 44)
    t = np.arange(10 * 128)
    tone = np.round(0.3 * 32767 * np.exp(2j * np.pi * 7000.0 / 44100.0 * t))
    x[5:10] = np.random.default_rng(6).integers(-400, 401, (5, 44 * 128, 2))                 # weak noise: audible through the AGC, far below the thresholds
    x[5:10, :10 * 128, 0], x[5:10, :10 * 128, 1] = tone.real, tone.imag
    plain = _Run(_engine(meter=False), meter=False).play(x, 44).cat()
    m = Meter(NCH)
    top = m.run(plain[1], Squelch(attack=0.5, decay=0.5))[0][5:10].max()
    s = Squelch(F32(0.2 * top), F32(0.02 * top), 12, attack=0.5, decay=0.5)
    m = Meter(NCH)
    want_level, _, want_gate = m.run(plain[1], s)
    assert np.all(m.cases[5:10, 19] == 3) and np.all((m.hangs[5:10, 19] > 0) & (m.hangs[5:10, 19] < 12))   # the hang is running at the cut
    assert np.all(want_gate[5:10, 20] == 1) and not want_gate[5:10, 43].any()                          # and runs out after it

    def metered(n, max_blocks):
        e = _engine(n, max_blocks)
        e.set_meter(0.5, 0.5)
        e.set_squelch(s.open_ms, s.close_ms, s.hang_blocks)
        return e
    a = metered(NCH, MAXB)
    first = _Run(a).play(x[:, :20 * 128], 20).cat()
    assert np.array_equal(first[4], want_gate[:, :20])
    blob = a.save_state(5, 5)
    assert len(blob) == 16 + 5 * (STATE_CH_BYTES + 12) == a.lib.rdsp_engine_state_bytes(a.h, 5) and blob[12:16].view(np.uint32)[0] == 2
    tail = blob[16 + 5 * STATE_CH_BYTES:].view(np.uint32).reshape(5, 3)
    assert np.array_equal(tail[:, 0], want_level[5:10, 19].view(np.uint32)) and np.all(tail[:, 1] == 1) and np.array_equal(tail[:, 2], m.hangs[5:10, 19])
    b = metered(40, 16)
    b.update(torch.zeros((40, 3 * 128, 2), dtype=torch.int16, device="cuda"))           # a past of its own
    b.load_state(21, blob)
    y = np.zeros((40, 24 * 128, 2), np.int16)
    y[21:26] = x[5:10, 20 * 128:]
    rest = _Run(b).play(y, 7).cat()
    assert same_bits(rest[2][21:26], want_level[5:10, 20:]) and np.array_equal(rest[4][21:26], want_gate[5:10, 20:])
    assert np.array_equal(rest[0][21:26], M.gated(plain[0], want_gate)[5:10, 20 * 128:])
    assert rest[0][21:26, :4 * 128].any() and not rest[0][21:26, -128:].any() and plain[0][5:10, -128:].any()   # heard while the hang ran
    # an engine without the meter: the blob it always wrote, whatever meter settings it was given
    u, v = _engine(NCH, MAXB, meter=False), _engine(NCH, MAXB, meter=False)
    u.set_squelch(s.open_ms, s.close_ms, 4)
    u.set_meter(0.25, 0.25)
    d = torch.from_numpy(x[:, :20 * 128]).cuda()
    u.update(d); v.update(d)
    bu, bv = u.save_state(5, 5), v.save_state(5, 5)
    assert len(bu) == 16 + 5 * STATE_CH_BYTES and bu[12:16].view(np.uint32)[0] == 0 and np.array_equal(bu, bv)
    assert np.array_equal(bu[16:], blob[16:16 + 5 * STATE_CH_BYTES])                      # and the metered engine's channel words are those
    with pytest.raises(RdspError) as ex:
        u.load_state(0, blob)                                                           # meter words, no meter
    assert ex.value.code == -4 and np.array_equal(u.save_state(5, 5), bu)
    before = a.meter()
    assert before[5:10].any()
    a.load_state(7, bu)                                                                 # no meter words: channels 7 ... 11 start from zero
    after = a.meter()
    assert not after[7:12].any() and np.array_equal(after[:7], before[:7]) and np.array_equal(after[12:], before[12:])
    # with sources: the phase word, then the meter words
    a.set_sources(2, [c % 2 for c in range(NCH)])
    both = a.save_state(5, 5)
    assert len(both) == 16 + 5 * (STATE_CH_BYTES + 4 + 12) == a.lib.rdsp_engine_state_bytes(a.h, 5) and both[12:16].view(np.uint32)[0] == 3
    assert np.array_equal(both[16 + 5 * (STATE_CH_BYTES + 4):].view(np.uint32).reshape(5, 3)[:2], tail[:2])   # channels 5, 6 were not overwritten


@pytest.mark.gpu
@pytest.mark.parametrize("nch", [300, 1100])
def test_gpu_active_list(rdsp, nch):
    """300 channels (75 meter workgroups; the list kernel's one chunk, ragged) and 1100 (two chunks), a drawn pattern of loud and
    all-zero rows, 4 blocks: the list is ascending and numpy's, with its count; then all rows zero (count 0) and the squelch off
    (every channel, in order)"""
    import torch
    r = np.random.default_rng(nch)
    loud = r.random(nch) < 0.4
    loud[[0, 63, 64, nch - 1]] = [True, False, True, True]
    x = _bursts(25, nch, 4, quiet=(1,))
    x[~loud] = 0
    eng = _engine(nch, 4)
    eng.set_squelch(1e-7, 1e-7, 0)
    eng.update(torch.from_numpy(x).cuda())
    lst, cnt = eng.active()
    gate = eng.read_meter(4)[2].cpu().numpy()
    assert cnt == int(loud.sum()) and np.array_equal(lst.cpu().numpy(), np.flatnonzero(loud)) and np.array_equal(gate.any(1), loud)
    zero = torch.zeros((nch, 4 * 128, 2), dtype=torch.int16, device="cuda")
    eng.reset()
    eng.update(zero)
    lst, cnt = eng.active()
    assert cnt == 0 and len(lst) == 0
    eng.disable_squelch()
    eng.update(zero)
    lst, cnt = eng.active()
    assert cnt == nch and np.array_equal(lst.cpu().numpy(), np.arange(nch))


@pytest.mark.gpu
def test_gpu_meter_on_the_sources_path(rdsp):
    """update_sources at 44 100 Hz with two sources against update on the restated tuned rows: the same meter records, gates,
    active lists and audio"""
    import torch
    from engine_sources_model import TUNING_OFFSET, _band, _stations, dphi_of, stream, table
    nb = 8
    src = _band(31, 2, nb)
    src[0, :64] = src[0, 64:128]                                                       # no saturating head: the rows stay ordinary
    stations = _stations(3, NCH, 1, 1)
    source_of = [c % 2 for c in range(NCH)]
    tab = table(rdsp)
    steps = np.array([dphi_of(TUNING_OFFSET[0], f) for f in stations], np.uint64)
    tuned = np.zeros((NCH, nb * 128, 2), np.int16)
    for k in range(2):
        ch = [c for c in range(NCH) if source_of[c] == k]
        tuned[ch] = stream(src[k], 1, 1, None, np.repeat(steps[ch][:, None], nb, 1), tab)[0]
    a, b = _engine(NCH, nb), _engine(NCH, nb)
    for e in (a, b):
        e.set_meter(0.5, 0.25)
    a.set_sources(2, source_of)
    a.tune(0, stations)
    ya = a.update_sources(torch.from_numpy(src).cuda()).cpu().numpy()
    ra = [v.cpu().numpy() for v in a.read_meter(nb)]
    level = ra[0]
    open_ms = F32(np.median(level[:, -1]))
    for e in (a, b):
        e.reset()
        e.set_squelch(open_ms, F32(0.5) * open_ms, 1)
    ya = a.update_sources(torch.from_numpy(src).cuda()).cpu().numpy()
    yb = b.update(torch.from_numpy(tuned).cuda()).cpu().numpy()
    ra, rb = [v.cpu().numpy() for v in a.read_meter(nb)], [v.cpu().numpy() for v in b.read_meter(nb)]
    assert same_bits(a.read_demod(nb).cpu().numpy(), b.read_demod(nb).cpu().numpy())
    assert same_bits(ra[0], rb[0]) and same_bits(ra[1], rb[1]) and np.array_equal(ra[2], rb[2]) and np.array_equal(ya, yb)
    assert 0 < ra[2].mean() < 1 and same_bits(a.meter(), b.meter())
    assert np.array_equal(a.active()[0].cpu().numpy(), b.active()[0].cpu().numpy())
    want = Meter(NCH).run(b.read_demod(nb).cpu().numpy(), Squelch(open_ms, F32(0.5) * open_ms, 1, attack=0.5, decay=0.25))
    assert same_bits(ra[0], want[0]) and np.array_equal(ra[2], want[2])


@pytest.mark.gpu
def test_gpu_meter_refusals(rdsp):
    """RDSP_ERR_INVALID for NaN and out-of-range parameters, close above open, short strides and more blocks than the last call
    had; RDSP_ERR_NOT_READY for read_meter, active and get_meter before enable_meter; each leaves the object as it was: the next
    call's records equal those of a twin that was never asked"""
    import ctypes as C
    import torch
    x = _bursts(26, 5, 6)
    d = torch.from_numpy(x).cuda()
    e, twin = _engine(5, 8, meter=False), _engine(5, 8)
    lib = e.lib
    buf = torch.zeros(5 * 8 * 128, dtype=torch.float32, device="cuda")
    host = (C.c_float * 20)()
    p = buf.data_ptr()
    assert lib.rdsp_engine_meter_enabled(e.h) == 0
    assert lib.rdsp_engine_read_meter(e.h, 0, p, 8, p, 8, p, 8, None) == -4 and b"rdsp_engine_enable_meter" in lib.rdsp_last_error()
    assert lib.rdsp_engine_active(e.h, p, p, None) == -4 and lib.rdsp_engine_get_meter(e.h, host, None) == -4
    assert lib.rdsp_engine_read_demod(e.h, 1, p, 128, None) == -1                        # no call yet
    e.set_meter(0.5, 0.5)                                                                # the setters may precede the meter
    e.set_squelch(1e-4, 1e-5, 2)
    twin.set_meter(0.5, 0.5)
    twin.set_squelch(1e-4, 1e-5, 2)
    e.enable_meter()
    e.enable_meter()                                                                     # again: a no-op
    assert lib.rdsp_engine_meter_enabled(e.h) == 1
    nan, inf = float("nan"), float("inf")
    for att, dec in ((0.0, 0.5), (0.5, 0.0), (1.5, 0.5), (0.5, -0.25), (nan, 0.5), (0.5, nan), (inf, 0.5)):
        assert lib.rdsp_engine_set_meter(e.h, att, dec) == -1, (att, dec)
    for o, c, h in ((1e-5, 1e-4, 2), (-1.0, -2.0, 2), (nan, 0.0, 2), (1.0, nan, 2), (inf, 0.0, 2), (1e-4, 1e-5, -1), (1e-4, 1e-5, 65536)):
        assert lib.rdsp_engine_set_squelch(e.h, o, c, h) == -1, (o, c, h)
    assert b"hang_blocks" in lib.rdsp_last_error()
    assert lib.rdsp_engine_set_meter(None, 0.5, 0.5) == -1 and lib.rdsp_engine_enable_meter(None) == -1
    e.update(d); twin.update(d)
    assert not e.read_meter(6)[2].all().item()                                           # the squelch set before enable_meter is in force
    assert lib.rdsp_engine_read_meter(e.h, 7, p, 8, p, 8, p, 8, None) == -1               # the last call had 6
    assert lib.rdsp_engine_read_meter(e.h, 6, p, 5, None, 0, None, 0, None) == -1         # a short stride
    assert lib.rdsp_engine_read_meter(e.h, 6, None, 0, None, 0, p, 5, None) == -1
    assert lib.rdsp_engine_read_meter(e.h, -1, p, 8, p, 8, p, 8, None) == -1
    assert lib.rdsp_engine_read_meter(e.h, 6, None, 0, None, 0, None, 0, None) == 0       # every pointer may be NULL
    assert lib.rdsp_engine_read_demod(e.h, 7, p, 8 * 128, None) == -1 and lib.rdsp_engine_read_demod(e.h, 6, p, 5 * 128, None) == -1
    assert lib.rdsp_engine_read_demod(e.h, 6, None, 8 * 128, None) == -1 and lib.rdsp_engine_get_meter(e.h, None, None) == -1
    torch.cuda.synchronize()
    assert not buf.any()                                                                 # no refused call wrote
    for v, w in zip(e.read_meter(6), twin.read_meter(6)):
        assert torch.equal(v, w)
    assert same_bits(e.meter(), twin.meter()) and e.meter()[:, 0].any()
    e.update(d); twin.update(d)
    for v, w in zip(e.read_meter(6), twin.read_meter(6)):
        assert torch.equal(v, w)


# ---- state blobs with both optional parts: tuning phases and meter words ---------------------------------------------------
SRC_D, SRC_NB, SRC_CUT = 2, 12, 6                                 # sources at 88 200 Hz, 12 blocks, saved after 6


def _on_sources(x, stations, source_of, D):
    """the rows of x (int16 [n, t, 2] at 44 100 Hz, as update takes them) as int16 source rows at D x 44 100 Hz: every row held
    D times at an eighth of its size, moved from the LSB tuning offset, where update expects it, to its receiver's station, and
    summed into its receiver's source"""
    from engine_sources_model import TUNING_OFFSET
    z = np.repeat(x[..., 0] + 1j * x[..., 1], D, 1) / 8.0
    z = z * np.exp(2j * np.pi * ((np.asarray(stations)[:, None] - TUNING_OFFSET[0]) / (D * 44100.0)) * np.arange(z.shape[1]))
    src = np.stack([z[[c for c in range(len(z)) if source_of[c] == k]].sum(0) for k in range(max(source_of) + 1)])
    return np.stack([np.round(src.real), np.round(src.imag)], -1).astype(np.int16)


def _sourced(n, max_blocks, stations, s=None, meter=True):
    """an engine of n receivers, receiver c on source c % 2 of two int16 sources at D = 2, tuned to `stations`, with squelch s"""
    e = _engine(n, max_blocks, meter)
    e.set_meter(0.5, 0.5)
    if s is not None:
        e.set_squelch(s.open_ms, s.close_ms, s.hang_blocks)
    e.set_sources(2, [c % 2 for c in range(n)])
    e.set_source_decimation(SRC_D)
    e.tune(0, stations)
    return e


def _play_sources(e, src, a, b, split):
    """blocks a ... b - 1 of the source rows in calls of `split` -> audio [n, t]; level and gate [n, b - a] of an engine with the meter"""
    import torch
    audio, level, gate = [], [], []
    for k in range(a, b, split):
        m = min(b, k + split)
        y = e.update_sources(torch.from_numpy(np.ascontiguousarray(src[:, k * 128 * SRC_D:m * 128 * SRC_D])).cuda()).cpu().numpy()
        assert np.array_equal(y[..., 0], y[..., 1])
        audio.append(y[..., 0])
        if e.meter_enabled():
            lv, _, g = (v.cpu().numpy() for v in e.read_meter(m - k))
            level.append(lv); gate.append(g)
    return np.concatenate(audio, 1), (np.concatenate(level, 1) if level else None), (np.concatenate(gate, 1) if gate else None)


@functools.lru_cache(maxsize=None)
def _source_case():
    """-> source rows int16 [2, 12 x 256, 2], the 12 stations, the squelch.  The bursts of _bursts at distinct stations, 6 kHz
    apart, of two sources; a hang of 6 blocks and thresholds between the loud and the quiet levels an engine with the squelch
    off measures on these rows.  The last 32 pairs in front of the cut are zero: a source's last 15 D pairs are its history,
    which is in no blob, so an engine that takes the receivers over from a past of zero rows holds the same history."""
    stations = -33000.0 + 6000.0 * np.arange(12)
    src = _on_sources(_bursts(27, 12, SRC_NB, quiet=(9, 10, 12)), stations, [c % 2 for c in range(12)], SRC_D)
    cut = SRC_CUT * 128 * SRC_D
    src[:, cut - 32:cut] = 0
    level = _play_sources(_sourced(12, 8, stations), src, 0, SRC_NB, SRC_CUT)[1]
    open_ms, close_ms = _thresholds(level)
    return src, stations, Squelch(open_ms, close_ms, 6, attack=0.5, decay=0.5)


def _tail(blob, n):
    """the words of a blob of n channels behind its channel words: the phases, then the meter words"""
    return blob[16 + n * STATE_CH_BYTES:].view(np.uint32)


@pytest.mark.gpu
def test_gpu_state_with_phases_and_meter_continues(rdsp):
    """engine A (12 receivers, max_blocks 8, two sources at D = 2, meter and squelch) plays 6 blocks and saves receivers 3 ... 6:
    flags 3, a phase word and three meter words per channel behind the channel words.  Engine B (20 receivers, max_blocks 4, a
    past of two zero blocks) takes them at 9 ... 12: the blob it saves there carries A's phase and meter words, and over the next
    6 blocks -- A in one call, B in calls of 3 -- audio, level and gate of the four receivers agree bit for bit"""
    src, stations, s = _source_case()
    a = _sourced(12, 8, stations, s)
    first = _play_sources(a, src, 0, SRC_CUT, SRC_CUT)
    assert 0 < first[2].mean() < 1                                                       # gates open and closed
    blob = a.save_state(3, 4)
    assert len(blob) == 16 + 4 * (STATE_CH_BYTES + 4 + 12) == a.lib.rdsp_engine_state_bytes(a.h, 4)
    assert list(blob[:16].view(np.uint32)) == [0x45534452, 1, 4, 3]
    assert _tail(blob, 4)[:4].all() and _tail(blob, 4)[4::3].all()                       # phases that moved, levels above zero
    b = _sourced(20, 4, np.zeros(20), s)
    _play_sources(b, np.zeros((2, 2 * 128 * SRC_D, 2), np.int16), 0, 2, 2)              # a past of its own
    b.tune(9, stations[3:7])
    b.load_state(9, blob)
    assert np.array_equal(_tail(b.save_state(9, 4), 4), _tail(blob, 4))
    ra, rb = _play_sources(a, src, SRC_CUT, SRC_NB, SRC_NB - SRC_CUT), _play_sources(b, src, SRC_CUT, SRC_NB, 3)
    assert np.array_equal(ra[0][3:7], rb[0][9:13]) and ra[0][3:7].any()
    assert same_bits(ra[1][3:7], rb[1][9:13]) and np.array_equal(ra[2][3:7], rb[2][9:13])


@pytest.mark.gpu
def test_gpu_state_without_meter_words_zeroes_them(rdsp):
    """receivers 3 ... 6 of an engine with sources and no meter, saved after 6 blocks (flags 1: phases only), loaded into engine A
    at channel 0: A's meter state of channels 0 ... 3 is zero, that of 4 ... 11 as it was, and the blob A saves of 0 ... 3 carries
    the loaded phase words and zero meter words"""
    src, stations, s = _source_case()
    a, u = _sourced(12, 8, stations, s), _sourced(12, 8, stations, s, meter=False)
    for e in (a, u):
        _play_sources(e, src, 0, SRC_CUT, SRC_CUT)
    bu = u.save_state(3, 4)
    assert len(bu) == 16 + 4 * (STATE_CH_BYTES + 4) == u.lib.rdsp_engine_state_bytes(u.h, 4)
    assert list(bu[:16].view(np.uint32)) == [0x45534452, 1, 4, 1]
    before, own = a.meter(), a.save_state(0, 4)
    assert before[:4, 0].all() and before[4:, 0].all()
    a.load_state(0, bu)
    after, got = a.meter(), a.save_state(0, 4)
    assert not after[:4].any() and np.array_equal(after[4:], before[4:])
    assert np.array_equal(_tail(got, 4)[:4], _tail(bu, 4)) and not np.array_equal(_tail(got, 4)[:4], _tail(own, 4)[:4])
    assert not _tail(got, 4)[4:].any() and _tail(own, 4)[4:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("nb", [7, 8, 9, 17])
def test_gpu_meter_at_the_eight_block_steps(rdsp, nb):
    """5 channels (a ragged workgroup of the meter's four) x 7, 8, 9 and 17 blocks in one call -- below, on and above the eight
    blocks the meter kernel takes a step, and two steps and one block: levels, peaks and gates equal the restatement applied to
    read_demod's rows, bit for bit, the gates open and close inside the call, and on output rows nb x 128 + 2 pairs apart that
    start at an odd word a closed block is 128 zero words on both sides, an open one the meterless engine's"""
    import torch
    x = _bursts(70 + nb, 5, nb, quiet=(1, 2, 3))
    plain = _Run(_engine(5, 17, meter=False), meter=False).play(x, nb).cat()
    open_ms, close_ms = _thresholds(Meter(5).run(plain[1], Squelch(attack=0.5, decay=0.5))[0])
    s = Squelch(open_ms, close_ms, 1, attack=0.5, decay=0.5)
    m = Meter(5)
    want_level, want_peak, want_gate = m.run(plain[1], s)
    assert want_gate.any() and not want_gate.all()
    eng = _engine(5, 17)
    eng.set_meter(0.5, 0.5)
    eng.set_squelch(open_ms, close_ms, 1)
    stride = nb * 128 + 2
    buf = torch.full((5 * stride + 1, 2), 7, dtype=torch.int16, device="cuda")
    assert (buf.data_ptr() + 4) % 16 != 0
    assert eng.lib.rdsp_engine_update(eng.h, torch.from_numpy(x).cuda().data_ptr(), nb * 128, nb, buf.data_ptr() + 4, stride, None) == 0
    level, peak, gate = (v.cpu().numpy() for v in eng.read_meter(nb))
    assert same_bits(eng.read_demod(nb).cpu().numpy(), plain[1])
    assert same_bits(level, want_level) and same_bits(peak, want_peak) and np.array_equal(gate, want_gate)
    assert same_bits(eng.meter(), m.scalars())
    got = buf[1:].reshape(5, stride, 2).cpu().numpy()
    assert np.all(got[:, nb * 128:] == 7) and np.all(buf[0].cpu().numpy() == 7)
    assert np.array_equal(got[:, :nb * 128, 0], got[:, :nb * 128, 1]) and np.array_equal(got[:, :nb * 128, 0], M.gated(plain[0], want_gate))
    a3 = got[:, :nb * 128, 0].reshape(5, nb, 128)
    assert not a3[gate == 0].any() and a3[gate == 1].any() and plain[0].reshape(5, nb, 128)[gate == 0].any()
    lst, cnt = eng.active()
    assert cnt == len(lst) and np.array_equal(lst.cpu().numpy(), np.flatnonzero(want_gate.any(1)))
