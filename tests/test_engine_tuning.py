"""rdsp_engine_t on shared IQ streams: receivers tuned to stations inside a few source rows (rdsp_engine_set_sources /
rdsp_engine_tune / rdsp_engine_update_sources, include/rdsp.h).

`-m "not gpu"`: csrc/rdsp_tune.h compiled on the host (tests/host/host_source_pass_check.cpp, -ffp-contract=off as the kernel
is): the phasor table gives exactly (1, 0) at phase 0 and stays within 2^-17 of cos / sin, a shift of 0 is the identity,
full-scale rotations saturate, the accumulator after calls of any size is the closed form; and the numpy restatement
(tests/engine_sources_model.py) is that header's arithmetic bit for bit, its table the library's.
`-m gpu`: the audio of every receiver, bit for bit, against the CPU restatement of the engine (oracle_lib.OracleEngine) run
on the restated tuned row -- which is the image's arithmetic (tests/test_engine_kat.py) -- across call splits, retunes, mode
changes, regroupings, state moved between objects, and the refusals."""
import os
import subprocess

import numpy as np
import pytest

from engine_sources_model import HERE, TUNING_OFFSET, Rx, _band, dphi_of, engine, host_program, tune_pairs, tuned_row


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_check():
    return host_program()


def test_tuning_arithmetic_on_the_host(host_check):
    """phase 0 -> exactly (1, 0); phasor error below 2^-17 over every 512th phase, the neighbours of every table entry and a
    million random phases; shift 0 the identity on the edge pairs (+-32767, -32768, 0, ...) and a million random pairs; the
    full-scale pairs saturate at every rotation; the accumulator after calls of 1 ... 128 blocks is ph0 + total dphi; a tone
    at +5000 Hz tuned for USB comes out at the USB tuning offset, 5390 Hz"""
    out = subprocess.run([host_check, "check"], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.rstrip().endswith("OK"), out.stdout + out.stderr


def test_numpy_restatement_is_the_headers_arithmetic(host_check, tmp_path, rdsp):
    """the restatement the GPU tests use, against rdsp_tune.h compiled on the host: 400 000 pairs at drawn phases (edge
    pairs, phase 0, phases next to table entries and to midpoints among them), the steps of drawn stations in every mode, and
    the table, which must also be the library's (rdsp_engine_tune_table)"""
    r = np.random.default_rng(3)
    n = 400000
    words = r.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    edge = np.array([-32768, -32767, -1, 0, 1, 32767], np.int16)
    e = np.stack(np.meshgrid(edge, edge), -1).reshape(-1, 2)
    words[:len(e)] = e.view(np.uint32).reshape(-1)
    phases = r.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    phases[:n // 8] = 0
    phases[n // 8:n // 4] = (r.integers(0, 1024, n // 8).astype(np.uint32) << np.uint32(22)) + r.integers(-3, 4, n // 8).astype(np.uint32)
    phases[n // 4:n // 4 + 1000] = np.arange(1000, dtype=np.uint32) * np.uint32(4294967)
    words[n // 2:n // 2 + 4000] = np.array([[32767, 32767], [-32768, -32768], [32767, -32768], [-32768, 32767]], np.int16)[np.arange(4000) % 4].view(np.uint32).reshape(-1)
    stations = np.concatenate([r.uniform(-22049.0, 22049.0, 3000), [0.0, 8390.0, 5390.0, -22049.9, 22049.9, 0.5, -0.5]])
    modes = r.integers(0, 7, len(stations))
    to = np.array([TUNING_OFFSET[int(m)] for m in modes], np.float32)
    words.tofile(tmp_path / "words.bin")
    phases.tofile(tmp_path / "phases.bin")
    to.tofile(tmp_path / "to.bin")
    stations.astype(np.float64).tofile(tmp_path / "station.bin")
    out = subprocess.run([host_check, "vectors", str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    table = np.fromfile(tmp_path / "table.bin", np.float32).reshape(1024, 4)
    lib_table = np.ctypeslib.as_array(rdsp.load().rdsp_engine_tune_table(), (1024, 4)).copy()
    assert np.array_equal(table.view(np.uint32), lib_table.view(np.uint32))
    assert table[0, 0] == 1.0 and table[0, 1] == 0.0
    want = np.fromfile(tmp_path / "tuned.bin", np.uint32)
    got = tune_pairs(words.view(np.int16).reshape(-1, 2), phases, table).view(np.uint32).reshape(-1)
    assert np.array_equal(got, want), int(np.argmax(got != want))
    assert np.array_equal(words[:n // 8], got[:n // 8])                                  # phase 0: the identity
    assert [dphi_of(t, s) for t, s in zip(to, stations)] == list(np.fromfile(tmp_path / "dphi.bin", np.uint32))


# ---- GPU ------------------------------------------------------------------------------------------------------------------


@pytest.mark.gpu
def test_gpu_tuning_shift_zero_is_update_on_the_fixture(rdsp):
    """every case of tests/golden/engine_kat.npz as the one source of two receivers tuned to station = TuningOffset of
    their mode (retuned at every setDemodMode of the case): a shift of 0, so update_sources must return the image's own
    audio, bit for bit, in calls of 16 blocks and at every setter"""
    import torch
    kat = np.load(os.path.join(HERE, "golden", "engine_kat.npz"))
    import json
    for name in [str(n) for n in kat["case_names"]]:
        iq, calls, want = kat[name + "_iq"], json.loads(str(kat[name + "_calls"])), kat[name + "_out"]
        nb = len(iq) // 128
        eng = engine(2, 16)
        to = eng.sketch_setup()
        eng.set_sources(1, [0, 0])
        eng.tune(0, [to, to])
        d = torch.from_numpy(iq[None].copy()).cuda()
        marks = sorted({0, nb} | {c[0] for c in calls} | set(range(0, nb, 16)))
        outs = []
        for a, b in zip(marks[:-1], marks[1:]):
            for c in calls:
                if c[0] == a:
                    r = getattr(eng, c[1])(*c[2:])
                    if c[1] == "setDemodMode":
                        eng.tune(0, [r, r])
            outs.append(eng.update_sources(d[:, a * 128:b * 128].contiguous()))
        y = torch.cat(outs, 1)[..., 0].cpu().numpy()
        assert np.array_equal(y[0], want), (name, int(np.argmax(y[0] != want)))
        assert np.array_equal(y[1], want), name
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("split", [1, 7, 64])
def test_gpu_tuning_against_the_restatement(rdsp, split):
    """3 sources x 97 receivers (ragged last workgroups) in five groups -- LSB, USB, CW, AM, SAM -- at drawn stations, 256
    blocks cut into calls of `split`; at block 90 a third of the receivers retune, at block 150 two groups change mode and one
    its audio filter: every receiver against the restatement of its own tuned row and calls, bit for bit"""
    r = np.random.default_rng(20 + split)
    nch, nb = 97, 256
    src = _band(40, 3, nb)
    source_of = r.integers(0, 3, nch)
    firsts = [0, 19, 40, 58, 77]
    eng = engine(nch, 64)
    eng.sketch_setup()
    R = Rx(eng, src, source_of, firsts, r.uniform(-21500, 21500, nch))
    for g, m in enumerate([0, 1, 2, 4, 5]):
        R.call(0, g, "setDemodMode", m)
    R.run(0, 90, split)
    R.tune(5, r.uniform(-21500, 21500, 32))
    R.run(90, 150, split)
    R.call(150, 2, "setDemodMode", 3)
    R.call(150, 4, "setDemodMode", 1)
    R.call(150, 1, "setAudioFilter", 3)
    R.run(150, nb, split)
    R.check(R.result())


@pytest.mark.gpu
def test_gpu_tuning_sign_convention(rdsp):
    """one source, two USB stations: A at +5000 Hz carrying a 1000 Hz tone (+6000 Hz in the stream), B at -8000 Hz carrying
    600 Hz (-7400 Hz).  A receiver in USB tuned to each hears its own tone at its audio frequency, the other's at least
    40 dB down (and both bit for bit the restatement)"""
    t = np.arange(96 * 128)
    z = 0.2 * np.exp(2j * np.pi * 6000.0 / 44100.0 * t) + 0.2 * np.exp(2j * np.pi * -7400.0 / 44100.0 * t + 1.0)
    src = np.stack([np.round(z.real * 32767), np.round(z.imag * 32767)], 1).astype(np.int16)[None]
    eng = engine(2, 32)
    eng.sketch_setup()
    R = Rx(eng, src, [0, 0], [0], [5000.0, -8000.0])
    R.call(0, -1, "setDemodMode", 1)
    R.run(0, 96, 32)
    y = R.result()
    R.check(y)
    w = np.hanning(8192)   # the last 64 blocks, the AGC settled
    f = np.fft.rfftfreq(8192, 1 / 44100.0)
    for c, (mine, other) in enumerate(((1000.0, 600.0), (600.0, 1000.0))):
        p = np.abs(np.fft.rfft(y[c, -8192:] * w)) ** 2
        at = lambda hz: p[np.abs(f - hz) <= 25].max()
        assert abs(f[np.argmax(p)] - mine) < 10, (c, f[np.argmax(p)])
        assert 10 * np.log10(at(mine) / at(other)) >= 40, (c, 10 * np.log10(at(mine) / at(other)))


@pytest.mark.gpu
def test_gpu_tuning_at_the_bench_shape(rdsp):
    """`bench.py --config ENGINE`'s shape -- 4096 receivers x 32 blocks, two calls -- on 256 sources of the synthetic
    generator, receiver c on source c % 256 (so the pass's source order is not the channel order) at drawn stations: 44
    sampled receivers, the pass's and the engine's workgroup boundaries among them, bit for bit"""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    nch, nblk, nsrc = 4096, 32, 256
    src = synth_iq(nsrc, 2 * nblk * 128, n_threads=8)
    eng = engine(nch, nblk)
    eng.sketch_setup()
    R = Rx(eng, src, np.arange(nch) % nsrc, [0], np.random.default_rng(5).uniform(-21000, 21000, nch))
    R.run(0, 2 * nblk, nblk)
    y = R.result()
    by_source = lambda p: (p % 16) * nsrc + p // 16        # the receiver at position p of the pass's order (4 per workgroup)
    pick = {0, 1, 7, 8, 15, 16, 255, 256, 1023, 1024, 4095} | {by_source(p) for p in (3, 4, 7, 8, 1023, 1024, 2047, 2048, 4091, 4092, 4095)}
    pick |= set(int(c) for c in np.random.default_rng(2).integers(0, nch, 22))
    R.check(y, sorted(pick))


@pytest.mark.gpu
def test_gpu_tuning_regroup_keeps_every_receiver_on_its_station(rdsp):
    """one group split in mid-stream into three (channels 0-6, 7-12, 13-19: none aligned to a workgroup) that go to USB,
    AM and SAM -- each receiver's step follows its new group's mode from the next call on -- then all to CW and merged
    again, a retune after the merge: every receiver against the restatement, bit for bit"""
    nch, nb = 20, 160
    r = np.random.default_rng(8)
    src = _band(50, 2, nb)
    eng = engine(nch, 8)
    eng.sketch_setup()
    R = Rx(eng, src, r.integers(0, 2, nch), [0], r.uniform(-21000, 21000, nch))
    R.run(0, 12, 8)
    R.set_groups([0, 7, 13])
    for g, m in ((1, 1), (2, 4)):
        R.call(12, g, "setDemodMode", m)
    R.run(12, 30, 8)
    R.call(30, 2, "setDemodMode", 5)
    R.run(30, 60, 8)
    R.call(60, -1, "setDemodMode", 2)
    R.run(60, 61, 8)
    R.set_groups([0])
    R.run(61, 100, 8)
    R.tune(3, r.uniform(-21000, 21000, 9))
    R.run(100, nb, 8)
    R.check(R.result())


@pytest.mark.gpu
def test_gpu_tuning_state_as_data(rdsp):
    """a tuned range saved after 21 blocks and loaded into an object of another channel count and call size, at another
    channel index, after that object ran a block of its own: the receivers continue bit for bit.  A blob of an engine
    without sources loaded there sets the phase to 0; a blob with phases is refused by an engine without sources"""
    import torch
    import oracle_lib
    from radiodsp_sdr_rx_amd._lib import RdspError
    nb, k = 60, 21
    r = np.random.default_rng(9)
    src = _band(60, 2, nb)
    a = engine(6, 8)
    a.sketch_setup()
    A = Rx(a, src, [0, 1, 1, 0, 1, 0], [0], r.uniform(-21000, 21000, 6))
    A.run(0, k, 8)
    blob = a.save_state(2, 2)
    assert blob.size == a.lib.rdsp_engine_state_bytes(a.h, 2) == 16 + 2 * (10368 + 4)
    assert list(blob[:16].view(np.uint32)) == [0x45534452, 1, 2, 1]
    b = engine(9, 16)
    b.sketch_setup()
    B = Rx(b, src, [0] * 5 + [1, 0] + [1] * 2, [0], r.uniform(-21000, 21000, 9))
    B.tune(5, A.station[2:4])
    b.update_sources(torch.zeros((2, 128, 2), dtype=torch.int16, device="cuda"))        # b has a past of its own
    b.load_state(5, blob)
    B.steps = [[None] * k + s for s in B.steps]
    B.run(k, nb, 16)
    y = B.result()
    for cb, ca in ((5, 2), (6, 3)):
        steps = A.steps[ca] + B.steps[cb][k:]
        w = oracle_lib.OracleEngine().run(tuned_row(src[A.source_of[ca]], steps, A.tab), [])
        assert np.array_equal(y[cb], w[k * 128:]), cb
    # a blob without phases (an engine that never had sources) into an engine with them: the phase starts at 0
    u = engine(1, 32)
    u.sketch_setup()
    x0 = _band(70, 1, k)[0]
    u.update(torch.from_numpy(x0[None].copy()).cuda())
    ublob = u.save_state(0, 1)
    assert ublob.size == 16 + 10368 and list(ublob[:16].view(np.uint32)) == [0x45534452, 1, 1, 0]
    c = engine(3, 8)
    c.sketch_setup()
    C_ = Rx(c, src, [1, 1, 0], [0], r.uniform(-21000, 21000, 3))
    C_.run(0, 5, 8)
    c.load_state(1, ublob)
    C_.steps = [[] for _ in range(3)]
    C_.outs = []
    C_.run(0, nb - 5, 8)
    got = C_.result()[1]
    step = dphi_of(8390.0, C_.station[1])
    head = x0
    w = oracle_lib.OracleEngine().run(np.concatenate([head, tuned_row(src[1], [step] * (nb - 5), C_.tab)]), [])
    assert np.array_equal(got, w[len(head):])
    with pytest.raises(RdspError) as ex:
        u.load_state(0, a.save_state(2, 1))                          # phases, and no sources to put them in
    assert ex.value.code == -4


@pytest.mark.gpu
def test_gpu_tuning_untuned_state_is_unchanged(rdsp):
    """an engine that never had sources -- tuned stations or not -- keeps rdsp_engine_state_bytes and its blob layout:
    16 + n x 10 368 bytes, header word 3 zero; and two such engines with the same past give byte-identical blobs"""
    import torch
    x = _band(80, 3, 8)
    blobs = []
    for tune in (False, True):
        e = engine(3, 8)
        e.sketch_setup()
        if tune:
            e.tune(0, [100.0, 200.0, 300.0])
        assert e.lib.rdsp_engine_state_bytes(e.h, 3) == 16 + 3 * 10368
        e.update(torch.from_numpy(x).cuda())
        blobs.append(e.save_state(0, 3))
        assert blobs[-1].size == 16 + 3 * 10368 and list(blobs[-1][:16].view(np.uint32)) == [0x45534452, 1, 3, 0]
    assert np.array_equal(blobs[0], blobs[1])


@pytest.mark.gpu
def test_gpu_tuning_reset_zeroes_phases_and_keeps_stations(rdsp):
    """reset, then the same source rows again: the same audio as the first time (phases from 0, stations as tuned)"""
    import torch
    src = _band(90, 2, 24)
    eng = engine(5, 8)
    eng.sketch_setup()
    eng.set_sources(2, [0, 1, 0, 1, 1])
    eng.tune(0, [-15000.0, 3000.0, 12345.6, -700.0, 20000.0])
    d = torch.from_numpy(src).cuda()
    run = lambda: torch.cat([eng.update_sources(d[:, a * 128:(a + 8) * 128].contiguous()) for a in (0, 8, 16)], 1).cpu().numpy()
    first = run()
    eng.reset()
    assert np.array_equal(run(), first)
    eng.reset()
    eng.tune(2, [0.0])
    again = run()
    assert np.array_equal(np.delete(again, 2, 0), np.delete(first, 2, 0)) and not np.array_equal(again[2], first[2])


@pytest.mark.gpu
def test_gpu_tuning_refusals(rdsp):
    """refused with nothing changed: update_sources before set_sources (NOT_READY), a source index out of range, n_sources
    < 1, |station| >= 22 050 or NaN (one bad station among good ones changes none), a channel range outside the object, a
    short or misaligned source stride or row, n_blocks > max_blocks -- the object then runs on exactly as a twin that
    never saw those calls"""
    import torch
    from radiodsp_sdr_rx_amd._lib import RdspError
    src = torch.from_numpy(_band(95, 2, 16)).cuda()
    out = torch.empty((4, 8 * 128, 2), dtype=torch.int16, device="cuda")
    eng, twin = engine(4, 8), engine(4, 8)
    for e in (eng, twin):
        e.sketch_setup()
    with pytest.raises(RdspError) as ex:
        eng.update_sources(src[:, :128].contiguous())
    assert ex.value.code == -4 and b"set_sources" in eng.lib.rdsp_last_error()
    for n_src, m in ((2, [0, 1, 2, 0]), (2, [0, -1, 0, 0]), (0, [0, 0, 0, 0])):
        with pytest.raises(RdspError) as ex:
            eng.set_sources(n_src, m)
        assert ex.value.code == -1
    for e in (eng, twin):
        e.set_sources(2, [0, 1, 1, 0])
        e.tune(0, [-9000.0, 100.0, 4000.0, 21000.0])
    y = [e.update_sources(src[:, :8 * 128].contiguous()).cpu().numpy() for e in (eng, twin)]
    for first, st in ((0, [22050.0]), (1, [-22050.0]), (0, [float("nan")]), (0, [1000.0, 2000.0, 22051.0]), (3, [1.0, 2.0]), (-1, [1.0])):
        with pytest.raises(RdspError) as ex:
            eng.tune(first, st)
        assert ex.value.code == -1
    with pytest.raises(RdspError):
        eng.set_sources(1, [0, 1, 1, 0])
    lib, p, o = eng.lib, src.data_ptr(), out.data_ptr()
    row = src.shape[1]
    assert lib.rdsp_engine_update_sources(eng.h, p, 127, 1, o, 8 * 128, None) == -1          # shorter than a block
    assert lib.rdsp_engine_update_sources(eng.h, p, 130, 1, o, 8 * 128, None) == -1          # rows not 16 bytes apart
    assert lib.rdsp_engine_update_sources(eng.h, p + 4, row, 1, o, 8 * 128, None) == -1      # a row not 16-byte aligned
    assert lib.rdsp_engine_update_sources(eng.h, p, row, 9, o, 8 * 128, None) == -1          # more than max_blocks
    assert lib.rdsp_engine_update_sources(eng.h, p, row, 0, o, 8 * 128, None) == 0           # zero blocks: a no-op
    with pytest.raises(RdspError):
        eng.update_sources(src[:, :9 * 128].contiguous())
    y2 = [e.update_sources(src[:, 8 * 128:].contiguous()).cpu().numpy() for e in (eng, twin)]
    assert np.array_equal(y[0], y[1]) and np.array_equal(y2[0], y2[1])
