"""rdsp_channelizer_t on the GPU (include/rdsp.h "channelizer"; kernel csrc/rdsp_channelizer.hip): every comparison exact.
The sub-band rows against tests/channelizer_model.py bit for bit in every format and call split, the widened formats, the
refusals, and the whole line place -> Channelizer.update -> an Engine on the float rows at D2, against the engine on the
model's rows and against OracleEngine on the decimating pass's restatement of each receiver.  The edges (CM.EDGE: T mod M != 0
at M = 16 and 64, Tb <= M, P1 = Q1, the largest LDS plan, D2 = 16), one source and 67, a call whose schedule passes 2^32, float
rows with NaN, infinities and subnormals, and a second whole line through row M / 2 have tests of their own; docs/engine.md
lists what each pins."""
import ctypes as C
import functools

import numpy as np
import pytest

import channelizer_model as CM
from engine_sources_model import DTYPE, FL, S8, S16, U8, TUNING_OFFSET, _int16, _to_u8, dphi_of, engine, fma32, lib_taps, stream, table, values, widened

pytestmark = pytest.mark.gpu
F32 = np.float32
NSRC, NB = 2, 3
ROT = (U8, S8, FL, S16)
# the formats rotate over CM.EDGE, and its two M = 16 entries come once more two formats on: every format meets T mod M != 0 at M = 16
EDGE_CASES = [(c, ROT[i % 4]) for i, c in enumerate(CM.EDGE)] + [(c, ROT[(i + 2) % 4]) for i, c in enumerate(CM.EDGE) if c[2] == 16]
CASES = ([(c, S16) for c in CM.CONFIGS[:5]] + [((640, 147, 8, 2), U8), ((16, 1, 16, 3), S8), ((16, 1, 16, 4), FL)]
         + [((20480, 441, 32, 4), S8)] + EDGE_CASES)
assert {f for c, f in EDGE_CASES if c[2] == 16} == set(ROT) and {c for c, _ in EDGE_CASES} == set(CM.EDGE)


def _blocks(cfg):
    """blocks of a bit-for-bit case: 3, and 2 for the M = 64 entries of CM.EDGE (the model's time)"""
    return 2 if cfg in CM.EDGE and cfg[2] == 64 else NB


def _raw(cfg, fmt, n_blocks=NB, seed=3, n_sources=NSRC):
    """rows [n_sources, pairs of n_blocks, 2] of format fmt: noise over the whole range, source 0 starting on the rails"""
    m = CM.Model(n_sources, *cfg)
    pairs = m.source_pairs(n_blocks)
    r = np.random.default_rng(seed + fmt)
    if fmt == FL:
        x = (r.uniform(-32768.0, 32767.0, (n_sources, pairs, 2)) / 32768.0).astype(F32)
        x[0, :64] = [[-1.0, 32767.0 / 32768.0], [32767.0 / 32768.0, -1.0]] * 32
        return x
    lo, hi = {S16: (-32768, 32767), U8: (0, 255), S8: (-128, 127)}[fmt]
    x = r.integers(lo, hi + 1, (n_sources, pairs, 2)).astype(DTYPE[fmt])
    x[0, :64] = [[lo, hi], [hi, lo]] * 32
    x[0, 64:128] = hi
    return x


@functools.lru_cache(maxsize=None)
def _want(cfg, fmt):
    """the model's rows of the case's blocks in one call, computed once"""
    w = CM.Model(NSRC, *cfg).stream(fmt, _raw(cfg, fmt, _blocks(cfg)), [_blocks(cfg)])
    w.setflags(write=False)
    return w


def _device_rows(raw):
    """the rows inside a longer buffer, a ragged (odd) number of pairs apart, from pair 3 on"""
    import torch
    buf = torch.zeros((raw.shape[0], raw.shape[1] + 16 - raw.shape[1] % 2 + 1, 2), dtype=torch.from_numpy(raw[:1, :1]).dtype, device="cuda")
    assert buf.shape[1] % 2 == 1
    buf[:, 3:3 + raw.shape[1]] = torch.from_numpy(raw).cuda()
    return buf[:, 3:3 + raw.shape[1]]


def _run(ch, d, cuts, out_pad=0, rest=False):
    """the calls of `cuts` blocks through the wrapper, walking through d -> the rows of all calls, on the host; with rest, a
    call is handed all the pairs from its first on, more than it takes"""
    import torch
    at, outs = 0, []
    for nb in cuts:
        pairs = ch.source_pairs(nb)
        out = None if not out_pad else torch.full((ch.n_sources * ch.M, nb * 128 * ch.D2 + out_pad, 2), 7.0, dtype=torch.float32, device="cuda")
        y = ch.update(d[:, at:] if rest else d[:, at:at + pairs], nb, out=out)
        if out_pad:
            assert bool((out[:, nb * 128 * ch.D2:] == 7.0).all())
        outs.append(y.cpu().numpy())
        at += pairs
    assert at == d.shape[1]
    return np.concatenate(outs, 1)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("cfg,fmt", CASES)
def test_rows_equal_the_model_bit_for_bit(rdsp, cfg, fmt):
    """two sources, rows a ragged stride apart inside a longer buffer, source 0 on the rails: 3 blocks as one call, as 1 + 2 and
    as 1 + 1 + 1 each equal the model's rows (hence each other); after reset the first call gives the same rows again.  The
    cases: five of the six configurations as int16 and three in the other formats; 20480 / 441 (Q1 = 441) as int8; and every
    entry of CM.EDGE, the formats rotating, its M = 64 entries on 2 blocks as one call and as 1 + 1"""
    from radiodsp_sdr_rx_amd.channelizer import Channelizer
    nb = _blocks(cfg)
    raw, want = _raw(cfg, fmt, nb), _want(cfg, fmt)
    d = _device_rows(raw)
    ch = Channelizer(NSRC, *cfg, fmt=fmt, max_blocks_per_call=nb)
    assert (ch.P, ch.Q, ch.M, ch.D2) == cfg and ch.source_pairs(nb) == raw.shape[1]
    for cuts, pad in ((([3], 0), ([1, 2], 6), ([1, 1, 1], 0)) if nb == NB else (([2], 0), ([1, 1], 6))):
        ch.reset()
        got = _run(ch, d, cuts, pad)
        assert got.shape == want.shape and _same(got, want), (cfg, fmt, cuts, int(np.argmax((got != want).reshape(len(got), -1).any(1))))
    ch.reset()
    first = ch.update(d[:, :ch.source_pairs(1)], 1).cpu().numpy()
    assert _same(first, want[:, :128 * cfg[3]])


@pytest.mark.parametrize("n_sources", [1, 67])
def test_one_source_and_many(rdsp, n_sources):
    """(2, 1, 8, 2), int16, 2 + 1 blocks against the model: one source (the wrapper's stride of a lone row, with exactly the
    pairs a call takes and with more), and 67 sources (blockIdx.y far past 1).  Every source row is distinct and starts with
    three pairs of its own number, and so is every row of the model's answer: a swap of sources or rows cannot pass"""
    from radiodsp_sdr_rx_amd.channelizer import Channelizer
    cfg = (2, 1, 8, 2)
    raw = _raw(cfg, S16, n_sources=n_sources, seed=40)
    raw[:, :3] = np.arange(n_sources, dtype=np.int16)[:, None, None]
    want = CM.Model(n_sources, *cfg).stream(S16, raw, [2, 1])
    assert len({x.tobytes() for x in raw}) == n_sources and len({w.tobytes() for w in want}) == len({w[:64].tobytes() for w in want}) == n_sources * 8
    d = _device_rows(raw)
    ch = Channelizer(n_sources, *cfg, max_blocks_per_call=2)
    for rest in ((False, True) if n_sources == 1 else (False,)):
        ch.reset()
        got = _run(ch, d, [2, 1], rest=rest)
        assert got.shape == want.shape and _same(got, want), (n_sources, rest, int(np.argmax((got != want).reshape(len(got), -1).any(1))))


def test_a_call_past_2_to_the_32(rdsp):
    """(20480, 441, 32, 4), uint8, one source, ONE call of 1640 blocks: 839 680 outputs a sub-band, and frac + (i + 1) P1 with
    P1 = 5120 passes 2^32 from output 838 860 on, where a schedule formed in 32 bits takes other branches (asserted).  Tiles of
    64 instants, picked on the device, equal the model's (Model.call's at=): the first two, the tile that holds output 838 860
    and the one before it, the last, four drawn.  A second call of one block, which carries the large call's frac, T mod M
    and history, equals the model's whole"""
    import torch
    from radiodsp_sdr_rx_amd.channelizer import Channelizer
    cfg, nb = (20480, 441, 32, 4), 1640
    m = CM.Model(1, *cfg)
    n_out = nb * 128 * cfg[3]
    first = -(-(1 << 32) // m.P1) - 1                       # the first output i with (i + 1) P1 >= 2^32
    assert (m.P1, m.Q1) == (5120, 441) and (n_out + 1) * m.P1 >= 1 << 32 and first == 838860 and first + 64 < n_out
    r = np.random.default_rng(32)
    tiles = np.concatenate([[0, 1, first // 64 - 1, first // 64, n_out // 64 - 1], r.integers(2, first // 64 - 1, 4)])
    idx = (tiles[:, None] * 64 + np.arange(64)[None, :]).reshape(-1)
    late = idx[idx >= first]
    assert len(late) >= 64 + 64 - first % 64 and np.all((((late + 1) * m.P1) % (1 << 32)) % m.Q1 != ((late + 1) * m.P1) % m.Q1)
    pairs, total = m.source_pairs(nb), CM.Model(1, *cfg).source_pairs(nb + 1)
    raw = r.integers(0, 256, (1, total, 2)).astype(np.uint8)
    vals = values(U8, raw)
    want = m.call(vals[:, :pairs], nb, at=idx)
    assert (m.frac, m.T % 32) != (0, 0)
    d = torch.from_numpy(raw).cuda()
    ch = Channelizer(1, *cfg, fmt=U8, max_blocks_per_call=nb)
    assert ch.source_pairs(nb) == pairs
    y = ch.update(d[:, :pairs], nb)
    assert tuple(y.shape) == (32, n_out, 2)
    got = y[:, torch.from_numpy(idx).cuda()].cpu().numpy()
    del y
    bad = (got != want).reshape(32, len(tiles), -1).any((0, 2))
    assert _same(got, want), [int(t) for t in tiles[bad]]
    assert ch.source_pairs(1) == total - pairs == m.source_pairs(1)
    assert _same(ch.update(d[:, pairs:], 1).cpu().numpy(), m.call(vals[:, pairs:], 1))


SALT = np.array([np.nan, np.inf, -np.inf, 3e38, -3e38, 256.5, -256.5, -0.0, 1e-40], F32)


def _flushing_fma32(a, b, c):
    """fma32 as an object built to flush subnormals would compute it: subnormal operands read as zeros, a subnormal result
    leaves as zero"""
    tiny = np.finfo(F32).tiny
    a, b, c = (np.where(np.abs(v) < tiny, F32(0.0), np.asarray(v, F32)).astype(F32) for v in (a, b, c))
    y = fma32(a, b, c)
    return np.where(np.abs(y) < tiny, F32(0.0), y).astype(F32)


def _special_rows(cfg):
    """-> (F32 rows [2, pairs of 3 blocks, 2], the model's rows of them).  Noise at +-0.05 of full scale.  Source 1 carries NaN,
    +-inf, +-3e38, +-256.5, -0.0 and 1e-40 (each of them, in a drawn component) among its first Tb pairs, among the last Tb
    pairs of every call of 1 + 1 + 1 (so they pass through the kept history) and at forty drawn places; and, behind Tb pairs
    of zeros, one run of 64 pairs (longer than Tb) of magnitudes rising from 1e-38 to 1e-33, with no salt within Tb of it.
    No NaN is in the model's rows.  That subnormals take part is read off them in two ways, both asserted: outputs of
    source 1 are themselves subnormal (a zero exponent field over a non-zero mantissa), and the model evaluated once more
    with _flushing_fma32 in place of fma32 gives other bits in outputs that are not subnormal: those depend on a subnormal
    term"""
    M = cfg[2]
    m = CM.Model(NSRC, *cfg)
    Tb = m.Tb
    ends = [m.source_pairs(b) for b in (1, 2, 3)]
    pairs = ends[-1]
    r = np.random.default_rng(29)
    x = r.uniform(-0.05, 0.05, (NSRC, pairs, 2)).astype(F32)
    run = ends[0] + 4 * Tb
    assert Tb < 64 and run + 64 + Tb < ends[1] - Tb
    x[1, run - Tb:run] = 0.0
    x[1, run:run + 64] = (r.choice([-1.0, 1.0], (64, 2)) * 10.0 ** np.linspace(-38.0, -33.0, 128).reshape(64, 2)).astype(F32)
    assert np.abs(x[1, run:run + 64]).min() > 0 and (np.abs(x[1, run:run + 64]) < np.finfo(F32).tiny).any()
    free = np.setdiff1d(np.arange(Tb, pairs), np.concatenate([np.arange(run - 2 * Tb, run + 64 + Tb)] + [np.arange(e - Tb, e) for e in ends]))
    for start in [0] + [e - Tb for e in ends]:
        x[1, start + r.choice(Tb, len(SALT), replace=False), r.integers(0, 2, len(SALT))] = SALT
    x[1, r.choice(free, 40, replace=False), r.integers(0, 2, 40)] = r.choice(SALT, 40)
    for e in ends:
        assert np.isnan(x[1, e - Tb:e]).any() and np.isinf(x[1, e - Tb:e]).any()
    assert np.isnan(x[1, :Tb]).any() and np.signbit(x[1][x[1] == 0]).any() and not np.isnan(x[0]).any()
    want = m.stream(FL, x, [3])
    bits = want.view(np.uint32)
    sub = ((bits & np.uint32(0x7F800000)) == 0) & ((bits & np.uint32(0x007FFFFF)) != 0)
    CM.fma32 = _flushing_fma32
    try:
        other = (CM.Model(NSRC, *cfg).stream(FL, x, [3]).view(np.uint32) != bits) & ~sub
    finally:
        CM.fma32 = fma32
    print(f"{cfg}: {int(sub.sum())} subnormal outputs in {int(sub.any((1, 2)).sum())} rows; flushing changes {int(other.sum())} more in "
          f"{int(other.any((1, 2)).sum())} rows; the largest output {np.abs(want).max():.1f}")
    assert not np.isnan(want).any() and not sub[:M].any() and not other[:M].any()
    assert sub[M:].any((1, 2)).sum() >= M // 2 and other[M:].any((1, 2)).all() and other.sum() >= 4 * M
    return x, want


@pytest.mark.parametrize("cfg", [(640, 147, 8, 2), (320, 147, 16, 2)])
def test_float_rows_with_specials(rdsp, cfg):
    """the rows of _special_rows (NaN, +-inf, wild, clamped, -0.0 and subnormal values among noise; subnormal terms and outputs):
    3 blocks as one call and as 1 + 1 + 1 equal the model's rows bit for bit, and no NaN is in them"""
    from radiodsp_sdr_rx_amd.channelizer import Channelizer
    x, want = _special_rows(cfg)
    d = _device_rows(x)
    ch = Channelizer(NSRC, *cfg, fmt=FL, max_blocks_per_call=NB)
    for cuts in ([3], [1, 1, 1]):
        ch.reset()
        got = _run(ch, d, cuts)
        assert not np.isnan(got).any(), cuts
        assert got.shape == want.shape and _same(got, want), (cfg, cuts, int(np.argmax((got != want).reshape(len(got), -1).any(1))))


def test_widened_formats(rdsp):
    """U8 and S8 rows give the bits of S16 on the row widened by the table of values; F32 rows of k / 32768 the bits of the
    int16 row k"""
    from radiodsp_sdr_rx_amd.channelizer import Channelizer
    cfg = (640, 147, 8, 2)
    for fmt in (U8, S8, FL):
        raw = _raw(cfg, S16, seed=9).astype(np.float32) / np.float32(32768.0) if fmt == FL else _raw(cfg, fmt, seed=9)
        wide16 = _raw(cfg, S16, seed=9) if fmt == FL else widened(fmt, raw)
        assert np.array_equal(values(fmt, raw), values(S16, wide16))
        a = _run(Channelizer(NSRC, *cfg, fmt=fmt, max_blocks_per_call=NB), _device_rows(raw), [1, 2])
        b = _run(Channelizer(NSRC, *cfg, fmt=S16, max_blocks_per_call=NB), _device_rows(wide16), [3])
        assert _same(a, b), fmt


def test_refusals_change_nothing(rdsp):
    """the configurations include/rdsp.h refuses are refused at create; a refused update (short stride, too many blocks, a
    misaligned or short output, a misaligned source row) returns RDSP_ERR_INVALID with a text and leaves the object as it was:
    the next good call equals the model, in the middle of a stream as well"""
    import torch
    from radiodsp_sdr_rx_amd.channelizer import Channelizer
    for P, Q, M, D2 in CM.REFUSED + [(16, 1, 12, 4), (16, 1, 16, 1)]:
        with pytest.raises(rdsp.RdspError):
            Channelizer(NSRC, P, Q, M, D2)
    for bad in (dict(n_sources=0), dict(fmt=4), dict(max_blocks_per_call=0)):
        with pytest.raises(rdsp.RdspError):
            Channelizer(**{**dict(n_sources=NSRC, P=16, Q=1, M=16, D2=4), **bad})
    cfg = (16, 1, 16, 3)
    raw, want = _raw(cfg, S16), _want(cfg, S16)
    d = _device_rows(raw)
    ch = Channelizer(NSRC, *cfg, max_blocks_per_call=2)
    lib, s = ch.lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n1 = 128 * cfg[3]
    out = torch.zeros((NSRC * 16, 2 * n1 + 2, 2), dtype=torch.float32, device="cuda")
    stride = d.stride(0) // 2

    def refused(at):
        pairs = ch.source_pairs(1)
        src = d[:, at:].data_ptr()
        calls = [(src, pairs - 1, 1, out.data_ptr(), out.stride(0) // 2),            # a stride below source_pairs
                 (src, stride, 3, out.data_ptr(), out.stride(0) // 2),               # more blocks than the object was made for
                 (src, stride, -1, out.data_ptr(), out.stride(0) // 2),
                 (src, stride, 1, out.data_ptr() + 8, out.stride(0) // 2),           # d_sub not 16-byte aligned
                 (src, stride, 1, out.data_ptr(), n1 + 1),                           # an odd sub_stride
                 (src, stride, 1, out.data_ptr(), n1 - 2),                           # a short one
                 (src + 2, stride, 1, out.data_ptr(), out.stride(0) // 2),           # a source row off its pair
                 (None, stride, 1, out.data_ptr(), out.stride(0) // 2),
                 (src, stride, 1, None, out.stride(0) // 2)]
        for a in calls:
            assert lib.rdsp_channelizer_update(ch.h, a[0], a[1], a[2], a[3], a[4], s) == -1 and lib.rdsp_last_error()
        assert ch.source_pairs(1) == pairs

    refused(0)
    p1 = ch.source_pairs(1)
    a = ch.update(d[:, :p1], 1, out=out).cpu().numpy()
    assert _same(a, want[:, :n1])
    refused(p1)
    b = ch.update(d[:, p1:], 2, out=out).cpu().numpy()
    assert _same(b, want[:, n1:])
    assert lib.rdsp_channelizer_update(ch.h, None, 0, 0, None, 0, s) == 0                # a call of no blocks is a good call


def _am_band(cfg, stations, seed, nb=4):
    """2 sources at the rate of cfg, nb blocks: noise and, per source, its stations as AM carriers -> [2, pairs, 2] in counts"""
    P, Q, M, D2 = cfg
    fs = (P * 44100.0) / Q
    pairs = CM.Model(2, *cfg).source_pairs(nb)
    t = np.arange(pairs)
    r = np.random.default_rng(seed)
    z = 0.02 * (r.standard_normal((2, pairs)) + 1j * r.standard_normal((2, pairs)))
    for s in range(2):
        for f in stations[s]:
            z[s] += 0.25 * (1 + 0.6 * np.sin(2 * np.pi * r.uniform(300, 2500) / fs * t)) * np.exp(2j * np.pi * f / fs * t + 1j * r.uniform(0, 6))
    return np.stack([z.real, z.imag], -1) * 32767.0


def _to_audio(rdsp, oracle, cfg, fmt, raw, stations, n_lsb=0, nb=4, gain=4.0):
    """the whole line on rows `raw` [2, pairs of nb blocks, 2] of format fmt, a receiver on each of the three stations a source,
    the first n_lsb of them a group in LSB and the rest in AM: place -> Channelizer.update -> an Engine on the float rows at
    D2, two calls of nb / 2 blocks.  The rows equal the model's; the int16 audio equals bit for bit the engine's on the
    model's rows; every receiver is heard and equals OracleEngine on the decimating pass's restatement
    (engine_sources_model.stream) of its model row"""
    import torch
    from radiodsp_sdr_rx_amd.channelizer import Channelizer
    from radiodsp_sdr_rx_amd.engine import SRC_F32, AMmode, LSBmode
    P, Q, M, D2 = cfg
    model = CM.Model(2, *cfg)
    ch = Channelizer(2, *cfg, fmt=fmt, max_blocks_per_call=nb // 2)
    ks, res = ch.place(stations.reshape(-1))
    source_of = [int(s * M + k) for s, k in zip([0, 0, 0, 1, 1, 1], ks)]

    def receivers():
        e = engine(6, nb // 2)
        e.sketch_setup()
        if n_lsb:
            e.set_groups([0, n_lsb])
            e.select_group(1)
        e.setDemodMode(AMmode)
        if n_lsb:
            e.select_group(-1)
        e.set_sources(2 * M, source_of)
        e.set_source_decimation(D2, gain)
        e.set_source_format(SRC_F32)
        e.tune(0, res)
        return e

    want_rows = model.stream(fmt, raw, [nb])
    d, e1, e2 = _device_rows(raw), receivers(), receivers()
    dm = torch.from_numpy(want_rows).cuda()
    at, y1, y2 = 0, [], []
    for b in (0, nb // 2):
        p = ch.source_pairs(nb // 2)
        rows = ch.update(d[:, at:at + p], nb // 2)
        at += p
        assert _same(rows.cpu().numpy(), want_rows[:, b * 128 * D2:(b + nb // 2) * 128 * D2])
        y1.append(e1.update_sources(rows, n_blocks=nb // 2).cpu().numpy())
        y2.append(e2.update_sources(dm[:, b * 128 * D2:(b + nb // 2) * 128 * D2], n_blocks=nb // 2).cpu().numpy())
    y1, y2 = np.concatenate(y1, 1), np.concatenate(y2, 1)
    assert np.array_equal(y1, y2) and np.array_equal(y1[..., 0], y1[..., 1]) and np.abs(y1).max() > 1000
    tab, h2 = table(rdsp), lib_taps(D2, 1, gain)
    for c in range(6):
        mode = LSBmode if c < n_lsb else AMmode
        step = dphi_of(TUNING_OFFSET[mode], res[c], D2, 1)
        tuned = stream(values(FL, want_rows[source_of[c]]), D2, 1, h2, np.full((1, nb), step, np.uint64), tab)[0][0]
        calls = [] if mode == LSBmode else [[0, "setDemodMode", AMmode]]
        assert np.array_equal(y1[c, :, 0], oracle.OracleEngine().run(tuned, calls)), c
        assert np.abs(y1[c]).max() > 100, c


def test_stations_to_audio(rdsp, oracle):
    """2 sources at 192 kHz (640 / 147, M = 8, D2 = 2), uint8, three AM stations each, one of them half a spacing less 1 Hz from
    a sub-band centre: place -> Channelizer.update -> an Engine of 6 receivers on the float rows at D2, 4 blocks in two calls.
    The int16 audio equals bit for bit the engine's on the model's rows, and every receiver equals OracleEngine on the
    decimating pass's restatement (engine_sources_model.stream) of its model row"""
    from radiodsp_sdr_rx_amd import channelizer
    cfg, sp = (640, 147, 8, 2), 24000.0
    stations = np.array([[2 * sp + sp / 2 - 1.0, -31000.0, 5200.0], [-3 * sp - (sp / 2 - 1.0), 47111.0, -90500.0]])
    raw = _to_u8(_am_band(cfg, stations, 21))
    ks, res = channelizer.place(*cfg[:3], stations.reshape(-1))
    assert list(ks[:3]) == [2, 7, 0] and res[0] == sp / 2 - 1.0 and res[3] == -(sp / 2 - 1.0) and np.all(np.abs(res) <= sp / 2)
    _to_audio(rdsp, oracle, cfg, U8, raw, stations)


def test_stations_to_audio_at_the_band_edge(rdsp, oracle):
    """a second whole line: 2 sources at 192 kHz as (640, 147, 16, 3) -- M = 16 with T mod M != 0 in the second call --, int16,
    per source a station half a spacing less 1 Hz from a centre, one at -(fs / 2 - 5000) Hz in row M / 2 (the band's edge, whose
    centre -fs / 2 is negative) and one in row M - 3; the first two receivers are a group in LSB, the rest AM.  What is
    asserted is _to_audio's, as for test_stations_to_audio"""
    from radiodsp_sdr_rx_amd import channelizer
    cfg, fs, sp = (640, 147, 16, 3), 192000.0, 12000.0
    edge = -(fs / 2 - 5000.0)
    stations = np.array([[2 * sp + sp / 2 - 1.0, edge, -3 * sp + 1234.5], [-5 * sp - (sp / 2 - 1.0), edge, -3 * sp - 2750.0]])
    z = _am_band(cfg, stations, 22)
    raw = _int16(z[..., 0] + 1j * z[..., 1])
    ks, res = channelizer.place(*cfg[:3], stations.reshape(-1))
    assert list(ks) == [2, 8, 13, 11, 8, 13] and list(res) == [sp / 2 - 1.0, 5000.0, 1234.5, -(sp / 2 - 1.0), 5000.0, -2750.0]
    assert CM.centre_hz(*cfg[:3], 8) == -fs / 2 and CM.Model(2, *cfg).source_pairs(2) % 16 != 0
    _to_audio(rdsp, oracle, cfg, S16, raw, stations, n_lsb=2)
