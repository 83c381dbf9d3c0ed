"""rdsp_channelizer_t on the GPU (include/rdsp.h "channelizer"; kernel csrc/rdsp_channelizer.hip): every comparison exact.
The sub-band rows against tests/channelizer_model.py bit for bit in every format and call split, the widened formats, the
refusals, and the whole line place -> Channelizer.update -> an Engine on the float rows at D2, against the engine on the
model's rows and against OracleEngine on the decimating pass's restatement of each receiver."""
import ctypes as C
import functools

import numpy as np
import pytest

import channelizer_model as CM
from engine_sources_model import DTYPE, FL, S8, S16, U8, TUNING_OFFSET, _to_u8, dphi_of, engine, lib_taps, stream, table, values, widened

pytestmark = pytest.mark.gpu
F32 = np.float32
NSRC, NB = 2, 3
CASES = [(c, S16) for c in CM.CONFIGS[:5]] + [((640, 147, 8, 2), U8), ((16, 1, 16, 3), S8), ((16, 1, 16, 4), FL)]


def _raw(cfg, fmt, n_blocks=NB, seed=3):
    """rows [NSRC, pairs of n_blocks, 2] of format fmt: noise over the whole range, source 0 starting on the rails"""
    m = CM.Model(NSRC, *cfg)
    pairs = m.source_pairs(n_blocks)
    r = np.random.default_rng(seed + fmt)
    if fmt == FL:
        x = (r.uniform(-32768.0, 32767.0, (NSRC, pairs, 2)) / 32768.0).astype(F32)
        x[0, :64] = [[-1.0, 32767.0 / 32768.0], [32767.0 / 32768.0, -1.0]] * 32
        return x
    lo, hi = {S16: (-32768, 32767), U8: (0, 255), S8: (-128, 127)}[fmt]
    x = r.integers(lo, hi + 1, (NSRC, pairs, 2)).astype(DTYPE[fmt])
    x[0, :64] = [[lo, hi], [hi, lo]] * 32
    x[0, 64:128] = hi
    return x


@functools.lru_cache(maxsize=None)
def _want(cfg, fmt):
    """the model's rows of the NB blocks in one call, computed once"""
    w = CM.Model(NSRC, *cfg).stream(fmt, _raw(cfg, fmt), [NB])
    w.setflags(write=False)
    return w


def _device_rows(raw):
    """the rows inside a longer buffer, a ragged (odd) number of pairs apart, from pair 3 on"""
    import torch
    buf = torch.zeros((raw.shape[0], raw.shape[1] + 16 - raw.shape[1] % 2 + 1, 2), dtype=torch.from_numpy(raw[:1, :1]).dtype, device="cuda")
    assert buf.shape[1] % 2 == 1
    buf[:, 3:3 + raw.shape[1]] = torch.from_numpy(raw).cuda()
    return buf[:, 3:3 + raw.shape[1]]


def _run(ch, d, cuts, out_pad=0):
    """the calls of `cuts` blocks through the wrapper, walking through d -> the rows of all calls, on the host"""
    import torch
    at, outs = 0, []
    for nb in cuts:
        pairs = ch.source_pairs(nb)
        out = None if not out_pad else torch.full((ch.n_sources * ch.M, nb * 128 * ch.D2 + out_pad, 2), 7.0, dtype=torch.float32, device="cuda")
        y = ch.update(d[:, at:at + pairs], nb, out=out)
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
    as 1 + 1 + 1 each equal the model's rows (hence each other); after reset the first call gives the same rows again"""
    from radiodsp_sdr_rx_amd.channelizer import Channelizer
    raw, want = _raw(cfg, fmt), _want(cfg, fmt)
    d = _device_rows(raw)
    ch = Channelizer(NSRC, *cfg, fmt=fmt, max_blocks_per_call=NB)
    assert (ch.P, ch.Q, ch.M, ch.D2) == cfg and ch.source_pairs(NB) == raw.shape[1]
    for cuts, pad in (([3], 0), ([1, 2], 6), ([1, 1, 1], 0)):
        ch.reset()
        got = _run(ch, d, cuts, pad)
        assert got.shape == want.shape and _same(got, want), (cfg, fmt, cuts, int(np.argmax((got != want).reshape(len(got), -1).any(1))))
    ch.reset()
    first = ch.update(d[:, :ch.source_pairs(1)], 1).cpu().numpy()
    assert _same(first, want[:, :128 * cfg[3]])


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


def test_stations_to_audio(rdsp, oracle):
    """2 sources at 192 kHz (640 / 147, M = 8, D2 = 2), uint8, three AM stations each, one of them half a spacing less 1 Hz from
    a sub-band centre: place -> Channelizer.update -> an Engine of 6 receivers on the float rows at D2, 4 blocks in two calls.
    The int16 audio equals bit for bit the engine's on the model's rows, and every receiver equals OracleEngine on the
    decimating pass's restatement (engine_sources_model.stream) of its model row"""
    import torch
    from radiodsp_sdr_rx_amd.channelizer import Channelizer
    from radiodsp_sdr_rx_amd.engine import SRC_F32, AMmode
    P, Q, M, D2 = cfg = (640, 147, 8, 2)
    fs, sp, gain, nb = 192000.0, 24000.0, 4.0, 4
    stations = np.array([[2 * sp + sp / 2 - 1.0, -31000.0, 5200.0], [-3 * sp - (sp / 2 - 1.0), 47111.0, -90500.0]])
    model = CM.Model(2, *cfg)
    pairs = model.source_pairs(nb)
    t = np.arange(pairs)
    r = np.random.default_rng(21)
    z = 0.02 * (r.standard_normal((2, pairs)) + 1j * r.standard_normal((2, pairs)))
    for s in range(2):
        for f in stations[s]:
            z[s] += 0.25 * (1 + 0.6 * np.sin(2 * np.pi * r.uniform(300, 2500) / fs * t)) * np.exp(2j * np.pi * f / fs * t + 1j * r.uniform(0, 6))
    raw = _to_u8(np.stack([z.real, z.imag], -1) * 32767.0)
    ch = Channelizer(2, *cfg, fmt=U8, max_blocks_per_call=2)
    ks, res = ch.place(stations.reshape(-1))
    assert list(ks[:3]) == [2, 7, 0] and res[0] == sp / 2 - 1.0 and res[3] == -(sp / 2 - 1.0) and np.all(np.abs(res) <= sp / 2)
    source_of = [int(s * M + k) for s, k in zip([0, 0, 0, 1, 1, 1], ks)]

    def receivers():
        e = engine(6, 2)
        e.sketch_setup()
        e.setDemodMode(AMmode)
        e.set_sources(2 * M, source_of)
        e.set_source_decimation(D2, gain)
        e.set_source_format(SRC_F32)
        e.tune(0, res)
        return e

    want_rows = model.stream(U8, raw, [nb])
    d, e1, e2 = _device_rows(raw), receivers(), receivers()
    dm = torch.from_numpy(want_rows).cuda()
    at, y1, y2 = 0, [], []
    for b in (0, 2):
        p = ch.source_pairs(2)
        rows = ch.update(d[:, at:at + p], 2)
        at += p
        assert _same(rows.cpu().numpy(), want_rows[:, b * 128 * D2:(b + 2) * 128 * D2])
        y1.append(e1.update_sources(rows, n_blocks=2).cpu().numpy())
        y2.append(e2.update_sources(dm[:, b * 128 * D2:(b + 2) * 128 * D2], n_blocks=2).cpu().numpy())
    y1, y2 = np.concatenate(y1, 1), np.concatenate(y2, 1)
    assert np.array_equal(y1, y2) and np.array_equal(y1[..., 0], y1[..., 1]) and np.abs(y1).max() > 1000
    tab, h2 = table(rdsp), lib_taps(D2, 1, gain)
    for c in range(6):
        step = dphi_of(TUNING_OFFSET[AMmode], res[c], D2, 1)
        tuned = stream(values(FL, want_rows[source_of[c]]), D2, 1, h2, np.full((1, nb), step, np.uint64), tab)[0][0]
        assert np.array_equal(y1[c, :, 0], oracle.OracleEngine().run(tuned, [[0, "setDemodMode", AMmode]])), c
