"""The engine law of the chain's tail stage (rdsp_chain_set_tail_law(chain, RDSP_TAIL_ENGINE), include/rdsp.h).

Under RDSP_TAIL_ENGINE, A9 and A8 are the reference engine's own hang AGC and 55-tap ALS filter, in the engine's order,
and the chain's float audio is held to the image's stage taps bit for bit: on the fixture's own taps
(tests/golden/engine_kat.npz), on long streams the CPU restatement taps (`OracleEngine(taps=True)`, pinned on the fixture
by tests/test_tail_law_oracle.py), and through the whole chain at the bench shapes by composition: the chain with the law
equals the same chain without AGC / ALS, fed through rdsp_chain_run_tail_f32 of a fresh engine-law chain, then the
output gain.  Comparisons are bit for bit (uint32 views) throughout.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ENGINE_RATE = dict(fs_in=44100.0, decim=1, nco_hz=0.0, fft_l=256, demod="IQ")   # the engine's 44.1 kHz, no decimation
SKETCH = [[0, "enableAGC"], [0, "setAGCmode", 2], [0, "disableALSfilter"]]       # OracleEngine's sketch set-up: AGC / ALS part


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def assert_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, (what, bad.size, bad[:4], got.reshape(-1)[bad[:4]], want.reshape(-1)[bad[:4]])


def tail_calls(calls):
    """the calls of a case that concern the AGC / ALS filter (the only settings the tail stage reads)"""
    return [c for c in calls if "AGC" in c[1] or "ALS" in c[1]]


def apply_calls(ch, calls, block=None):
    for c in calls:
        if block is None or c[0] == block:
            getattr(ch, c[1])(*c[2:])


def engine_chain(nch, nblk, **cfg):
    from radiodsp_sdr_rx_amd.chain import Chain
    ch = Chain(nch, max_blocks_per_call=nblk, **dict(ENGINE_RATE, **cfg))
    ch.set_tail_law("engine")
    assert ch.tail_law == 1
    return ch


def engine_state(ch, n):
    """(env, gain, hang) of every channel, out of the state blob's engine-law part (its last two parts)"""
    blob = ch.save_state()
    st = blob[blob.size - n * (16 + 512): blob.size - n * 512].view(np.float32).reshape(n, 4)
    return st[:, 0], st[:, 1], st[:, 2].view(np.int32)


def q15(rdsp, x):
    import ctypes as C
    import torch
    x = x.contiguous()
    y = torch.empty(x.shape, dtype=torch.int16, device=x.device)
    from radiodsp_sdr_rx_amd import _lib
    _lib.check(_lib.load().rdsp_float_to_q15(C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), x.numel(), None))
    torch.cuda.synchronize()
    return y


# ---- 1. the fixture's own stage taps --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nch", [1, 97])
def test_engine_law_reproduces_the_images_stage_taps(rdsp, nch):
    import torch
    kat = np.load(os.path.join(HERE, "golden", "engine_kat.npz"))
    cases = [n[:-len("_tap_filt")] for n in kat.files if n.endswith("_tap_filt")]
    assert len(cases) == 9
    for name in cases:
        calls = tail_calls(SKETCH + json.loads(str(kat[name + "_calls"])))
        assert all(c[0] == 0 for c in calls)
        filt = kat[name + "_tap_filt"][:, 0, :].reshape(-1)
        nblk = len(filt) // 128
        for als_off, key in ((True, "agc"), (False, "als")):
            ch = engine_chain(nch, nblk)
            apply_calls(ch, calls)
            if als_off:
                ch.disableALSfilter()
            x = torch.from_numpy(np.tile(filt, (nch, 1))).cuda()
            ch.run_tail_f32(x)
            got = x.cpu().numpy()
            want = kat[f"{name}_tap_{key}"][:, 0, :].reshape(-1)
            assert_bits(got, np.tile(want, (nch, 1)), (name, key, nch))


# ---- 2. long streams against the restatement --------------------------------------------------------------------------
def test_engine_law_follows_the_restatement_over_long_streams_in_ragged_calls(rdsp, oracle):
    """64 channels x 864 blocks: the slow mode's 88 200-sample hang (689 blocks) starts at the last loud block (~100) and
    ends inside the run; setAGCmode 1 -> 3, ALS off / on (the line and taps cleared), notch <-> peak mid-stream, all at
    boundaries of calls of 1, 7 and 64 blocks"""
    import torch
    nch, nblk, sizes = 64, 864, (1, 7, 64)
    calls = [[0, "setAGCmode", 1], [0, "enableALSfilter"], [0, "setALSfilterNotch"], [72, "setAGCmode", 3],
             [216, "disableALSfilter"], [289, "enableALSfilter"], [432, "setALSfilterPeak"], [577, "setALSfilterNotch"]]
    n = nblk * 128
    t = np.arange(n) / 44100.0
    filt, als, fin = [], [], []
    for c in range(nch):
        rng = np.random.default_rng(1000 + c)
        env = np.where(np.arange(n) < 100 * 128, 0.3 + 0.05 * (c % 5), 0.004)
        f = 8390.0 - (500.0 + 23.0 * c)
        i = env * (np.cos(2 * np.pi * f * t) + 0.03 * rng.standard_normal(n))
        q = env * (np.sin(2 * np.pi * f * t) + 0.03 * rng.standard_normal(n))
        iq = np.clip(np.round(np.stack([i, q], 1) * 32767), -32768, 32767).astype(np.int16)
        e = oracle.OracleEngine(taps=True)
        e.run(iq, calls)
        filt.append(np.stack(e.taps["filt"])[:, 0, :].reshape(-1))
        als.append(np.stack(e.taps["als"])[:, 0, :].reshape(-1))
        fin.append(e.final())
    filt, als, fin = np.stack(filt), np.stack(als), np.stack(fin)
    assert (fin[:, 3] == 0).all()                                 # every slow hang ran out inside the run
    ch = engine_chain(nch, 64)
    apply_calls(ch, tail_calls(SKETCH))
    x = torch.from_numpy(filt).cuda()
    b, k = 0, 0
    while b < nblk:
        m = min(sizes[k % 3], nblk - b)
        apply_calls(ch, calls, block=b)
        assert all(c[0] < b or c[0] >= b + m or c[0] == b for c in calls)
        ch.run_tail_f32(x[:, b * 128:(b + m) * 128])
        b, k = b + m, k + 1
    assert_bits(x.cpu().numpy(), als, "ALS tap")
    env, gain, hang = engine_state(ch, nch)
    assert_bits(ch.scalars()[:, 1], fin[:, 1], "gain (scalars slot 1)")
    assert_bits(gain, fin[:, 1], "gain")
    assert_bits(env, fin[:, 2], "envelope")
    assert np.array_equal(hang.astype(np.float32), fin[:, 3])


# ---- 3 - 5. composition through the whole chain -------------------------------------------------------------------------
def compose(rdsp, cfg, nch, nblk, fir_a, fir_b, sub_batch=None, timing=False):
    """chain A (engine law) against chain B (no AGC / ALS, output gain 1) -> run_tail_f32 of a fresh engine-law chain ->
    x output gain, bit for bit; A's int16 against rdsp_float_to_q15 of A's floats"""
    import torch
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    dev = torch.from_numpy(synth_iq(nch, nblk * 128, cw=cfg.get("demod") == "CW_USB", n_threads=16)).cuda()
    a = Chain(nch, max_blocks_per_call=nblk, fir_variant=fir_a, **cfg)
    a.set_tail_law("engine")
    a.set_pipelined(True)
    if sub_batch is not None:
        a.set_sub_batch(sub_batch)
    if timing:
        a.set_timing(True)
    a16, a32 = a.process(dev, want_f32=True)
    a.flush()
    b = Chain(nch, max_blocks_per_call=nblk, fir_variant=fir_b, **dict(cfg, agc_mode="off", als_mode="off", output_gain=1.0))
    b.set_pipelined(True)
    _, b32 = b.process(dev, want_f32=True)
    b.flush()
    torch.cuda.synchronize()
    c = Chain(nch, max_blocks_per_call=nblk, **cfg)
    c.set_tail_law("engine")
    y = b32[..., 0].contiguous()
    c.run_tail_f32(y)
    y = y * np.float32(cfg.get("output_gain", 1.0))
    torch.cuda.synchronize()
    for side in (0, 1):
        got = a32[..., side].cpu().numpy()
        assert_bits(got, y.cpu().numpy(), ("out_f32", side))
    assert torch.equal(a16, q15(rdsp, a32))
    assert float(a32[..., 0].abs().max()) > 0.01
    return a


@pytest.mark.parametrize("fir", [2, None])
def test_engine_law_composes_at_k3s_shape(rdsp, fir):
    from cases import K3
    compose(rdsp, K3, 4096, 512, fir, 4 if fir is None else fir)   # B has no tail: its default would be the row form


def test_engine_law_composes_at_k5s_shape_in_sub_batches(rdsp):
    from cases import K3
    compose(rdsp, K3, 8192, 512, 2, 2, sub_batch=4096)


def test_engine_law_composes_behind_dsp_nr(rdsp, front_form):
    """lms_nr 15: A7 runs as today (x 1.1, CONV:334), then the engine AGC and ALS filter"""
    from cases import K3
    compose(rdsp, dict(K3, lms_nr=15), 256, 64, None, None)


@pytest.mark.parametrize("fir", [2, None])
def test_engine_agc_alone_launches_a_tail_stage_at_k4s_shape(rdsp, fir):
    from cases import K4
    a = compose(rdsp, K4, 8192, 512, fir, 4 if fir is None else fir, timing=True)
    front_ms, tail_ms, calls = a.get_timing()
    assert calls == 1 and tail_ms > 0.0
    assert a.front_kernel_name() == "rdsp_front_fd_kernel"


# ---- 6. invariances -------------------------------------------------------------------------------------------------------
def run_stream(ch, dev, splits):
    import torch
    outs, b = [], 0
    for m in splits:
        o16, o32 = ch.process(dev[:, b * 128:(b + m) * 128], want_f32=True)
        outs.append((o16, o32))
        b += m
    ch.flush()
    torch.cuda.synchronize()
    return (np.concatenate([o[0].cpu().numpy() for o in outs], 1), np.concatenate([o[1].cpu().numpy() for o in outs], 1))


def engine_k3(nch, nblk, fir=None, pipelined=False, sub_batch=None):
    from cases import K3
    from radiodsp_sdr_rx_amd.chain import Chain
    ch = Chain(nch, max_blocks_per_call=nblk, fir_variant=fir, **K3)
    ch.set_tail_law("engine")
    ch.set_pipelined(pipelined)
    if sub_batch is not None:
        ch.set_sub_batch(sub_batch)
    return ch


def test_engine_law_bits_do_not_depend_on_pipelining_sub_batches_or_splits(rdsp, front_form):
    import torch
    from radiodsp_sdr_rx_amd.chain import synth_iq
    nch, nblk = 256, 64
    dev = torch.from_numpy(synth_iq(nch, 2 * nblk * 128, n_threads=16)).cuda()
    ref = run_stream(engine_k3(nch, nblk), dev, [nblk, nblk])
    for kw in (dict(pipelined=True), dict(pipelined=True, sub_batch=64), dict(pipelined=True, sub_batch=0)):
        got = run_stream(engine_k3(nch, nblk, **kw), dev, [nblk, nblk])
        assert np.array_equal(got[0], ref[0]), kw
        assert_bits(got[1], ref[1], kw)
    if front_form == "default":   # split-invariant decimator: any cut of the stream into calls
        a = run_stream(engine_k3(nch, 2 * nblk), dev, [8, 120])
        b = run_stream(engine_k3(nch, 2 * nblk), dev, [72, 40, 16])
        assert np.array_equal(a[0], ref[0]) and np.array_equal(b[0], ref[0])
        assert_bits(a[1], ref[1], "split 8 + 120")
        assert_bits(b[1], ref[1], "split 72 + 40 + 16")


def test_engine_law_state_saves_loads_and_resets(rdsp, front_form):
    import torch
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    from cases import K3
    nch, nblk = 128, 32
    dev = torch.from_numpy(synth_iq(nch, 2 * nblk * 128, n_threads=16)).cuda()
    plain = Chain(nch, max_blocks_per_call=nblk, **K3)
    size0 = plain.lib.rdsp_chain_state_bytes(plain.h, nch)
    ch = engine_k3(nch, nblk)
    assert ch.lib.rdsp_chain_state_bytes(ch.h, nch) == size0 + nch * (16 + 512)   # the optional part, once allocated
    whole = run_stream(ch, dev, [nblk, nblk])
    ch.reset()
    again = run_stream(ch, dev, [nblk, nblk])
    assert np.array_equal(again[0], whole[0])
    assert_bits(again[1], whole[1], "after reset")
    first = engine_k3(nch, nblk)
    run_stream(first, dev[:, :nblk * 128], [nblk])
    blob = first.save_state()
    resumed = engine_k3(nch, nblk)
    resumed.load_state(blob)
    second = run_stream(resumed, dev[:, nblk * 128:], [nblk])
    assert np.array_equal(second[0], whole[0][:, nblk * 128 // 4:])
    assert_bits(second[1], whole[1][:, nblk * 128 // 4:], "resumed")
    from radiodsp_sdr_rx_amd._lib import RdspError
    with pytest.raises(RdspError):   # the blob's engine-law part has no place in a chain without the law
        Chain(nch, max_blocks_per_call=nblk, **K3).load_state(blob)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------
def test_tail_law_refusals(rdsp):
    import torch
    from cases import CONV_LITERAL
    from radiodsp_sdr_rx_amd.chain import Chain
    from radiodsp_sdr_rx_amd._lib import RdspError as E
    ch = Chain(4, max_blocks_per_call=8, **ENGINE_RATE)
    assert ch.tail_law == 0
    for law in (2, -1):
        with pytest.raises(E) as ex:
            ch.set_tail_law(law)
        assert ex.value.code == -1
    x = torch.zeros((4, 256), dtype=torch.float32, device="cuda")
    with pytest.raises(E) as ex:
        ch.run_tail_f32(x)                                  # build law
    assert ex.value.code == -5
    ch.set_tail_law("engine")
    with pytest.raises(E) as ex:
        ch.run_tail_f32(x[:, :200])                         # not a multiple of 128
    assert ex.value.code == -1
    ch.run_tail_f32(x)
    ch.set_tail_law("build")
    assert ch.tail_law == 0
    lit = Chain(1, max_blocks_per_call=8, **CONV_LITERAL)
    lit.set_engine_literal(True)
    with pytest.raises(E) as ex:
        lit.set_tail_law("engine")
    assert ex.value.code == -5 and lit.tail_law == 0
