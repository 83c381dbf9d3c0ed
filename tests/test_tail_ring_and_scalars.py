"""The tail kernel's block ring and step scalars (csrc/rdsp_tail.hip).

The kernel keeps [previous block | current block] contiguous in a ring of four slots, [M | S0 | S1 | S2]: block b of
a launch lives in S(b mod 3), M mirrors S2, nothing is copied between blocks.  The per-step scalars of the NLMS
(step size, lag-1 correlation B, energy E) stay in the registers of the lane that prepared them, in two sets: the
64-step group that runs and the one being prepared.  What can go wrong is therefore a matter of how many audio blocks
one launch processes (which slot it ends in, whether the mirror was written, which register set is live at the end)
and of partly filled waves.  One stream of 48 input blocks (12 audio blocks at the default decimation by 4) is run

  * through the whole chain in one call and in calls of 8 / 16 / 24 / 40 + 8 input blocks, i.e. launches of 2, 4, 6
    and 10 (+ 2) audio blocks -- they end in S1, S0, S2 and S0; the chain's call unit is 8 input blocks, so a launch
    of an odd number of audio blocks cannot be reached through rdsp_chain_process --
  * and through the isolated DSP-NR call (rdsp_LMS_NoiseReduction, the kernel's raw output), which takes any number of
    blocks: 12 in one call and in calls of 1 / 2 / 3 / 5 (+ 5 + 2) blocks, every residue of the three slots,

with 5 channels (one row of the last wave valid, three not) and 8.  All with the library's default decimator, whose
bits do not depend on the call split, so every split must reproduce the one-call result bit for bit; the one-call
result is held against the CPU oracle by the criteria of tests/parity_util.py (NLMS chains: no further from the float64
evaluation than 1.5 x the oracle's own distance; the isolated stage on identical float input: TOL)."""
import ctypes as C

import numpy as np
import pytest

from cases import K1, K3, TOL
from parity_util import assert_truth_anchored, model_run, oracle_run

pytestmark = pytest.mark.gpu

NBLK = 48                                              # input blocks: 12 audio blocks
CHAIN_CUTS = {"8": [8] * 6, "16": [16] * 3, "24": [24] * 2, "40+8": [40, 8]}   # input blocks per call
NR_CUTS = {"1": [1] * 12, "2": [2] * 6, "3": [3] * 4, "5": [5, 5, 2]}          # audio blocks per call
CASES = {
    "k3": (K3, 0),                                                             # ALS notch: the block's output is e
    "als_peak": (dict(fft_l=256, demod="USB", als_mode="peak", als_strength=20, agc_mode="medium", output_gain=0.5), 0),
    "nr_alone": (dict(fft_l=256, demod="USB", lms_nr=30), 0),                  # one instance, x 1.1
    "nr_plus_als": (dict(fft_l=256, demod="USB", als_mode="peak", als_strength=20, lms_nr=20), 0),   # two instances: ring B
    "k3_running_energy": (K3, 1),                                              # rdsp_set_nlms_energy_mode(chain, 1)
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def iq8(rdsp):
    from radiodsp_sdr_rx_amd.chain import synth_iq
    return synth_iq(8, NBLK * 128)


def _chain(nch, case, max_blocks=NBLK):
    from radiodsp_sdr_rx_amd.chain import Chain
    cfg, running = CASES[case]
    ch = Chain(nch, max_blocks_per_call=max_blocks, **cfg)   # the library's default decimator
    if running:
        ch.set_nlms_energy_mode(1)
    return ch


def _run(torch, ch, iq, cuts, start=0):
    """the calls `cuts` (input blocks each) from block `start` on: (int16, float32) audio"""
    o16, o32, at = [], [], start
    for n in cuts:
        part = torch.from_numpy(np.ascontiguousarray(iq[:, at * 128:(at + n) * 128])).cuda()
        a, b = ch.process(part, want_f32=True)
        torch.cuda.synchronize()
        o16.append(a.cpu().numpy())
        o32.append(b.cpu().numpy())
        at += n
    return np.concatenate(o16, 1), np.concatenate(o32, 1)


_ONE_CALL = {}


def one_call(torch, iq8, case, nch):
    """the stream in one call (computed once per case and channel count, never modified)"""
    key = (case, nch)
    if key not in _ONE_CALL:
        o16, o32 = _run(torch, _chain(nch, case), iq8[:nch], [NBLK])
        o16.setflags(write=False)
        o32.setflags(write=False)
        _ONE_CALL[key] = (o16, o32)
    return _ONE_CALL[key]


@pytest.mark.parametrize("case", sorted(CASES))
def test_one_call_is_as_close_to_float64_truth_as_the_oracle(rdsp, oracle, torch_cuda, iq8, case):
    cfg = CASES[case][0]
    g16, g32 = one_call(torch_cuda, iq8, case, 8)
    r16, r32 = oracle_run(oracle, iq8, cfg)
    assert_truth_anchored(g32, r32, model_run(iq8, cfg), case, g16, r16)
    # 5 channels: the last wave has one valid row; the channels do not know of each other
    p16, p32 = one_call(torch_cuda, iq8, case, 5)
    assert np.array_equal(p16, g16[:5]) and np.array_equal(p32, g32[:5])


@pytest.mark.parametrize("nch", [5, 8])
@pytest.mark.parametrize("cut", sorted(CHAIN_CUTS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_call_splits_are_bit_equal(rdsp, torch_cuda, iq8, case, cut, nch):
    ref16, ref32 = one_call(torch_cuda, iq8, case, nch)
    ch = _chain(nch, case)
    g16, g32 = _run(torch_cuda, ch, iq8[:nch], CHAIN_CUTS[cut])
    assert np.array_equal(g32, ref32) and np.array_equal(g16, ref16)


@pytest.mark.parametrize("case", sorted(CASES))
def test_reset_in_mid_stream_starts_the_stream_again(rdsp, torch_cuda, iq8, case):
    """after reset() the instances are at their first block again (d = x instead of the previous block), in a launch
    that follows launches which left other slots and register sets behind"""
    nch = 5
    a = _chain(nch, case)
    _run(torch_cuda, a, iq8[:nch], [24])               # six audio blocks: ends in S2, the mirror written
    a.reset()
    g16, g32 = _run(torch_cuda, a, iq8[:nch], [8, 16], start=24)
    f16, f32 = _run(torch_cuda, _chain(nch, case), iq8[:nch], [24], start=24)
    assert np.array_equal(g32, f32) and np.array_equal(g16, f16)


@pytest.mark.parametrize("at", [8, 24])                # the saved launch ended in S1 / in S2
@pytest.mark.parametrize("case", sorted(CASES))
def test_state_saved_and_loaded_between_two_calls(rdsp, torch_cuda, iq8, case, at):
    """the state a launch leaves (`*_prev`: the last block processed, wherever it lay in the ring) continues the stream in
    a fresh chain bit for bit"""
    nch = 5
    ref16, ref32 = one_call(torch_cuda, iq8, case, nch)
    a = _chain(nch, case)
    _run(torch_cuda, a, iq8[:nch], [at])
    blob = a.save_state()
    b = _chain(nch, case)
    b.load_state(blob)
    g16, g32 = _run(torch_cuda, b, iq8[:nch], [NBLK - at], start=at)
    assert np.array_equal(g32, ref32[:, at * 32:]) and np.array_equal(g16, ref16[:, at * 32:])


@pytest.fixture(scope="module")
def nr_stream():
    rng = np.random.default_rng(31)
    n = np.arange(12 * 128)
    x = np.stack([0.3 * np.sin(2 * np.pi * (450 + 310 * c) / 24000 * n + c) + 0.05 * rng.standard_normal(len(n))
                  for c in range(8)]).astype(np.float32)
    x.setflags(write=False)
    return x


def _nr_run(torch, x, cuts, running):
    from radiodsp_sdr_rx_amd.chain import Chain
    ch = Chain(x.shape[0], **K1)
    ch.set_nlms_energy_mode(running)
    ch.Init_LMS_NR(30)
    out, at = [], 0
    for n in cuts:
        buf = torch.from_numpy(x[:, at * 128:(at + n) * 128].copy()).cuda()
        ch.LMS_NoiseReduction(buf)
        torch.cuda.synchronize()
        out.append(buf.cpu().numpy())
        at += n
    return np.concatenate(out, 1), ch.lms_coeffs(0)


@pytest.mark.parametrize("running", [0, 1])
@pytest.mark.parametrize("nch", [5, 8])
def test_isolated_nr_in_launches_of_1_2_3_5_blocks(rdsp, oracle, torch_cuda, nr_stream, nch, running):
    """rdsp_LMS_NoiseReduction (the kernel's raw output): every residue of the three-slot ring per launch, bit equal to
    the one-call run, which meets TOL against the oracle on identical float input, weights included"""
    x = nr_stream[:nch]
    ref, wref = _nr_run(torch_cuda, x, [12], running)
    lib = oracle.load()
    for c in range(nch):
        oc = oracle.OracleChain(**K1)
        lib.orc_Init_LMS_NR(oc.h, 30)
        o = []
        for k in range(12):
            blk = x[c, k * 128:(k + 1) * 128].copy()
            lib.orc_LMS_NoiseReduction(oc.h, 128, blk.ctypes.data_as(C.POINTER(C.c_float)))
            o.append(blk)
        o = np.concatenate(o)
        assert np.abs(ref[c] - o).max() / np.abs(o).max() <= TOL, c
        w = oc.lms_coeffs(0)
        assert np.abs(wref[c] - w).max() <= 2e-5 * np.abs(w).max(), c
    for name, cuts in sorted(NR_CUTS.items()):
        got, w = _nr_run(torch_cuda, x, cuts, running)
        assert np.array_equal(got, ref), name
        assert np.array_equal(w, wref), name
