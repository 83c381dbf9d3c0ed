"""GPU parity tests: every call goes through the C-ABI (librdsp_hip.so) and is
compared with the CPU oracle on identical seeded inputs, with the committed golden
vectors, and -- at BASELINE.json's full sizes -- through size-independent properties.

Tolerances (written here, used below):
  * int16 -> float unpack, float -> int16 pack: bit-exact.
  * feed-forward chains (mixer, decimator, overlap-save filter, spectral NR, demod,
    AGC): TOL = 1e-5 normwise per channel, max|y - y_ref| / max|y_ref| (north-star).
  * chains with an NLMS stage (DSP-NR, ALS notch/peak): the NLMS kernel itself meets
    1e-5 on identical float input (test_lms_noise_reduction_isolated).  Through a whole
    chain the start-up of the recursion (energy ~ 0) amplifies float32 rounding: the
    float32 oracle itself sits 4e-5 .. 1.1e-4 away from the float64 evaluation of the same
    chain (tests/np_model.py), so two float32 implementations cannot agree to 1e-5 there
    and a bound against the oracle would only measure the oracle's own noise.  The
    criterion is anchored on truth instead:
        err(gpu, f64) <= max(TOL, 1.5 * err(oracle, f64))
    for the worst and for the median channel of the test's channel set (and 5 x per channel),
    i.e. the GPU may not be further from the exact result than the reference arithmetic
    is (assert_truth_anchored; measured: the GPU sits at about half the oracle's distance).  No tolerance looser than 1e-5 is expressed against the
    float32 oracle.
  * int16 outputs: +-1 LSB where the float audio differs across a rounding
    boundary (count reported), never more; on NLMS chains the same truth-anchored rule
    in LSB against the int16 of the float64 result.
"""
import os

import numpy as np
import pytest

from cases import CONV_LITERAL, GOLDEN_CASES, K1, K3, K4, TOL, apply_setup
from parity_util import assert_truth_anchored, check_i16, model_run, normwise, oracle_run, q15_of  # noqa: F401 (re-exported)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("front_form")]   # every test under both front kernels (conftest.py)
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


TAILS = ["16r"]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch


def gpu_run(torch, iq, cfg, calls=1, tail=None, setup=None, fir=None):
    """tail: None or "16r" (the tail kernel: a channel per 16-lane row, two steps per reduction)"""
    from radiodsp_sdr_rx_amd.chain import Chain
    nch, n = iq.shape[0], iq.shape[1]
    ch = Chain(nch, max_blocks_per_call=n // 128 // calls, **cfg)
    assert tail in (None, "16r")
    apply_setup(ch, setup)
    if fir is not None:   # stage A3: 0 direct form, 2 frequency domain with 448-sample frames, -1 / 4 granule frames (None: the module's `front_form`)
        ch.set_fir_variant(fir)
    o16, o32 = [], []
    step = n // calls
    for k in range(calls):
        part = torch.from_numpy(np.ascontiguousarray(iq[:, k * step:(k + 1) * step])).cuda()
        a, b = ch.process(part, want_f32=True)
        torch.cuda.synchronize()
        o16.append(a.cpu().numpy())
        o32.append(b.cpu().numpy())
    return np.concatenate(o16, 1), np.concatenate(o32, 1), ch



# ---- A1 / A10: the int16 edges, bit-exact ------------------------------------
def test_unpack_all_int16_values_bit_exact(rdsp, torch_cuda):
    import ctypes as C
    torch = torch_cuda
    lib = rdsp.load()
    src = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).cuda()
    dst = torch.empty(65536, dtype=torch.float32, device="cuda")
    assert lib.rdsp_q15_to_float(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), 65536, None) == 0
    torch.cuda.synchronize()
    exp = np.arange(-32768, 32768).astype(np.float32) / np.float32(32768.0)
    assert np.array_equal(dst.cpu().numpy(), exp)


def test_pack_matches_oracle_bit_exact(rdsp, oracle, torch_cuda):
    import ctypes as C
    torch = torch_cuda
    lib = rdsp.load()
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.uniform(-1.2, 1.2, 200000), [0.0, 1.0, -1.0, 0.99999, -0.99999, 3e-5, -3e-5, 1e9, -1e9]]
                       ).astype(np.float32)
    src = torch.from_numpy(x).cuda()
    dst = torch.empty(len(x), dtype=torch.int16, device="cuda")
    assert lib.rdsp_float_to_q15(C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), len(x), None) == 0
    torch.cuda.synchronize()
    ref = np.zeros(len(x), np.int16)
    oracle.load().orc_float_to_q15(x.ctypes.data_as(C.POINTER(C.c_float)), ref.ctypes.data_as(C.POINTER(C.c_int16)), len(x))
    assert np.array_equal(dst.cpu().numpy(), ref)


# ---- feed-forward chains vs oracle ---------------------------------------------
FF_CASES = {
    "conv_literal_256": (CONV_LITERAL, 3, 16, False),
    "conv_literal_512": (dict(CONV_LITERAL, fft_l=512), 2, 16, False),
    "conv_literal_4096": (dict(CONV_LITERAL, fft_l=4096), 2, 64, False),
    # the spectral-NR variant of the in-tree loop as the file has it (SPEC:112-269: native rate, FFT_L 256,
    # no filter mask, iNRLevel 2) and the older one (BK_INO:1520-1669) at the native rate
    "spec_literal_256": (dict(CONV_LITERAL, filter_on=0, spectral_nr=1, spectral_level=2.0), 3, 32, False),
    "spec_old_literal_256": (dict(CONV_LITERAL, spectral_nr=2), 2, 32, False),
    "k1_one_channel": (K1, 1, 16, False),
    "k2_usb_256": (K1, 5, 32, False),
    "usb_512": (dict(fft_l=512, demod="USB"), 4, 32, False),
    "usb_1024": (dict(fft_l=1024, demod="USB"), 3, 32, False),
    "lsb_2048": (dict(fft_l=2048, demod="LSB", nco_hz=14600.0, flo_hz=-2700.0, fhi_hz=-300.0), 2, 64, False),
    "k4_cw_4096_agc": (K4, 3, 128, True),
    "spectral_512": (dict(fft_l=512, demod="USB", spectral_nr=1, spectral_level=2.0), 4, 32, False),
    "spectral_256_level3": (dict(fft_l=256, demod="USB", spectral_nr=1, spectral_level=3.0), 3, 32, False),
    "spectral_old_512": (dict(fft_l=512, demod="USB", spectral_nr=2), 4, 32, False),        # BK_INO:1586-1630
    "spectral_old_256_agc": (dict(fft_l=256, demod="USB", spectral_nr=2, agc_mode="medium"), 3, 32, False),
    "window2_512": (dict(fft_l=512, demod="USB", window=2), 2, 32, False),                 # CONV:159-179: the other
    "window3_256": (dict(fft_l=256, demod="LSB", flo_hz=-2700.0, fhi_hz=-300.0, window=3), 2, 32, False),  # window ids
    "window4_1024": (dict(fft_l=1024, demod="USB", window=4), 2, 32, False),
    "window5_512_agc": (dict(fft_l=512, demod="USB", window=5, agc_mode="fast"), 2, 32, False),
    "agc_fast_slow": (dict(fft_l=512, demod="USB", agc_mode="slow", output_gain=0.5), 4, 64, False),
    "am_agc": (dict(fft_l=512, demod="AM", flo_hz=-3900.0, fhi_hz=3900.0, agc_mode="medium"), 3, 32, False),
    "iq_gains": (dict(fft_l=512, demod="IQ", agc_mode="fast", input_gain=0.7, iq_balance=1.02, output_gain=0.5), 3, 32, False),
    # one gain for I and Q that is not a power of two: the kernels without PRE carry it on the mixer phasors
    "input_gain_0p7_usb": (dict(fft_l=512, demod="USB", input_gain=0.7, agc_mode="medium"), 3, 32, False),
    "input_gain_1p3_cw_4096": (dict(K4, input_gain=1.3), 2, 128, True),
    "nco_off_filter_off": (dict(fft_l=256, demod="IQ", nco_hz=0.0, filter_on=0), 2, 16, False),
    "odd_nco": (dict(fft_l=256, demod="USB", nco_hz=12345.678), 3, 32, False),
}


LITERAL_SPEC_CASES = {
    "spec_literal_256": FF_CASES["spec_literal_256"],          # SPEC:112-269 as the file has it: native rate, FFT_L 256, no mask
    "spec_literal_512": (dict(CONV_LITERAL, fft_l=512, spectral_nr=1, spectral_level=2.0), 2, 32, False),
    "spectral_256": (dict(fft_l=256, demod="USB", spectral_nr=1, spectral_level=2.0), 3, 32, False),   # four frames per pass behind the fd decimator
    "spectral_512": FF_CASES["spectral_512"],
    "spectral_1024_level3": (dict(fft_l=1024, demod="USB", spectral_nr=1, spectral_level=3.0), 2, 32, False),
    "spectral_2048": (dict(fft_l=2048, demod="LSB", flo_hz=-2700.0, fhi_hz=-300.0, spectral_nr=1, spectral_level=2.0), 2, 64, False),  # four waves per channel
    "k3_front": (dict(K3, als_mode="off"), 4, 64, False),      # K3 without its recursion: spectral stage + AGC
}


@pytest.mark.parametrize("name", sorted(LITERAL_SPEC_CASES))
def test_spectral_stage_as_written_matches_the_oracle_as_written(rdsp, oracle, torch_cuda, name, front_form):
    """rdsp_set_spectral_resynthesis(chain, 1): SPEC:226-235 evaluated as the file writes it -- phi = atan2(im, re),
    mag' * arm_cos_f32(phi), mag' * arm_sin_f32(phi), CMSIS' 513-entry table with linear interpolation -- against the
    oracle evaluating the same lines (orc_set_literal_resynthesis): <= 1e-5 normwise per channel, under all three
    decimator forms.  The two FORMS (as written / X mag'/mag) are 1.7e-5 ... 1.9e-5 apart, which the same run shows:
    each GPU form is within 1e-5 of the oracle's same form and NOT of the other one."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    cfg, nch, nblk, cw = LITERAL_SPEC_CASES[name]
    iq = synth_iq(nch, nblk * 128, cw=cw)
    dev = torch.from_numpy(iq).cuda()

    def gpu(literal):
        ch = Chain(nch, max_blocks_per_call=nblk // 2, **cfg)
        ch.set_spectral_resynthesis(literal)
        o = [ch.process(dev[:, k * (nblk // 2) * 128:(k + 1) * (nblk // 2) * 128].contiguous(), want_f32=True)[1].cpu().numpy()
             for k in range(2)]
        return np.concatenate(o, 1), ch.scalars()

    def orc(literal):
        out = []
        for c in range(nch):
            oc = oracle.OracleChain(**cfg)
            oc.set_literal_resynthesis(literal)
            out.append(oc.process(iq[c])[1])
        return np.stack(out)

    g_lit, s_lit = gpu(1)            # the table's interpolation in closed form (csrc/rdsp_front_frame.h spec_table_factor)
    g_tab, _ = gpu(2)                # atan2f and the table looked up
    g_eq, s_eq = gpu(False)
    o_lit, o_eq = orc(True), orc(False)
    e_ll, e_ee = normwise(g_lit, o_lit), normwise(g_eq, o_eq)
    e_tab, e_lt = normwise(g_tab, o_lit), normwise(g_lit, g_tab)
    print(f"{name}: as written, table looked up, gpu vs oracle {e_tab:.2e}; closed form vs looked up {e_lt:.2e}")
    cross = normwise(g_lit, o_eq)
    # SPEC:213-217 is discontinuous at mag = NFloor (0.2 mag below, mag - NFloor above: a jump of 0.2 NFloor), so one
    # bin whose comparison flips under float32 rounding moves a frame by more than rounding; where the float32 oracle
    # itself sits further than that from the float64 evaluation of the chain (FFT_L 2048: 8.9e-6), the bound follows it
    bound = max(TOL, 1.5 * normwise(o_eq, model_run(iq, cfg)))
    print(f"{name}: as written gpu vs oracle {e_ll:.2e}; equivalent form gpu vs oracle {e_ee:.2e}; as written vs equivalent {cross:.2e}; bound {bound:.2e}")
    assert e_ll <= bound and e_ee <= bound and e_tab <= bound
    assert e_lt <= max(2e-6, 0.5 * bound)                          # the two evaluations of the as-written form: one result
    assert np.allclose(s_lit[:, 0], s_eq[:, 0], rtol=1e-5)         # NFloor: the threshold logic does not depend on the form
    assert 5e-6 <= cross <= 5e-5                                    # the table's interpolation error separates the forms


@pytest.mark.parametrize("name", ["k1_one_channel", "k2_usb_256", "usb_512", "usb_1024", "lsb_2048", "k4_cw_4096_agc", "spectral_512",
                                  "spectral_256_level3", "spectral_old_512",
                                  "agc_fast_slow", "am_agc", "iq_gains", "odd_nco"])
@pytest.mark.parametrize("calls", [1, 4])
def test_frequency_domain_decimator_matches_oracle(rdsp, oracle, torch_cuda, name, calls):
    """rdsp_chain_set_fir_variant(2): stage A3 as a polyphase overlap-save convolution (four
    low-rate transforms, branch spectra, one inverse) instead of the direct form.  Same taps, exact
    linear convolution: TOL against the oracle, whatever the call split (the frame grid is
    anchored at each call's first sample; a call of one granule is a single partial frame)."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    cfg, nch, nblk, cw = FF_CASES[name]
    nblk = max(nblk, {4096: 256, 2048: 128}.get(cfg.get("fft_l", 256), 64))   # four calls of at least one granule
    iq = synth_iq(nch, nblk * 128, cw=cw)
    ch = Chain(nch, max_blocks_per_call=nblk // calls, **cfg)
    ch.set_fir_variant(2)
    step = nblk // calls * 128
    outs = [ch.process(torch.from_numpy(np.ascontiguousarray(iq[:, k * step:(k + 1) * step])).cuda(), want_f32=True)
            for k in range(calls)]
    torch.cuda.synchronize()
    o16 = np.concatenate([o[0].cpu().numpy() for o in outs], 1)
    o32 = np.concatenate([o[1].cpu().numpy() for o in outs], 1)
    r16, r32 = oracle_run(oracle, iq, cfg)
    err = normwise(o32, r32)
    assert err <= TOL, f"{name}: normwise err {err:.3e}"
    assert check_i16(o16, r16) < 0.02 * o16.size


@pytest.mark.parametrize("name", sorted(FF_CASES))
def test_feed_forward_chain_matches_oracle(rdsp, oracle, torch_cuda, name):
    from radiodsp_sdr_rx_amd.chain import synth_iq
    cfg, nch, nblk, cw = FF_CASES[name]
    iq = synth_iq(nch, nblk * 128, cw=cw)
    if "spectral" in name:
        pytest.importorskip("numpy")
    o16, o32, _ = gpu_run(torch_cuda, iq, cfg)
    r16, r32 = oracle_run(oracle, iq, cfg)
    err = normwise(o32, r32)
    assert err <= TOL, f"{name}: normwise err {err:.3e}"
    flips = check_i16(o16, r16)
    assert flips < 0.02 * o16.size


def test_spectral_threshold_flip_is_the_only_discontinuity(rdsp, oracle, torch_cuda):
    """SPEC:213-217 selects 0.2*mag vs mag-NFloor per bin: a bin within float rounding
    of the threshold may fall on the other side.  Over a longer run the result must
    still be within TOL except for frames where the oracle itself has a bin that close."""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    cfg = dict(fft_l=512, demod="USB", spectral_nr=1, spectral_level=2.0)
    iq = synth_iq(8, 256 * 128)
    _, o32, ch = gpu_run(torch_cuda, iq, cfg)
    _, r32 = oracle_run(oracle, iq, cfg)
    per_frame = np.abs(o32 - r32).max(axis=2).reshape(8, -1, 256).max(axis=2) / np.abs(r32).max()
    assert (per_frame > TOL).mean() < 0.01  # at most a stray frame
    nf = ch.scalars()[:, 0]
    for c in range(8):
        oc = oracle.OracleChain(**cfg)
        oc.process(iq[c])
        assert abs(nf[c] - oc.nfloor()) <= 2e-6 * oc.nfloor()


# ---- golden vectors ---------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(GOLDEN_CASES))
def test_golden_vectors(rdsp, torch_cuda, name):
    case = GOLDEN_CASES[name]
    g = np.load(os.path.join(GOLD, name + ".npz"))
    o16, o32, _ = gpu_run(torch_cuda, g["iq"], case["cfg"], setup=case.get("setup"))
    recursive = (case["cfg"].get("lms_nr", 0) > 0 or case["cfg"].get("als_mode", "off") != "off"
                 or case["cfg"].get("demod") == "SAM")
    if recursive:   # truth-anchored (module docstring): the fixture carries the float64 result too
        assert_truth_anchored(o32, g["out_f32"], g["out_f64"], name, o16, g["out_i16"])
        if name == "k3_full_512":   # the metric configuration also meets the north-star's 1e-5 against the oracle
            assert normwise(o32, g["out_f32"]) <= TOL
        return
    assert normwise(o32, g["out_f32"]) <= TOL
    d = np.abs(o16.astype(np.int32) - g["out_i16"].astype(np.int32))
    assert d.max() <= 1


# ---- NLMS stages --------------------------------------------------------------------
def test_lms_noise_reduction_isolated(rdsp, oracle, torch_cuda):
    """LMS_NoiseReduction (NR:66) alone, identical float input: the kernel's own
    arithmetic meets TOL; weights, the first-call quirk and call splitting included."""
    import ctypes as C
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain
    rng = np.random.default_rng(11)
    nch, nblk = 6, 48
    n = np.arange(nblk * 128)
    x = np.stack([0.3 * np.sin(2 * np.pi * (500 + 300 * c) / 24000 * n + c) + 0.05 * rng.standard_normal(len(n))
                  for c in range(nch)]).astype(np.float32)
    ch = Chain(nch, **K1)
    ch.Init_LMS_NR(30)
    buf = torch.from_numpy(x.copy()).cuda()
    ch.LMS_NoiseReduction(buf[:, :16 * 128].contiguous())  # warm the path, then the real run
    ch = Chain(nch, **K1)
    ch.Init_LMS_NR(30)
    a = torch.from_numpy(x[:, :20 * 128].copy()).cuda()
    b = torch.from_numpy(x[:, 20 * 128:].copy()).cuda()
    ch.LMS_NoiseReduction(a)
    ch.LMS_NoiseReduction(b)  # split calls: state carried in HBM
    torch.cuda.synchronize()
    got = np.concatenate([a.cpu().numpy(), b.cpu().numpy()], axis=1)
    wg = ch.lms_coeffs(0)
    lib = oracle.load()
    for c in range(nch):
        oc = oracle.OracleChain(**K1)
        lib.orc_Init_LMS_NR(oc.h, 30)
        ref = []
        for k in range(nblk):
            blk = x[c, k * 128:(k + 1) * 128].copy()
            lib.orc_LMS_NoiseReduction(oc.h, 128, blk.ctypes.data_as(C.POINTER(C.c_float)))
            ref.append(blk)
        ref = np.concatenate(ref)
        assert np.abs(got[c] - ref).max() / np.abs(ref).max() <= TOL
        w = oc.lms_coeffs(0)
        assert np.abs(wg[c] - w).max() <= 2e-5 * np.abs(w).max()


@pytest.mark.parametrize("name", ["nr_30", "k3", "literal_512_nr_40"])
def test_nlms_running_energy_mode_is_the_references_arithmetic(rdsp, oracle, torch_cuda, name):
    """rdsp_set_nlms_energy_mode(chain, 1): arm_lms_norm_f32's energy as NR:73 runs it -- one running difference for
    the whole stream, no re-start from the window sum at block boundaries (the default's deviation).  On ordinary
    signals: the isolated stage (identical float input) within 1e-5 of the oracle, weights included, and the two modes
    within 1e-5 of each other; through whole chains as close to the float64 evaluation as the oracle, like every
    chain that ends in this recursion."""
    import ctypes as C
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    if name == "nr_30":
        rng = np.random.default_rng(12)
        nch, nblk = 5, 40
        n = np.arange(nblk * 128)
        x = np.stack([0.3 * np.sin(2 * np.pi * (400 + 350 * c) / 24000 * n + c) + 0.05 * rng.standard_normal(len(n))
                      for c in range(nch)]).astype(np.float32)
        outs = {}
        for mode in (0, 1):
            ch = Chain(nch, **K1)
            ch.set_nlms_energy_mode(mode)
            ch.Init_LMS_NR(30)
            a, b = torch.from_numpy(x[:, :16 * 128].copy()).cuda(), torch.from_numpy(x[:, 16 * 128:].copy()).cuda()
            ch.LMS_NoiseReduction(a)
            ch.LMS_NoiseReduction(b)
            torch.cuda.synchronize()
            outs[mode] = (np.concatenate([a.cpu().numpy(), b.cpu().numpy()], 1), ch.lms_coeffs(0))
        lib = oracle.load()
        for c in range(nch):
            oc = oracle.OracleChain(**K1)
            lib.orc_Init_LMS_NR(oc.h, 30)
            ref = []
            for k in range(nblk):
                blk = x[c, k * 128:(k + 1) * 128].copy()
                lib.orc_LMS_NoiseReduction(oc.h, 128, blk.ctypes.data_as(C.POINTER(C.c_float)))
                ref.append(blk)
            ref = np.concatenate(ref)
            for mode in (0, 1):
                assert np.abs(outs[mode][0][c] - ref).max() / np.abs(ref).max() <= TOL, (mode, c)
                assert np.abs(outs[mode][1][c] - oc.lms_coeffs(0)).max() <= 2e-5 * np.abs(oc.lms_coeffs(0)).max()
        assert not np.array_equal(outs[0][0], outs[1][0])                      # two arithmetics ...
        assert normwise(outs[1][0], outs[0][0]) <= TOL                         # ... one result on an ordinary signal
        return
    cfg = {"k3": K3, "literal_512_nr_40": NLMS_CASES["literal_512_nr_40"]}[name]
    nch, nblk = 5, 64
    iq = synth_iq(nch, nblk * 128)
    ch = Chain(nch, max_blocks_per_call=nblk // 2, **cfg)
    ch.set_nlms_energy_mode(1)
    o = [ch.process(torch.from_numpy(np.ascontiguousarray(iq[:, k * (nblk // 2) * 128:(k + 1) * (nblk // 2) * 128])).cuda(), want_f32=True)
         for k in range(2)]
    torch.cuda.synchronize()
    o16 = np.concatenate([a[0].cpu().numpy() for a in o], 1)
    o32 = np.concatenate([a[1].cpu().numpy() for a in o], 1)
    r16, r32 = oracle_run(oracle, iq, cfg)
    assert_truth_anchored(o32, r32, model_run(iq, cfg), name + " (running energy)", o16, r16)
    if name == "k3":
        assert normwise(o32, r32) <= TOL


def test_nlms_health_word_and_the_energy_anchor(rdsp, oracle, torch_cuda):
    """The reference's NLMS keeps its window energy as a running difference for the whole stream (NR:73 ->
    arm_lms_norm_f32): after a loud-to-quiet transition the rounding residue of everything that went through
    can leave energy + 1.19e-7 at or below zero, the step size turns negative or infinite and the channel's
    weights run away -- in the CPU restatement 1 of 320 such transitions ends with non-finite weights.  The
    tail kernel starts the same difference from the exact 96-sample window sum at every 128-sample block, so a
    residue lives for one block at most: it must not lose MORE channels than the restatement (round 3's
    un-anchored prefix-scan form lost 8 and flagged 90; now 0 and 9, the 9 being transitions inside a block).
    The health words (rdsp_chain_get_status) stay: the energy bit for a divisor <= 0, the non-finite bit for
    exactly the channels whose weights are not finite (driven here by an infinite input sample), sticky,
    cured per channel by rdsp_chain_reset_nlms_channels with every other channel continuing bit for bit,
    cleared by Init_LMS_NR."""
    import ctypes as C
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain
    nch, loud, quiet = 640, 768, 1792
    rng = np.random.default_rng(2024)
    x = np.concatenate([0.3 * rng.standard_normal((nch, loud)), 1e-4 * rng.standard_normal((nch, quiet))], axis=1).astype(np.float32)
    x[::2, loud:] = (0.3 * rng.standard_normal((nch // 2, quiet))).astype(np.float32)   # every second channel stays loud: the control group
    ch = Chain(nch, **K1)
    ch.Init_LMS_NR(20)
    assert not ch.get_status().any()
    buf = torch.from_numpy(x.copy()).cuda()
    ch.LMS_NoiseReduction(buf[:, :loud].contiguous())
    assert not ch.get_status().any()             # nothing happens while the input is loud
    ch.LMS_NoiseReduction(buf[:, loud:].contiguous())
    torch.cuda.synchronize()
    st = ch.get_status()
    w = ch.lms_coeffs(0)
    dead = ~np.isfinite(w).all(axis=1)
    assert ((st & ch.STATUS_NR_NONFINITE) != 0).tolist() == dead.tolist()
    assert ((st[dead] & ch.STATUS_NR_ENERGY) != 0).all()
    assert not (st & (ch.STATUS_ALS_ENERGY | ch.STATUS_ALS_NONFINITE)).any()
    assert not st[::2].any() and not dead[::2].any()   # the control group
    # the same script through the CPU restatement
    lib = oracle.load()
    odead = np.zeros(nch, bool)
    for c in range(nch):
        oc = oracle.OracleChain(**K1)
        lib.orc_Init_LMS_NR(oc.h, 20)
        for k in range((loud + quiet) // 128):
            blk = x[c, k * 128:(k + 1) * 128].copy()
            lib.orc_LMS_NoiseReduction(oc.h, 128, blk.ctypes.data_as(C.POINTER(C.c_float)))
        odead[c] = not np.isfinite(oc.lms_coeffs(0)).all()
    flagged = int(((st & ch.STATUS_NR_ENERGY) != 0).sum())
    # how often the reference's own recursion (`energy -= x0 * x0; energy += in * in`, float32, sequential)
    # divides by something <= 0 on this input: the energy depends on the input only
    f = np.float32
    E, hist, oflag = np.zeros(nch, f), np.zeros((nch, 97), f), np.zeros(nch, bool)
    for n in range(x.shape[1]):
        hist = np.concatenate([hist[:, 1:], x[:, n:n + 1]], axis=1)
        E = ((E - hist[:, 0] * hist[:, 0]).astype(f) + x[:, n] * x[:, n]).astype(f)
        oflag |= (E + f(1.19209289e-7)).astype(f) <= 0
    print(f"blow-ups: gpu {int(dead.sum())} dead, divisor <= 0 on {flagged}; reference form {int(odead.sum())} dead, "
          f"divisor <= 0 on {int(oflag.sum())} (and it stays there) of {nch // 2} transitions")
    assert not odead[::2].any() and not oflag[::2].any()
    # measured: 0 <= 1 dead, 9 <= 164 flagged (8 and 90 in round 3, before the anchor)
    assert dead.sum() <= odead.sum() and flagged <= 16 and flagged <= oflag.sum()
    # rdsp_set_nlms_energy_mode(1) takes the anchor away again: the reference's fragility, for hosts that ask for it
    run = Chain(nch, **K1)
    run.set_nlms_energy_mode(1)
    run.Init_LMS_NR(20)
    rbuf = torch.from_numpy(x.copy()).cuda()
    run.LMS_NoiseReduction(rbuf[:, :loud].contiguous())
    run.LMS_NoiseReduction(rbuf[:, loud:].contiguous())
    torch.cuda.synchronize()
    rst = run.get_status()
    rflag = int(((rst & run.STATUS_NR_ENERGY) != 0).sum())
    rdead = int((~np.isfinite(run.lms_coeffs(0)).all(axis=1)).sum())
    print(f"running-energy mode: {rdead} dead, divisor <= 0 on {rflag}")
    assert not rst[::2].any() and rflag > flagged          # measured 90 against 9 in round 3's un-anchored form
    # the non-finite bit, stickiness and the per-channel cure, on channels killed by an infinite sample
    victims = np.array([3, 64, 637])
    more = (1e-4 * rng.standard_normal((nch, 256))).astype(np.float32)
    poison = more.copy()
    poison[victims, 5] = np.inf
    ref = Chain(nch, **K1)                      # the same stream without the cure
    ref.Init_LMS_NR(20)
    rb = torch.from_numpy(x.copy()).cuda()
    ref.LMS_NoiseReduction(rb[:, :loud].contiguous())
    ref.LMS_NoiseReduction(rb[:, loud:].contiguous())
    a, b = torch.from_numpy(poison).cuda(), torch.from_numpy(poison).cuda()
    ch.LMS_NoiseReduction(a[:, :128].contiguous())
    st2 = ch.get_status()
    assert ((st2 & st) == st).all()             # sticky: bits are only ever added
    dead = (st2 & ch.STATUS_NR_NONFINITE) != 0
    assert dead.tolist() == (~np.isfinite(ch.lms_coeffs(0)).all(axis=1)).tolist() and dead[victims].all()
    assert dead.sum() <= len(victims) + 2     # (a channel whose divisor dipped during the transition may still run away later)
    # Init_LMS_NR would not cure a dead channel (NR:62 leaves the coefficients): the host resets just the
    # channels the words name, every other channel continues bit for bit
    for c in np.where(dead)[0]:
        ch.reset_nlms_channels(0, int(c))
    assert not (ch.get_status()[dead]).any() and (ch.get_status()[~dead] == st2[~dead]).all()
    oa = ch.LMS_NoiseReduction(a[:, 128:].contiguous()).cpu().numpy()
    ref.LMS_NoiseReduction(b[:, :128].contiguous())
    ob = ref.LMS_NoiseReduction(b[:, 128:].contiguous()).cpu().numpy()
    assert np.isfinite(oa[dead]).all() and np.isfinite(ch.lms_coeffs(0)[dead]).all() and not ch.get_status()[dead].any()
    assert np.array_equal(oa[~dead], ob[~dead], equal_nan=True)
    ch.Init_LMS_NR(20)
    assert not ch.get_status().any()


NLMS_CASES = {
    "dsp_nr_30": dict(fft_l=256, demod="USB", lms_nr=30),
    "als_notch": dict(fft_l=256, demod="USB", als_mode="notch", als_strength=20),
    "als_peak_plus_nr": dict(fft_l=256, demod="USB", als_mode="peak", als_strength=20, lms_nr=20),
    "k3_full": K3,
    # the in-tree loop itself with nr_level on (CONV:228-353 at its native rate: no mixer, no decimator;
    # LMS_NoiseReduction on the L side, x 1.1, R = L, CONV:326-337), 256- and 512-point filter
    "literal_nr_20": dict(CONV_LITERAL, lms_nr=20),
    "literal_512_nr_40": dict(CONV_LITERAL, fft_l=512, lms_nr=40),
}


@pytest.mark.parametrize("tail", TAILS)
@pytest.mark.parametrize("name", sorted(NLMS_CASES))
def test_chain_with_nlms_is_as_close_to_float64_truth_as_the_oracle(rdsp, oracle, torch_cuda, name, tail):
    """tail "16r": the tail kernel (row layout, two steps per reduction).  The layouts that were measured and not
    adopted (delay line shifted by DPP, half a row, reduction on the matrix pipe) are in docs/history.md."""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    cfg = NLMS_CASES[name]
    nch, nblk = 5, 64          # a partly filled last wave (4 channels per wave)
    iq = synth_iq(nch, nblk * 128)
    o16, o32, _ = gpu_run(torch_cuda, iq, cfg, calls=2, tail=tail)
    r16, r32 = oracle_run(oracle, iq, cfg)
    # the front end alone (recursive stages off) meets the north-star tolerance against the oracle
    ff = dict(cfg, lms_nr=0, als_mode="off", agc_mode="off")
    _, f32, _ = gpu_run(torch_cuda, iq, ff)
    _, fr32 = oracle_run(oracle, iq, ff)
    assert normwise(f32, fr32) <= TOL
    ratio = assert_truth_anchored(o32, r32, model_run(iq, cfg), name, o16, r16)
    print(f"{name}: max err(gpu,f64) / max err(oracle,f64) = {ratio:.2f}; gpu vs oracle {normwise(o32, r32):.2e}")


# ---- streaming state ---------------------------------------------------------------------
@pytest.mark.parametrize("name,cfg,nblk", [("k2", K1, 64), ("k3", K3, 64), ("k4", K4, 256),
                                           ("k3_odd_nco", dict(K3, nco_hz=12345.678), 64)])
def test_split_calls_are_bitwise_identical_to_one_call(rdsp, torch_cuda, name, cfg, nblk):
    """State (FIR history, overlap block, NFloor, AGC, NLMS) is carried in HBM across launches, and the default
    decimator (frequency domain, one granule per frame: every frame's input is a function of the absolute
    sample position) as well as the direct form give the same bits for any call split, as the reference's fixed
    128-sample blocks do (CONV:231-245).  The throughput form (448-sample frames anchored at each call's first
    sample) rounds differently under another split: same result to TOL."""
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    iq = synth_iq(3, nblk * 128, cw=(name == "k4"))
    calls = 4 if name != "k4" else 2
    saved, Chain.default_fir_variant = Chain.default_fir_variant, None   # the library's default, whatever the module runs under
    try:
        a16, a32, ach = gpu_run(torch_cuda, iq, cfg, calls=1)
        b16, b32, _ = gpu_run(torch_cuda, iq, cfg, calls=calls)
        # the default picks between its two split-invariant forms by what follows the front kernel (rdsp.h)
        assert ach.front_kernel_name() == ("rdsp_front_fd_kernel" if name.startswith("k3") else "rdsp_front_rd_kernel")
    finally:
        Chain.default_fir_variant = saved
    assert np.array_equal(a16, b16) and np.array_equal(a32, b32)
    d16, d32, _ = gpu_run(torch_cuda, iq, cfg, calls=1, fir=0)
    e16, e32, _ = gpu_run(torch_cuda, iq, cfg, calls=calls, fir=0)
    assert np.array_equal(d16, e16) and np.array_equal(d32, e32) and normwise(d32, a32) <= TOL
    _, f1, _ = gpu_run(torch_cuda, iq, cfg, calls=1, fir=2)
    _, f4, _ = gpu_run(torch_cuda, iq, cfg, calls=calls, fir=2)
    assert normwise(f4, f1) <= TOL and normwise(f1, a32) <= TOL
    if name.startswith("k3"):  # the other tail kernels carry the same state
        for tail in TAILS:
            c16, c32, _ = gpu_run(torch_cuda, iq, cfg, calls=1, tail=tail, fir=0)
            d16, d32, _ = gpu_run(torch_cuda, iq, cfg, calls=calls, tail=tail, fir=0)
            assert np.array_equal(c16, d16) and np.array_equal(c32, d32)
            assert np.abs(c32 - a32).max() <= 1e-5 * np.abs(a32).max()


@pytest.mark.parametrize("nco_hz", [12000.0, 12345.678])
@pytest.mark.parametrize("name,cfg", [("k2", K1), ("k3", K3), ("usb_2048_agc", dict(fft_l=2048, demod="USB", agc_mode="fast"))])
def test_default_decimator_gives_the_same_bits_for_random_call_splits(rdsp, torch_cuda, name, cfg, nco_hz):
    """The library's default (frequency domain, one granule per decimator frame) over random call splits: int16,
    float32 and the per-channel scalars bit-identical to one call -- the streaming runner and the graph's engine
    node pick their own batch sizes and must not change a bit of a recording's audio.  The noise blanker is on,
    and a session of control calls runs at fixed stream positions (which every split therefore has as call
    boundaries): a retune, a non-power-of-two input gain, an IQ balance, an IQ swap.  nco_hz 12000 at fs 96000 is
    the degenerate case (every column phasor is exactly +-1 or +-j); 12345.678 is a generic increment, where a
    frame's column phasors only agree between splits if they are a function of the absolute position alone."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    nch, nblk = 4, 128
    iq = synth_iq(nch, nblk * 128)
    iq[:, 5000:5003] = 30000
    rng = np.random.default_rng(17)
    cfg = dict(cfg, nco_hz=nco_hz)
    gran = Chain(nch, max_blocks_per_call=nblk, **cfg).call_unit_blocks
    n_gran = nblk // gran
    script = {n_gran // 4: lambda ch: ch.setTuningOffsetHz(nco_hz - 2468.3),
              n_gran // 2: lambda ch: ch.setInputGain(0.7),
              5 * n_gran // 8: lambda ch: ch.swapIQ(True),
              3 * n_gran // 4: lambda ch: ch.setIQgainBalance(1.02),
              7 * n_gran // 8: lambda ch: (ch.setIQgainBalance(1.0), ch.swapIQ(False), ch.setInputGain(1.3))}

    def run(cuts):
        ch = Chain(nch, max_blocks_per_call=nblk, fir_variant=-1, **cfg)
        ch.enableNoiseBlanker()
        o, f = [], []
        edges = sorted(set(cuts) | set(script))
        for a, b in zip([0] + edges, edges + [n_gran]):
            if a in script:
                script[a](ch)
            part = torch.from_numpy(np.ascontiguousarray(iq[:, a * gran * 128:b * gran * 128])).cuda()
            x16, x32 = ch.process(part, want_f32=True)
            torch.cuda.synchronize()
            o.append(x16.cpu().numpy())
            f.append(x32.cpu().numpy())
        return np.concatenate(o, 1), np.concatenate(f, 1), ch.scalars()

    one, one32, sc = run([])
    assert np.abs(one32).max() > 0.01
    for trial in range(5):
        cuts = sorted(set(int(x) for x in rng.integers(1, n_gran, size=rng.integers(1, 7))))
        o, f, s2 = run(cuts)
        assert np.array_equal(o, one) and np.array_equal(f, one32) and np.array_equal(s2, sc), (name, cuts)


@pytest.mark.parametrize("nco_hz", [12000.0, 12345.678])
@pytest.mark.parametrize("name,cfg", [("k2", K1), ("k3", K3), ("k4", K4), ("usb_1024", dict(fft_l=1024, demod="USB", agc_mode="medium"))])
def test_throughput_decimator_is_split_invariant_on_whole_frames(rdsp, torch_cuda, name, cfg, nco_hz):
    """rdsp_chain_set_fir_variant(2) (448-sample decimator frames, what bench.py runs): a stream cut into calls that
    are multiples of rdsp_chain_granule_blocks() = lcm(14 blocks, call unit) is cut at frame boundaries, the frame
    grid sits at absolute stream positions and int16, float32 and scalars are bit-identical to one call for any
    such split -- with the blanker on and a retune / gain / balance / swap session at granule positions."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    probe = Chain(2, max_blocks_per_call=8, fir_variant=2, **cfg)
    gran, unit = probe.granule_blocks, probe.call_unit_blocks
    assert gran % 14 == 0 and gran % unit == 0 and gran == unit * 14 // np.gcd(unit, 14)
    assert Chain(2, max_blocks_per_call=8, fir_variant=-1, **cfg).granule_blocks == unit
    n_gran = 8 if gran <= 112 else 4
    nch, nblk = 3, n_gran * gran
    iq = synth_iq(nch, nblk * 128, cw=(name == "k4"))
    iq[:, 7000:7003] = 30000
    cfg = dict(cfg, nco_hz=nco_hz)
    script = {n_gran // 4: lambda ch: ch.setTuningOffsetHz(nco_hz - 1357.9),
              n_gran // 2: lambda ch: (ch.setInputGain(0.7), ch.swapIQ(True)),
              3 * n_gran // 4: lambda ch: (ch.setIQgainBalance(1.02), ch.swapIQ(False))}

    def run(cuts):
        ch = Chain(nch, max_blocks_per_call=nblk, fir_variant=2, **cfg)
        ch.enableNoiseBlanker()
        o, f = [], []
        edges = sorted(set(cuts) | set(script))
        for a, b in zip([0] + edges, edges + [n_gran]):
            if a in script:
                script[a](ch)
            x16, x32 = ch.process(torch.from_numpy(np.ascontiguousarray(iq[:, a * gran * 128:b * gran * 128])).cuda(), want_f32=True)
            torch.cuda.synchronize()
            o.append(x16.cpu().numpy())
            f.append(x32.cpu().numpy())
        return np.concatenate(o, 1), np.concatenate(f, 1), ch.scalars()

    one, one32, sc = run([])
    assert np.abs(one32).max() > 0.01
    rng = np.random.default_rng(23)
    for trial in range(4):
        cuts = sorted(set(int(x) for x in rng.integers(1, n_gran, size=rng.integers(1, 5))))
        o, f, s2 = run(cuts)
        assert np.array_equal(o, one) and np.array_equal(f, one32) and np.array_equal(s2, sc), (name, cuts)
    o, f, s2 = run(list(range(1, n_gran)))      # every granule its own call
    assert np.array_equal(o, one) and np.array_equal(f, one32) and np.array_equal(s2, sc)


@pytest.mark.parametrize("name,cfg,bound", [("k2", K1, 1e-6), ("k3", K3, TOL)])
def test_frequency_domain_decimator_call_split_sensitivity_is_pinned(rdsp, torch_cuda, name, cfg, bound):
    """The throughput form of the frequency-domain decimator (rdsp_chain_set_fir_variant 2; bench.py: 448-sample
    frames) anchors its frames at each call's first sample: the same stream cut into calls differently is framed differently and rounds
    differently.  Pinned here over random call splits: the worst difference from the one-call result stays
    at float32 rounding for the feed-forward chain (measured 2.6e-7 of the output's peak, bound 1e-6; int16
    within 1 LSB) and inside the north-star's 1e-5 (measured 2.8e-6) through K3's recursive stages.  The
    default (one granule per frame) and the direct form give the same BITS for any split:
    test_split_calls_are_bitwise_identical_to_one_call."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    nch, nblk = 4, 128
    iq = synth_iq(nch, nblk * 128)
    gran = Chain(nch, max_blocks_per_call=nblk, **cfg).call_unit_blocks   # cuts off the frame grid (granule_blocks is 56 here)
    one16, one32, _ = gpu_run(torch, iq, cfg, calls=1, fir=2)
    rng = np.random.default_rng(5)
    worst, worst_lsb = 0.0, 0
    for trial in range(6):
        cuts = sorted(set(int(x) * gran for x in rng.integers(1, nblk // gran, size=rng.integers(1, 6))))
        ch = Chain(nch, max_blocks_per_call=nblk, fir_variant=2, **cfg)
        o16, o32 = [], []
        for a, b in zip([0] + cuts, cuts + [nblk]):
            x16, x32 = ch.process(torch.from_numpy(np.ascontiguousarray(iq[:, a * 128:b * 128])).cuda(), want_f32=True)
            torch.cuda.synchronize()
            o16.append(x16.cpu().numpy()); o32.append(x32.cpu().numpy())
        worst = max(worst, normwise(np.concatenate(o32, 1), one32))
        worst_lsb = max(worst_lsb, int(np.abs(np.concatenate(o16, 1).astype(np.int32) - one16).max()))
    print(f"{name}: worst difference over random call splits {worst:.2e} of the peak, {worst_lsb} LSB")
    assert worst <= bound
    if name == "k2":
        assert worst_lsb <= 1


@pytest.mark.parametrize("name,cfg,nch,nblk", [
    ("k3", K3, 64, 32),
    ("usb256_nr", dict(fft_l=256, demod="USB", lms_nr=10, agc_mode="slow"), 24, 16),           # DSP-NR instance, radix 4
    ("lsb2048_notch", dict(fft_l=2048, demod="LSB", als_mode="notch", als_strength=15), 9, 32),  # four waves per channel
    ("am1024_peak", dict(fft_l=1024, demod="AM", als_mode="peak", agc_mode="fast"), 5, 32),      # radix 16, lean kernel
])
def test_pipelined_mode_is_bitwise_identical(rdsp, torch_cuda, name, cfg, nch, nblk):
    """rdsp_chain_set_pipelined: the tail stage of call k overlaps the front stage of
    call k+1 on an internal stream; results must not change by a bit -- at every FFT size
    (front kernels of 1 and 4 waves, full-register and lean) and tail instance."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    calls = 6
    K3 = cfg  # noqa: N806 -- the body below was written for the K3 case
    iq = synth_iq(nch, nblk * 128 * calls)
    parts = [torch.from_numpy(np.ascontiguousarray(iq[:, k * nblk * 128:(k + 1) * nblk * 128])).cuda()
             for k in range(calls)]
    ref_chain = Chain(nch, max_blocks_per_call=nblk, **K3)
    ref = [ref_chain.process(p).cpu().numpy() for p in parts]
    ch = Chain(nch, max_blocks_per_call=nblk, **K3)
    ch.set_pipelined(True)
    outs = [torch.empty((nch, nblk * 32, 2), dtype=torch.int16, device="cuda") for _ in range(calls)]
    for p, o in zip(parts, outs):
        ch.process(p, out=o)
    ch.flush()
    torch.cuda.synchronize()
    for a, b in zip(ref, outs):
        assert np.array_equal(a, b.cpu().numpy())
    assert np.array_equal(ref_chain.scalars(), ch.scalars())
    for which in (0, 1):   # DSP-NR and ALS instances
        assert np.array_equal(ref_chain.lms_coeffs(which), ch.lms_coeffs(which))


def test_tail_stage_toggled_between_pipelined_calls_is_bitwise_identical(rdsp, torch_cuda):
    """disableALSfilter / enableALSfilter / set_nr_level between pipelined calls: a call whose tail
    stage is off packs in the front kernel on the caller's stream, and must wait for the previous
    call's tail stage (internal stream), which still owns that call's output and the AGC gain."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    nch, nblk = 70, 32
    plan = ["on", "on", "off", "off", "on", "nr", "off", "on"]   # ALS on/off, DSP-NR instead of ALS
    iq = synth_iq(nch, nblk * 128 * len(plan))
    parts = [torch.from_numpy(np.ascontiguousarray(iq[:, k * nblk * 128:(k + 1) * nblk * 128])).cuda()
             for k in range(len(plan))]

    def run(pipelined):
        ch = Chain(nch, max_blocks_per_call=nblk, **K3)
        ch.set_pipelined(pipelined)
        out = torch.zeros((nch, nblk * 32 * len(plan), 2), dtype=torch.int16, device="cuda")
        for k, what in enumerate(plan):
            ch.disableALSfilter() if what in ("off", "nr") else ch.enableALSfilter()
            ch.set_nr_level(20 if what == "nr" else 0)
            # all calls write into ONE buffer back to back, as a streaming sink would
            ch.process(parts[k], out=out[:, k * nblk * 32:(k + 1) * nblk * 32])
        ch.flush()
        torch.cuda.synchronize()
        return out.cpu().numpy(), ch.scalars(), ch.lms_coeffs(0), ch.lms_coeffs(1)

    a, b = run(False), run(True)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_channel_sub_batches_are_bitwise_identical(rdsp, torch_cuda):
    """rdsp_chain_set_sub_batch: a pipelined call goes out as launches of `sub` channels each
    (ragged last one), front and tail of a sub-batch chained by their own event; nothing changes."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    nch, nblk, calls = 202, 16, 4   # the last sub-batch is ragged and so is its last tail workgroup (2 of 4 channels)
    iq = synth_iq(nch, nblk * 128 * calls)
    parts = [torch.from_numpy(np.ascontiguousarray(iq[:, k * nblk * 128:(k + 1) * nblk * 128])).cuda()
             for k in range(calls)]

    def run(sub):
        ch = Chain(nch, max_blocks_per_call=nblk, **K3)
        ch.set_pipelined(True)
        ch.set_sub_batch(sub)
        outs = [ch.process(p, want_f32=True) for p in parts]
        ch.flush()
        torch.cuda.synchronize()
        return (np.concatenate([o[0].cpu().numpy() for o in outs], 1),
                np.concatenate([o[1].cpu().numpy() for o in outs], 1))

    a16, a32 = run(0)
    for sub in (64, 128):       # 64: four launches (64, 64, 64, 10 channels); 128: two (128, 74)
        b16, b32 = run(sub)
        assert np.array_equal(a16, b16) and np.array_equal(a32, b32), sub
    with pytest.raises(Exception):
        Chain(4, max_blocks_per_call=8, **K3).set_sub_batch(100)   # not a multiple of 64


def test_front_kernel_variants_agree(rdsp, oracle, torch_cuda):
    """The full-register and the register-lean front kernels are the same chain with
    differently rounded FFT twiddles: both meet TOL against the oracle."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    cfg = dict(fft_l=512, demod="USB", spectral_nr=1, spectral_level=2.0, agc_mode="medium")
    iq = synth_iq(4, 32 * 128)
    _, r32 = oracle_run(oracle, iq, cfg)
    # register-lean x stage A3 (0 direct form, 2 frequency domain)
    for lean, fir in ((0, 0), (1, 0), (0, 2), (1, 2)):
        ch = Chain(4, max_blocks_per_call=32, **cfg)
        ch.set_front_variant(lean)
        ch.set_fir_variant(fir)
        f = ch.process(torch.from_numpy(iq).cuda(), want_f32=True)[1].cpu().numpy()
        assert normwise(f, r32) <= TOL, (lean, fir)


def test_channel_partition_invariance(rdsp, torch_cuda):
    """Multi-GPU sharding contract: a channel's output does not depend on
    which shard / position it is processed at -- bitwise."""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    iq = synth_iq(12, 32 * 128)
    full, _, _ = gpu_run(torch_cuda, iq, K3)
    lo, _, _ = gpu_run(torch_cuda, iq[:5], K3)
    hi, _, _ = gpu_run(torch_cuda, iq[5:], K3)
    assert np.array_equal(full, np.concatenate([lo, hi]))
    perm = np.array([7, 2, 11, 0, 5])
    sub, _, _ = gpu_run(torch_cuda, iq[perm], K3)
    assert np.array_equal(sub, full[perm])


def test_retune_mid_stream_matches_oracle(rdsp, oracle, torch_cuda):
    """reInitializeFilter (CONV:209, the PBT path CTL:569-612) between calls."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    iq = synth_iq(2, 32 * 128)
    ch = Chain(2, max_blocks_per_call=16, **K1)
    a = ch.process(torch.from_numpy(iq[:, :2048].copy()).cuda(), want_f32=True)[1].cpu().numpy()
    ch.reInitializeFilter(350.0, 2650.0)
    b = ch.process(torch.from_numpy(iq[:, 2048:].copy()).cuda(), want_f32=True)[1].cpu().numpy()
    got = np.concatenate([a, b], 1)
    for c in range(2):
        oc = oracle.OracleChain(**K1)
        r1 = oc.process(iq[c, :2048])[1]
        oc.reinit_filter(350.0, 2650.0)
        r2 = oc.process(iq[c, 2048:])[1]
        ref = np.concatenate([r1, r2])
        assert np.abs(got[c] - ref).max() / np.abs(ref).max() <= TOL
    assert np.abs(ch.mask() - oc.mask()).max() < 2e-6


def test_engine_setters_and_reference_shaped_call(rdsp, oracle, torch_cuda):
    torch = torch_cuda
    from radiodsp_sdr_rx_amd import RdspError
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    iq = synth_iq(2, 16 * 128)
    dev = torch.from_numpy(iq).cuda()
    ch = Chain(2, max_blocks_per_call=16, **K1)
    assert ch.setDemodMode(rdsp.DEMOD["CW_USB"]) == 6390 and ch.setDemodMode(rdsp.DEMOD["USB"]) == 5390   # the engine's own answers (test_firmware_kat.py)
    ch.setAudioFilter(rdsp.AUDIO_FILTER["audio2700"])
    ch.setInputGain(1.0); ch.setOutputGain(0.5); ch.setIQgainBalance(1.02)
    ch.enableAGC(); ch.setAGCmode(rdsp.AGC["medium"]); ch.disableALSfilter(); ch.disableNoiseBlanker()
    with pytest.raises(RdspError):
        ch.setNoiseBlankerThresholdDb(-3.0)  # outside 0..60 dB
    ch.reset()
    out = ch.doConvolutionalProcessing(0, True, 300.0, 4000.0, dev)  # cut-offs ignored like CONV:300
    torch.cuda.synchronize()
    ref = oracle_run(oracle, iq, dict(K1, flo_hz=150.0, fhi_hz=2700.0, agc_mode="medium", output_gain=0.5,
                                      iq_balance=1.02))[0]
    assert check_i16(out.cpu().numpy(), ref) < 50
    ch.setMute(True)
    assert not ch.process(dev).cpu().numpy().any()
    # granule / argument errors are loud
    with pytest.raises(RdspError):
        ch.process(dev[:, :128 * 3].contiguous())
    big = Chain(1, max_blocks_per_call=8, **K1)
    with pytest.raises(RdspError):
        big.process(dev[:1].contiguous())


# ---- full-size properties (BASELINE.json sizes) -------------------------------------------
def test_full_size_k2_sampled_channels_and_linearity(rdsp, oracle, torch_cuda):
    """4096 channels (K2): sampled channels against the oracle, and homogeneity --
    the filter chain is linear, so input/2 gives output/2 within TOL."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    nch, nblk = 4096, 64
    iq = synth_iq(nch, nblk * 128)
    dev = torch.from_numpy(iq).cuda()
    ch = Chain(nch, max_blocks_per_call=nblk, **K1)
    o16, o32 = ch.process(dev, want_f32=True)
    torch.cuda.synchronize()
    sample = [0, 1, 63, 64, 1000, 2047, 2048, 4095]
    f = o32[sample].cpu().numpy()
    r16, r32 = oracle_run(oracle, iq[sample], K1)
    assert normwise(f, r32) <= TOL
    check_i16(o16[sample].cpu().numpy(), r16)
    half = torch.from_numpy((iq // 2 * 2 // 2).astype(np.int16)).cuda()  # exact halves of even values
    ch2 = Chain(nch, max_blocks_per_call=nblk, **K1)
    h32 = ch2.process(half, want_f32=True)[1]
    even = torch.from_numpy((iq // 2 * 2).astype(np.int16)).cuda()
    ch3 = Chain(nch, max_blocks_per_call=nblk, **K1)
    e32 = ch3.process(even, want_f32=True)[1]
    torch.cuda.synchronize()
    num = (e32 * 0.5 - h32).abs().amax(dim=(1, 2))
    den = h32.abs().amax(dim=(1, 2))
    assert float((num / den).max()) <= TOL


def test_full_size_k3_sampled_channels(rdsp, oracle, torch_cuda):
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    nch, nblk = 4096, 64
    iq = synth_iq(nch, nblk * 128)
    ch = Chain(nch, max_blocks_per_call=nblk, **K3)
    o16, o32 = ch.process(torch.from_numpy(iq).cuda(), want_f32=True)
    torch.cuda.synchronize()
    sample = [0, 3, 4, 1023, 2048, 4093, 4095]
    r16, r32 = oracle_run(oracle, iq[sample], K3)
    assert_truth_anchored(o32[sample].cpu().numpy(), r32, model_run(iq[sample], K3), "K3 full size",
                          o16[sample].cpu().numpy(), r16)
    # the metric configuration meets the north-star's tolerance against the float32 oracle directly
    # (measured 3e-6 .. 6e-6: the spectral stage's floor and the AGC keep the notch's start-up small)
    assert normwise(o32[sample].cpu().numpy(), r32) <= TOL
    # every channel produced finite, non-trivial audio under AGC
    pw = o32[..., 0].float().pow(2).mean(dim=1)
    assert bool(torch.isfinite(pw).all()) and float(pw.min()) > 1e-6


def test_k5_per_gpu_shape_pipelined_sub_batched(rdsp, oracle, torch_cuda):
    """BASELINE config K5 as one GPU sees it: 8192 channels of the K3 chain in pipelined mode, which
    is the shape that takes the default 4096-channel sub-batch path (front(A), front(B) on the
    caller's stream, tail(A), tail(B) on the tail stream).  Three calls of 32 blocks: sampled
    channels of both sub-batches against the oracle (truth-anchored NLMS criterion), and the
    whole output bitwise equal to the same chain un-pipelined, state included."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    nch, nblk, calls = 8192, 32, 3
    iq = synth_iq(nch, nblk * 128 * calls, n_threads=16)
    dev = torch.from_numpy(iq).cuda()
    n_out = nblk * 32

    def run(pipelined):
        ch = Chain(nch, max_blocks_per_call=nblk, **K3)
        ch.set_pipelined(pipelined)            # sub_batch stays at its default (4096)
        o16 = torch.zeros((nch, n_out * calls, 2), dtype=torch.int16, device="cuda")
        o32 = torch.zeros((nch, n_out * calls, 2), dtype=torch.float32, device="cuda")
        for k in range(calls):
            ch.process(dev[:, k * nblk * 128:(k + 1) * nblk * 128], out=o16[:, k * n_out:(k + 1) * n_out],
                       out_f32=o32[:, k * n_out:(k + 1) * n_out])
        ch.flush()
        torch.cuda.synchronize()
        return o16, o32, ch.scalars(), ch.lms_coeffs(1)

    p16, p32, psc, pw = run(True)
    sample = [0, 1, 2047, 4095, 4096, 4097, 6000, 8191]
    r16, r32 = oracle_run(oracle, iq[sample], K3)
    assert_truth_anchored(p32[sample].cpu().numpy(), r32, model_run(iq[sample], K3), "K5 shape",
                          p16[sample].cpu().numpy(), r16)
    u16, u32, usc, uw = run(False)
    assert bool((p16 == u16).all()) and bool((p32 == u32).all())
    assert np.array_equal(psc, usc) and np.array_equal(pw, uw)
    pw_ch = p32[..., 0].pow(2).mean(dim=1)
    assert bool(torch.isfinite(pw_ch).all()) and float(pw_ch.min()) > 1e-6


def test_full_size_k4_sampled_channels(rdsp, oracle, torch_cuda):
    """8192 channels, CW, FFT_L = 4096 (2049-tap overlap-save) + AGC: sampled channels
    against the oracle at the BASELINE channel count."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    nch, nblk = 8192, 128
    iq = synth_iq(nch, nblk * 128, cw=True)
    ch = Chain(nch, max_blocks_per_call=nblk, **K4)
    o16, o32 = ch.process(torch.from_numpy(iq).cuda(), want_f32=True)
    torch.cuda.synchronize()
    sample = [0, 1, 4095, 4096, 8190, 8191]
    r16, r32 = oracle_run(oracle, iq[sample], K4)
    assert normwise(o32[sample].cpu().numpy(), r32) <= TOL
    check_i16(o16[sample].cpu().numpy(), r16)
    g = ch.scalars()[:, 1]
    assert np.isfinite(g).all() and (g > 0).all()


def test_long_stream_many_calls_stays_on_the_oracle(rdsp, oracle, torch_cuda):
    """40 consecutive calls (state carried in HBM the whole time, pipelined mode on):
    no drift against the oracle on a feed-forward chain, AGC gain and NFloor included."""
    torch = torch_cuda
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    cfg = dict(fft_l=512, demod="USB", spectral_nr=1, spectral_level=2.0, agc_mode="slow", output_gain=0.5)
    nch, nblk, calls = 3, 16, 40
    iq = synth_iq(nch, nblk * 128 * calls)
    ch = Chain(nch, max_blocks_per_call=nblk, **cfg)
    ch.set_pipelined(True)
    outs = []
    for k in range(calls):
        part = torch.from_numpy(np.ascontiguousarray(iq[:, k * nblk * 128:(k + 1) * nblk * 128])).cuda()
        outs.append(ch.process(part, want_f32=True)[1])
    ch.flush()
    torch.cuda.synchronize()
    got = np.concatenate([o.cpu().numpy() for o in outs], axis=1)
    _, r32 = oracle_run(oracle, iq, cfg)
    per_call = np.abs(got - r32).max(axis=2).reshape(nch, calls, -1).max(axis=2) / np.abs(r32).max()
    assert per_call.max() <= TOL   # measured 5.3e-7: no bin lands on the other side of the spectral threshold
    sc = ch.scalars()
    for c in range(nch):
        oc = oracle.OracleChain(**cfg)
        oc.process(iq[c])
        assert abs(sc[c, 0] - oc.nfloor()) <= 2e-6 * oc.nfloor()       # measured <= 3.7e-7
        assert abs(sc[c, 1] - oc.agc_gain()) <= 2e-6 * oc.agc_gain()   # measured <= 7.3e-8


# ---- edge inputs ---------------------------------------------------------------------
def _edge_inputs(n):
    """one channel each: silence; silence then signal; rail-to-rail square waves (periods 2 and 96 samples);
    full-scale DC; one full-scale impulse; full-scale noise; signal then silence"""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    sig = synth_iq(2, n)
    rng = np.random.default_rng(5)
    t = np.arange(n)
    x = np.zeros((9, n, 2), np.int16)
    x[1, n // 2:] = sig[0, n // 2:]
    x[2, :, 0] = np.where(t % 2 == 0, 32767, -32768); x[2, :, 1] = -x[2, :, 0] - 1
    x[3, :, 0] = np.where((t // 48) % 2 == 0, 32767, -32768); x[3, :, 1] = np.where((t // 48 + 1) % 2 == 0, 32767, -32768)
    x[4, :, 0] = 32767; x[4, :, 1] = -32768
    x[5, n // 3] = (32767, -32768)
    x[6] = rng.integers(-32768, 32768, size=(n, 2)).astype(np.int16)
    x[7, :n // 2] = sig[1, :n // 2]
    x[8] = sig[1]; x[8, ::1000] = (-32768, -32768)
    return x


EDGE_CFGS = {
    "k1_agc": dict(K1, agc_mode="medium"),
    "am_slow": dict(fft_l=512, demod="AM", flo_hz=-3900.0, fhi_hz=3900.0, agc_mode="slow"),
    "spectral_fast": dict(fft_l=256, demod="USB", spectral_nr=1, spectral_level=2.0, agc_mode="fast", output_gain=0.5),
    "spectral_old_lsb": dict(fft_l=512, demod="LSB", flo_hz=-2700.0, fhi_hz=-300.0, spectral_nr=2, output_gain=0.5),
    "cw_2048": dict(fft_l=2048, demod="CW_USB", flo_hz=450.0, fhi_hz=950.0, nco_hz=11300.0, agc_mode="fast"),
    "literal": CONV_LITERAL,
}


@pytest.mark.parametrize("name", sorted(EDGE_CFGS))
def test_edge_inputs_feed_forward(rdsp, oracle, torch_cuda, name):
    """silence, rails, DC, an impulse, full-scale noise, signal switching on and off: every division,
    square root and saturation of the chain at its corner (0/0 in the spectral stage's gain, an AGC
    looking at zero power, the pack's saturation); against the oracle at TOL, exact zeros where the
    oracle gives exact zeros, nothing non-finite"""
    cfg = EDGE_CFGS[name]
    n = 128 * (64 if cfg.get("fft_l", 256) >= 2048 else 32)
    iq = _edge_inputs(n)
    o16, o32, ch = gpu_run(torch_cuda, iq, cfg, calls=2)
    r16, r32 = oracle_run(oracle, iq, cfg)
    assert np.isfinite(o32).all() and np.isfinite(r32).all()
    sc = ch.scalars()
    assert np.isfinite(sc).all()
    f64 = None
    for c in range(iq.shape[0]):
        if c in (2, 4) and cfg.get("agc_mode", "off") != "off" and cfg.get("decim", 4) == 4:
            continue   # the rejected inputs under an AGC: test_rejected_full_scale_input_error_floor
        peak = np.abs(r32[c]).max()
        if peak == 0.0:
            assert np.abs(o32[c]).max() == 0.0 and not o16[c].any(), f"channel {c}: output on silence"
            continue
        err = np.abs(o32[c] - r32[c]).max() / peak
        if err > TOL:
            # weak in-band content under strong components elsewhere in the band (the even harmonic of a
            # rail-to-rail square wave in a 500 Hz CW filter, brought up to level by the AGC): both float32
            # FFT filters sit on their rounding floor and neither is the yardstick -- the float64
            # evaluation is, with the criterion of the recursive chains
            if f64 is None:
                f64 = model_run(iq, cfg)
            den = np.abs(f64[c]).max()
            eg, eo = np.abs(o32[c] - f64[c]).max() / den, np.abs(r32[c] - f64[c]).max() / den
            print(f"  {name} channel {c}: gpu {eg:.2e} oracle {eo:.2e} from the float64 result (gpu vs oracle {err:.2e})")
            assert eg <= max(TOL, 1.5 * eo), f"{name} channel {c}: gpu {eg:.2e} vs oracle {eo:.2e} from the float64 result"
            continue
        d = np.abs(o16[c].astype(np.int32) - r16[c].astype(np.int32))
        assert d.max() <= 1, f"{name} channel {c}: int16 differs by {d.max()}"


@pytest.mark.parametrize("fft_l", [256, 2048])
def test_rejected_full_scale_input_error_floor(rdsp, oracle, torch_cuda, fft_l):
    """A full-scale square wave at fs/2 -- or full-scale DC, which the mixer turns into a tone 11.3 kHz off
    tune -- lies 100 dB down in the stop bands: what comes out is the -1 LSB asymmetry of the rails plus
    rounding residue.  An FFT convolution's rounding error is
    relative to the strongest component in the band (float32 eps x full scale here), a direct form's to
    its tap-weighted partial sums, so in *absolute* terms both are far below the int16 input's own
    quantisation (1.5e-5 of full scale), but relative to that residual output the frequency-domain
    decimator can pass 1e-5 once an AGC has brought the residue up to level.  Stated as what it is: the
    absolute floor of both forms against the float64 evaluation, AGC off."""
    from radiodsp_sdr_rx_amd.chain import Chain
    torch = torch_cuda
    n = 128 * 64
    iq = _edge_inputs(n)[[2, 4]]
    cfg = dict(fft_l=fft_l, demod="CW_USB", flo_hz=450.0, fhi_hz=950.0, nco_hz=11300.0)
    f64 = model_run(iq, cfg)
    _, r32 = oracle_run(oracle, iq, cfg)
    floor = {}
    for fir in (2, 0):
        ch = Chain(2, max_blocks_per_call=n // 128, **cfg)
        ch.set_fir_variant(fir)
        g = ch.process(torch.from_numpy(iq).cuda(), want_f32=True)[1].cpu().numpy()
        floor[fir] = np.abs(g - f64).max()
    eo = np.abs(r32 - f64).max()
    assert np.abs(f64).max() < 1e-2                      # the inputs are rejected (full scale is 1.0)
    assert floor[2] <= 1e-7 and floor[0] <= 4e-8, floor  # square wave: 2.9e-8 and 1.0e-8; the oracle 9.5e-9
    assert floor[0] <= max(4e-8, 1.5 * eo)


def test_edge_inputs_full_chain_truth_anchored(rdsp, oracle, torch_cuda):
    """the same inputs through K3 (spectral NR + LMS notch + AGC): finite everywhere, silence stays
    silence, the rest under the truth-anchored criterion"""
    n = 128 * 64
    iq = _edge_inputs(n)
    o16, o32, ch = gpu_run(torch_cuda, iq, K3, calls=2)
    r16, r32 = oracle_run(oracle, iq, K3)
    f64 = model_run(iq, K3)
    assert np.isfinite(o32).all() and np.isfinite(r32).all() and np.isfinite(f64).all()
    assert np.isfinite(ch.scalars()).all() and np.isfinite(ch.lms_coeffs(1)).all()
    live = [c for c in range(iq.shape[0]) if np.abs(f64[c]).max() > 0.0]
    for c in range(iq.shape[0]):
        if c not in live:
            assert np.abs(o32[c]).max() == 0.0 and np.abs(r32[c]).max() == 0.0
    assert_truth_anchored(o32[live], r32[live], f64[live], "edge inputs through K3", o16[live], r16[live])
