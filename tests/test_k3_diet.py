"""The tail kernel's epilogue (rdsp_tail.hip: AGC, output gain, A10 pack), pinned for any rewrite of it: the int16 it
writes is arm_float_to_q15 of the float it writes, to the bit, and the float is (AGC output) x out_gain, rounded once.
(Written with the 69-instruction epilogue of docs/history.md, "The K3 diet, part A", which passed it and left the tree on
its timing; the epilogue there is today passes it too.)

The chain is the one the K3 step ends in -- 512-point filter, ALS notch, AGC on and off -- on 6 channels (not a multiple
of the four a tail wave holds) and 8 input blocks per run.  Two float32 implementations of an NLMS chain do not agree
to the last bit (tests/parity_util.py), so "against the oracle's int16" is taken where it can hold exactly: the
oracle's own arm_float_to_q15 (orc_float_to_q15: x 32768, +-0.5 by sign, truncate, saturate) applied to the float
output of the same GPU run must give the int16 output of that run, every sample.  What this is about are the ties
(float x 32768 = k + 0.5, rounded away from zero) and the two rails.  A float32 near full scale lands on a tie once in
512 samples, so each case runs the same 8 blocks at 64 amplitudes (a ladder of eighth-octaves that ends in hard
clipping: constant-amplitude tones) behind an input gain of 8, which takes the audio over both rails; the oracle
chain, on the CPU, is checked first to produce ties and both rails on these inputs (24 to 48 ties per case)."""
import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu

NCH, NBLK = 6, 8
CFG = dict(fft_l=512, demod="USB", als_mode="notch", als_strength=20, input_gain=8.0)
SCALES = [2.0 ** (k / 8) for k in range(-8, 56)]


def q15_ref(x):
    """arm_float_to_q15 in float32 steps, defined for every float (the oracle's C cast is not, for infinities)"""
    v = x.astype(np.float32) * np.float32(32768.0)
    v = v + np.where(v > 0, np.float32(0.5), np.float32(-0.5)).astype(np.float32)
    return np.clip(np.trunc(np.nan_to_num(v.astype(np.float64), nan=0.0)), -32768, 32767).astype(np.int16)


def is_tie(x):
    """float x 32768 is k + 0.5 inside the rails"""
    t = np.abs(x.astype(np.float32) * np.float32(32768.0))
    return (t - np.floor(t) == 0.5) & (t < 32767)


@pytest.fixture(scope="module")
def inputs(rdsp):
    from radiodsp_sdr_rx_amd.chain import synth_iq
    iq0 = synth_iq(NCH, NBLK * 128).astype(np.float64)
    return np.stack([np.clip(np.rint(iq0 * s), -32768, 32767).astype(np.int16) for s in SCALES])


def gpu_runs(inputs, agc, og):
    """int16 and float32 outputs [scale, ch, n, 2] of fresh chains at output gain og"""
    from radiodsp_sdr_rx_amd.chain import Chain
    ch = Chain(NCH, max_blocks_per_call=NBLK, fir_variant=2, **dict(CFG, agc_mode=agc, output_gain=og))
    o16, o32 = [], []
    for iq in torch.from_numpy(inputs).cuda():
        ch.reset()
        a, b = ch.process(iq, want_f32=True)
        o16.append(a.clone())
        o32.append(b.clone())
    torch.cuda.synchronize()
    return torch.stack(o16).cpu().numpy(), torch.stack(o32).cpu().numpy()


@gpu
@pytest.mark.parametrize("agc", ["off", "medium"])
@pytest.mark.parametrize("og", [0.5, 0.37, 3.0])
def test_pack_is_the_oracles_q15_of_the_float_output(oracle, inputs, agc, og):
    import ctypes as C
    lib = oracle.load()
    # the oracle chain itself, on the CPU: these inputs give it ties and both rails, or the test shows nothing
    ties = hi = lo = 0
    for iq in inputs:
        for c in range(NCH):
            r16, r32 = oracle.OracleChain(**dict(CFG, agc_mode=agc, output_gain=og)).process(iq[c])
            ties += int(is_tie(r32).sum())
            hi += int((r16 == 32767).sum())
            lo += int((r16 == -32768).sum())
    print(f"oracle, agc {agc} gain {og}: {ties} ties, {hi} / {lo} samples on the rails")
    assert ties > 0 and hi > 0 and lo > 0

    g16, g32 = gpu_runs(inputs, agc, og)
    u32 = gpu_runs(inputs, agc, 1.0)[1]
    gt, ghi, glo = int(is_tie(g32).sum()), int((g16 == 32767).sum()), int((g16 == -32768).sum())
    print(f"gpu: {gt} ties, {ghi} / {glo} samples on the rails")
    assert gt > 0 and ghi > 0 and glo > 0
    # the float output: the audio behind the AGC (the same run at gain 1) times out_gain, one rounding
    assert np.array_equal(g32, u32 * np.float32(og))
    assert np.array_equal(g32[..., 0], g32[..., 1]) and np.array_equal(g16[..., 0], g16[..., 1])
    # the int16 output: the oracle's arm_float_to_q15 of that float, every sample
    x = np.ascontiguousarray(g32.reshape(-1))
    want = np.zeros(x.size, np.int16)
    lib.orc_float_to_q15(x.ctypes.data_as(C.POINTER(C.c_float)), want.ctypes.data_as(C.POINTER(C.c_int16)), x.size)
    assert np.array_equal(want, q15_ref(x))          # the restatement used below for gains the C cast cannot take
    bad = np.flatnonzero(want != g16.reshape(-1))
    assert bad.size == 0, (bad[:8], x[bad[:8]], want[bad[:8]], g16.reshape(-1)[bad[:8]])


@gpu
def test_pack_with_a_gain_whose_product_with_32768_overflows(inputs):
    """out_gain 2^114: out_gain x 32768 is infinite, so an epilogue that folds the two factors into one has to multiply
    twice here, as the reference does; every sample that is not zero is on a rail"""
    og = 2.0 ** 114
    g16, g32 = gpu_runs(inputs[::16], "off", og)
    u32 = gpu_runs(inputs[::16], "off", 1.0)[1]
    with np.errstate(over="ignore"):
        assert np.array_equal(g32, u32 * np.float32(og))
    assert np.array_equal(g16, q15_ref(g32))
    assert (g16 == 32767).any() and (g16 == -32768).any()


# ---- the decimator's branch rotations, folded into per-group branch spectra (rdsp_front_fd.hip, ROTG) -------------------------
# Chains of at most RDSP_FD_ROT_GROUPS (64) groups mix every polyphase branch with the column phasors alone and read
# rot_r x G_r from the group's slot of a pool the host fills at every retune; column 0 of the first frame behind a retune,
# mixed with the old rotations, takes roth_r conj(rot_r).  Criterion: tests/parity_util.py, 1e-5 normwise per channel
# against one oracle chain per channel (feed-forward chains); groups that were not retuned to the bit against a run without
# the retune.  Calls are 8 + 16 input blocks: a call is a multiple of the 8-block call unit.
from cases import TOL  # noqa: E402
from parity_util import normwise  # noqa: E402

GROUP_OF = [0, 1, 2, 1, 0]
CALLS = (8, 16)
FOLD_CASES = {
    "tuned": dict(nco=(12000.0, 14600.0, 9300.0), retune=(1, 13150.0), setup={}),
    "nco_off": dict(nco=(0.0, 0.0, 0.0), retune=(1, 0.0), setup={}),                 # dphi = 0: every rotation is 1
    "from_off": dict(nco=(0.0, 0.0, 12000.0), retune=(1, 2500.0), setup={}),           # the history column came in unmixed
    "swap": dict(nco=(12000.0, 14600.0, 9300.0), retune=(1, 13150.0), setup=dict(swap_iq=True)),     # the PRE instance
    "blanker": dict(nco=(12000.0, 14600.0, 9300.0), retune=(1, 13150.0), setup=dict(noise_blanker_db=8.0)),
}


def fold_run(iq, group_of, case, retune=True, fir_variant=2, pipelined=None, cfg=None, calls=CALLS):
    """float32 output [ch, n, 2] of the two calls, the group's tuning offset changed between them"""
    import radiodsp_sdr_rx_amd as R
    from cases import apply_setup
    from radiodsp_sdr_rx_amd.chain import Chain
    ch = Chain(len(group_of), max_blocks_per_call=max(calls), fir_variant=fir_variant, **(cfg or dict(fft_l=512, demod="USB")))
    ch.set_groups(np.asarray(group_of, np.uint16))
    for g, hz in enumerate(case["nco"]):
        ch.group_setTuningOffsetHz(g, hz)
    for g, (demod, lo, hi) in enumerate(case.get("modes", ())):     # a demodulator and a pass band of the group's own
        ch.group_setDemodMode(g, R.DEMOD[demod])
        ch.group_reInitializeFilter(g, lo, hi)
    apply_setup(ch, case["setup"])
    if pipelined is not None:
        ch.set_pipelined(pipelined)
    dev = torch.from_numpy(iq).cuda()
    parts = [dev[:, :calls[0] * 128].contiguous(), dev[:, calls[0] * 128:].contiguous()]
    a = ch.process(parts[0], want_f32=True)[1]
    if retune:                                          # no synchronisation: the first call may still be queued
        ch.group_setTuningOffsetHz(*case["retune"])
    b = ch.process(parts[1], want_f32=True)[1]
    ch.flush()                                          # pipelined: the outputs are final behind the tail stream
    torch.cuda.synchronize()
    return torch.cat([a, b], 1).cpu().numpy()


def fold_oracle(oracle, iq, group_of, case, cfg=None, calls=CALLS):
    from cases import apply_setup
    outs = []
    for c, g in enumerate(group_of):
        g = g if g < len(case["nco"]) else 0               # a group set_groups made and nobody tuned is a copy of group 0
        kw = dict(cfg or dict(fft_l=512, demod="USB"), nco_hz=case["nco"][g])
        if "modes" in case:
            kw.update(demod=case["modes"][g][0], flo_hz=case["modes"][g][1], fhi_hz=case["modes"][g][2])
        oc = oracle.OracleChain(**kw)
        apply_setup(oc, case["setup"], oracle=True)
        a = oc.process(iq[c, :calls[0] * 128])[1]
        if g == case["retune"][0]:
            oc.set_nco_hz(case["retune"][1])
        outs.append(np.concatenate([a, oc.process(iq[c, calls[0] * 128:])[1]]))
    return np.stack(outs)


@pytest.fixture(scope="module")
def fold_iq(rdsp):
    from cases import add_impulses
    from radiodsp_sdr_rx_amd.chain import synth_iq
    return add_impulses(synth_iq(len(GROUP_OF), sum(CALLS) * 128), every=577)   # bursts for the blanker case to blank


@gpu
@pytest.mark.parametrize("name", list(FOLD_CASES))
def test_rotation_fold_against_the_oracle_with_a_retune_between_two_calls(oracle, fold_iq, name):
    case = FOLD_CASES[name]
    got = fold_run(fold_iq, GROUP_OF, case)
    ref = fold_oracle(oracle, fold_iq, GROUP_OF, case)
    err = [float(np.abs(got[c] - ref[c]).max() / max(np.abs(ref[c]).max(), 1e-30)) for c in range(len(GROUP_OF))]
    print(name, "normwise per channel:", ["%.2e" % e for e in err])
    assert normwise(got, ref) <= TOL
    plain = fold_run(fold_iq, GROUP_OF, case, retune=False)
    for c, g in enumerate(GROUP_OF):
        if g != case["retune"][0]:
            assert np.array_equal(got[c], plain[c]), f"channel {c} of untouched group {g}"
    if case["retune"][1] != case["nco"][case["retune"][0]]:
        assert not np.array_equal(got[1][CALLS[0] * 32:], plain[1][CALLS[0] * 32:])     # the retune did something


@gpu
def test_rotation_fold_default_decimator_frames(oracle, fold_iq):
    """the library's default form (one granule per frame, VC 4) reads the same pool"""
    case = FOLD_CASES["tuned"]
    assert normwise(fold_run(fold_iq, GROUP_OF, case, fir_variant=4), fold_oracle(oracle, fold_iq, GROUP_OF, case)) <= TOL


@gpu
def test_one_group_more_than_the_pool_holds_runs_the_per_frame_rotations(oracle, fold_iq):
    """RDSP_FD_ROT_GROUPS + 1 groups: no pool, today's instance; the same chain, the same criterion -- and the two
    instances agree far inside it without being the same bits"""
    case = FOLD_CASES["tuned"]
    many = [0, 1, 2, 1, 64]             # 65 groups, most of them empty; group 64 is a copy of group 0
    got = fold_run(fold_iq, many, case)
    ref = fold_oracle(oracle, fold_iq, many, case)
    assert normwise(got, ref) <= TOL
    few = fold_run(fold_iq, GROUP_OF, case)            # group 64 and group 0 are tuned alike: the same receivers
    d = normwise(got, few)
    print(f"pool against per-frame rotations: {d:.2e} normwise")
    assert d <= 2e-6
    # ... and they are two instances: were the pool never read (no pool, or the pick never taking it) these would be one
    # kernel's bits twice
    assert not np.array_equal(got, few)


@gpu
def test_rotation_fold_with_an_am_group_beside_two_side_band_groups(oracle, fold_iq):
    """the demodulator is the group's own too: the AM group (the detector behind the same decimator) is the one retuned"""
    case = dict(FOLD_CASES["tuned"], modes=[("USB", 300.0, 2700.0), ("AM", -3900.0, 3900.0), ("LSB", -2400.0, -200.0)])
    got = fold_run(fold_iq, GROUP_OF, case, cfg=dict(fft_l=512, demod="USB", agc_mode="medium", output_gain=0.5))
    ref = fold_oracle(oracle, fold_iq, GROUP_OF, case, cfg=dict(fft_l=512, agc_mode="medium", output_gain=0.5))
    assert normwise(got, ref) <= TOL


@gpu
@pytest.mark.parametrize("fft_l,calls", [(256, (8, 16)), (1024, (16, 32)), (4096, (64, 128))])
def test_rotation_fold_at_the_other_filter_lengths(oracle, fft_l, calls):
    """FFT_L 256 is the four-frames-per-pass instance, 1024 the register-lean radix-16 one, 4096 four waves per channel:
    each has its own copy of the decimator's frame loop, history column included; calls of one and two call units"""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    iq = synth_iq(len(GROUP_OF), sum(calls) * 128)
    cfg = dict(fft_l=fft_l, demod="USB") if fft_l < 4096 else dict(fft_l=4096, demod="CW_USB", flo_hz=450.0, fhi_hz=950.0)
    case = FOLD_CASES["tuned"]
    got = fold_run(iq, GROUP_OF, case, cfg=cfg, calls=calls)
    ref = fold_oracle(oracle, iq, GROUP_OF, case, cfg=cfg, calls=calls)
    assert normwise(got, ref) <= TOL
    plain = fold_run(iq, GROUP_OF, case, retune=False, cfg=cfg, calls=calls)
    assert np.array_equal(got[0], plain[0]) and not np.array_equal(got[1], plain[1])


@gpu
def test_bench_input_of_a_sensitive_channel_is_truth_anchored(oracle):
    """bench.py's K3 input of channel 741 (row 42 of its --dump-outputs draw: the one channel where the per-frame
    rotations and the pool end up 321 LSB apart after 90 steps), 680 and 42, eight steps of 512 blocks
    through the chain bench.py runs: the rule of tests/parity_util.py against the float64 model, float and int16"""
    import radiodsp_sdr_rx_amd as R
    from parity_util import assert_truth_anchored
    import np_model
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    cfg, chans, nblk, steps = dict(R.K_CONFIGS["K3"]["cfg"]), [741, 680, 42], 512, 8
    iq = np.concatenate([synth_iq(1, nblk * 128, ch0=c) for c in chans])
    ch = Chain(len(chans), max_blocks_per_call=nblk, fir_variant=2, **cfg)
    ch.set_pipelined(True)
    dev = torch.from_numpy(iq).cuda()
    o16 = torch.empty((len(chans), nblk * 32, 2), dtype=torch.int16, device="cuda")
    o32 = torch.empty((len(chans), nblk * 32, 2), dtype=torch.float32, device="cuda")
    for _ in range(steps):
        ch.process(dev, out=o16, out_f32=o32)
    ch.flush()
    torch.cuda.synchronize()
    f64, r16, r32 = [], [], []
    for c in range(len(chans)):
        m, oc = np_model.Model(**cfg), oracle.OracleChain(**cfg)
        for _ in range(steps):
            y, (a, b) = m.process(iq[c]), oc.process(iq[c])
        f64.append(y); r16.append(a); r32.append(b)
    ratio = assert_truth_anchored(o32.cpu().numpy(), np.stack(r32), np.stack(f64), "bench input", o16.cpu().numpy(), np.stack(r16))
    print(f"worst gpu / worst oracle distance from the float64 model: {ratio:.2f}")


@gpu
def test_rotation_fold_pipelined_is_the_unpipelined_result_to_the_bit(fold_iq):
    """with a tail stage behind the front kernel (ALS notch, AGC): the tail of one call overlaps the front of the next"""
    cfg = dict(fft_l=512, demod="USB", als_mode="notch", als_strength=20, agc_mode="medium", output_gain=0.5)
    a = fold_run(fold_iq, GROUP_OF, FOLD_CASES["tuned"], pipelined=True, cfg=cfg)
    b = fold_run(fold_iq, GROUP_OF, FOLD_CASES["tuned"], pipelined=False, cfg=cfg)
    assert np.array_equal(a, b)


# ---- a burst of retunes: both pinned images, the host's wait for an upload two retunes old, both halves of the slot -----------
ROT_NCO = (12000.0, 14600.0, 9300.0)
ROT_OFFSETS = (13150.0, 9300.0, 9300.0, 14600.0, 11250.0, 12000.0, 0.0, 2500.0)   # the third repeats the second: nothing is staged


def rot_burst_run(parts, first, offsets, sync_before_retune=False, want_f32=False):
    """eight calls on three groups (channel % 3); from call `first` on group 1 is retuned before every call.  Outputs per call"""
    from radiodsp_sdr_rx_amd.chain import Chain
    nch = parts[0].shape[0]
    ch = Chain(nch, max_blocks_per_call=parts[0].shape[1] // 128, fir_variant=2, fft_l=512, demod="USB")
    ch.set_groups((np.arange(nch) % 3).astype(np.uint16))
    for g, hz in enumerate(ROT_NCO):
        ch.group_setTuningOffsetHz(g, hz)
    outs = []
    for k, part in enumerate(parts):
        if k >= first and offsets:
            if sync_before_retune:
                torch.cuda.synchronize()
            ch.group_setTuningOffsetHz(1, offsets[k - first])
        o = ch.process(part, want_f32=want_f32)
        outs.append(o[1] if want_f32 else o)
    ch.flush()
    torch.cuda.synchronize()
    return np.stack([o.cpu().numpy() for o in outs])


@gpu
def test_back_to_back_retunes_of_the_rotated_spectra_while_the_device_is_calls_behind():
    """the counterpart of tests/test_groups.py's burst test of the masks, for the other slot: a retune of group 1 before each of five calls, issued
    while the device is still working on earlier calls.  An upload of the rotated spectra is queued behind those calls when
    the next retune but one fills the same pinned image, and must still carry its own spectra.  The reference run
    synchronises before every retune; both must give the same bits."""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    nch, per, calls = 1024, 32, 8
    iq = torch.from_numpy(synth_iq(nch, per * 128)).cuda()       # every call gets the same block of input
    parts, offsets = [iq] * calls, ROT_OFFSETS[:5]
    ref = rot_burst_run(parts, 3, offsets, sync_before_retune=True)
    got = rot_burst_run(parts, 3, offsets)
    assert np.array_equal(got, ref)
    for k in range(3, calls - 1):                                # the retunes do change group 1 from call to call
        assert not np.array_equal(ref[k][1::3], ref[k + 1][1::3]), f"calls {k} and {k + 1}"
    plain = rot_burst_run(parts, 3, ())
    assert np.array_equal(got[:, 0::3], plain[:, 0::3]) and np.array_equal(got[:, 2::3], plain[:, 2::3])
    assert not np.array_equal(got[3:, 1::3], plain[3:, 1::3])


@gpu
def test_a_retune_before_every_call_against_the_oracle(oracle):
    """the same burst on five channels and calls of 8 blocks, a retune before every one of them, by value: one oracle chain
    per channel, the criterion of the fold tests above"""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    nch, per, calls = 5, 8, 8
    iq = synth_iq(nch, calls * per * 128)
    parts = [np.ascontiguousarray(iq[:, k * per * 128:(k + 1) * per * 128]) for k in range(calls)]
    got = rot_burst_run([torch.from_numpy(p).cuda() for p in parts], 0, ROT_OFFSETS, want_f32=True)
    got = np.concatenate(list(got), 1)
    ref = []
    for c in range(nch):
        oc, outs = oracle.OracleChain(fft_l=512, demod="USB", nco_hz=ROT_NCO[c % 3]), []
        for k in range(calls):
            if c % 3 == 1:
                oc.set_nco_hz(ROT_OFFSETS[k])
            outs.append(oc.process(parts[k][c])[1])
        ref.append(np.concatenate(outs))
    ref = np.stack(ref)
    err = [float(np.abs(got[c] - ref[c]).max() / max(np.abs(ref[c]).max(), 1e-30)) for c in range(nch)]
    print("normwise per channel:", ["%.2e" % e for e in err])
    assert normwise(got, ref) <= TOL


# ---- host: a group's slot of the pool against rot_r x G_r in double (no GPU) -------------------------------------------------
def test_rotated_pool_image_on_the_host(rdsp, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pkg = os.path.join(root, "radiodsp_sdr_rx_amd")
    exe = str(tmp_path / "host_rot_pool_check")
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                           "-I", os.path.join(pkg, "csrc"), os.path.join(root, "tests", "host", "host_rot_pool_check.c"), "-o", exe,
                           "-L", pkg, "-lrdsp_hip", "-L", "/opt/rocm/lib", "-lamdhip64", "-lm",
                           "-Wl,-rpath," + pkg, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
