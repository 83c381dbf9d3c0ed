"""The NCO behind the frequency-domain decimator (rdsp_front_fd.hip, template SHF; rdsp_fd_shift_image, rdsp_design.c).

Chains of at most RDSP_FD_ROT_GROUPS groups whose filter runs on a one-wave plan (FFT_L 256, 512, 1024) transform the
converted raw samples, read the branch spectra of the frequency-shifted taps from the group's slot of the pool and multiply
the decimated samples by gain x exp(-j phi) on their way into the ring.  What can go wrong there and nowhere else: the
sign and the origin of the shift, the history column of the first frame behind a retune (it came in under the old
increment and takes the per-sample phasor of the difference), the gain rule (one common gain of the window on the output
phasor, anything else per sample), the slot's switch-over, and the host image.

Shapes: the fold tests of tests/test_k3_diet.py -- five channels in three groups, calls of 8 and 16 input blocks (one and
two call units; 16 and 32 at FFT_L 1024) -- whose runners this file uses.  Criterion: tests/parity_util.py, 1e-5 normwise
per channel against one oracle chain per channel (feed-forward chains), the truth-anchored rule where an NLMS follows."""
import os
import subprocess

import numpy as np
import pytest
import torch

import test_k3_diet as k3
from cases import TOL
from parity_util import normwise

gpu = pytest.mark.gpu

GROUP_OF = k3.GROUP_OF
TUNED = k3.FOLD_CASES["tuned"]
PLANS = [(256, (8, 16)), (512, (8, 16)), (1024, (16, 32))]      # the one-wave plans; calls of one and two call units
FORMS = [2, 4]                                                   # 448-sample frames (bench.py); one granule per frame (VC 4)


@pytest.fixture(scope="module")
def streams(rdsp):
    """one input per call pattern, shared by every test of this file"""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    return {calls: synth_iq(len(GROUP_OF), sum(calls) * 128) for _, calls in PLANS}


def _cfg(fft_l):
    return dict(fft_l=fft_l, demod="USB")


# ---- 1. tuned groups, and 2. a retune between two calls -------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fir_variant", FORMS)
@pytest.mark.parametrize("fft_l,calls", PLANS)
def test_tuned_groups_against_the_oracle(oracle, streams, fft_l, calls, fir_variant):
    iq = streams[calls]
    got = k3.fold_run(iq, GROUP_OF, TUNED, retune=False, fir_variant=fir_variant, cfg=_cfg(fft_l), calls=calls)
    ref = k3.fold_oracle(oracle, iq, GROUP_OF, dict(TUNED, retune=(99, 0.0)), cfg=_cfg(fft_l), calls=calls)
    err = normwise(got, ref)
    print(f"FFT_L {fft_l} form {fir_variant}: {err:.2e} normwise")
    assert err <= TOL


@gpu
@pytest.mark.parametrize("fir_variant", FORMS)
@pytest.mark.parametrize("fft_l,calls", PLANS)
def test_a_tuning_offset_change_between_two_calls(oracle, streams, fft_l, calls, fir_variant):
    """the second call's first frame has the old increment's samples in column 0; groups 0 and 2 keep their bits"""
    iq = streams[calls]
    got = k3.fold_run(iq, GROUP_OF, TUNED, fir_variant=fir_variant, cfg=_cfg(fft_l), calls=calls)
    ref = k3.fold_oracle(oracle, iq, GROUP_OF, TUNED, cfg=_cfg(fft_l), calls=calls)
    err = normwise(got, ref)
    print(f"FFT_L {fft_l} form {fir_variant}: {err:.2e} normwise")
    assert err <= TOL
    plain = k3.fold_run(iq, GROUP_OF, TUNED, retune=False, fir_variant=fir_variant, cfg=_cfg(fft_l), calls=calls)
    for c, g in enumerate(GROUP_OF):
        assert np.array_equal(got[c], plain[c]) == (g != TUNED["retune"][0]), f"channel {c} of group {g}"


@gpu
@pytest.mark.parametrize("name", ["nco_off", "from_off"])
def test_a_tuning_offset_change_from_and_to_no_offset(oracle, streams, name):
    """dphi = 0 on either side of the change: the output phasor is 1, the history came in unmixed"""
    case, iq = k3.FOLD_CASES[name], streams[(8, 16)]
    for fir_variant in FORMS:
        assert normwise(k3.fold_run(iq, GROUP_OF, case, fir_variant=fir_variant), k3.fold_oracle(oracle, iq, GROUP_OF, case)) <= TOL


def burst_run(parts, offsets, fir_variant, sync_before_retune=False, first=0, pipelined=None):
    """three groups (channel % 3); from call `first` on group 1 is retuned before every call.  float32 outputs per call"""
    from radiodsp_sdr_rx_amd.chain import Chain
    nch = parts[0].shape[0]
    ch = Chain(nch, max_blocks_per_call=parts[0].shape[1] // 128, fir_variant=fir_variant, fft_l=512, demod="USB")
    ch.set_groups((np.arange(nch) % 3).astype(np.uint16))
    for g, hz in enumerate(k3.ROT_NCO):
        ch.group_setTuningOffsetHz(g, hz)
    if pipelined is not None:
        ch.set_pipelined(pipelined)
    outs = []
    for k, part in enumerate(parts):
        if k >= first:
            if sync_before_retune:
                torch.cuda.synchronize()
            ch.group_setTuningOffsetHz(1, offsets[k - first])
        outs.append(ch.process(part, want_f32=True)[1])
    ch.flush()
    torch.cuda.synchronize()
    return np.stack([o.cpu().numpy() for o in outs])


@gpu
@pytest.mark.parametrize("fir_variant", FORMS)
def test_a_tuning_offset_change_before_every_one_of_eight_calls(oracle, fir_variant):
    """every call's first frame is one behind a retune (the third offset repeats the second: none there), by value.
    (With the difference phasor of the history column left out -- x = raw samples in that frame too -- this test and the
    two-call ones above fail, all but the 0 -> 0 case: 0.95 to 1.55 normwise, measured on that mutation of the kernel.)"""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    nch, per, calls = 5, 8, 8
    iq = synth_iq(nch, calls * per * 128)
    parts = [np.ascontiguousarray(iq[:, k * per * 128:(k + 1) * per * 128]) for k in range(calls)]
    got = np.concatenate(list(burst_run([torch.from_numpy(p).cuda() for p in parts], k3.ROT_OFFSETS, fir_variant)), 1)
    ref = []
    for c in range(nch):
        oc, outs = oracle.OracleChain(fft_l=512, demod="USB", nco_hz=k3.ROT_NCO[c % 3]), []
        for k in range(calls):
            if c % 3 == 1:
                oc.set_nco_hz(k3.ROT_OFFSETS[k])
            outs.append(oc.process(parts[k][c])[1])
        ref.append(np.concatenate(outs))
    err = [float(np.abs(got[c] - ref[c]).max() / max(np.abs(ref[c]).max(), 1e-30)) for c in range(nch)]
    print("normwise per channel:", ["%.2e" % e for e in err])
    assert max(err) <= TOL


# ---- 3. the gain rule: a gain, a balance and a swap change between two calls ------------------------------------------------
SETTINGS = {
    "gain": dict(input_gain=0.37),            # one common gain before, another after: the history column is scaled per sample
    "balance": dict(iq_balance=1.07),         # two gains from here on: every sample is scaled, the phasor carries none
    "swap": dict(swap_iq=True),
    "all": dict(input_gain=2.5, iq_balance=0.93, swap_iq=True),
}


def settings_run(iq, calls, change, fir_variant, at=1):
    """three calls on the tuned groups; `change` is applied before call `at` (0: before the first, i.e. throughout)"""
    from radiodsp_sdr_rx_amd.chain import Chain
    ch = Chain(len(GROUP_OF), max_blocks_per_call=max(calls), fir_variant=fir_variant, fft_l=512, demod="USB")
    ch.set_groups(np.asarray(GROUP_OF, np.uint16))
    for g, hz in enumerate(TUNED["nco"]):
        ch.group_setTuningOffsetHz(g, hz)
    dev, outs, pos = torch.from_numpy(iq).cuda(), [], 0
    for k, nb in enumerate(calls):
        if k == at:
            if "input_gain" in change:
                ch.setInputGain(change["input_gain"])
            if "iq_balance" in change:
                ch.setIQgainBalance(change["iq_balance"])
            if "swap_iq" in change:
                ch.swapIQ(True)
        outs.append(ch.process(dev[:, pos:pos + nb * 128].contiguous(), want_f32=True)[1])
        pos += nb * 128
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in outs]


def settings_oracle(oracle, iq, calls, change, at=1):
    outs = []
    for c, g in enumerate(GROUP_OF):
        oc, o, pos = oracle.OracleChain(fft_l=512, demod="USB", nco_hz=TUNED["nco"][g]), [], 0
        for k, nb in enumerate(calls):
            if k == at:
                oc.set_gains(change.get("input_gain", 1.0), change.get("iq_balance", 1.0), 1.0)
                if "swap_iq" in change:
                    oc.set_swap_iq(True)
            o.append(oc.process(iq[c, pos:pos + nb * 128])[1])
            pos += nb * 128
        outs.append(np.concatenate(o))
    return np.stack(outs)


@gpu
@pytest.mark.parametrize("fir_variant", FORMS)
@pytest.mark.parametrize("name", list(SETTINGS))
def test_a_gain_and_a_swap_change_between_two_calls(oracle, name, fir_variant):
    """the call behind the change runs the PRE instance (its history came in under other settings), the one after it the
    instance the settings themselves ask for"""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    calls = (8, 8, 16)
    iq = synth_iq(len(GROUP_OF), sum(calls) * 128)
    got = settings_run(iq, calls, SETTINGS[name], fir_variant)
    ref = settings_oracle(oracle, iq, calls, SETTINGS[name])
    err = normwise(np.concatenate(got, 1), ref)
    print(f"{name}, form {fir_variant}: {err:.2e} normwise")
    assert err <= TOL
    if name == "gain":
        # From where the decimator's window holds the one new gain -- every frame behind the second call's first -- the gain
        # rides on the output phasor in the PRE kernel as in the other, so the samples round as in a chain that ran with
        # this gain, and without PRE, from the start.  The second call (256 outputs) is one frame with the old gain in its
        # history column: scaled per sample.  The third call's first overlap-save hop (256 outputs) still filters that
        # frame's samples; behind it the bits are the other chain's.
        always = settings_run(iq, calls, SETTINGS[name], fir_variant, at=0)
        assert np.array_equal(got[2][:, 256:], always[2][:, 256:])
        assert not np.array_equal(got[1], always[1])          # ... and the second call did differ


# ---- 4. pipelined / un-pipelined, queued / synchronised retunes: to the bit -------------------------------------------------
@gpu
@pytest.mark.parametrize("fft_l,calls", [(512, (8, 16)), (1024, (16, 32))])
def test_pipelined_is_the_unpipelined_result_to_the_bit(streams, fft_l, calls):
    """the default form with a tail stage behind it (ALS notch, AGC): the tail of one call overlaps the front of the next,
    the retune's upload is queued behind the first call"""
    cfg = dict(fft_l=fft_l, demod="USB", als_mode="notch", als_strength=20, agc_mode="medium", output_gain=0.5)
    a = k3.fold_run(streams[calls], GROUP_OF, TUNED, pipelined=True, cfg=cfg, calls=calls, fir_variant=4)
    b = k3.fold_run(streams[calls], GROUP_OF, TUNED, pipelined=False, cfg=cfg, calls=calls, fir_variant=4)
    assert np.array_equal(a, b)


@gpu
def test_back_to_back_retunes_are_the_synchronised_ones_to_the_bit():
    """five retunes of group 1 while the device is calls behind: each upload carries its own spectra although the pinned
    images are reused (tests/test_k3_diet.py has this for 448-sample frames; here the default form)"""
    from radiodsp_sdr_rx_amd.chain import synth_iq
    nch, per, calls = 768, 16, 8
    iq = torch.from_numpy(synth_iq(nch, per * 128)).cuda()
    parts, offsets = [iq] * calls, k3.ROT_OFFSETS[:5]
    ref = burst_run(parts, offsets, 4, sync_before_retune=True, first=3)
    got = burst_run(parts, offsets, 4, first=3)
    assert np.array_equal(got, ref)
    for k in range(3, calls - 1):
        assert not np.array_equal(ref[k][1::3], ref[k + 1][1::3]), f"calls {k} and {k + 1}"


# ---- 5. the default form: the same bits for any split of the stream ---------------------------------------------------------
@gpu
def test_default_form_gives_the_same_bits_for_three_splits(streams):
    from radiodsp_sdr_rx_amd.chain import Chain
    iq = streams[(16, 32)]                                   # 48 blocks
    dev = torch.from_numpy(iq).cuda()

    def run(calls):
        ch = Chain(len(GROUP_OF), max_blocks_per_call=max(calls), fir_variant=4, fft_l=512, demod="USB")
        ch.set_groups(np.asarray(GROUP_OF, np.uint16))
        for g, hz in enumerate(TUNED["nco"]):
            ch.group_setTuningOffsetHz(g, hz)
        outs, pos = [], 0
        for nb in calls:
            outs.append(ch.process(dev[:, pos:pos + nb * 128].contiguous(), want_f32=True)[1])
            pos += nb * 128
        torch.cuda.synchronize()
        return torch.cat(outs, 1).cpu().numpy()

    a, b, c = run((48,)), run((8, 16, 24)), run((8, 8, 8, 8, 8, 8))
    assert np.array_equal(a, b) and np.array_equal(a, c)


# ---- 6. state saved and loaded mid-stream -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("fir_variant", FORMS)
def test_saved_and_loaded_state_continues_to_the_bit(streams, fir_variant):
    """a fresh chain with the blob of the first call continues as the uninterrupted run does, a retune of group 1 right
    behind the load included (the blob carries the increment the history came in with); its pool is made anew at its first
    commit -- the blob holds none"""
    from radiodsp_sdr_rx_amd.chain import Chain
    calls = (8, 16)
    iq = streams[calls]
    whole = k3.fold_run(iq, GROUP_OF, TUNED, fir_variant=fir_variant, calls=calls)

    def chain():
        ch = Chain(len(GROUP_OF), max_blocks_per_call=max(calls), fir_variant=fir_variant, fft_l=512, demod="USB")
        ch.set_groups(np.asarray(GROUP_OF, np.uint16))
        for g, hz in enumerate(TUNED["nco"]):
            ch.group_setTuningOffsetHz(g, hz)
        return ch

    dev = torch.from_numpy(iq).cuda()
    first = chain()
    a = first.process(dev[:, :calls[0] * 128].contiguous(), want_f32=True)[1].cpu().numpy()
    blob = first.save_state()
    second = chain()
    second.load_state(blob)
    second.group_setTuningOffsetHz(*TUNED["retune"])
    b = second.process(dev[:, calls[0] * 128:].contiguous(), want_f32=True)[1]
    torch.cuda.synchronize()
    assert np.array_equal(np.concatenate([a, b.cpu().numpy()], 1), whole)


# ---- 7. the bench's sensitive channels, the default form --------------------------------------------------------------------
@gpu
def test_bench_inputs_of_the_sensitive_channels_through_the_default_form(oracle):
    """the inputs of tests/test_k3_diet.py's test_bench_input_of_a_sensitive_channel_is_truth_anchored (bench.py's K3
    channels 741, 680, 42; eight pipelined steps of 512 blocks).  That test runs them through the 448-sample frames, the
    instance bench.py times; this one through the one-granule frames, under the same rule"""
    import radiodsp_sdr_rx_amd as R
    from parity_util import assert_truth_anchored
    import np_model
    from radiodsp_sdr_rx_amd.chain import Chain, synth_iq
    cfg, chans, nblk, steps = dict(R.K_CONFIGS["K3"]["cfg"]), [741, 680, 42], 512, 8
    iq = np.concatenate([synth_iq(1, nblk * 128, ch0=c) for c in chans])
    ch = Chain(len(chans), max_blocks_per_call=nblk, fir_variant=4, **cfg)
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
    ratio = assert_truth_anchored(o32.cpu().numpy(), np.stack(r32), np.stack(f64), "bench input, default form", o16.cpu().numpy(), np.stack(r16))
    print(f"worst gpu / worst oracle distance from the float64 model: {ratio:.2f}")


# ---- 8. host: the shifted image against the direct sum in long double (no GPU) ----------------------------------------------
SHIFT_IMAGE_ULPS = 0.5   # measured: 0.500 float ulps of the branch's peak component (one rounding of a double result)


def test_shifted_image_on_the_host(tmp_path):
    """tests/host/host_shift_image_check.c with csrc/rdsp_design.c, a program of its own under ASan + UBSan: seven
    increments (0, two tuning offsets, 1, 2^31 - 1, 2^32 - 1, 0xC0000001), every branch and bin against the sum over the 65
    taps in long double.  Worst error measured: 0.500 float ulps of the branch's peak component; bound: that plus one ulp."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "radiodsp_sdr_rx_amd", "csrc")
    exe = str(tmp_path / "host_shift_image_check")
    subprocess.check_call(["gcc", "-std=c11", "-D_GNU_SOURCE", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(root, "include"), "-I", csrc,
                           os.path.join(root, "tests", "host", "host_shift_image_check.c"), os.path.join(csrc, "rdsp_design.c"),
                           "-o", exe, "-lm"])
    out = subprocess.run([exe, str(SHIFT_IMAGE_ULPS + 1.0)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.startswith("OK"), out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr
