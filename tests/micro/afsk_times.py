"""What the AFSK 1200 packet decoder (rdsp_engine_enable_afsk) costs at the ENGINE bench shape (4096 receivers x 32 blocks a call,
sketch set-up): HIP-event times over --calls calls, --runs runs, every leg interleaved in one session, the order rotating from
run to run.  Legs, all rdsp_engine_update alone (what bench.py --config ENGINE runs):
  parent       another build of the library (--parent-lib PATH: the commit before the decoder), if given
  never        this build, rdsp_engine_enable_afsk never called
  afsk_idle    this build, rdsp_engine_enable_fm and rdsp_engine_enable_afsk called, the decoder on nowhere, no group in NFM
  nfm_meter    every receiver in NFM with the meter and a carrier squelch, the decoder never enabled: the comparison for the next
  nfm_packet   the same with the decoder on, every receiver fed a station that sends packets without a pause: eight consecutive
               calls' worth of its stream, cycled (a frame of 40 bytes spans three calls)
  nfm_noise    the same, every receiver fed noise without a carrier: an idle discriminator, the worst case for the bit machine
The first three run on the synthetic generator's IQ, the NFM legs on the packet station (nfm_noise on the noise).
Prints ms per call for every run, then min / median / max per leg.
--only LEG runs one leg alone (for a kernel trace in a run of its own).
usage (GPU box): python tests/micro/afsk_times.py [--parent-lib PATH] [--calls 200] [--runs 3] [--only nfm_packet]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--only", default=None)
args = ap.parse_args()
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import engine_afsk_model as A  # noqa: E402  (the test signal only)
import oracle_lib  # noqa: E402  (the tables only)
from radiodsp_sdr_rx_amd import _lib  # noqa: E402
from radiodsp_sdr_rx_amd.chain import synth_iq  # noqa: E402

NCH, NBLK = 4096, 32
F32P = C.POINTER(C.c_float)


def bind(path):
    """a build of the library by its path, with the signatures of the entry points it has"""
    lib = C.CDLL(path)
    for name, res, argtypes in _lib.SYMBOLS:
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, argtypes
    return lib


def engine(lib, fm=False, afsk=False, on=0, nfm=False, meter=False):
    """sketch set-up; fm / afsk: the enable calls; on: the decoder's switch in every group; nfm: every receiver in mode 7; meter:
    the meter with a squelch at -40 / -46 dB"""
    h = C.c_void_p()
    assert lib.rdsp_engine_create(NCH, 0, NBLK, C.byref(h)) == 0
    bq, hil = oracle_lib.engine_tables()
    assert lib.rdsp_engine_load_tables(h, bq.ctypes.data_as(F32P), hil.ctypes.data_as(F32P)) == 0
    lib.rdsp_engine_enableAGC(h); lib.rdsp_engine_setAGCmode(h, 2); lib.rdsp_engine_disableALSfilter(h); lib.rdsp_engine_disableNoiseBlanker(h)
    lib.rdsp_engine_setInputGain(h, 1.0); lib.rdsp_engine_setOutputGain(h, 0.5); lib.rdsp_engine_setIQgainBalance(h, 1.02)
    lib.rdsp_engine_enableAudioFilter(h); lib.rdsp_engine_setAudioFilter(h, 6); lib.rdsp_engine_setDemodMode(h, 0)
    if meter:
        assert lib.rdsp_engine_enable_meter(h) == 0 and lib.rdsp_engine_set_squelch(h, 5e-5, 1.25e-5, 2) == 0
    if fm:
        assert lib.rdsp_engine_enable_fm(h) == 0
    if afsk:
        assert lib.rdsp_engine_enable_afsk(h) == 0 and lib.rdsp_engine_set_afsk(h, on, 1.0, 2, 17) == 0
    if nfm:
        lib.rdsp_engine_setDemodMode(h, 7)
    return h


def timed(fn, calls):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


PACKET_CALLS = 8


def packet_iq():
    """PACKET_CALLS arrays int16 [NCH, NBLK * 128, 2], consecutive calls of sixteen stations that send frames of 40 drawn bytes
    without a pause, each at a drawn carrier level, cycled over the receivers (behind the last call the stream starts again:
    one frame in eight calls is cut)"""
    r = np.random.default_rng(1)
    t = PACKET_CALLS * NBLK * 128
    rows = []
    for k in range(16):
        bits = []
        while len(bits) * 36.75 < t:
            bits += A.frame_bits(bytes(r.integers(0, 256, 40, dtype=np.uint8)), 2, 1)
        mod = A.audio(A.nrzi(bits), 0.3, phase=r.uniform(0, 6), total=t)
        z = r.uniform(2000, 20000) * np.exp(1j * (2 * np.pi * 5000.0 / 44100.0 * np.cumsum(mod))) + 3.0 * (r.standard_normal(t) + 1j * r.standard_normal(t))
        rows.append(np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16))
    rows = np.stack(rows)
    return [rows[:, k * NBLK * 128:(k + 1) * NBLK * 128][np.arange(NCH) % 16] for k in range(PACKET_CALLS)]


def noise_iq():
    r = np.random.default_rng(2)
    return np.rint(300.0 * r.standard_normal((64, NBLK * 128, 2))).astype(np.int16)[np.arange(NCH) % 64]


this = _lib.load()
inputs = {"synth": [torch.from_numpy(synth_iq(NCH, NBLK * 128, n_threads=8)).cuda()], "packet": [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in packet_iq()],
          "noise": [torch.from_numpy(noise_iq()).cuda()]}
out = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda")
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def updater(lib, h, d_iqs):
    """the calls cycle d_iqs"""
    at = [0]

    def update():
        d_iq = d_iqs[at[0] % len(d_iqs)]
        at[0] += 1
        rc = lib.rdsp_engine_update(h, d_iq.data_ptr(), NBLK * 128, NBLK, out.data_ptr(), NBLK * 128, stream)
        assert rc == 0, rc
    return update


plan = [("never", this, "synth", {}), ("afsk_idle", this, "synth", dict(fm=True, afsk=True)),
        ("nfm_meter", this, "packet", dict(fm=True, nfm=True, meter=True)),
        ("nfm_packet", this, "packet", dict(fm=True, afsk=True, on=1, nfm=True, meter=True)),
        ("nfm_noise", this, "noise", dict(fm=True, afsk=True, on=1, nfm=True, meter=True))]
if args.parent_lib:
    plan.insert(0, ("parent", bind(os.path.abspath(args.parent_lib)), "synth", {}))
legs = {name: updater(lib, engine(lib, **kw), inputs[src]) for name, lib, src, kw in plan if args.only is None or args.only == name}
times = {name: [] for name in legs}
order = list(legs)
for run in range(args.runs):
    for name in order[run % len(order):] + order[:run % len(order)]:   # the order rotates: no leg always runs first
        times[name].append(timed(legs[name], args.calls))
        print(f"run {run}  {name:11s} {times[name][-1]:8.4f} ms per call", flush=True)
for name, t in times.items():
    print(f"{name:11s} min {min(t):.4f}  median {statistics.median(t):.4f}  max {max(t):.4f} ms per call of {NCH} x {NBLK} blocks")
if args.only in ("nfm_packet", "nfm_noise"):
    # a fresh engine: how many frames does the decoder read on this input?
    lib, kw, src = next((lib, kw, src) for n, lib, src, kw in plan if n == args.only)
    e = engine(lib, **kw)
    up = updater(lib, e, inputs[src])
    for _ in range(4 * PACKET_CALLS):
        up()
    count = torch.zeros((NCH,), dtype=torch.int32, device="cuda")
    assert lib.rdsp_engine_read_afsk_frames(e, 0, NCH, count.data_ptr(), None, stream) == 0
    torch.cuda.synchronize()
    print(f"{args.only}: {int(count.sum())} frames read by {NCH} receivers in {4 * PACKET_CALLS} calls")
