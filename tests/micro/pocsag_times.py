"""What the POCSAG pager decoder (rdsp_engine_enable_pocsag) costs at the ENGINE bench shape (4096 receivers x 32 blocks a call,
sketch set-up): HIP-event times over --calls calls, --runs runs, every leg interleaved in one session, the order rotating from
run to run.  Legs, all rdsp_engine_update alone (what bench.py --config ENGINE runs):
  parent          another build of the library (--parent-lib PATH: the commit before the decoder), if given
  never           this build, rdsp_engine_enable_pocsag never called
  pocsag_idle     this build, rdsp_engine_enable_fm and rdsp_engine_enable_pocsag called, no group with a baud, no group in NFM
  nfm_off         every receiver in NFM (a paging channel: W = 2, 7500 Hz, no de-emphasis) with the meter and a carrier squelch,
                  the decoder enabled with baud 0: the comparison for the next
  paging_BAUD     the same at 512, 1200 and 2400 baud, every receiver fed a station that sends batches without a pause: eight
                  consecutive calls' worth of its stream, cycled
  noise_BAUD      the same, every receiver fed noise without a carrier: an idle discriminator
  both_1200       paging_1200 with the AFSK 1200 decoder on beside it: for a kernel trace that holds both kernels
The first three run on the synthetic generator's IQ.  Prints ms per call for every run, then min / median / max per leg.
--only LEG runs one leg alone (for a kernel trace in a run of its own).
usage (GPU box): python tests/micro/pocsag_times.py [--parent-lib PATH] [--calls 200] [--runs 3] [--only paging_1200]"""
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
import oracle_lib  # noqa: E402  (the tables only)
from radiodsp_sdr_rx_amd import _lib, pocsag as P  # noqa: E402
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


def engine(lib, fm=False, pocsag=False, baud=0, nfm=False, meter=False, afsk=False):
    """sketch set-up; fm / pocsag / afsk: the enable calls; baud: the decoder's in every group; nfm: every receiver in mode 7 as a
    paging channel; meter: the meter with a squelch at -40 / -46 dB"""
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
        assert lib.rdsp_engine_enable_afsk(h) == 0 and lib.rdsp_engine_set_afsk(h, 1, 1.0, 2, 17) == 0
    if pocsag:
        assert lib.rdsp_engine_enable_pocsag(h) == 0 and lib.rdsp_engine_set_pocsag(h, baud, 2, 3, 2, 1, 2) == 0
    if nfm:
        lib.rdsp_engine_setDemodMode(h, 7)
        assert lib.rdsp_engine_set_fm(h, 2, 7500.0, 0.0) == 0
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


def paging_iq(baud):
    """PACKET_CALLS arrays int16 [NCH, NBLK * 128, 2], consecutive calls of sixteen stations that send batches of drawn
    alphanumeric messages without a pause, each at a drawn carrier level, cycled over the receivers (behind the last call the
    stream starts again)"""
    r = np.random.default_rng(baud)
    t = PACKET_CALLS * NBLK * 128
    rows = []
    for k in range(16):
        msgs = [(int(r.integers(0, 1 << 21)), 3, [int(v) for v in r.integers(0, 1 << 20, int(r.integers(2, 14)))]) for _ in range(40)]
        mod = P.transmit(P.bits(P.batches(msgs), 64), baud, 0.6, ppm=r.uniform(-100, 100), total=t)
        z = r.uniform(2000, 20000) * np.exp(1j * (2 * np.pi * 7500.0 / 44100.0 * np.cumsum(mod))) + 3.0 * (r.standard_normal(t) + 1j * r.standard_normal(t))
        rows.append(np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16))
    rows = np.stack(rows)
    return [rows[:, k * NBLK * 128:(k + 1) * NBLK * 128][np.arange(NCH) % 16] for k in range(PACKET_CALLS)]


def noise_iq():
    r = np.random.default_rng(2)
    return np.rint(300.0 * r.standard_normal((64, NBLK * 128, 2))).astype(np.int16)[np.arange(NCH) % 64]


this = _lib.load()
BAUDS = (512, 1200, 2400)
inputs = {"synth": [torch.from_numpy(synth_iq(NCH, NBLK * 128, n_threads=8)).cuda()], "noise": [torch.from_numpy(noise_iq()).cuda()]}
for baud in BAUDS:
    if args.only is None or args.only.endswith(str(baud)):
        inputs[f"paging_{baud}"] = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in paging_iq(baud)]
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


NFM = dict(fm=True, pocsag=True, nfm=True, meter=True)
plan = [("never", this, "synth", {}), ("pocsag_idle", this, "synth", dict(fm=True, pocsag=True)), ("nfm_off", this, "noise", dict(NFM))]
plan += [(f"paging_{b}", this, f"paging_{b}", dict(NFM, baud=b)) for b in BAUDS] + [(f"noise_{b}", this, "noise", dict(NFM, baud=b)) for b in BAUDS]
plan += [("both_1200", this, "paging_1200", dict(NFM, baud=1200, afsk=True))]
if args.parent_lib:
    plan.insert(0, ("parent", bind(os.path.abspath(args.parent_lib)), "synth", {}))
legs = {name: updater(lib, engine(lib, **kw), inputs[src]) for name, lib, src, kw in plan if (args.only is None and name != "both_1200") or args.only == name}
times = {name: [] for name in legs}
order = list(legs)
for run in range(args.runs):
    for name in order[run % len(order):] + order[:run % len(order)]:   # the order rotates: no leg always runs first
        times[name].append(timed(legs[name], args.calls))
        print(f"run {run}  {name:12s} {times[name][-1]:8.4f} ms per call", flush=True)
for name, t in times.items():
    print(f"{name:12s} min {min(t):.4f}  median {statistics.median(t):.4f}  max {max(t):.4f} ms per call of {NCH} x {NBLK} blocks")
if args.only is not None and args.only != "parent":
    # a fresh engine: how many messages does the decoder read on this input?
    lib, kw, src = next((lib, kw, src) for n, lib, src, kw in plan if n == args.only)
    if kw.get("baud"):
        e = engine(lib, **kw)
        up = updater(lib, e, inputs[src])
        for _ in range(4 * PACKET_CALLS):
            up()
        count = torch.zeros((NCH,), dtype=torch.int32, device="cuda")
        assert lib.rdsp_engine_read_pocsag_messages(e, 0, NCH, count.data_ptr(), None, stream) == 0
        torch.cuda.synchronize()
        print(f"{args.only}: {int(count.sum())} messages closed by {NCH} receivers in {4 * PACKET_CALLS} calls")
