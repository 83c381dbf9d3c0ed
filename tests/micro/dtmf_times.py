"""What the DTMF decoder (rdsp_engine_enable_dtmf) costs at the ENGINE bench shape (4096 receivers x 32 blocks a call, sketch
set-up, the synthetic generator's IQ): HIP-event times over --calls calls, --runs runs, every leg interleaved in one session,
the order rotating from run to run.  Legs, all rdsp_engine_update alone (what bench.py --config ENGINE runs):
  parent       another build of the library (--parent-lib PATH: the commit before the decoder), if given
  never        this build, rdsp_engine_enable_dtmf never called
  dtmf_idle    this build, rdsp_engine_enable_fm and rdsp_engine_enable_dtmf called, K = 0 everywhere, no group in NFM
  nfm_meter    every receiver in NFM with the meter and a carrier squelch, the decoder never enabled: the comparison for the next
  nfm_dtmf     the same with the decoder at K = 4 and the defaults
  nfm_both     the same with the tone search at K = 128 as well (its kernel beside the decoder's in one kernel trace)
Prints ms per call for every run, then min / median / max per leg.
--only LEG runs one leg alone (for a kernel trace in a run of its own).
usage (GPU box): python tests/micro/dtmf_times.py [--parent-lib PATH] [--calls 200] [--runs 3] [--only nfm_dtmf]"""
import argparse
import ctypes as C
import os
import statistics
import sys

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


def engine(lib, fm=False, dtmf=False, K=0, search=False, nfm=False, meter=False):
    """sketch set-up; fm / dtmf / search: the enable calls; K: the decoder's frame length in every group; nfm: every receiver in
    mode 7; meter: the meter with a squelch at -40 / -46 dB"""
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
    if search:
        assert lib.rdsp_engine_enable_tone_search(h) == 0 and lib.rdsp_engine_set_tone_search(h, 128, 0.04, 4.0) == 0
    if dtmf:
        assert lib.rdsp_engine_enable_dtmf(h) == 0 and lib.rdsp_engine_set_dtmf(h, K, 0.015, 4.0, 16.0, 0.5, 2, 2) == 0
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


this = _lib.load()
d_iq = torch.from_numpy(synth_iq(NCH, NBLK * 128, n_threads=8)).cuda()
out = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda")
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)


def updater(lib, h):
    def update():
        rc = lib.rdsp_engine_update(h, d_iq.data_ptr(), NBLK * 128, NBLK, out.data_ptr(), NBLK * 128, stream)
        assert rc == 0, rc
    return update


plan = [("never", this, {}), ("dtmf_idle", this, dict(fm=True, dtmf=True)), ("nfm_meter", this, dict(fm=True, nfm=True, meter=True)),
        ("nfm_dtmf", this, dict(fm=True, dtmf=True, K=4, nfm=True, meter=True)),
        ("nfm_both", this, dict(fm=True, dtmf=True, K=4, search=True, nfm=True, meter=True))]
if args.parent_lib:
    plan.insert(0, ("parent", bind(os.path.abspath(args.parent_lib)), {}))
legs = {name: updater(lib, engine(lib, **kw)) for name, lib, kw in plan if args.only is None or args.only == name}
times = {name: [] for name in legs}
order = list(legs)
for run in range(args.runs):
    for name in order[run % len(order):] + order[:run % len(order)]:   # the order rotates: no leg always runs first
        times[name].append(timed(legs[name], args.calls))
        print(f"run {run}  {name:11s} {times[name][-1]:8.4f} ms per call", flush=True)
for name, t in times.items():
    print(f"{name:11s} min {min(t):.4f}  median {statistics.median(t):.4f}  max {max(t):.4f} ms per call of {NCH} x {NBLK} blocks")
