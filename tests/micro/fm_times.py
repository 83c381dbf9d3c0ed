"""What narrow-band FM (rdsp_engine_enable_fm) costs at the ENGINE bench shape (4096 receivers x 32 blocks a call, sketch set-up,
the synthetic generator's IQ): HIP-event times over --calls calls, --runs runs, every leg interleaved in one session, the order
rotating from run to run.  Legs, all rdsp_engine_update alone (what bench.py --config ENGINE runs):
  parent    another build of the library (--parent-lib PATH: the commit before the mode), if given
  never     this build, rdsp_engine_enable_fm never called
  fm_idle   this build, rdsp_engine_enable_fm called, no group in NFM
  nfm2/3    every receiver in NFM, W = 2 / 3 (defaults otherwise: deviation 5000 Hz, de-emphasis 750 us)
  nfm2_flat W = 2 without de-emphasis
  am        every receiver in AM, the comparison
Prints ms per call for every run, then min / median / max per leg.
--only LEG runs one leg alone (for a kernel trace in a run of its own).
usage (GPU box): python tests/micro/fm_times.py [--parent-lib PATH] [--calls 200] [--runs 3] [--only nfm2]"""
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


def engine(lib, fm=False, mode=0, W=2, tau=750.0):
    """sketch set-up; fm: rdsp_engine_enable_fm; mode: the demodulator of every receiver"""
    h = C.c_void_p()
    assert lib.rdsp_engine_create(NCH, 0, NBLK, C.byref(h)) == 0
    bq, hil = oracle_lib.engine_tables()
    assert lib.rdsp_engine_load_tables(h, bq.ctypes.data_as(F32P), hil.ctypes.data_as(F32P)) == 0
    lib.rdsp_engine_enableAGC(h); lib.rdsp_engine_setAGCmode(h, 2); lib.rdsp_engine_disableALSfilter(h); lib.rdsp_engine_disableNoiseBlanker(h)
    lib.rdsp_engine_setInputGain(h, 1.0); lib.rdsp_engine_setOutputGain(h, 0.5); lib.rdsp_engine_setIQgainBalance(h, 1.02)
    lib.rdsp_engine_enableAudioFilter(h); lib.rdsp_engine_setAudioFilter(h, 6); lib.rdsp_engine_setDemodMode(h, 0)
    if fm:
        assert lib.rdsp_engine_set_fm(h, W, 5000.0, tau) == 0 and lib.rdsp_engine_enable_fm(h) == 0
    if mode:
        lib.rdsp_engine_setDemodMode(h, mode)
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


plan = [("never", this, {}), ("fm_idle", this, dict(fm=True)), ("nfm2", this, dict(fm=True, mode=7, W=2)), ("nfm3", this, dict(fm=True, mode=7, W=3)),
        ("nfm2_flat", this, dict(fm=True, mode=7, W=2, tau=0.0)), ("am", this, dict(mode=4))]
if args.parent_lib:
    plan.insert(0, ("parent", bind(os.path.abspath(args.parent_lib)), {}))
legs = {name: updater(lib, engine(lib, **kw)) for name, lib, kw in plan if args.only is None or args.only == name}
times = {name: [] for name in legs}
order = list(legs)
for run in range(args.runs):
    for name in order[run % len(order):] + order[:run % len(order)]:   # the order rotates: no leg always runs first
        times[name].append(timed(legs[name], args.calls))
        print(f"run {run}  {name:10s} {times[name][-1]:8.4f} ms per call", flush=True)
for name, t in times.items():
    print(f"{name:10s} min {min(t):.4f}  median {statistics.median(t):.4f}  max {max(t):.4f} ms per call of {NCH} x {NBLK} blocks")
