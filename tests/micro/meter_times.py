"""What the signal meter costs at the ENGINE bench shape (4096 receivers x 32 blocks a call, sketch set-up, the synthetic
generator's IQ): HIP-event times of rdsp_engine_update over --calls calls, --runs runs, the variants interleaved in one
session:
  parent    another build of the library (--parent-lib PATH: the commit before the meter), if given
  never     this build, rdsp_engine_enable_meter never called
  meter     this build, the meter on, the squelch off
  squelch   this build, the meter on, the squelch closing half the receivers (every odd row is all zero)
  parent2, never2   with --control: a second object of the same build and settings, created last -- what two objects of ONE
            build differ by in one session (where their buffers landed), to read the difference between the builds against
The order of the variants rotates from run to run.  Prints ms per call for every run and variant, then min / median / max
per variant.
usage (GPU box): python tests/micro/meter_times.py [--parent-lib PATH] [--calls 200] [--runs 3] [--control]"""
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
ap.add_argument("--control", action="store_true")
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


def engine(lib, meter, squelch):
    h = C.c_void_p()
    assert lib.rdsp_engine_create(NCH, 0, NBLK, C.byref(h)) == 0
    bq, hil = oracle_lib.engine_tables()
    assert lib.rdsp_engine_load_tables(h, bq.ctypes.data_as(F32P), hil.ctypes.data_as(F32P)) == 0
    lib.rdsp_engine_enableAGC(h); lib.rdsp_engine_setAGCmode(h, 2); lib.rdsp_engine_disableALSfilter(h); lib.rdsp_engine_disableNoiseBlanker(h)
    lib.rdsp_engine_setInputGain(h, 1.0); lib.rdsp_engine_setOutputGain(h, 0.5); lib.rdsp_engine_setIQgainBalance(h, 1.02)
    lib.rdsp_engine_enableAudioFilter(h); lib.rdsp_engine_setAudioFilter(h, 6); lib.rdsp_engine_setDemodMode(h, 0)
    if meter:
        assert lib.rdsp_engine_enable_meter(h) == 0
    if squelch:
        assert lib.rdsp_engine_set_squelch(h, 1e-7, 1e-7, 2) == 0
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
host = synth_iq(NCH, NBLK * 128, n_threads=8)
full = torch.from_numpy(host).cuda()
half = full.clone()
half[1::2] = 0
out = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda")
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
variants = []
if args.parent_lib:
    variants.append(("parent", bind(os.path.abspath(args.parent_lib)), False, False, full))
variants += [("never", this, False, False, full), ("meter", this, True, False, full), ("squelch", this, True, True, half)]
if args.control:
    variants += [(n + "2", lib, False, False, d) for n, lib, _, _, d in variants if n in ("parent", "never")]
calls, handles = {}, {}
for name, lib, meter, squelch, d in variants:
    h = engine(lib, meter, squelch)

    def call(lib=lib, h=h, d=d):
        rc = lib.rdsp_engine_update(h, d.data_ptr(), NBLK * 128, NBLK, out.data_ptr(), NBLK * 128, stream)
        assert rc == 0, rc
    calls[name], handles[name] = call, h
times = {name: [] for name in calls}
order = list(calls)
for run in range(args.runs):
    for name in order[run % len(order):] + order[:run % len(order)]:   # the order rotates: no variant always runs first
        times[name].append(timed(calls[name], args.calls))
        print(f"run {run}  {name:8s} {times[name][-1]:8.4f} ms per call", flush=True)
cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
for name in ("meter", "squelch"):
    assert this.rdsp_engine_active(handles[name], None, cnt.data_ptr(), stream) == 0
    print(f"{name:8s} receivers open in the last call: {int(cnt.item())} of {NCH}")
for name, lib, meter, squelch, d in variants:
    t = times[name]
    print(f"{name:8s} min {min(t):.4f}  median {statistics.median(t):.4f}  max {max(t):.4f} ms per call of {NCH} x {NBLK} blocks")
if "parent" in times:
    lo, hi = min(times["parent"]), max(times["parent"])
    inside = all(lo <= t <= hi for t in times["never"])
    print(f"never enabled inside the parent's spread [{lo:.4f}, {hi:.4f}]: {inside} (median {statistics.median(times['never']):.4f})")
