"""What the decimating pass costs: HIP-event times of rdsp_engine_update and rdsp_engine_update_sources at the ENGINE bench
shape (4096 receivers x 32 blocks a call), 16 sources, D = 1, 4, 16, 64, and the share of the fp32 vector peak that
64 D fused multiply-adds per receiver-output come to if the whole difference to D = 1 is the pass.
usage (GPU box): python tests/micro/ddc_times.py [--lib other/librdsp_hip.so] [--runs 3] [--calls 100] [--only D]
A library without rdsp_engine_set_source_decimation (an older build, for a same-box A/B) is timed at D = 1 only.
For the pass alone: rocprofv3 --kernel-trace --stats -- python tests/micro/ddc_times.py --only 16 --runs 1"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle_lib  # noqa: E402  (the tables only)

ap = argparse.ArgumentParser()
ap.add_argument("--lib")
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--only", type=int, default=0)
args = ap.parse_args()
from radiodsp_sdr_rx_amd import _lib  # noqa: E402
if args.lib:   # another build of the library (same-box A/B); an older one lacks the newest entry points
    _lib.use_library(args.lib)
    probe = ctypes.CDLL(os.path.abspath(args.lib))
    _lib.SYMBOLS[:] = [s for s in _lib.SYMBOLS if hasattr(probe, s[0])]
from radiodsp_sdr_rx_amd.engine import Engine  # noqa: E402

NCH, NBLK, NSRC = 4096, 32, 16
PEAK_FP32 = 157.3e12   # flop/s, vector, the data sheet's


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


def engine(D):
    e = Engine(NCH, max_blocks_per_call=NBLK, tables=oracle_lib.engine_tables())
    e.sketch_setup()
    e.set_sources(NSRC, np.arange(NCH) % NSRC)
    if has_ddc:
        e.set_source_decimation(D, 4.0)
    lim = D * 22050.0
    e.tune(0, np.random.default_rng(5).uniform(-lim + 1, lim - 1, NCH))
    return e


def sources(e, src):
    """rdsp_engine_update_sources itself (the wrapper of engine.py asks the library for D, which an older one cannot say)"""
    n = src.shape[1]
    rc = e.lib.rdsp_engine_update_sources(e.h, src.data_ptr(), n, NBLK, out.data_ptr(), NBLK * 128, ctypes_stream())
    assert rc == 0, rc


def ctypes_stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


has_ddc = hasattr(_lib.load(), "rdsp_engine_set_source_decimation") and any(s[0] == "rdsp_engine_set_source_decimation" for s in _lib.SYMBOLS)
g = torch.Generator(device="cuda").manual_seed(1)
out = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda")
rows = torch.randint(-3000, 3000, (NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda", generator=g)
label = args.lib or "this build"
for run in range(args.runs):
    if not args.only:
        e = engine(1)
        print(f"{label} run {run}: update                     {timed(lambda: e.update(rows, out=out), args.calls):7.3f} ms per call", flush=True)
        e.close()
    base = None
    for D in ([args.only] if args.only else [1, 4, 16, 64] if has_ddc else [1]):
        src = torch.randint(-3000, 3000, (NSRC, NBLK * 128 * D, 2), dtype=torch.int16, device="cuda", generator=g)
        e = engine(D)
        ms = timed(lambda: sources(e, src), args.calls)
        note = ""
        if D == 1:
            base = ms
        elif base is not None:
            flop = 2.0 * 64 * D * NCH * NBLK * 128
            note = f"  pass <= {ms - base:6.3f} ms = {flop / ((ms - base) * 1e-3) / PEAK_FP32 * 100:5.1f} % of the fp32 vector peak"
        print(f"{label} run {run}: update_sources D = {D:2d}      {ms:7.3f} ms per call{note}", flush=True)
        e.close()
        del src
