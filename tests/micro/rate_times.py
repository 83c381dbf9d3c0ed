"""What the polyphase pass costs: HIP-event times of rdsp_engine_update_sources at the ENGINE bench shape (4096 receivers x 32
blocks a call), 16 sources, at 160 / 147 (48 kHz), 640 / 147 (192 kHz), 2500 / 441 (250 kHz), 8000 / 147 (2.4 MHz), interleaved
with the decimating pass at the integer neighbours D = Dc and D = Dc - 1 (Dc = ceil(P / Q)): both do 64 Dc fused multiply-adds
per receiver-output.  The share of the fp32 vector peak is what that work comes to if the whole difference to D = 1 is the pass.
usage (GPU box): python tests/micro/rate_times.py [--runs 3] [--calls 200] [--only P/Q | --only D]
For the filter bank alone: rocprofv3 --kernel-trace --stats -- python tests/micro/rate_times.py --only 160/147 --runs 1"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle_lib  # noqa: E402  (the tables only)
from radiodsp_sdr_rx_amd.engine import Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--only", default="")
args = ap.parse_args()

NCH, NBLK, NSRC = 4096, 32, 16
PEAK_FP32 = 157.3e12   # flop/s, vector, the data sheet's
RATES = [(160, 147), (640, 147), (2500, 441), (8000, 147)]


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


def engine(P, Q):
    e = Engine(NCH, max_blocks_per_call=NBLK, tables=oracle_lib.engine_tables())
    e.sketch_setup()
    e.set_sources(NSRC, np.arange(NCH) % NSRC)
    e.set_source_rate(P, Q, 4.0)
    lim = 22050.0 * P / Q
    e.tune(0, np.random.default_rng(5).uniform(-lim + 1, lim - 1, NCH))
    return e


def measure(P, Q):
    """ms per call of update_sources on rows long enough for any call (the pairs vary by one between calls)"""
    e = engine(P, Q)
    n = NBLK * 128 * P // Q + 4
    src = torch.randint(-3000, 3000, (NSRC, n, 2), dtype=torch.int16, device="cuda", generator=g)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call():
        rc = e.lib.rdsp_engine_update_sources(e.h, src.data_ptr(), n, NBLK, out.data_ptr(), NBLK * 128, stream)
        assert rc == 0, rc
    ms = timed(call, args.calls)
    e.close()
    return ms


g = torch.Generator(device="cuda").manual_seed(1)
out = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda")
if args.only:
    only = tuple(int(v) for v in args.only.split("/"))
    plan = [[only if len(only) == 2 else (only[0], 1)]]
else:
    plan = [[(-(-P // Q) - 1, 1), (P, Q), (-(-P // Q), 1)] for P, Q in RATES]   # each rate between its integer neighbours
for run in range(args.runs):
    base = measure(1, 1) if not args.only else None
    if base is not None:
        print(f"run {run}: update_sources 1 / 1 (the tuning pass)   {base:7.3f} ms per call", flush=True)
    for group in plan:
        for P, Q in group:
            ms = measure(P, Q)
            note = ""
            if base is not None:
                flop = 2.0 * 64 * (-(-P // Q)) * NCH * NBLK * 128
                note = f"  pass <= {ms - base:6.3f} ms = {flop / ((ms - base) * 1e-3) / PEAK_FP32 * 100:5.1f} % of the fp32 vector peak"
            print(f"run {run}: update_sources {P:5d} / {Q:3d} (Dc = {-(-P // Q):2d})      {ms:7.3f} ms per call{note}", flush=True)
