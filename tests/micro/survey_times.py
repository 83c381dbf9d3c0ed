"""What a band survey costs beside the receivers it serves: HIP-event times of Survey.update alone and of
rdsp_engine_update_source_samples alone at the ENGINE bench shape's sources (16 sources, the pairs of 32 blocks a call, 4096
receivers) at 8000 / 147 and 160 / 147, int16 and uint8 rows, N = 4096, navg = 8.  The two are interleaved in one session,
three runs of --calls calls each; prints ms per call and the ratio.
usage (GPU box): python tests/micro/survey_times.py [--calls 200] [--runs 3]"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle_lib  # noqa: E402  (the tables only)
from radiodsp_sdr_rx_amd.engine import Engine  # noqa: E402
from radiodsp_sdr_rx_amd.survey import Survey  # noqa: E402

NCH, NBLK, NSRC, FFT_N, NAVG = 4096, 32, 16, 4096, 8
RATES = [(8000, 147), (160, 147)]
FORMATS = {"s16": (0, torch.int16), "u8": (1, torch.uint8)}


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


def measure(P, Q, name):
    fmt, dtype = FORMATS[name]
    e = Engine(NCH, max_blocks_per_call=NBLK, tables=oracle_lib.engine_tables())
    e.sketch_setup()
    e.set_sources(NSRC, np.arange(NCH) % NSRC)
    e.set_source_rate(P, Q, 4.0)
    if fmt:
        e.set_source_format(fmt)
    lim = 22050.0 * P / Q
    e.tune(0, np.random.default_rng(5).uniform(-lim + 1, lim - 1, NCH))
    pairs = NBLK * 128 * P // Q
    n = (pairs + 4 + 7) // 8 * 8
    g = torch.Generator(device="cuda").manual_seed(1)
    if name == "s16":
        src = torch.randint(-3000, 3000, (NSRC, n, 2), dtype=torch.int16, device="cuda", generator=g)
    else:
        src = torch.randint(116, 140, (NSRC, n, 2), device="cuda", generator=g).to(torch.uint8)
    assert src.dtype == dtype
    out = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    sv = Survey(NSRC, FFT_N, NAVG, fmt, n)
    rows = torch.empty((NSRC, pairs // (FFT_N // 2) // NAVG + 2, FFT_N), dtype=torch.float32, device="cuda")

    def engine_call():
        rc = e.lib.rdsp_engine_update_source_samples(e.h, src.data_ptr(), n, NBLK, out.data_ptr(), NBLK * 128, stream)
        assert rc == 0, rc

    def survey_call():
        sv.update(src, pairs=pairs, out=rows)

    for run in range(args.runs):
        te = timed(engine_call, args.calls)
        ts = timed(survey_call, args.calls)
        print(f"{P:5d} / {Q:3d}  {name:>3}  run {run}: update_sources {te:7.3f} ms, survey {ts:7.3f} ms per call of {pairs} pairs, "
              f"ratio {ts / te:.3f}", flush=True)
    sv.close()
    e.close()


for P, Q in RATES:
    for name in FORMATS:
        measure(P, Q, name)
