"""What a source sample format costs: HIP-event times of rdsp_engine_update_source_samples at the ENGINE bench shape (4096
receivers x 32 blocks a call, 16 sources) at D = 1, 160 / 147, D = 16 and 8000 / 147, under int16, uint8, int8 and float32 rows.
usage (GPU box): python tests/micro/format_times.py [--calls 200] [--formats s16,u8,s8,f32] [--tree DIR] [--tag NAME]
--tree DIR measures the package of another checkout (the parent commit, built, which knows int16 only: --formats s16);
tests/micro/format_times.sh interleaves the two builds, three runs, every process under a time limit of its own."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--formats", default="s16,u8,s8,f32")
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(HERE)))
ap.add_argument("--tag", default="this build")
args = ap.parse_args()
sys.path[:0] = [os.path.abspath(args.tree), os.path.join(os.path.dirname(os.path.dirname(HERE)), "tests")]
import oracle_lib  # noqa: E402  (the tables only)
from radiodsp_sdr_rx_amd.engine import Engine  # noqa: E402

NCH, NBLK, NSRC = 4096, 32, 16
RATES = [(1, 1), (160, 147), (16, 1), (8000, 147)]
FORMATS = {"s16": (0, torch.int16), "u8": (1, torch.uint8), "s8": (2, torch.int8), "f32": (3, torch.float32)}


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
    """ms per call on rows long enough for any call (the pairs vary by one between calls), 16-byte aligned and apart"""
    fmt, dtype = FORMATS[name]
    e = Engine(NCH, max_blocks_per_call=NBLK, tables=oracle_lib.engine_tables())
    e.sketch_setup()
    e.set_sources(NSRC, np.arange(NCH) % NSRC)
    if (P, Q) != (1, 1):
        e.set_source_rate(P, Q, 4.0)
    if fmt:
        e.set_source_format(fmt)
    lim = 22050.0 * P / Q
    e.tune(0, np.random.default_rng(5).uniform(-lim + 1, lim - 1, NCH))
    n = (NBLK * 128 * P // Q + 4 + 7) // 8 * 8
    g = torch.Generator(device="cuda").manual_seed(1)
    if name == "f32":
        src = (torch.rand((NSRC, n, 2), device="cuda", generator=g) - 0.5) * 0.18
    elif name == "s16":
        src = torch.randint(-3000, 3000, (NSRC, n, 2), dtype=torch.int16, device="cuda", generator=g)
    else:
        src = torch.randint(116, 140, (NSRC, n, 2), device="cuda", generator=g).to(torch.uint8)
        src = src if name == "u8" else (src.to(torch.int16) - 128).to(torch.int8)
    assert src.dtype == dtype
    out = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    entry = e.lib.rdsp_engine_update_source_samples if fmt else e.lib.rdsp_engine_update_sources

    def call():
        rc = entry(e.h, src.data_ptr(), n, NBLK, out.data_ptr(), NBLK * 128, stream)
        assert rc == 0, rc
    ms = timed(call, args.calls)
    e.close()
    return ms


for P, Q in RATES:
    for name in args.formats.split(","):
        print(f"{args.tag}: {P:5d} / {Q:3d}  {name:>3}  {measure(P, Q, name):7.3f} ms per call", flush=True)
