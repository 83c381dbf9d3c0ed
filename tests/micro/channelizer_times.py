"""What two stages cost against one: HIP-event times at the ENGINE bench shape (4096 receivers x 32 blocks a call, 16 sources) of
  one     rdsp_engine_update_source_samples on the wide rows (the one-stage filter bank, the baseline)
  chan    rdsp_channelizer_update alone (the sub-band rows of all sources)
  two     rdsp_channelizer_update, then rdsp_engine_update_source_samples on the sub-band rows at D2 (RDSP_SRC_F32)
for 8000 / 147 (M = 32, D2 = 5 and M = 64, D2 = 3), 20480 / 441 (M = 32, D2 = 4) and 640 / 147 (M = 8, D2 = 2), on uint8 and int16
rows, the stations drawn uniformly over the band.  The legs of a configuration are interleaved in one session and their order
rotates from run to run.
usage (GPU box): python tests/micro/channelizer_times.py [--runs 3] [--calls 200] [--only P/Q/M/D2] [--legs one,chan,two]
For the kernels alone: rocprofv3 --kernel-trace --stats -- python tests/micro/channelizer_times.py --only 8000/147/32/5 --runs 1"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import oracle_lib  # noqa: E402  (the tables only)
from radiodsp_sdr_rx_amd.channelizer import Channelizer, rate  # noqa: E402
from radiodsp_sdr_rx_amd.engine import SRC_F32, SRC_S16, SRC_U8, Engine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--only", default="")
ap.add_argument("--legs", default="one,chan,two")
args = ap.parse_args()

NCH, NBLK, NSRC = 4096, 32, 16
PEAK_FP32 = 157.3e12   # flop/s, vector, the data sheet's
CONFIGS = [(8000, 147, 32, 5), (8000, 147, 64, 3), (20480, 441, 32, 4), (640, 147, 8, 2)]
TORCH = {SRC_S16: torch.int16, SRC_U8: torch.uint8}


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


class Legs:
    def __init__(self, P, Q, M, D2, fmt):
        self.stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        lim = 22050.0 * P / Q
        stations = np.random.default_rng(5).uniform(-lim + 1, lim - 1, NCH)
        src_of = np.arange(NCH) % NSRC
        self.n = NBLK * 128 * P // Q + 4        # long enough for any call (the pairs vary by one between calls)
        lo, hi = (0, 256) if fmt == SRC_U8 else (-3000, 3000)
        self.src = torch.randint(lo, hi, (NSRC, self.n, 2), dtype=TORCH[fmt], device="cuda", generator=g)
        self.one = Engine(NCH, max_blocks_per_call=NBLK, tables=oracle_lib.engine_tables())
        self.one.sketch_setup()
        self.one.set_sources(NSRC, src_of)
        self.one.set_source_rate(P, Q, 4.0)
        self.one.set_source_format(fmt)
        self.one.tune(0, stations)
        self.ch = Channelizer(NSRC, P, Q, M, D2, fmt=fmt, max_blocks_per_call=NBLK)
        ks, res = self.ch.place(stations)
        self.n_sub = NBLK * 128 * D2
        self.sub = torch.zeros((NSRC * M, self.n_sub, 2), dtype=torch.float32, device="cuda")
        self.two = Engine(NCH, max_blocks_per_call=NBLK, tables=oracle_lib.engine_tables())
        self.two.sketch_setup()
        self.two.set_sources(NSRC * M, src_of * M + ks)
        self.two.set_source_decimation(D2, 4.0)
        self.two.set_source_format(SRC_F32)
        self.two.tune(0, res)

    def leg_one(self):
        assert self.one.lib.rdsp_engine_update_source_samples(self.one.h, self.src.data_ptr(), self.n, NBLK, out.data_ptr(), NBLK * 128, self.stream) == 0

    def leg_chan(self):
        assert self.ch.lib.rdsp_channelizer_update(self.ch.h, self.src.data_ptr(), self.n, NBLK, self.sub.data_ptr(), self.n_sub, self.stream) == 0

    def leg_two(self):
        self.leg_chan()
        assert self.two.lib.rdsp_engine_update_source_samples(self.two.h, self.sub.data_ptr(), self.n_sub, NBLK, out.data_ptr(), NBLK * 128, self.stream) == 0

    def close(self):
        for o in (self.one, self.two, self.ch):
            o.close()


g = torch.Generator(device="cuda").manual_seed(1)
out = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda")
configs = [tuple(int(v) for v in args.only.split("/"))] if args.only else CONFIGS
names = args.legs.split(",")
for P, Q, M, D2 in configs:
    P1, Q1 = rate(P, Q, D2)
    Tb = 16 * -(-P1 // Q1)
    flop = (4.0 * Tb + 8.0 * M * M) * NSRC * NBLK * 128 * D2     # the fold's 2 Tb and the DFT's 4 M^2 fmaf an instant
    for fmt, fname in ((SRC_U8, "u8"), (SRC_S16, "s16")):
        legs = Legs(P, Q, M, D2, fmt)
        print(f"{P} / {Q}, M = {M}, D2 = {D2}, {fname}: d_sub {legs.sub.numel() * 4 / 1e6:.1f} MB, channelizer {flop / 1e9:.2f} Gflop a call", flush=True)
        for run in range(args.runs):
            order = names[run % len(names):] + names[:run % len(names)]
            ms = {name: timed(getattr(legs, "leg_" + name), args.calls) for name in order}
            text = "  ".join(f"{name} {ms[name]:7.3f} ms" for name in names)
            if "chan" in ms:
                text += f"  (chan = {flop / (ms['chan'] * 1e-3) / PEAK_FP32 * 100:4.1f} % of the fp32 vector peak, launches included)"
            print(f"  run {run} (order {' '.join(order)}): {text}", flush=True)
        legs.close()
