"""What rdsp_engine_pack_active costs and saves at the ENGINE bench shape (4096 receivers x 32 blocks a call, sketch set-up, the
meter on, the synthetic generator's IQ): HIP-event times over --calls calls, --runs runs, every leg of every gate pattern
interleaved in one session, the order rotating from run to run.  Gate patterns, set by receiver groups (squelch off: always
open; set_squelch(1e30, 1e30, 0): never open):
  all        every receiver open
  half       receivers 0 ... 2047 open, the rest never
  one16th    receivers 0 ... 255 open, the rest never
Legs:
  update     rdsp_engine_update alone                                                                       (a)
  pack       update + rdsp_engine_pack_active with capacity = needed                                        (b)
  full_d2h   update + an asynchronous device-to-host copy of the full [4096][32 x 128][2] rows into pinned memory   (c, before)
  pack_d2h   update + pack + device-to-host copies of written x 256 bytes of audio and written x 8 of records      (c, after)
The feature's purpose is pack_d2h against full_d2h; the kernels' cost is pack - update.  Prints ms per call for every run, then
min / median / max per leg, the differences of the medians, and the bytes a call takes off the device either way.
--only PATTERN:LEG runs one leg alone (for a kernel trace in a run of its own).
usage (GPU box): python tests/micro/pack_times.py [--calls 200] [--runs 3] [--only half:pack]"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ap = argparse.ArgumentParser()
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
PATTERNS = {"all": NCH, "half": NCH // 2, "one16th": NCH // 16}   # receivers 0 ... open - 1 are open
LEGS = ("update", "pack", "full_d2h", "pack_d2h")
lib = _lib.load()


def engine(n_open):
    h = C.c_void_p()
    assert lib.rdsp_engine_create(NCH, 0, NBLK, C.byref(h)) == 0
    bq, hil = oracle_lib.engine_tables()
    assert lib.rdsp_engine_load_tables(h, bq.ctypes.data_as(F32P), hil.ctypes.data_as(F32P)) == 0
    lib.rdsp_engine_enableAGC(h); lib.rdsp_engine_setAGCmode(h, 2); lib.rdsp_engine_disableALSfilter(h); lib.rdsp_engine_disableNoiseBlanker(h)
    lib.rdsp_engine_setInputGain(h, 1.0); lib.rdsp_engine_setOutputGain(h, 0.5); lib.rdsp_engine_setIQgainBalance(h, 1.02)
    lib.rdsp_engine_enableAudioFilter(h); lib.rdsp_engine_setAudioFilter(h, 6); lib.rdsp_engine_setDemodMode(h, 0)
    assert lib.rdsp_engine_enable_meter(h) == 0
    if n_open < NCH:
        assert lib.rdsp_engine_set_groups(h, 2, (C.c_int * 2)(0, n_open)) == 0
        assert lib.rdsp_engine_select_group(h, 1) == 0 and lib.rdsp_engine_set_squelch(h, 1e30, 1e30, 0) == 0
        assert lib.rdsp_engine_select_group(h, -1) == 0
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


d_iq = torch.from_numpy(synth_iq(NCH, NBLK * 128, n_threads=8)).cuda()
out = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda")
host_full = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16).pin_memory()
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
legs, moved = {}, {}
if args.only:   # that pattern's engine alone: a kernel trace then holds no other pattern's launches
    PATTERNS = {args.only.split(":")[0]: PATTERNS[args.only.split(":")[0]]}
for pat, n_open in PATTERNS.items():
    h = engine(n_open)

    def update(h=h):
        rc = lib.rdsp_engine_update(h, d_iq.data_ptr(), NBLK * 128, NBLK, out.data_ptr(), NBLK * 128, stream)
        assert rc == 0, rc
    update()
    assert lib.rdsp_engine_pack_active(h, out.data_ptr(), NBLK * 128, NBLK, None, None, 0, cnt.data_ptr(), stream) == 0   # the sizing call
    needed = int(cnt.tolist()[0])
    assert needed == n_open * NBLK, (pat, needed)
    audio = torch.empty((needed, 128), dtype=torch.int16, device="cuda")
    records = torch.empty((needed, 2), dtype=torch.int32, device="cuda")
    host_audio, host_records = torch.empty((needed, 128), dtype=torch.int16).pin_memory(), torch.empty((needed, 2), dtype=torch.int32).pin_memory()

    def pack(h=h, update=update, audio=audio, records=records, needed=needed):
        update()
        rc = lib.rdsp_engine_pack_active(h, out.data_ptr(), NBLK * 128, NBLK, audio.data_ptr(), records.data_ptr(), needed, cnt.data_ptr(), stream)
        assert rc == 0, rc

    def full_d2h(update=update):
        update()
        host_full.copy_(out, non_blocking=True)

    def pack_d2h(pack=pack, audio=audio, records=records, host_audio=host_audio, host_records=host_records):
        pack()
        host_audio.copy_(audio, non_blocking=True)
        host_records.copy_(records, non_blocking=True)
    pack()
    torch.cuda.synchronize()
    assert cnt.tolist() == [needed, needed]
    left = out.view(NCH, NBLK, 128, 2)[:n_open, :, :, 0].reshape(needed, 128)
    assert torch.equal(audio, left) and torch.equal(records[:, 0], torch.arange(needed, device="cuda", dtype=torch.int32) // NBLK)   # what is timed is right
    for name, fn in zip(LEGS, (update, pack, full_d2h, pack_d2h)):
        legs[f"{pat}:{name}"] = fn
    moved[pat] = (needed, out.numel() * 2, needed * (256 + 8))
if args.only:
    legs = {args.only: legs[args.only]}
times = {name: [] for name in legs}
order = list(legs)
for run in range(args.runs):
    for name in order[run % len(order):] + order[:run % len(order)]:   # the order rotates: no leg always runs first
        times[name].append(timed(legs[name], args.calls))
        print(f"run {run}  {name:18s} {times[name][-1]:8.4f} ms per call", flush=True)
for name, t in times.items():
    print(f"{name:18s} min {min(t):.4f}  median {statistics.median(t):.4f}  max {max(t):.4f} ms per call of {NCH} x {NBLK} blocks")
med = {name: statistics.median(t) for name, t in times.items()}
for pat in PATTERNS:
    needed, full_bytes, pack_bytes = moved[pat]
    line = f"{pat:8s} needed {needed} blocks; off the device: {full_bytes} bytes as full rows, {pack_bytes} bytes packed"
    if all(f"{pat}:{leg}" in med for leg in LEGS):
        line += (f"; pack - update {med[pat + ':pack'] - med[pat + ':update']:+.4f} ms; pack_d2h {med[pat + ':pack_d2h']:.4f} against full_d2h "
                 f"{med[pat + ':full_d2h']:.4f} ms ({med[pat + ':full_d2h'] / med[pat + ':pack_d2h']:.2f} x)")
    print(line)
