"""What the voice-rate audio (rdsp_engine_enable_voice) costs and saves at the ENGINE bench shape (4096 receivers x 32 blocks a
call, sketch set-up, the synthetic generator's IQ): HIP-event times over --calls calls, --runs runs, every leg interleaved in one
session, the order rotating from run to run.
Legs without the meter (what bench.py --config ENGINE runs):
  parent       another build of the library (--parent-lib PATH: the commit before the stage), if given: update alone
  never        this build, rdsp_engine_enable_voice never called: update alone
  voice2/4     this build with the stage on at R = 2 / 4: update alone (the stage runs inside it)
Legs with the meter, per gate pattern of pack_times.py (all, half, one16th: receivers 0 ... open - 1 open, the rest never):
  PAT:pack_d2h     update + rdsp_engine_pack_active + device-to-host copies of the packed audio and records (stage off)
  PAT:voiceR_d2h   update + rdsp_engine_pack_voice + the same copies, R = 2 and 4
Prints ms per call for every run, then min / median / max per leg and the bytes a call takes off the device.
--only LEG runs one leg alone (for a kernel trace in a run of its own).
usage (GPU box): python tests/micro/voice_times.py [--parent-lib PATH] [--calls 200] [--runs 3] [--only voice4]"""
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
PATTERNS = {"all": NCH, "half": NCH // 2, "one16th": NCH // 16}


def bind(path):
    """a build of the library by its path, with the signatures of the entry points it has"""
    lib = C.CDLL(path)
    for name, res, argtypes in _lib.SYMBOLS:
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, argtypes
    return lib


def engine(lib, R=0, n_open=None):
    """sketch set-up; R: the stage's rate (0: never enabled); n_open: with the meter, receivers n_open ... never open"""
    h = C.c_void_p()
    assert lib.rdsp_engine_create(NCH, 0, NBLK, C.byref(h)) == 0
    bq, hil = oracle_lib.engine_tables()
    assert lib.rdsp_engine_load_tables(h, bq.ctypes.data_as(F32P), hil.ctypes.data_as(F32P)) == 0
    lib.rdsp_engine_enableAGC(h); lib.rdsp_engine_setAGCmode(h, 2); lib.rdsp_engine_disableALSfilter(h); lib.rdsp_engine_disableNoiseBlanker(h)
    lib.rdsp_engine_setInputGain(h, 1.0); lib.rdsp_engine_setOutputGain(h, 0.5); lib.rdsp_engine_setIQgainBalance(h, 1.02)
    lib.rdsp_engine_enableAudioFilter(h); lib.rdsp_engine_setAudioFilter(h, 6); lib.rdsp_engine_setDemodMode(h, 0)
    if n_open is not None:
        assert lib.rdsp_engine_enable_meter(h) == 0
        if n_open < NCH:
            assert lib.rdsp_engine_set_groups(h, 2, (C.c_int * 2)(0, n_open)) == 0
            assert lib.rdsp_engine_select_group(h, 1) == 0 and lib.rdsp_engine_set_squelch(h, 1e30, 1e30, 0) == 0
            assert lib.rdsp_engine_select_group(h, -1) == 0
    if R:
        assert lib.rdsp_engine_enable_voice(h, R) == 0
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
cnt = torch.zeros(2, dtype=torch.int32, device="cuda")
legs, moved = {}, {}


def wanted(name):
    return args.only is None or args.only == name


def updater(lib, h):
    def update():
        rc = lib.rdsp_engine_update(h, d_iq.data_ptr(), NBLK * 128, NBLK, out.data_ptr(), NBLK * 128, stream)
        assert rc == 0, rc
    return update


plain = [("never", this, 0), ("voice2", this, 2), ("voice4", this, 4)]
if args.parent_lib:
    plain.insert(0, ("parent", bind(os.path.abspath(args.parent_lib)), 0))
for name, lib, R in plain:
    if wanted(name):
        legs[name] = updater(lib, engine(lib, R))
for pat, n_open in PATTERNS.items():
    for R in (0, 2, 4):
        name = f"{pat}:" + (f"voice{R}_d2h" if R else "pack_d2h")
        if not wanted(name):
            continue
        h = engine(this, R, n_open)
        update = updater(this, h)
        update()
        width = 128 // R if R else 128
        needed = n_open * NBLK
        audio = torch.empty((needed, width), dtype=torch.int16, device="cuda")
        records = torch.empty((needed, 2), dtype=torch.int32, device="cuda")
        host_audio, host_records = torch.empty((needed, width), dtype=torch.int16).pin_memory(), torch.empty((needed, 2), dtype=torch.int32).pin_memory()

        def leg(h=h, R=R, update=update, audio=audio, records=records, host_audio=host_audio, host_records=host_records, needed=needed):
            update()
            if R:
                rc = this.rdsp_engine_pack_voice(h, NBLK, audio.data_ptr(), records.data_ptr(), needed, cnt.data_ptr(), stream)
            else:
                rc = this.rdsp_engine_pack_active(h, out.data_ptr(), NBLK * 128, NBLK, audio.data_ptr(), records.data_ptr(), needed, cnt.data_ptr(), stream)
            assert rc == 0, rc
            host_audio.copy_(audio, non_blocking=True)
            host_records.copy_(records, non_blocking=True)
        leg()
        torch.cuda.synchronize()
        assert cnt.tolist() == [needed, needed], (name, cnt.tolist())                       # what is timed is right
        assert torch.equal(records[:, 0], torch.arange(needed, device="cuda", dtype=torch.int32) // NBLK)
        if R:
            rows = torch.empty((NCH, NBLK * width), dtype=torch.int16, device="cuda")
            assert this.rdsp_engine_read_voice(h, NBLK, rows.data_ptr(), NBLK * width, stream) == 0
            assert torch.equal(audio, rows[:n_open].reshape(needed, width))
        legs[name] = leg
        moved[name] = needed * (2 * width + 8)
times = {name: [] for name in legs}
order = list(legs)
for run in range(args.runs):
    for name in order[run % len(order):] + order[:run % len(order)]:   # the order rotates: no leg always runs first
        times[name].append(timed(legs[name], args.calls))
        print(f"run {run}  {name:20s} {times[name][-1]:8.4f} ms per call", flush=True)
for name, t in times.items():
    tail = f"; {moved[name]} bytes off the device" if name in moved else ""
    print(f"{name:20s} min {min(t):.4f}  median {statistics.median(t):.4f}  max {max(t):.4f} ms per call of {NCH} x {NBLK} blocks{tail}")
