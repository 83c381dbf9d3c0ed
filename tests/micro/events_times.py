"""What it costs to learn what the decoders decoded, at the ENGINE bench shape (4096 receivers x 32 blocks a call, sketch set-up,
every receiver in NFM as a paging channel, the DTMF, AFSK 1200 and POCSAG decoders on): WALL time around a host synchronise,
because the copy to the host is the point.  Inputs (pocsag_times.py's paging leg at 2400 baud, afsk_times.py's packet leg, idle
noise), each with these legs, all interleaved in one session, the order rotating from run to run, --runs runs of --calls calls:
  update     rdsp_engine_update and a synchronise: what the others contain
  dense      (a) what a caller does without the gather: update, the three dense read-outs (rdsp_engine_read_dtmf_digits,
             _read_afsk_frames, _read_pocsag_messages), the copy of all counts and rings to pinned host memory, a synchronise
  gather     (b) update, rdsp_engine_gather_events with a fixed capacity (--cap-events, --cap-words), the copy of the five counts
             and a synchronise, then the copy of the written prefix and a synchronise
  sizing     (c) update, the sizing call, the copy of the counts, a synchronise
Also, with HIP-event times as the earlier scripts take them, rdsp_engine_update alone on the synthetic generator's IQ with no
decoder enabled and the gather never called (`never`), against another build of the library (--parent-lib PATH: the commit
before this feature; `parent`).  Prints ms per call for every run, then min / median / max per leg, the bytes a call of (a) and
of (b) moves to the host, and the events a call gathers.
--only INPUT:LEG runs one leg alone (for a kernel trace in a run of its own).
usage (GPU box): python tests/micro/events_times.py [--parent-lib PATH] [--calls 200] [--runs 3] [--only paging:gather]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--cap-events", type=int, default=16384)
ap.add_argument("--cap-words", type=int, default=262144)
ap.add_argument("--only", default=None)
args = ap.parse_args()
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import engine_afsk_model as A  # noqa: E402  (the transmitter only)
import oracle_lib  # noqa: E402  (the tables only)
from radiodsp_sdr_rx_amd import _lib, pocsag as P  # noqa: E402
from radiodsp_sdr_rx_amd.chain import synth_iq  # noqa: E402

NCH, NBLK = 4096, 32
F32P = C.POINTER(C.c_float)
CALLS_OF_INPUT = 8


def bind(path):
    """a build of the library by its path, with the signatures of the entry points it has"""
    lib = C.CDLL(path)
    for name, res, argtypes in _lib.SYMBOLS:
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, argtypes
    return lib


def engine(lib, decoders):
    """sketch set-up; decoders: every receiver in mode 7 as a paging channel with the meter, a carrier squelch and the three
    decoders on (DTMF frames of 4 blocks, AFSK, POCSAG at 2400 baud)"""
    h = C.c_void_p()
    assert lib.rdsp_engine_create(NCH, 0, NBLK, C.byref(h)) == 0
    bq, hil = oracle_lib.engine_tables()
    assert lib.rdsp_engine_load_tables(h, bq.ctypes.data_as(F32P), hil.ctypes.data_as(F32P)) == 0
    lib.rdsp_engine_enableAGC(h); lib.rdsp_engine_setAGCmode(h, 2); lib.rdsp_engine_disableALSfilter(h); lib.rdsp_engine_disableNoiseBlanker(h)
    lib.rdsp_engine_setInputGain(h, 1.0); lib.rdsp_engine_setOutputGain(h, 0.5); lib.rdsp_engine_setIQgainBalance(h, 1.02)
    lib.rdsp_engine_enableAudioFilter(h); lib.rdsp_engine_setAudioFilter(h, 6); lib.rdsp_engine_setDemodMode(h, 0)
    if decoders:
        assert lib.rdsp_engine_enable_meter(h) == 0 and lib.rdsp_engine_set_squelch(h, 5e-5, 1.25e-5, 2) == 0
        assert lib.rdsp_engine_enable_fm(h) == 0
        assert lib.rdsp_engine_enable_dtmf(h) == 0 and lib.rdsp_engine_set_dtmf(h, 4, 0.015, 4.0, 16.0, 0.5, 2, 2) == 0
        assert lib.rdsp_engine_enable_afsk(h) == 0 and lib.rdsp_engine_set_afsk(h, 1, 1.0, 2, 17) == 0
        assert lib.rdsp_engine_enable_pocsag(h) == 0 and lib.rdsp_engine_set_pocsag(h, 2400, 2, 3, 2, 1, 2) == 0
        lib.rdsp_engine_setDemodMode(h, 7)
        assert lib.rdsp_engine_set_fm(h, 2, 7500.0, 0.0) == 0
    return h


def stations(mods, seed):
    """sixteen modulating signals -> CALLS_OF_INPUT arrays int16 [NCH, NBLK * 128, 2], consecutive calls, cycled over the receivers"""
    r = np.random.default_rng(seed)
    rows = []
    for mod in mods:
        t = len(mod)
        z = r.uniform(2000, 20000) * np.exp(1j * (2 * np.pi * 7500.0 / 44100.0 * np.cumsum(mod))) + 3.0 * (r.standard_normal(t) + 1j * r.standard_normal(t))
        rows.append(np.stack([np.rint(z.real), np.rint(z.imag)], 1).astype(np.int16))
    rows = np.stack(rows)
    return [rows[:, k * NBLK * 128:(k + 1) * NBLK * 128][np.arange(NCH) % 16] for k in range(CALLS_OF_INPUT)]


def paging_iq():
    """pocsag_times.py's paging leg at 2400 baud: batches of drawn alphanumeric messages without a pause"""
    r = np.random.default_rng(2400)
    t = CALLS_OF_INPUT * NBLK * 128
    mods = []
    for k in range(16):
        msgs = [(int(r.integers(0, 1 << 21)), 3, [int(v) for v in r.integers(0, 1 << 20, int(r.integers(2, 14)))]) for _ in range(40)]
        mods.append(P.transmit(P.bits(P.batches(msgs), 64), 2400, 0.6, ppm=r.uniform(-100, 100), total=t))
    return stations(mods, 1)


def packet_iq():
    """afsk_times.py's packet leg: frames of 40 drawn bytes without a pause"""
    r = np.random.default_rng(1)
    t = CALLS_OF_INPUT * NBLK * 128
    mods = []
    for k in range(16):
        bits = []
        while len(bits) * 36.75 < t:
            bits += A.frame_bits(bytes(r.integers(0, 256, 40, dtype=np.uint8)), 2, 1)
        mods.append(A.audio(A.nrzi(bits), 0.3, phase=r.uniform(0, 6), total=t))
    return stations(mods, 2)


def noise_iq():
    r = np.random.default_rng(2)
    return [np.rint(300.0 * r.standard_normal((64, NBLK * 128, 2))).astype(np.int16)[np.arange(NCH) % 64]]


this = _lib.load()
out = torch.empty((NCH, NBLK * 128, 2), dtype=torch.int16, device="cuda")
stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
# (a)'s buffers: the counts and rings of the three decoders, on the device and pinned on the host
DENSE = [("rdsp_engine_read_dtmf_digits", 16), ("rdsp_engine_read_afsk_frames", 4 * 84), ("rdsp_engine_read_pocsag_messages", 4 * 84)]
d_count = [torch.empty((NCH,), dtype=torch.int32, device="cuda") for _ in DENSE]
d_ring = [torch.empty((NCH, w), dtype=torch.int32, device="cuda") for _, w in DENSE]
h_count = [torch.empty((NCH,), dtype=torch.int32).pin_memory() for _ in DENSE]
h_ring = [torch.empty((NCH, w), dtype=torch.int32).pin_memory() for _, w in DENSE]
# (b)'s
d_rec = torch.empty((args.cap_events, 4), dtype=torch.int32, device="cuda")
d_words = torch.empty((args.cap_words,), dtype=torch.int32, device="cuda")
d_cnt = torch.empty((5,), dtype=torch.int32, device="cuda")
h_rec = torch.empty((args.cap_events, 4), dtype=torch.int32).pin_memory()
h_words = torch.empty((args.cap_words,), dtype=torch.int32).pin_memory()
h_cnt = torch.empty((5,), dtype=torch.int32).pin_memory()
moved = {"dense": sum(4 * NCH * (1 + w) for _, w in DENSE), "gather": [], "events": [], "lost": []}


def leg(lib, h, d_iqs, kind):
    """one call of a leg: the update on the next input of the cycle, then what the leg does, through its last synchronise"""
    at = [0]

    def call():
        d_iq = d_iqs[at[0] % len(d_iqs)]
        at[0] += 1
        rc = lib.rdsp_engine_update(h, d_iq.data_ptr(), NBLK * 128, NBLK, out.data_ptr(), NBLK * 128, stream)
        assert rc == 0, rc
        if kind == "dense":
            for k, (name, _) in enumerate(DENSE):
                assert getattr(lib, name)(h, 0, NCH, d_count[k].data_ptr(), d_ring[k].data_ptr(), stream) == 0
                h_count[k].copy_(d_count[k], non_blocking=True)
                h_ring[k].copy_(d_ring[k], non_blocking=True)
        elif kind == "gather":
            assert lib.rdsp_engine_gather_events(h, d_rec.data_ptr(), args.cap_events, d_words.data_ptr(), args.cap_words, d_cnt.data_ptr(), stream) == 0
            h_cnt.copy_(d_cnt, non_blocking=True)
            torch.cuda.synchronize()
            needed, we, _, ww, lost = h_cnt.tolist()
            h_rec[:we].copy_(d_rec[:we], non_blocking=True)
            h_words[:ww].copy_(d_words[:ww], non_blocking=True)
            moved["gather"].append(20 + 16 * we + 4 * ww)
            moved["events"].append(needed)
            moved["lost"].append(lost)
        elif kind == "sizing":
            assert lib.rdsp_engine_gather_events(h, None, 0, None, 0, d_cnt.data_ptr(), stream) == 0
            h_cnt.copy_(d_cnt, non_blocking=True)
        torch.cuda.synchronize()
    return call


def wall(fn, calls):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return (time.perf_counter() - t0) * 1e3 / calls


def hip_events(fn, calls):
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


def updater(lib, h, d_iq):
    def update():
        assert lib.rdsp_engine_update(h, d_iq.data_ptr(), NBLK * 128, NBLK, out.data_ptr(), NBLK * 128, stream) == 0
    return update


makers = {"paging": paging_iq, "packet": packet_iq, "noise": noise_iq}
legs, timer = {}, {}
for name, make in makers.items():
    if args.only is not None and not args.only.startswith(name + ":"):
        continue
    d_iqs = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in make()]
    for kind in ("update", "dense", "gather", "sizing"):
        if args.only is None or args.only == f"{name}:{kind}":
            legs[f"{name}:{kind}"] = leg(this, engine(this, True), d_iqs, kind)
            timer[f"{name}:{kind}"] = wall
if args.only is None or args.only in ("never", "parent"):
    synth = torch.from_numpy(synth_iq(NCH, NBLK * 128, n_threads=8)).cuda()
    if args.only in (None, "never"):
        legs["never"], timer["never"] = updater(this, engine(this, False), synth), hip_events
    if args.parent_lib and args.only in (None, "parent"):
        parent = bind(os.path.abspath(args.parent_lib))
        legs["parent"], timer["parent"] = updater(parent, engine(parent, False), synth), hip_events
times = {name: [] for name in legs}
order = list(legs)
for run in range(args.runs):
    for name in order[run % len(order):] + order[:run % len(order)]:   # the order rotates: no leg always runs first
        moved["gather"].clear(), moved["events"].clear(), moved["lost"].clear()
        times[name].append(timer[name](legs[name], args.calls))
        note = ""
        if name.endswith(":gather"):
            note = (f"  {statistics.mean(moved['gather']):.0f} bytes, {statistics.mean(moved['events']):.1f} events, {statistics.mean(moved['lost']):.2f} lost "
                    f"a call (most {max(moved['events'])} events)")
        print(f"run {run}  {name:16s} {times[name][-1]:8.4f} ms per call{note}", flush=True)
for name, t in times.items():
    how = "HIP events" if timer[name] is hip_events else "wall"
    print(f"{name:16s} min {min(t):.4f}  median {statistics.median(t):.4f}  max {max(t):.4f} ms per call of {NCH} x {NBLK} blocks ({how})")
print(f"(a) moves {moved['dense']} bytes a call")
