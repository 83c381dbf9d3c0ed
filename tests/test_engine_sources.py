"""The source front end of rdsp_engine_t as one object (csrc/rdsp_engine_sources.hip): the map, the rate P / Q, the format, the
taps and ONE history per source, restarted by one rule.

`-m "not gpu"`: tests/host/host_sources_check.cpp, the host-only logic of csrc/rdsp_tune.h -- the workgroup run lists of both
filter-bank passes (source_runs) and the size of a source's history (rate_keep pairs of src_hist_words words) -- plain and
under the address and undefined-behaviour sanitizers.
`-m gpu`: a walk through every kind of reconfiguration.  A restart zeroes exactly the histories and frac and keeps the phases;
a call that sets what the engine already has changes no bit."""
import os
import subprocess

import numpy as np
import pytest

from engine_sources_model import HERE, ROOT, S16, U8, _raw_of, _setup, _stations, _stream, wide


# ---- CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sanitize", [False, True])
def test_sources_host_logic(tmp_path, sanitize):
    """source_runs for max = DDC_RPW and RATE_RPW on one source of max - 1, max, max + 1 and 2 max + 1 receivers, an
    interleaved map c % 3, a map that leaves a source without receivers and n = 1: the runs partition 0 ... n - 1 in order,
    hold at most max receivers of one source, and two neighbours share a source only if the first is full.  The history of
    the rates (1, 1), (2, 1), (64, 1), (3, 2), (160, 147), (20480, 441): 0, 15 D and 16 ceil(P / Q) pairs, of 1 word for S16
    and 2 for the other formats.  Once plain and once under ASan + UBSan (a program of its own, run directly)."""
    exe = str(tmp_path / "host_sources_check")
    extra = ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all"] if sanitize else []
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O1" if sanitize else "-O2", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off",
                           "-Wall", "-Werror"] + extra + ["-I", os.path.join(ROOT, "radiodsp_sdr_rx_amd", "csrc"),
                           os.path.join(HERE, "host", "host_sources_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "host_sources_check OK" in out.stdout, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "Sanitizer" not in out.stderr, out.stderr


# ---- GPU ------------------------------------------------------------------------------------------------------------------
NCH, GAIN = 19, 2.0
SOURCE_OF = [0] * 17 + [1] * 2      # the decimating pass: a full workgroup of 16, a ragged one of one receiver, and a third


def _rows(seed, n_sources, n_blocks, P, Q, fmt):
    import torch
    return torch.from_numpy(_raw_of(fmt, wide(seed, n_sources, n_blocks, P, Q, level=0.3))).cuda()


@pytest.mark.gpu
def test_gpu_sources_configuration_walk(rdsp):
    """19 receivers on 2 sources, max_blocks = 2.  The engine walks (1, 1) -> (3, 1) -> (3, 2) -> (3, 1) -> set_sources with 3
    rows (the third without a listener) -> U8 -> (1, 1) -> (5, 1) -> S16 and runs a 2-block call after every step.  Before that
    call its state blob goes into a fresh engine configured directly to the step's configuration (after one plain update,
    which takes the pending resets of its set-up and touches nothing of the front end): both then give the same audio (not
    all zero) and the same blob -- every restart zeroes exactly the histories and frac and keeps the phases.
    Then, one block into a stream at (3, 2), (3, 1) under U8 and (160, 147) (where frac is not 0): set_source_rate with the
    rate and gain the engine has, set_sources with its map and set_source_format with its format change no bit of the next
    block against a twin that made none of these calls."""
    import torch
    stations = _stations(1, NCH, 1, 1)                       # inside the band of every rate of the walk
    cfg = dict(P=1, Q=1, n=2, fmt=S16)
    walk = [dict(), dict(P=3), dict(Q=2), dict(Q=1), dict(n=3), dict(fmt=U8), dict(P=1), dict(P=5), dict(fmt=S16)]
    e = None
    idle = torch.zeros((NCH, 128, 2), dtype=torch.int16, device="cuda")
    for k, step in enumerate(walk):
        cfg.update(step)
        P, Q, n, fmt = cfg["P"], cfg["Q"], cfg["n"], cfg["fmt"]
        if e is None:
            e = _setup(NCH, n, SOURCE_OF, P, Q, GAIN, stations, fmt, max_blocks=2)
        elif "n" in step:
            e.set_sources(n, SOURCE_OF)
        elif "fmt" in step:
            e.set_source_format(fmt)
        else:
            e.set_source_rate(P, Q, GAIN)
        assert e.source_rate() == (P, Q) and e.source_format() == fmt
        blob = e.save_state(0, NCH)
        t = _setup(NCH, n, SOURCE_OF, P, Q, GAIN, stations, fmt, max_blocks=2)
        t.update(idle)                                       # takes the resets that sketch_setup left pending, as e's first call did
        t.load_state(0, blob)
        d = _rows(10 + k, n, 2, P, Q, fmt)
        e.pos_pairs = t.pos_pairs = 0
        ya, yb = _stream(e, d, P, Q, 0, 2, 2)[0], _stream(t, d, P, Q, 0, 2, 2)[0]
        assert ya.any() and np.array_equal(ya, yb), (k, cfg, np.argwhere(ya != yb)[:3])
        after = e.save_state(0, NCH)
        assert np.array_equal(after, t.save_state(0, NCH)) and not np.array_equal(after, blob), (k, cfg)
        t.close()
    e.close()
    for P, Q, fmt in ((3, 2, S16), (3, 1, U8), (160, 147, S16)):
        d = _rows(30 + P, 2, 2, P, Q, fmt)
        a, b = (_setup(NCH, 2, SOURCE_OF, P, Q, GAIN, stations, fmt, max_blocks=2) for _ in range(2))
        a.pos_pairs = b.pos_pairs = 0
        first = [_stream(x, d, P, Q, 0, 1, 1)[0] for x in (a, b)]
        assert first[0].any() and np.array_equal(first[0], first[1])
        pairs = a.source_pairs(1)
        a.set_source_rate(P, Q, GAIN)
        a.set_sources(2, SOURCE_OF)
        a.set_source_format(fmt)
        assert a.source_pairs(1) == pairs == b.source_pairs(1)           # frac kept
        ya, yb = _stream(a, d, P, Q, 1, 2, 1)[0], _stream(b, d, P, Q, 1, 2, 1)[0]
        assert ya.any() and np.array_equal(ya, yb), (P, Q, np.argwhere(ya != yb)[:3])
        assert np.array_equal(a.save_state(0, NCH), b.save_state(0, NCH))
        a.close()
        b.close()
