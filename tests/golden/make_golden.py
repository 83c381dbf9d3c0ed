"""Generates the committed golden vectors in tests/golden/*.npz.

The reference ships no fixtures and cannot run here, so these are outputs of the
CPU oracle (oracle/rdsp_oracle.c) on deterministic synthetic IQ: they pin the
oracle against accidental change and give the GPU tests fixed expected outputs
that travel to the GPU box.  Fixtures of chains with an NLMS stage also carry the float64
result of tests/np_model.py (out_f64).  Regenerate with:  python tests/golden/make_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import np_model  # noqa: E402
import oracle_lib  # noqa: E402
from cases import GOLDEN_CASES, add_impulses, apply_setup  # noqa: E402
from nodes_oracle import TeensyBiquadOracle, _olib, oracle_fft1024, oracle_spectra  # noqa: E402
from radiodsp_sdr_rx_amd.chain import synth_iq  # noqa: E402


def make_nodes():
    """graph nodes beside the chain (integer analysers, int16 biquad): nodes.npz holds one input and what
    the oracle's restatements give for it -- the panadapter analyser (naverage 5, AudioWindowHanning256), the
    audio analyser on the I side (AudioWindowHanning1024; both tables as in the reference's firmware image) and
    `setHighpass(0, 500, 0.5)` + a notch in stage 1 on the I side (the Teensy library's fixed-point AudioFilterBiquad)"""
    lib = _olib(oracle_lib)
    nch, nblk = 2, 40
    iq = synth_iq(nch, nblk * 128)
    iq[1] = np.clip(iq[1].astype(np.int32) * 4, -32768, 32767).astype(np.int16)
    spec256, spec1024, bq = [], [], []
    for c in range(nch):
        i = np.ascontiguousarray(iq[c, :, 0])
        spec256.append(np.stack(oracle_spectra(lib, iq[c], 5, 1)))
        spec1024.append(oracle_fft1024(lib, i, 1))
        o = TeensyBiquadOracle(lib)
        o.set(0, "highpass", 500.0, 0.5)
        o.set(1, "notch", 1000.0, 4.0)
        bq.append(o.update(i))
    np.savez_compressed(os.path.join(HERE, "nodes.npz"), iq=iq, spectrum256=np.stack(spec256),
                        fft1024=np.stack(spec1024), biquad=np.stack(bq))
    print("nodes", iq.shape, np.stack(spec256).shape, np.stack(spec1024).shape)


def main():
    oracle_lib.build()
    only = set(sys.argv[1:])   # e.g. `make_golden.py nodes` regenerates that fixture alone
    if not only or "nodes" in only:
        make_nodes()
    for name, case in GOLDEN_CASES.items():
        if only and name not in only:
            continue
        iq = synth_iq(case["channels"], case["blocks"] * 128, cw=case.get("cw", False))
        if case.get("impulses"):
            iq = add_impulses(iq)
        o16, o32 = [], []
        for c in range(case["channels"]):
            ch = oracle_lib.OracleChain(**case["cfg"])
            apply_setup(ch, case.get("setup"), oracle=True)
            a, b = ch.process(iq[c])
            o16.append(a)
            o32.append(b)
        extra = {}
        cfg = case["cfg"]
        if cfg.get("lms_nr", 0) > 0 or cfg.get("als_mode", "off") != "off" or cfg.get("demod") == "SAM":
            # recursive stages (NLMS, SAM PLL): the float64 evaluation of the same chain (tests/np_model.py) travels with
            # the fixture; the GPU test anchors its tolerance on it (truth), not on the float32 oracle
            extra["out_f64"] = np.stack([np_model.Model(**cfg).process(iq[c]) for c in range(case["channels"])])
        np.savez_compressed(os.path.join(HERE, name + ".npz"), iq=iq, out_i16=np.stack(o16),
                            out_f32=np.stack(o32), **extra)
        print(name, iq.shape, np.stack(o16).shape)


if __name__ == "__main__":
    main()
