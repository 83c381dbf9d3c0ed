"""CPU: the judge of the engine-law tail tests (tests/test_tail_law.py) on the image's own fixture.

tests/test_tail_law.py holds the chain's RDSP_TAIL_ENGINE stage to the stage taps `OracleEngine(taps=True)` yields for
streams the fixture does not have.  Here those taps are pinned on tests/golden/engine_kat.npz, the image's own: for each
of the 9 tapped cases, the audio after the audio filter (`_tap_filt`, the stage's input), after the AGC (`_tap_agc`)
and after the ALS filter (`_tap_als`), bit for bit.
"""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TAIL_TAPS = ("filt", "agc", "als")


def test_oracle_engine_tail_taps_are_the_fixtures(oracle):
    kat = np.load(os.path.join(HERE, "golden", "engine_kat.npz"))
    cases = [n[:-len("_tap_filt")] for n in kat.files if n.endswith("_tap_filt")]
    assert len(cases) == 9, cases
    for name in cases:
        e = oracle.OracleEngine(taps=True)
        e.run(kat[name + "_iq"], json.loads(str(kat[name + "_calls"])))
        for st in TAIL_TAPS:
            want = kat[f"{name}_tap_{st}"]
            got = np.stack(e.taps[st][:len(want)])[:, :want.shape[1]]
            assert got.shape == want.shape == (len(want), 1, 128), (name, st)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (name, st)
