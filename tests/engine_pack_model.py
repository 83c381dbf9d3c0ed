"""rdsp_engine_pack_active and rdsp_pack_runs (include/rdsp.h, "packed audio of the open receivers") restated in numpy: the
blocks of a call whose gate was open, by channel ascending, then block ascending, as dense mono blocks with a (channel, block)
record each; and the records merged into runs of consecutive blocks of one receiver."""
import numpy as np

BLOCK = 128


def pack(audio, gate, capacity=None):
    """audio int16 [n, nb * 128] (the left words of a call), gate [n, nb] -> (blocks int16 [written, 128], records int32
    [written, 2] = channel, block; needed); written = min(needed, capacity)"""
    audio, gate = np.asarray(audio), np.asarray(gate)
    n, nb = gate.shape
    assert audio.shape == (n, nb * BLOCK)
    blocks, records = [], []
    for ch in range(n):                                    # the definition's order, written out
        for b in range(nb):
            if gate[ch, b] != 0:
                records.append((ch, b))
                blocks.append(audio[ch, b * BLOCK:(b + 1) * BLOCK])
    needed = len(records)
    written = needed if capacity is None else min(needed, int(capacity))
    blocks = np.array(blocks[:written], np.int16).reshape(written, BLOCK)
    return blocks, np.array(records[:written], np.int32).reshape(written, 2), needed


def runs(records, first_block=0):
    """records int32 [n, 2], strictly ascending in (channel, block) (ValueError otherwise) -> int64 [m, 4]: channel, absolute
    first block, number of blocks, index of the run's first record"""
    rec = np.asarray(records, np.int64).reshape(-1, 2)
    out = []
    for k, (ch, b) in enumerate(rec):
        if ch < 0 or b < 0 or (k > 0 and (int(rec[k - 1, 0]), int(rec[k - 1, 1])) >= (int(ch), int(b))):
            raise ValueError(f"record {k} is negative or not above the record in front of it")
        if k > 0 and rec[k - 1, 0] == ch and rec[k - 1, 1] + 1 == b:
            out[-1][2] += 1
        else:
            out.append([int(ch), int(first_block) + int(b), 1, k])
    return np.array(out, np.int64).reshape(-1, 4)
