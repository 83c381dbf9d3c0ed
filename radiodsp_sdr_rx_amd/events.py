"""The decoders' events as Engine.gather_events returns them (include/rdsp.h "Decoder events"), read on the host.  Host only: no
device code, no library call.

    parse(records, words) -> [Event(channel, kind, seq, t_blocks, value)]

records is int32 or uint32 [n, 4] = channel, kind | n_words << 8, seq, offset; words the payload words.  value is the key's
character for DTMF, the frame's bytes (FCS checked and removed) for AFSK and a pocsag.Message for POCSAG; t_blocks is the block
stamp the decoder gave the item.
"""
from collections import namedtuple

import numpy as np

from . import pocsag

DTMF, AFSK, POCSAG = 0, 1, 2
KIND_NAMES = ("dtmf", "afsk", "pocsag")
DTMF_KEYS = "123A456B789C*0#D"
SLOT_WORDS = 84

Event = namedtuple("Event", "channel kind seq t_blocks value")
Counts = namedtuple("Counts", "needed_events written_events needed_words written_words lost")


def parse(records, words):
    records = np.asarray(records).reshape(-1, 4).astype(np.int64) & 0xFFFFFFFF
    words = np.ascontiguousarray(np.asarray(words).reshape(-1)).view(np.uint32)
    out = []
    for ch, kw, seq, off in records.tolist():
        kind, n = kw & 0xFF, kw >> 8
        w = words[off:off + n]
        if len(w) != n:
            raise ValueError("events.parse: the record at offset %d needs %d words, %d are there" % (off, n, len(w)))
        ch -= (ch >> 31) << 32
        if kind == DTMF:
            sym = int(w[0]) & 0xFF
            out.append(Event(ch, kind, seq, int(w[0]) >> 8, DTMF_KEYS[sym] if sym < 16 else ""))
        elif kind == AFSK:
            out.append(Event(ch, kind, seq, int(w[1]), w[2:].astype("<u4").tobytes()[:int(w[0])]))
        elif kind == POCSAG:
            m = pocsag.from_slot(np.concatenate([w, np.zeros(SLOT_WORDS - n, np.uint32)]))
            out.append(Event(ch, kind, seq, m.t_blocks, m))
        else:
            raise ValueError("events.parse: kind %d" % kind)
    return out
