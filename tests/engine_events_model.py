"""rdsp_engine_gather_events in numpy (include/rdsp.h "Decoder events"): the definition restated from `new` records, count words
and rings in the shapes Engine.read_dtmf / read_afsk / read_pocsag and read_dtmf_digits / read_afsk_ring / read_pocsag_ring
return them.  Host only.

    sequence(new, count, ring) -> (events, lost): events a list of (channel, kind, seq, payload uint32 array)
    gather(new, count, ring, capacity_events, capacity_words) -> (records uint32 [written, 4], words uint32 [written_words], counts)
    cut(events, lost, capacity_events, capacity_words) -> the same from a sequence
    states(count, ring) -> the three detector-word arrays rdsp_events_reference takes

new, count and ring are triples by kind (DTMF, AFSK, POCSAG); None in new switches a kind off.
"""
import numpy as np

DTMF, AFSK, POCSAG = 0, 1, 2
RING = (16, 4, 4)
SLOT = (1, 84, 84)
WORDS = (168, 448, 456)        # a channel's detector words
COUNT_AT = (6, 10, 13)         # n_digits, n_frames, n_msgs
RING_AT = (16, 112, 120)
U32 = np.uint32


def n_words(kind, head):
    head = int(head)
    if kind == DTMF:
        return 1
    if kind == AFSK:
        return 2 + (min(head, 328) + 3) // 4
    return 4 + min(head & 0xFF, 80)


def fresh_count(kind, new):
    """c per channel: new is uint8 [n, n_blocks]"""
    new = np.asarray(new)
    return (new != 255).sum(1).astype(np.int64) if kind == DTMF else new.astype(np.int64).sum(1)


def sequence(new, count, ring):
    events, lost = [], 0
    on = [k for k in range(3) if new[k] is not None]
    if not on:
        return events, lost
    c = {k: fresh_count(k, new[k]) for k in on}
    n_channels = len(c[on[0]])
    busy = np.zeros(n_channels, bool)
    for k in on:
        busy |= c[k] > 0
    for ch in np.flatnonzero(busy):
        for k in on:
            ck, n, R = int(c[k][ch]), int(np.asarray(count[k]).view(U32)[ch]), RING[k]
            assert ck <= n, "c <= n holds behind every update: channel %d kind %d has c %d, n %d" % (ch, k, ck, n)
            take = min(ck, R)
            lost += ck - take
            slots = np.asarray(ring[k]).view(U32).reshape(n_channels, R, SLOT[k])
            for seq in range(n - take, n):
                slot = slots[ch, seq % R]
                events.append((int(ch), k, seq, slot[:n_words(k, slot[0])].copy()))
    return events, lost


def gather(new, count, ring, capacity_events=None, capacity_words=None):
    return cut(*sequence(new, count, ring), capacity_events, capacity_words)


def cut(events, lost, capacity_events=None, capacity_words=None):
    """the prefix rule on a sequence: what a call with these capacities (None: all that is needed) writes"""
    needed_words = sum(len(p) for *_, p in events)
    ce = len(events) if capacity_events is None else capacity_events
    cw = needed_words if capacity_words is None else capacity_words
    records, words, offset = [], [], 0
    for k, (ch, kind, seq, p) in enumerate(events):
        if not (k < ce and offset + len(p) <= cw):
            break
        records.append((ch, kind | len(p) << 8, seq & 0xFFFFFFFF, offset))
        words.append(p)
        offset += len(p)
    counts = (len(events), len(records), needed_words, offset, lost)
    return (np.array(records, np.int64).astype(U32).reshape(-1, 4), np.concatenate(words).astype(U32) if words else np.zeros(0, U32), counts)


def states(count, ring):
    """detector words with nothing but the count word and the ring set; None stays None"""
    out = []
    for k in range(3):
        if count[k] is None:
            out.append(None)
            continue
        n = len(count[k])
        w = np.zeros((n, WORDS[k]), U32)
        w[:, COUNT_AT[k]] = np.asarray(count[k]).view(U32)
        w[:, RING_AT[k]:RING_AT[k] + RING[k] * SLOT[k]] = np.asarray(ring[k]).view(U32).reshape(n, -1)
        out.append(w)
    return out
