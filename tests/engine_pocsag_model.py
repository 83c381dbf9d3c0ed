"""rdsp_engine_t's POCSAG pager decoder (include/rdsp.h, "POCSAG pager decoder"; csrc/rdsp_pocsag.h) restated in numpy: the
decimation by 4 and the matched filter over its window (vectorised over the samples and the channels, the sums in the
definition's order), and a per-channel object with the 456 state words whose bit clock, framing, BCH correction and message ring
are plain Python integers.  The clock is walked per run between two transitions, not per sample: inside a run it is linear, so
the samples at which bits are taken follow from one division (the plain loop of rdsp_pocsag.h walks every sample, the kernel
every run cut at the blocks' ends: three statements of one definition).  The transmitter is radiodsp_sdr_rx_amd/pocsag.py's."""
import math

import numpy as np

import engine_dtmf_model as D

F32 = np.float32
M32 = 0xFFFFFFFF
BLOCK, DEC, PER_BLOCK, MAX_WINDOW, HIST = 128, 4, 32, 20, 19
WORDS, MSG_MAX, MSG_HEAD, RING, SLOT_WORDS, BATCH = 456, 80, 4, 4, 84, 16
BAUD, PLL, PREV_RAW, SR, INSYNC, POL, NBITS, NCW, OPEN, M_NCW, M_FLAGS, M_ADDR, M_COUNTS, NMSGS, NBAD, TBLOCKS = range(16)
HIST_, MSG, RING_ = 16, 36, 120
SYNC, IDLE, POLY = 0x7CD215D8, 0x7A89C197, 0x769
FLAG_CUT, FLAG_TRUNCATED, FLAG_UNCORRECTABLE = 1, 2, 4
DEFAULTS = dict(invert=2, pull=3, sync_errs=2, fix_addr=1, fix_data=2)
WINDOWS = {512: 20, 1200: 8, 2400: 4}


def step_of(baud):
    """(uint32) llround(baud 2^32 4 / 44100.0): half away from zero"""
    x = float(baud) * 4294967296.0 * 4.0 / 44100.0
    r = math.floor(x)
    if x - r >= 0.5:
        r += 1
    return r & M32


def lscale_of(window):
    return F32(1.0 / (32.0 * 4.0 * window))


DSCALE = F32(1.0 / 128.0)


def popcount(v):
    return bin(v & M32).count("1")


def syndrome(word):
    r = (word & M32) >> 1
    for i in range(30, 9, -1):
        if r >> i & 1:
            r ^= POLY << (i - 10)
    return r & 0x3FF


def codeword(data21):
    d = (data21 & 0x1FFFFF) << 11
    w = d | syndrome(d) << 1
    return w | (popcount(w) & 1)


def bch_table():
    """1024 entries by syndrome: b1 | b2 << 5 | ne << 10, 0xFFFF for none"""
    t = np.full(1024, 0xFFFF, np.uint16)
    t[0] = 0
    for b1 in range(1, 32):
        t[syndrome(1 << b1)] = b1 | 1 << 10
        for b2 in range(b1 + 1, 32):
            t[syndrome(1 << b1 | 1 << b2)] = b1 | b2 << 5 | 2 << 10
    return t


TABLE = [int(v) for v in bch_table()]


def correct(word, fix_addr, fix_data):
    """-> (accepted, corrected word, ne)"""
    e = TABLE[syndrome(word)]
    if e == 0xFFFF:
        return False, word, 0
    fixed, ne = word, e >> 10
    for b in (e & 31, e >> 5 & 31):
        if b:
            fixed ^= 1 << b
    if popcount(fixed) & 1:
        fixed ^= 1
        ne += 1
    return ne <= (fix_data if fixed >> 31 else fix_addr), fixed, ne


# ---- the definition ----

def _f(x):
    return np.asarray(x, F32)


def _group(t):
    """up to four terms, oldest first, as dtmf_quad adds them (a missing term is left out, not added as a zero)"""
    with np.errstate(all="ignore"):
        if len(t) == 4:
            return _f(_f(t[0] + t[1]) + _f(t[2] + t[3]))
        out = t[0]
        for v in t[1:]:
            out = _f(out + v)
        return out


def stage12(rows, hist, window):
    """rows float32 [n, nb 128], hist float32 [n, 19] -> (raw uint8 [n, nb 32], lvl float32 [n, nb], dc float32 [n, nb], the
    next hist [n, 19]).  window: the build's are 20, 8 and 4; any other, for the figures the choice rests on, sums the newest
    `window` samples in groups of four, oldest first, the groups folded from the left"""
    assert 1 <= window <= MAX_WINDOW
    rows = _f(rows)
    n, N = rows.shape[0], rows.shape[1] // DEC
    d = D.quad(rows)
    ext = np.concatenate([_f(hist), d], 1)                                                   # d[m0 - 19 ... m0 + N - 1]
    t = [ext[:, k:k + N] for k in range(MAX_WINDOW - window, MAX_WINDOW)]
    q = [_group(t[i:i + 4]) for i in range(0, window, 4)]
    with np.errstate(all="ignore"):
        S = q[0]
        for v in q[1:]:
            S = _f(S + v)
        raw = (S < 0).astype(np.uint8)

        def tree(v):
            v = _f(v).reshape(n, -1, PER_BLOCK)
            for _ in range(5):
                v = _f(v[..., 0::2] + v[..., 1::2])
            return v[..., 0]
        lvl = _f(tree(np.abs(S)) * lscale_of(window))
        dc = _f(tree(d) * DSCALE)
    return raw, lvl, dc, ext[:, N:].copy()


def machine(w, raw, baud, invert, pull, sync_errs, fix_addr, fix_data, trace=None, log=None):
    """stages 3 to 7 of one channel: w its 456 words (changed in place), raw the call's decisions (uint8 [nb 32]) -> (sync, new,
    bad) uint8 arrays over the call's blocks; trace receives (m, word index in the batch or -1 for a sync word, the word as read)
    of every word closed, m the sample's index since the detector's start; log receives read_slot() of every message closed"""
    pll, prev_raw, sr, insync, pol, nbits, ncw, opened, m_ncw, m_flags, m_addr, m_counts, n_msgs, n_bad, t_blocks = (int(v) for v in w[PLL:TBLOCKS + 1])
    step = step_of(baud)
    raw = np.asarray(raw, np.uint8)
    N = len(raw)
    nb = N // PER_BLOCK
    new, bad = np.zeros(nb, np.int64), np.zeros(nb, np.int64)
    sync_at = [(-1, insync)]                                                                  # (sample, insync from that sample on)

    def close(flag, at):
        nonlocal opened, m_ncw, m_flags, m_addr, m_counts, n_msgs
        if not opened:
            return
        slot = np.zeros(SLOT_WORDS, np.uint32)
        slot[0], slot[1], slot[2], slot[3] = m_ncw | (m_flags | flag) << 8 | pol << 16, (t_blocks + at // PER_BLOCK + 1) & M32, m_addr, m_counts
        slot[MSG_HEAD:MSG_HEAD + m_ncw] = w[MSG + MSG_HEAD:MSG + MSG_HEAD + m_ncw]
        w[RING_ + (n_msgs % RING) * SLOT_WORDS:RING_ + (n_msgs % RING + 1) * SLOT_WORDS] = slot
        if log is not None:
            log.append(read_slot(slot))
        n_msgs = (n_msgs + 1) & M32
        new[at // PER_BLOCK] += 1
        opened = m_ncw = m_flags = m_addr = m_counts = 0

    def append(word):
        nonlocal m_ncw, m_flags, m_counts
        if m_ncw < MSG_MAX:
            w[MSG + MSG_HEAD + m_ncw] = word
            m_ncw += 1
            if word >> 31:
                m_flags |= FLAG_UNCORRECTABLE
                m_counts += 1 << 16
            else:
                m_counts += word >> 24
        else:
            m_flags |= FLAG_TRUNCATED

    edges = np.flatnonzero(np.diff(np.concatenate([[prev_raw], raw]).astype(np.int64)) != 0).tolist()
    starts = edges if edges and edges[0] == 0 else [0] + edges
    for k, p0 in enumerate(starts):
        p1 = starts[k + 1] if k + 1 < len(starts) else N
        bit = int(raw[p0])
        if bit != prev_raw:
            sp = pll - (1 << 32) if pll & 0x80000000 else pll
            pll = (sp - (sp >> pull)) & M32
            prev_raw = bit
        u = pll ^ 0x80000000
        t = u + (p1 - p0) * step
        pll = (t & M32) ^ 0x80000000
        for i in range(1, (t >> 32) + 1):
            at = p0 + -((u - (i << 32)) // step) - 1                                          # the sample whose step carries for the i-th time
            sr = (sr << 1 | bit) & M32
            if not insync:
                plain = invert != 1 and popcount(sr ^ SYNC) <= sync_errs
                inverted = invert != 0 and popcount(~sr ^ SYNC) <= sync_errs
                if plain or inverted:
                    insync, pol, nbits, ncw = 1, 0 if plain else 1, 0, 0
                    sync_at.append((at, 1))
                continue
            nbits += 1
            if nbits < 32:
                continue
            nbits = 0
            word = (~sr & M32) if pol else sr
            if trace is not None:
                trace.append((PER_BLOCK * t_blocks + at, -1 if ncw == BATCH else ncw, word))
            if ncw == BATCH:
                if popcount(word ^ SYNC) > sync_errs:
                    close(FLAG_CUT, at)
                    insync = 0
                    sync_at.append((at, 0))
                ncw = 0
                continue
            ok, fixed, ne = correct(word, fix_addr, fix_data)
            if not ok:
                n_bad = (n_bad + 1) & M32
                bad[at // PER_BLOCK] += 1
                if opened:
                    append((word >> 11 & 0xFFFFF) | 1 << 31)
            elif fixed >> 31:
                if opened:
                    append((fixed >> 11 & 0xFFFFF) | ne << 24)
            else:
                close(0, at)
                if fixed != IDLE:
                    opened = 1
                    m_addr = (fixed >> 13 & 0x3FFFF) << 3 | ncw >> 1 | (fixed >> 11 & 3) << 21
                    m_counts = ne
            ncw += 1
    sync = np.zeros(nb, np.uint8)
    at_sample = np.array([a for a, _ in sync_at])
    value = np.array([v for _, v in sync_at], np.uint8)
    ends = PER_BLOCK * np.arange(1, nb + 1) - 1
    sync[:] = value[np.searchsorted(at_sample, ends, side="right") - 1]
    t_blocks = (t_blocks + nb) & M32
    w[PLL:TBLOCKS + 1] = [pll, prev_raw, sr, insync, pol, nbits, ncw, opened, m_ncw, m_flags, m_addr, m_counts, n_msgs, n_bad, t_blocks]
    return sync, (new & 0xFF).astype(np.uint8), np.minimum(bad, 255).astype(np.uint8)


def read_slot(slot):
    """a ring slot -> (t_blocks, address, function, the 20-bit words, flags, polarity)"""
    n = int(slot[0]) & 0xFF
    return (int(slot[1]), int(slot[2]) & 0x1FFFFF, int(slot[2]) >> 21 & 3, [int(v) & 0xFFFFF for v in slot[MSG_HEAD:MSG_HEAD + n]], int(slot[0]) >> 8 & 0xFF,
            int(slot[0]) >> 16 & 1)


class Pocsag:
    """n channels; run(rows) takes the demodulated rows float32 [n, nb * 128] of a call and returns (sync uint8, new uint8, bad
    uint8, lvl float32, dc float32) [n, nb]; the 456 words a channel carry on.  The settings are per channel here (the channel's
    group's).  A channel with baud 0 has zero words and zero records."""

    def __init__(self, n, baud=0, window=None, **kw):
        self.n, self.window = n, window                                                      # window: stage12's, None for the build's
        self.w = np.zeros((n, WORDS), np.uint32)
        self.log = [[] for _ in range(n)]                                                    # every message closed, ring or no ring
        self.baud, self.invert, self.pull, self.sync_errs, self.fix_addr, self.fix_data = (np.zeros(n, np.uint32) for _ in range(6))
        self.set(baud, **kw)

    def set(self, baud=1200, invert=2, pull=3, sync_errs=2, fix_addr=1, fix_data=2, channels=slice(None)):
        self.baud[channels], self.invert[channels], self.pull[channels] = baud, invert, pull
        self.sync_errs[channels], self.fix_addr[channels], self.fix_data[channels] = sync_errs, fix_addr, fix_data

    def reset(self, channels=slice(None)):
        self.w[channels] = 0

    def words(self):
        return self.w.copy()

    def ring(self):
        """(n_msgs uint32 [n], ring uint32 [n, 4, 84])"""
        return self.w[:, NMSGS].copy(), self.w[:, RING_:].reshape(self.n, RING, SLOT_WORDS).copy()

    def messages(self, c=0):
        """channel c's ring read by read_slot, oldest first: the last four at most"""
        n, ring = int(self.w[c, NMSGS]), self.w[c, RING_:].reshape(RING, SLOT_WORDS)
        return [read_slot(ring[k % RING]) for k in range(max(0, n - RING), n)]

    def run(self, rows, reset=None, raws=None, trace=None):
        """reset: channels whose group has an FM reset pending (a boolean mask or None); raws: a list that receives raw [n, nb 32];
        trace: a list that receives channel 0's words of machine()"""
        rows = np.asarray(rows, F32)
        n, nb = rows.shape[0], rows.shape[1] // BLOCK
        assert n == self.n
        w = self.w
        fresh = w[:, BAUD] != self.baud
        if reset is not None:
            fresh |= np.asarray(reset, bool)
        w[fresh] = 0
        live = self.baud != 0
        w[~live] = 0
        w[live, BAUD] = self.baud[live]
        sync, new, bad = (np.zeros((n, nb), np.uint8) for _ in range(3))
        lvl, dc = np.zeros((n, nb), F32), np.zeros((n, nb), F32)
        raw_all = np.zeros((n, nb * PER_BLOCK), np.uint8)
        for baud in sorted(set(int(b) for b in self.baud[live])):
            sel = np.flatnonzero(self.baud == baud)
            raw, lvl[sel], dc[sel], hist = stage12(rows[sel], w[sel, HIST_:HIST_ + HIST].copy().view(F32), self.window or WINDOWS[baud])
            raw_all[sel] = raw
            w[sel, HIST_:HIST_ + HIST] = np.ascontiguousarray(hist).view(np.uint32)
            for k, c in enumerate(sel):
                sync[c], new[c], bad[c] = machine(w[c], raw[k], baud, int(self.invert[c]), int(self.pull[c]), int(self.sync_errs[c]), int(self.fix_addr[c]),
                                                  int(self.fix_data[c]), trace if c == 0 else None, self.log[c])
        if raws is not None:
            raws.append(raw_all)
        return sync, new, bad, lvl, dc
