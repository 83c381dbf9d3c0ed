/*
 * rdsp_pocsag.h -- the arithmetic of rdsp_engine_t's POCSAG pager decoder (include/rdsp.h has the definition), shared by the
 * kernel (rdsp_engine_pocsag.hip), the host entry points (rdsp_engine_pocsag_host.hip) and the host program of the tests
 * (tests/host/host_pocsag_check.cpp).  Compile with -ffp-contract=off: every sum below is rounded on its own.
 *
 * Per channel, a[n] the receiver's "demod" tap (rdsp_fm.h's y[n]), blocks of 128 samples counted from the detector's start:
 *   d[m] = dtmf_quad(a[4 m ... 4 m + 3]), m = 32 t_blocks + r, 11 025 Hz; 0 before the start
 *   S[m] = the sum of d[m - W + 1 ... m], W = 20, 8, 4 at 512, 1200, 2400 baud, as dtmf_quads of four terms, oldest first,
 *          folded from the left; raw[m] = S[m] < 0 (POCSAG's 1 is the lower frequency)
 *   the bit clock (rdsp_afsk.h's afsk_pulled and afsk_clock), the framing, the BCH(31,21) correction and the message ring
 *   (pocsag_bit, pocsag_ring_word) are integers only.
 * A channel's state is POCSAG_WORDS = 456 words: baud, pll, prev_raw, sr, insync, pol, nbits, ncw, open, the open message's
 * n_cw, flags, address word and counts, n_msgs, n_bad, t_blocks; hist[19] (d[m - 19 ... m - 1] of the next m) and a zero; the
 * open message (four zeros -- its header lives in the scalars -- and 80 words); ring[4][84].  A detector whose stored baud is
 * not the one it is run with starts from zeros (pocsag_start).
 */
#ifndef RDSP_POCSAG_H
#define RDSP_POCSAG_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rdsp_afsk.h"
#include "rdsp_dtmf.h"

namespace rdsp_pocsag {

using rdsp_afsk::afsk_clock;
using rdsp_afsk::afsk_pulled;
using rdsp_dtmf::dtmf_quad;

constexpr int BLOCK = 128, DEC = 4, PER_BLOCK = BLOCK / DEC; /* 32 decimated samples a block */
constexpr int MAX_WINDOW = 20, HIST = MAX_WINDOW - 1;
constexpr int MSG_MAX = 80, MSG_HEAD = 4, RING = 4, SLOT_WORDS = MSG_HEAD + MSG_MAX;
constexpr int BATCH = 16; /* codewords between two sync words */
enum { PG_BAUD = 0, PG_PLL, PG_PREV_RAW, PG_SR, PG_INSYNC, PG_POL, PG_NBITS, PG_NCW, PG_OPEN, PG_M_NCW, PG_M_FLAGS, PG_M_ADDR, PG_M_COUNTS, PG_NMSGS,
       PG_NBAD, PG_TBLOCKS, PG_HIST = 16, PG_MSG = PG_HIST + MAX_WINDOW, PG_RING = PG_MSG + SLOT_WORDS, POCSAG_WORDS = PG_RING + RING * SLOT_WORDS };
static_assert(POCSAG_WORDS == 456, "the state layout of include/rdsp.h");
constexpr uint32_t POCSAG_SYNC = 0x7CD215D8u, POCSAG_IDLE = 0x7A89C197u, POCSAG_POLY = 0x769u;
constexpr int POCSAG_DEFAULT_INVERT = 2, POCSAG_DEFAULT_PULL = 3, POCSAG_DEFAULT_SYNC_ERRS = 2, POCSAG_DEFAULT_FIX_ADDR = 1, POCSAG_DEFAULT_FIX_DATA = 2;
enum { PG_FLAG_CUT = 1, PG_FLAG_TRUNCATED = 2, PG_FLAG_UNCORRECTABLE = 4 };
constexpr uint32_t PG_WORD_BAD = 0x80000000u;
constexpr uint16_t PG_NO_PATTERN = 0xFFFFu;

/* a group's settings (rdsp_engine_set_pocsag) */
struct PocsagSet {
  int baud, invert, pull, sync_errs, fix_addr, fix_data;
};
/* what the kernel is handed of them */
struct PocsagLaw {
  uint32_t baud, window, invert, pull, sync_errs, fix_addr, fix_data, step;
  float lscale, dscale;
};

inline bool pocsag_ok(int baud, int invert, int pull, int sync_errs, int fix_addr, int fix_data) {
  return (baud == 0 || baud == 512 || baud == 1200 || baud == 2400) && invert >= 0 && invert <= 2 && pull >= 1 && pull <= 4 && sync_errs >= 0 &&
         sync_errs <= 3 && fix_addr >= 0 && fix_addr <= 2 && fix_data >= 0 && fix_data <= 2;
}
inline int pocsag_window(int baud) { return baud == 512 ? 20 : baud == 1200 ? 8 : 4; }
/* host only, libm-free but for the rounding: the clock's step per DECIMATED sample */
inline uint32_t pocsag_step(int baud) { return (uint32_t)(unsigned long long)llround((double)baud * 4294967296.0 * (double)DEC / 44100.0); }
inline PocsagLaw pocsag_law(const PocsagSet &s) {
  PocsagLaw l;
  l.baud = (uint32_t)s.baud; l.window = (uint32_t)pocsag_window(s.baud); l.invert = (uint32_t)s.invert; l.pull = (uint32_t)s.pull;
  l.sync_errs = (uint32_t)s.sync_errs; l.fix_addr = (uint32_t)s.fix_addr; l.fix_data = (uint32_t)s.fix_data;
  l.step = pocsag_step(s.baud);
  l.lscale = (float)(1.0 / (32.0 * 4.0 * (double)l.window)); l.dscale = (float)(1.0 / 128.0);
  return l;
}

/* ---- stage 2: one window.  p: the window's samples, oldest first ---- */
template <int W, typename P>
RDSP_HD float pocsag_sum(P p) {
  static_assert(W % 4 == 0 && W >= 4 && W <= MAX_WINDOW, "whole quads");
  float s = dtmf_quad(p[0], p[1], p[2], p[3]);
#pragma unroll
  for (int q = 1; q < W / 4; q++) s = s + dtmf_quad(p[4 * q], p[4 * q + 1], p[4 * q + 2], p[4 * q + 3]);
  return s;
}
/* newest: the window's newest sample; the W - 1 before it lie below it */
template <typename P>
RDSP_HD float pocsag_window_sum(P newest, uint32_t window) {
  return window == 20u ? pocsag_sum<20>(newest - 19) : window == 8u ? pocsag_sum<8>(newest - 7) : pocsag_sum<4>(newest - 3);
}
RDSP_HD bool pocsag_raw(float S) { return S < 0.0f; }

/* ---- stage 5: BCH(31,21) and the parity bit ---- */
RDSP_HD constexpr uint32_t pocsag_popcount(uint32_t v) {
  v = v - ((v >> 1) & 0x55555555u);
  v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
  return (((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24;
}
/* the remainder of bits 31 ... 1 by x^10 + x^9 + x^8 + x^6 + x^5 + x^3 + 1 */
RDSP_HD constexpr uint32_t pocsag_syndrome(uint32_t word) {
  uint32_t r = word >> 1;
  for (int i = 30; i >= 10; i--)
    if (r & (1u << i)) r ^= POCSAG_POLY << (i - 10);
  return r & 0x3FFu;
}
/* the codeword of 21 data bits: data, the BCH remainder, even parity */
RDSP_HD constexpr uint32_t pocsag_codeword(uint32_t data21) {
  const uint32_t d = (data21 & 0x1FFFFFu) << 11;
  const uint32_t w = d | pocsag_syndrome(d) << 1;
  return w | (pocsag_popcount(w) & 1u);
}
/* entry [syndrome]: b1 | b2 << 5 | ne << 10, b the word's bit (1 ... 31) to flip, 0 for none; PG_NO_PATTERN where no pattern of
 * weight <= 2 has the syndrome */
struct PocsagTable {
  uint16_t e[1024];
};
constexpr PocsagTable pocsag_make_table() {
  PocsagTable t{};
  for (int k = 0; k < 1024; k++) t.e[k] = PG_NO_PATTERN;
  t.e[0] = 0;
  for (uint32_t b1 = 1; b1 < 32; b1++) {
    t.e[pocsag_syndrome(1u << b1)] = (uint16_t)(b1 | 1u << 10);
    for (uint32_t b2 = b1 + 1; b2 < 32; b2++) t.e[pocsag_syndrome(1u << b1 | 1u << b2)] = (uint16_t)(b1 | b2 << 5 | 2u << 10);
  }
  return t;
}
/* word as received -> the corrected word and ne in *ne; false: uncorrectable, or more errors than fix_addr / fix_data allows */
template <typename T>
RDSP_HD bool pocsag_correct(T tab, uint32_t word, uint32_t fix_addr, uint32_t fix_data, uint32_t &fixed, uint32_t &ne) {
  const uint32_t e = tab[pocsag_syndrome(word)];
  fixed = word; ne = 0u;
  if (e == PG_NO_PATTERN) return false;
  const uint32_t b1 = e & 31u, b2 = (e >> 5) & 31u;
  if (b1) fixed ^= 1u << b1;
  if (b2) fixed ^= 1u << b2;
  ne = e >> 10;
  if (pocsag_popcount(fixed) & 1u) { fixed ^= 1u; ne += 1u; }
  return ne <= ((fixed >> 31) ? fix_data : fix_addr);
}

/* ---- stages 4 and 6: the integers ---- */
struct PocsagBits {
  uint32_t pll, prev_raw, sr, insync, pol, nbits, ncw, open, m_ncw, m_flags, m_addr, m_counts, n_msgs, n_bad, t_blocks;
};
/* what one bit did: closed -- a message was closed, its header in head/addr/counts, its words in msg (the caller puts it into
 * the ring and counts n_msgs); bad -- an uncorrectable codeword (n_bad is counted here) */
struct PocsagEvent {
  uint32_t closed, bad, head, addr, counts;
};
RDSP_HD void pocsag_close(PocsagBits &s, PocsagEvent &ev, uint32_t flag) {
  if (!s.open) return;
  ev.closed = 1u;
  ev.head = s.m_ncw | (s.m_flags | flag) << 8 | s.pol << 16;
  ev.addr = s.m_addr; ev.counts = s.m_counts;
  s.open = 0u; s.m_ncw = 0u; s.m_flags = 0u; s.m_addr = 0u; s.m_counts = 0u;
}
template <typename M>
RDSP_HD void pocsag_append(PocsagBits &s, M msg, uint32_t w) {
  if (s.m_ncw < (uint32_t)MSG_MAX) {
    msg[s.m_ncw] = w;
    s.m_ncw += 1u;
    if (w & PG_WORD_BAD) { s.m_flags |= (uint32_t)PG_FLAG_UNCORRECTABLE; s.m_counts += 1u << 16; }
    else s.m_counts += w >> 24;
  } else {
    s.m_flags |= (uint32_t)PG_FLAG_TRUNCATED;
  }
}
/* one sampled bit: msg the open message's MSG_MAX words, tab the table's entries */
template <typename M, typename T>
RDSP_HD PocsagEvent pocsag_bit(PocsagBits &s, M msg, T tab, uint32_t bit, const PocsagLaw &law) {
  PocsagEvent ev{0u, 0u, 0u, 0u, 0u};
  s.sr = s.sr << 1 | (bit & 1u);
  if (!s.insync) {
    const bool plain = law.invert != 1u && pocsag_popcount(s.sr ^ POCSAG_SYNC) <= law.sync_errs;
    const bool inverted = law.invert != 0u && pocsag_popcount(~s.sr ^ POCSAG_SYNC) <= law.sync_errs;
    if (plain || inverted) { s.insync = 1u; s.pol = plain ? 0u : 1u; s.nbits = 0u; s.ncw = 0u; }
    return ev;
  }
  s.nbits += 1u;
  if (s.nbits < 32u) return ev;
  s.nbits = 0u;
  const uint32_t word = s.pol ? ~s.sr : s.sr;
  if (s.ncw == (uint32_t)BATCH) { /* the next batch's sync word, or the end */
    if (pocsag_popcount(word ^ POCSAG_SYNC) <= law.sync_errs) { s.ncw = 0u; }
    else { pocsag_close(s, ev, (uint32_t)PG_FLAG_CUT); s.insync = 0u; s.ncw = 0u; }
    return ev;
  }
  uint32_t fixed, ne;
  if (!pocsag_correct(tab, word, law.fix_addr, law.fix_data, fixed, ne)) {
    s.n_bad += 1u; ev.bad = 1u;
    if (s.open) pocsag_append(s, msg, ((word >> 11) & 0xFFFFFu) | PG_WORD_BAD);
  } else if (fixed >> 31) {
    if (s.open) pocsag_append(s, msg, ((fixed >> 11) & 0xFFFFFu) | ne << 24);
  } else {
    pocsag_close(s, ev, 0u);
    if (fixed != POCSAG_IDLE) {
      s.open = 1u;
      s.m_addr = ((fixed >> 13) & 0x3FFFFu) << 3 | s.ncw >> 1 | ((fixed >> 11) & 3u) << 21;
      s.m_counts = ne;
    }
  }
  s.ncw += 1u;
  return ev;
}
/* word k = 0 ... 83 of a ring slot (msgw: word k - 4 of the message) */
RDSP_HD uint32_t pocsag_ring_word(int k, const PocsagEvent &ev, uint32_t t_blocks, uint32_t msgw) {
  if (k == 0) return ev.head;
  if (k == 1) return t_blocks;
  if (k == 2) return ev.addr;
  if (k == 3) return ev.counts;
  return (uint32_t)(k - MSG_HEAD) < (ev.head & 0xFFu) ? msgw : 0u;
}
/* the pairwise tree over a block's 32 values */
inline float pocsag_tree32(const float *v) {
  float t[PER_BLOCK];
  memcpy(t, v, sizeof t);
  for (int n = PER_BLOCK; n > 1; n /= 2)
    for (int k = 0; k < n / 2; k++) t[k] = t[2 * k] + t[2 * k + 1];
  return t[0];
}
inline const PocsagTable &pocsag_table() {
  static constexpr PocsagTable t = pocsag_make_table();
  return t;
}

/* a channel's detector on the host: its 456 words */
struct PocsagState {
  uint32_t baud;
  PocsagBits s;
  float hist[MAX_WINDOW]; /* hist[19] stays 0 */
  uint32_t msg[SLOT_WORDS]; /* the first MSG_HEAD stay 0 */
  uint32_t ring[RING][SLOT_WORDS];
};
inline void pocsag_load(PocsagState &q, const uint32_t *w) {
  q.baud = w[PG_BAUD];
  q.s = {w[PG_PLL], w[PG_PREV_RAW], w[PG_SR], w[PG_INSYNC], w[PG_POL], w[PG_NBITS], w[PG_NCW], w[PG_OPEN], w[PG_M_NCW], w[PG_M_FLAGS], w[PG_M_ADDR],
         w[PG_M_COUNTS], w[PG_NMSGS], w[PG_NBAD], w[PG_TBLOCKS]};
  memcpy(q.hist, &w[PG_HIST], sizeof q.hist);
  memcpy(q.msg, &w[PG_MSG], sizeof q.msg);
  memcpy(q.ring, &w[PG_RING], sizeof q.ring);
}
inline void pocsag_store(const PocsagState &q, uint32_t *w) {
  const PocsagBits &s = q.s;
  w[PG_BAUD] = q.baud; w[PG_PLL] = s.pll; w[PG_PREV_RAW] = s.prev_raw; w[PG_SR] = s.sr; w[PG_INSYNC] = s.insync; w[PG_POL] = s.pol; w[PG_NBITS] = s.nbits;
  w[PG_NCW] = s.ncw; w[PG_OPEN] = s.open; w[PG_M_NCW] = s.m_ncw; w[PG_M_FLAGS] = s.m_flags; w[PG_M_ADDR] = s.m_addr; w[PG_M_COUNTS] = s.m_counts;
  w[PG_NMSGS] = s.n_msgs; w[PG_NBAD] = s.n_bad; w[PG_TBLOCKS] = s.t_blocks;
  memcpy(&w[PG_HIST], q.hist, sizeof q.hist);
  memcpy(&w[PG_MSG], q.msg, sizeof q.msg);
  memcpy(&w[PG_RING], q.ring, sizeof q.ring);
}
/* the detector a call begins with: zeros behind a reset or another baud */
inline void pocsag_start(PocsagState &q, uint32_t baud, bool reset) {
  if (reset || q.baud != baud) memset(&q, 0, sizeof q);
  q.baud = baud;
}
/* the plain loop, which is the definition: n_blocks blocks of a behind the channel's words -> the records of the call, the
 * words renewed */
inline void pocsag_reference(const PocsagLaw &law, bool reset, uint32_t *words /* [POCSAG_WORDS] */, const float *a, int n_blocks, uint8_t *sync_rec,
                             uint8_t *new_rec, uint8_t *bad_rec, float *lvl_rec, float *dc_rec) {
  PocsagState q;
  pocsag_load(q, words);
  pocsag_start(q, law.baud, reset);
  PocsagBits &s = q.s;
  const uint16_t *tab = pocsag_table().e;
  for (int b = 0; b < n_blocks; b++) {
    const float *x = a + (size_t)b * BLOCK;
    float lvl[PER_BLOCK], dc[PER_BLOCK];
    uint32_t fresh = 0u, bad = 0u;
    for (int r = 0; r < PER_BLOCK; r++) {
      float win[MAX_WINDOW];
      memcpy(win, q.hist, HIST * sizeof(float));
      const float d = dtmf_quad(x[4 * r], x[4 * r + 1], x[4 * r + 2], x[4 * r + 3]);
      win[HIST] = d;
      memcpy(q.hist, win + 1, HIST * sizeof(float));
      const float S = pocsag_window_sum((const float *)win + HIST, law.window);
      lvl[r] = fabsf(S);
      dc[r] = d;
      const uint32_t raw = pocsag_raw(S) ? 1u : 0u;
      if (raw != s.prev_raw) { s.pll = afsk_pulled(s.pll, law.pull); s.prev_raw = raw; }
      if (afsk_clock(s.pll, law.step, 1u)) {
        const PocsagEvent ev = pocsag_bit(s, q.msg + MSG_HEAD, tab, raw, law);
        if (ev.closed) {
          uint32_t *slot = q.ring[s.n_msgs % RING];
          for (int k = 0; k < SLOT_WORDS; k++) slot[k] = pocsag_ring_word(k, ev, s.t_blocks + 1u, q.msg[k]);
          s.n_msgs += 1u;
          fresh += 1u;
        }
        bad += ev.bad;
      }
    }
    s.t_blocks += 1u;
    sync_rec[b] = (uint8_t)s.insync;
    new_rec[b] = (uint8_t)fresh;
    bad_rec[b] = (uint8_t)(bad < 255u ? bad : 255u);
    lvl_rec[b] = pocsag_tree32(lvl) * law.lscale;
    dc_rec[b] = pocsag_tree32(dc) * law.dscale;
  }
  pocsag_store(q, words);
}

}  // namespace rdsp_pocsag

#endif
