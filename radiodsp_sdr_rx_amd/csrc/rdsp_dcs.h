/*
 * rdsp_dcs.h -- the arithmetic of rdsp_engine_t's DCS code squelch (include/rdsp.h has the definition), shared by the kernel
 * (rdsp_engine_dcs.hip), the host entry points (rdsp_engine_dcs_host.hip) and the host program of the tests
 * (tests/host/host_dcs_check.cpp).  Compile with -ffp-contract=off: every sum below is rounded on its own.
 *
 * Code words (host only): data = 0x800 | code, parity = data x^11 mod g, g = x^11 + x^10 + x^6 + x^5 + x^4 + x^2 + 1 (0xC75),
 * word = parity << 12 | data, sent LSB first, a 1 above the demod tap's mean; the inverted code is word ^ 0x7FFFFF.
 *
 * Per channel, a[n] the receiver's "demod" tap (rdsp_fm.h's y[n]), blocks of 128 samples counted from the detector's last reset:
 *   d[b][q], q = 0 ... 3: rdsp_tone_search.h's search_dec, the sum of 32 samples by the meter's tree
 *   step = (uint32) llround(134.4 32 2^32 / 44100.0); ms = M step (uint32, wraps), M the decimated values since the reset
 *   eight hypotheses p with the bit phase bp_p = p 2^29 + ms.  For every decimated value v in order: acc_p = acc_p + v for all p;
 *   ms += step; the p whose bp_p wrapped ticks (dcs_tick: at most one):
 *     ring_p[pos_p] = acc_p, pos_p = (pos_p + 1) mod 23, acc_p = 0, nb_p = min(nb_p + 1, 23)
 *     thr = (ring_p[0] + ... + ring_p[22]) (float)(1 / 23), the sum left to right (dcs_thr)
 *     w bit j = ring_p[(pos_p + j) mod 23] > thr                          j = 0: the oldest bit, the word's LSB
 *     nb_p == 23: a code matches when min over r of popcount(w ^ rot(want, r)) <= max_err, matched = canon(want);
 *                 ANY matches when parity(w & 0xFFF) == w >> 12 and some rot(w, r) has bits 9 ... 11 == 100, matched = canon(w)
 *                 (canon: the smallest of the 23 rotations); a match: hits_p += 1, last_p = matched
 *   after a block cnt += 1; cnt == K: best = the lowest p of the largest hits_p, H = hits_best,
 *     dcs = H >= (dcs ? off_hits : on_hits), word = H ? last_best : 0; every hits_p, last_p and cnt go to 0
 *
 * A channel's state is DCS_WORDS = 232 words: key, K, cnt, dcs, H, word, ms, 0, then per hypothesis acc, pos, nb, hits, last,
 * ring[23] (acc and ring floats).  key = 2^31 | ANY 2^30 | inverted 2^29 | max_err 2^24 | want (want: the wanted word as it is
 * looked for, inverted if asked; 0 for ANY).  A detector whose stored key or K is not the one it is run with starts from zeros.
 */
#ifndef RDSP_DCS_H
#define RDSP_DCS_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rdsp_tone_search.h"

namespace rdsp_dcs {

constexpr int BLOCK = 128, DEC = 32, PER_BLOCK = BLOCK / DEC;
constexpr int HYP = 8, BITS = 23;
constexpr uint32_t WORD_MASK = 0x7FFFFFu, GOLAY = 0xC75u;
enum { DC_KEY = 0, DC_K, DC_CNT, DC_DCS, DC_H, DC_WORD, DC_MS, DC_HYP = 8 };
enum { DH_ACC = 0, DH_POS, DH_NB, DH_HITS, DH_LAST, DH_RING, HYP_WORDS = DH_RING + BITS };
constexpr int DCS_WORDS = DC_HYP + HYP * HYP_WORDS;
constexpr uint16_t DCS_ANY = 0xFFFFu, DCS_INVERTED = 0x8000u;
constexpr int DCS_MAX_CODE = 511, STANDARD_CODES = 104;
constexpr uint32_t KEY_SET = 1u << 31, KEY_ANY = 1u << 30, KEY_INVERTED = 1u << 29;
constexpr int KEY_ERR_SHIFT = 24;
constexpr int DCS_MIN_K = 8, DCS_MAX_K = 512, DCS_MAX_ERR = 3;
constexpr int DCS_DEFAULT_K = 64, DCS_DEFAULT_ERR = 1, DCS_DEFAULT_ON = 16, DCS_DEFAULT_OFF = 12;

/* the 104 standard codes, the octal digits read as a number */
constexpr uint16_t STANDARD[STANDARD_CODES] = {
    0023, 0025, 0026, 0031, 0032, 0036, 0043, 0047, 0051, 0053, 0054, 0065, 0071, 0072, 0073, 0074, 0114, 0115, 0116, 0122, 0125,
    0131, 0132, 0134, 0143, 0145, 0152, 0155, 0156, 0162, 0165, 0172, 0174, 0205, 0212, 0223, 0225, 0226, 0243, 0244, 0245, 0246,
    0251, 0252, 0255, 0261, 0263, 0265, 0266, 0271, 0274, 0306, 0311, 0315, 0325, 0331, 0332, 0343, 0346, 0351, 0356, 0364, 0365,
    0371, 0411, 0412, 0413, 0423, 0431, 0432, 0445, 0446, 0452, 0454, 0455, 0462, 0464, 0465, 0466, 0503, 0506, 0516, 0523, 0526,
    0532, 0546, 0565, 0606, 0612, 0624, 0627, 0631, 0632, 0654, 0662, 0664, 0703, 0712, 0723, 0731, 0732, 0734, 0743, 0754};

/* a group's detector settings (rdsp_engine_set_dcs_squelch) */
struct DcsSet {
  int K, max_err, on_hits, off_hits;
};
/* what the kernel is handed of them */
struct DcsLaw {
  uint32_t K, max_err, on_hits, off_hits, step;
};

/* the rotations of a 23-bit word, r = 0 ... 22 */
RDSP_HD uint32_t dcs_rot(uint32_t w, int r) { return r ? ((w >> r) | (w << (BITS - r))) & WORD_MASK : w; }
/* the remainder of d x^11 by g, d of 12 bits */
RDSP_HD uint32_t dcs_parity(uint32_t d) {
  uint32_t r = d << 11;
  for (int i = 22; i >= 11; i--)
    if ((r >> i) & 1u) r ^= GOLAY << (i - 11);
  return r & 0x7FFu;
}
RDSP_HD uint32_t dcs_popcount(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
/* host: the smallest rotation */
inline uint32_t dcs_canon(uint32_t w) {
  uint32_t m = w;
  for (int r = 1; r < BITS; r++) m = dcs_rot(w, r) < m ? dcs_rot(w, r) : m;
  return m;
}
inline uint32_t dcs_codeword(int code) {
  const uint32_t data = 0x800u | (uint32_t)code;
  return dcs_parity(data) << 12 | data;
}

/* the setters' limits */
inline int dcs_max_hits(int K) { return K * 1024 / 2625; } /* K 128 134.4 / 44100 = K 1024 / 2625, rounded down */
inline bool code_ok(uint16_t c) { return c == DCS_ANY || ((c & 0x7FFFu) <= DCS_MAX_CODE && (c == 0 || (c & 0x7FFFu) != 0)); }
inline bool squelch_ok(int K, int max_err, int on_hits, int off_hits) {
  return K >= DCS_MIN_K && K <= DCS_MAX_K && max_err >= 0 && max_err <= DCS_MAX_ERR && off_hits >= 1 && off_hits <= on_hits &&
         on_hits <= dcs_max_hits(K);
}
/* host only */
inline uint32_t dcs_step() { return (uint32_t)(unsigned long long)llround(134.4 * 32.0 * 4294967296.0 / 44100.0); }
inline DcsLaw dcs_law(const DcsSet &s) { return {(uint32_t)s.K, (uint32_t)s.max_err, (uint32_t)s.on_hits, (uint32_t)s.off_hits, dcs_step()}; }
/* a channel's setting as the kernel reads it: 0 for none, else the key without max_err */
inline uint32_t dcs_sel(uint16_t c) {
  if (c == 0) return 0u;
  if (c == DCS_ANY) return KEY_SET | KEY_ANY;
  const uint32_t word = dcs_codeword(c & 0x7FFF);
  return (c & DCS_INVERTED) ? KEY_SET | KEY_INVERTED | (word ^ WORD_MASK) : KEY_SET | word;
}
RDSP_HD uint32_t dcs_key(uint32_t sel, uint32_t max_err) { return sel | max_err << KEY_ERR_SHIFT; }

/* ms already advanced by step: the hypothesis whose phase p 2^29 + ms wrapped, or -1 (step < 2^29: at most one) */
RDSP_HD int dcs_tick(uint32_t ms, uint32_t step) { return (ms & 0x1FFFFFFFu) < step ? (int)((8u - (ms >> 29)) & 7u) : -1; }
/* the slicing level of a ring */
RDSP_HD float dcs_thr(const float *ring) {
  float s = ring[0];
  for (int i = 1; i < BITS; i++) s = s + ring[i];
  return s * (float)(1.0 / 23.0);
}
/* rotation r of the tests a tick makes */
RDSP_HD bool dcs_code_rot(uint32_t w, uint32_t want, int r, uint32_t max_err) { return dcs_popcount(w ^ dcs_rot(want, r)) <= max_err; }
RDSP_HD bool dcs_any_word(uint32_t w) { return dcs_parity(w & 0xFFFu) == w >> 12; }
RDSP_HD bool dcs_any_rot(uint32_t w, int r) { return ((dcs_rot(w, r) >> 9) & 7u) == 4u; }
RDSP_HD uint32_t dcs_decide(uint32_t H, uint32_t dcs, const DcsLaw &law) { return H >= (dcs ? law.off_hits : law.on_hits) ? 1u : 0u; }

/* a channel's detector on the host: its 232 words */
struct DcsHyp {
  float acc;
  uint32_t pos, nb, hits, last;
  float ring[BITS];
};
struct DcsState {
  uint32_t key, K, cnt, dcs, H, word, ms, zero;
  DcsHyp h[HYP];
};
static_assert(sizeof(DcsState) == DCS_WORDS * 4, "the words of a channel");

/* host: a tick of hypothesis h -> the word matched or 0 is counted */
inline void dcs_tick_host(DcsHyp &h, uint32_t key, const DcsLaw &law) {
  h.ring[h.pos] = h.acc;
  h.pos = (h.pos + 1u) % BITS;
  h.acc = 0.0f;
  h.nb = h.nb + 1u < BITS ? h.nb + 1u : BITS;
  const float thr = dcs_thr(h.ring);
  uint32_t w = 0u;
  for (int j = 0; j < BITS; j++)
    if (h.ring[(h.pos + (uint32_t)j) % BITS] > thr) w |= 1u << j;
  if (h.nb != BITS) return;
  bool match = false;
  uint32_t matched = 0u;
  if (key & KEY_ANY) {
    if (dcs_any_word(w))
      for (int r = 0; r < BITS; r++) match = match || dcs_any_rot(w, r);
    matched = dcs_canon(w);
  } else {
    const uint32_t want = key & WORD_MASK;
    for (int r = 0; r < BITS; r++) match = match || dcs_code_rot(w, want, r, law.max_err);
    matched = dcs_canon(want);
  }
  if (match) { h.hits += 1u; h.last = matched; }
}
/* the plain loop: n_blocks blocks of a behind the channel's words -> the records of the call, the words renewed.  sel == 0: the
 * words and the records are zeros */
inline void dcs_reference(const DcsLaw &law, uint32_t sel, bool reset, uint32_t *words /* [DCS_WORDS] */, const float *a, int n_blocks,
                          uint8_t *dcs_rec, uint8_t *hits_rec, uint32_t *word_rec) {
  if (sel == 0u) {
    memset(words, 0, DCS_WORDS * 4);
    for (int b = 0; b < n_blocks; b++) { dcs_rec[b] = 0; hits_rec[b] = 0; word_rec[b] = 0u; }
    return;
  }
  DcsState s;
  memcpy(&s, words, sizeof s);
  const uint32_t key = dcs_key(sel, law.max_err);
  if (reset || s.key != key || s.K != law.K) memset(&s, 0, sizeof s);
  s.key = key; s.K = law.K;
  for (int b = 0; b < n_blocks; b++) {
    for (int q = 0; q < PER_BLOCK; q++) {
      const float v = rdsp_tone_search::search_dec(a + (size_t)b * BLOCK + (size_t)q * DEC);
      for (int p = 0; p < HYP; p++) s.h[p].acc = s.h[p].acc + v;
      s.ms += law.step;
      const int p = dcs_tick(s.ms, law.step);
      if (p >= 0) dcs_tick_host(s.h[p], key, law);
    }
    s.cnt += 1u;
    if (s.cnt == law.K) {
      int best = 0;
      for (int p = 1; p < HYP; p++)
        if (s.h[p].hits > s.h[best].hits) best = p;
      s.H = s.h[best].hits;
      s.dcs = dcs_decide(s.H, s.dcs, law);
      s.word = s.H ? s.h[best].last : 0u;
      for (int p = 0; p < HYP; p++) { s.h[p].hits = 0u; s.h[p].last = 0u; }
      s.cnt = 0u;
    }
    dcs_rec[b] = (uint8_t)s.dcs; hits_rec[b] = (uint8_t)s.H; word_rec[b] = s.word;
  }
  memcpy(words, &s, sizeof s);
}

}  // namespace rdsp_dcs

#endif
