/*
 * rdsp_dtmf.h -- the arithmetic of rdsp_engine_t's DTMF decoder (include/rdsp.h has the definition), shared by the kernel
 * (rdsp_engine_dtmf.hip), the host entry points (rdsp_engine_dtmf_host.hip) and the host program of the tests
 * (tests/host/host_dtmf_check.cpp).  Compile with -ffp-contract=off: every product and sum below is rounded on its own, the
 * fused operations are written as fmaf.
 *
 * Per channel, a[n] the receiver's "demod" tap (rdsp_fm.h's y[n]), blocks of 128 samples counted from the detector's start:
 *   tones    t = 0 ... 3: 697, 770, 852, 941 Hz (the low group), t = 4 ... 7: 1209, 1336, 1477, 1633 Hz (the high group)
 *   dphi_t = (uint32) llround(f_t 2^32 4 / 44100.0)                       the step per DECIMATED sample
 *   d[b][r], r = 0 ... 31: (a0 + a1) + (a2 + a3) over a[128 b + 4 r ... + 3] (search_quad's order); 11 025 Hz
 *   sub-chain j = 0 ... 7 of tone t takes r = 4 j ... 4 j + 3 of every block of a frame of K blocks, blocks ascending, r
 *     ascending in a block: m = 32 cnt + r; (c, s) = tune_phasor(tab, m dphi_t); re_tj = fmaf(d, c, re_tj), im_tj = fmaf(d, s,
 *     im_tj); beside them the energy chains e_j = fmaf(d, d, e_j)
 *   cnt += 1; cnt == K: RE_t, IM_t, E' the sums over j by the tree ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7));
 *     P_t = fmaf(RE_t, RE_t, IM_t IM_t) scale, scale = (float)(1 / (64 K)^2); E = E' (float)(1 / (256 K));
 *     per group i = the lowest index of the largest P, second = the largest of the other three; the symbol (dtmf_symbol);
 *     the digit logic (dtmf_digit); every chain and cnt to 0
 * A channel's state is DTMF_WORDS = 168 words: K, cnt, last1, run, cur1, miss, n_digits, t_blocks, P_L, P_H, six zeros, ring[16],
 * re[64], im[64] (chain 8 t + j), e[8].  last1 and cur1 are last + 1 and cur + 1 modulo 256, so that zeros are a detector that
 * has seen and holds no key (255).  A detector whose stored K is not the one it is run with starts from zeros (dtmf_start).
 */
#ifndef RDSP_DTMF_H
#define RDSP_DTMF_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rdsp_tune.h"

namespace rdsp_dtmf {

constexpr int BLOCK = 128, DEC = 4, PER_BLOCK = BLOCK / DEC;   /* 32 decimated samples a block */
constexpr int TONES = 8, SUBS = 8, PER_SUB = PER_BLOCK / SUBS; /* a sub-chain takes 4 of them */
constexpr int CHAINS = TONES * SUBS, RING = 16;
constexpr int DTMF_MIN_K = 4, DTMF_MAX_K = 32, DTMF_MAX_FRAMES = 16;
enum { DT_K = 0, DT_CNT, DT_LAST1, DT_RUN, DT_CUR1, DT_MISS, DT_NDIGITS, DT_TBLOCKS, DT_PL, DT_PH, DT_RING = 16, DT_RE = DT_RING + RING,
       DT_IM = DT_RE + CHAINS, DT_E = DT_IM + CHAINS, DTMF_WORDS = DT_E + SUBS };
constexpr float DTMF_DEFAULT_MIN = 0.015f, DTMF_DEFAULT_RATIO = 4.0f, DTMF_DEFAULT_TWIST = 16.0f, DTMF_DEFAULT_SHARE = 0.5f, DTMF_MAX_RATIO = 1e6f;
constexpr int DTMF_DEFAULT_ON = 2, DTMF_DEFAULT_OFF = 2;
constexpr uint32_t DTMF_NONE = 255u;
constexpr float DTMF_HZ[TONES] = {697.0f, 770.0f, 852.0f, 941.0f, 1209.0f, 1336.0f, 1477.0f, 1633.0f};
constexpr char DTMF_KEYS[17] = "123A456B789C*0#D";

/* a group's settings (rdsp_engine_set_dtmf); K == 0: off */
struct DtmfSet {
  int K;
  float min_amp, ratio, twist, share;
  int on_frames, off_frames;
};
/* what the kernel is handed of them */
struct DtmfLaw {
  uint32_t K, on_frames, off_frames;
  float scale, escale, min2, ratio, twist, share;
  uint32_t dphi[TONES];
};

/* the setter's limits (a NaN fails every comparison) */
inline bool dtmf_ok(int K, float min_amp, float ratio, float twist, float share, int on_frames, int off_frames) {
  return (K == 0 || (K >= DTMF_MIN_K && K <= DTMF_MAX_K)) && min_amp > 0.0f && min_amp <= 1.0f && ratio >= 1.0f && ratio <= DTMF_MAX_RATIO &&
         twist >= 1.0f && twist <= DTMF_MAX_RATIO && share > 0.0f && share <= 1.0f && on_frames >= 1 && on_frames <= DTMF_MAX_FRAMES &&
         off_frames >= 1 && off_frames <= DTMF_MAX_FRAMES;
}
/* host only, libm-free but for the rounding: every host and numpy compute the same bits */
inline uint32_t dtmf_dphi(int t) { return (uint32_t)(unsigned long long)llround((double)DTMF_HZ[t] * 4294967296.0 * (double)DEC / rdsp_tune::TUNE_FS); }
inline float dtmf_scale(int K) { return (float)(1.0 / ((64.0 * (double)K) * (64.0 * (double)K))); }
inline float dtmf_escale(int K) { return (float)(1.0 / (256.0 * (double)K)); }
inline DtmfLaw dtmf_law(const DtmfSet &s) {
  DtmfLaw l;
  l.K = (uint32_t)s.K; l.on_frames = (uint32_t)s.on_frames; l.off_frames = (uint32_t)s.off_frames;
  l.scale = s.K > 0 ? dtmf_scale(s.K) : 0.0f; l.escale = s.K > 0 ? dtmf_escale(s.K) : 0.0f;
  l.min2 = s.min_amp * s.min_amp; l.ratio = s.ratio; l.twist = s.twist; l.share = s.share;
  for (int t = 0; t < TONES; t++) l.dphi[t] = dtmf_dphi(t);
  return l;
}
/* host only: what the boxcar of 4 samples leaves of a sinusoid at hz, relative to its gain of 4 at 0 Hz */
inline double dtmf_boxcar_gain(float hz) {
  const double w = 3.141592653589793 * (double)hz / rdsp_tune::TUNE_FS;
  return fabs(sin((double)DEC * w) / ((double)DEC * sin(w)));
}
inline char dtmf_key(int sym) { return sym >= 0 && sym < 16 ? DTMF_KEYS[sym] : (char)0; }

/* a decimated sample: the tone search's levels 1 and 2 */
RDSP_HD float dtmf_quad(float a0, float a1, float a2, float a3) { return (a0 + a1) + (a2 + a3); }
/* one decimated sample into one sub-chain; ph = m dphi_t */
RDSP_HD void dtmf_mac(const float4 *tab, uint32_t ph, float d, float &re, float &im) {
  const float2 e = rdsp_tune::tune_phasor(tab, ph);
  re = fmaf(d, e.x, re);
  im = fmaf(d, e.y, im);
}
RDSP_HD float dtmf_power(float re, float im, float scale) { return fmaf(re, re, im * im) * scale; }
/* the order of a group's arg-max: does (Pb, b) beat (Pa, a)?  The larger power, the lower index on a tie */
RDSP_HD bool dtmf_beats(float Pb, int b, float Pa, int a) { return Pb > Pa || (Pb == Pa && b < a); }
/* the frame's symbol: iL of 0 ... 3, iH of 4 ... 7; every product a rounded float */
RDSP_HD uint32_t dtmf_symbol(float PL, int iL, float secL, float PH, int iH, float secH, float E, const DtmfLaw &law) {
  const bool ok = PL >= law.min2 && PH >= law.min2 && PL >= law.ratio * secL && PH >= law.ratio * secH && PL <= law.twist * PH &&
                  PH <= law.twist * PL && PL + PH >= law.share * E;
  return ok ? (uint32_t)(4 * iL + (iH - 4)) : DTMF_NONE;
}
/* the digit logic's words; last and cur as symbols (255: none) */
struct DtmfDigit {
  uint32_t last, run, cur, miss, n_digits, t_blocks;
};
/* once per frame with the frame's symbol s: the symbol emitted, or 255; an emitted digit is ring[(n_digits - 1) mod 16]'s */
RDSP_HD uint32_t dtmf_digit(DtmfDigit &g, uint32_t s, const DtmfLaw &law) {
  g.run = (s != DTMF_NONE && s == g.last) ? g.run + 1u : (s != DTMF_NONE ? 1u : 0u);
  g.last = s;
  if (g.cur != DTMF_NONE) {
    if (s == g.cur) g.miss = 0u;
    else if (++g.miss >= law.off_frames) g.cur = DTMF_NONE;
  }
  if (g.cur == DTMF_NONE && g.run >= law.on_frames) {
    g.cur = s; g.miss = 0u; g.n_digits += 1u;
    return s;
  }
  return DTMF_NONE;
}
RDSP_HD uint32_t dtmf_ring_word(uint32_t sym, uint32_t t_blocks) { return sym | (t_blocks & 0xFFFFFFu) << 8; }
/* last / cur <-> the stored words */
RDSP_HD uint32_t dtmf_plus1(uint32_t sym) { return (sym + 1u) & 0xFFu; }
RDSP_HD uint32_t dtmf_minus1(uint32_t w) { return (w - 1u) & 0xFFu; }

/* a channel's detector on the host: its 168 words */
struct DtmfState {
  uint32_t K, cnt;
  DtmfDigit g;
  float PL, PH;
  uint32_t ring[RING];
  float re[CHAINS], im[CHAINS], e[SUBS];
};
inline void dtmf_load(DtmfState &s, const uint32_t *w) {
  s.K = w[DT_K]; s.cnt = w[DT_CNT];
  s.g = {dtmf_minus1(w[DT_LAST1]), w[DT_RUN], dtmf_minus1(w[DT_CUR1]), w[DT_MISS], w[DT_NDIGITS], w[DT_TBLOCKS]};
  memcpy(&s.PL, &w[DT_PL], 4); memcpy(&s.PH, &w[DT_PH], 4);
  memcpy(s.ring, &w[DT_RING], sizeof s.ring);
  memcpy(s.re, &w[DT_RE], sizeof s.re); memcpy(s.im, &w[DT_IM], sizeof s.im); memcpy(s.e, &w[DT_E], sizeof s.e);
}
inline void dtmf_store(const DtmfState &s, uint32_t *w) {
  memset(w, 0, DTMF_WORDS * 4);
  w[DT_K] = s.K; w[DT_CNT] = s.cnt; w[DT_LAST1] = dtmf_plus1(s.g.last); w[DT_RUN] = s.g.run; w[DT_CUR1] = dtmf_plus1(s.g.cur);
  w[DT_MISS] = s.g.miss; w[DT_NDIGITS] = s.g.n_digits; w[DT_TBLOCKS] = s.g.t_blocks;
  memcpy(&w[DT_PL], &s.PL, 4); memcpy(&w[DT_PH], &s.PH, 4);
  memcpy(&w[DT_RING], s.ring, sizeof s.ring);
  memcpy(&w[DT_RE], s.re, sizeof s.re); memcpy(&w[DT_IM], s.im, sizeof s.im); memcpy(&w[DT_E], s.e, sizeof s.e);
}
/* the detector a call begins with: zeros behind a reset or another K */
inline void dtmf_start(DtmfState &s, uint32_t K, bool reset) {
  if (reset || s.K != K) {
    memset(&s, 0, sizeof s);
    s.g.last = s.g.cur = DTMF_NONE;
  }
  s.K = K;
}
inline float dtmf_tree8(const float *v) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }
/* the end of a frame on the host: the powers, the symbol, the digit logic; the chains and cnt to 0.  Returns the symbol emitted */
inline uint32_t dtmf_frame(DtmfState &s, const DtmfLaw &law) {
  float P[TONES];
  for (int t = 0; t < TONES; t++) P[t] = dtmf_power(dtmf_tree8(s.re + SUBS * t), dtmf_tree8(s.im + SUBS * t), law.scale);
  const float E = dtmf_tree8(s.e) * law.escale;
  int i[2];
  float sec[2];
  for (int g = 0; g < 2; g++) {
    i[g] = 4 * g;
    for (int t = 4 * g + 1; t < 4 * g + 4; t++)
      if (dtmf_beats(P[t], t, P[i[g]], i[g])) i[g] = t;
    sec[g] = 0.0f;
    for (int t = 4 * g; t < 4 * g + 4; t++)
      if (t != i[g] && P[t] > sec[g]) sec[g] = P[t];
  }
  s.PL = P[i[0]]; s.PH = P[i[1]];
  const uint32_t sym = dtmf_symbol(s.PL, i[0], sec[0], s.PH, i[1], sec[1], E, law);
  const uint32_t out = dtmf_digit(s.g, sym, law);
  if (out != DTMF_NONE) s.ring[(s.g.n_digits - 1u) % RING] = dtmf_ring_word(out, s.g.t_blocks);
  s.cnt = 0u;
  memset(s.re, 0, sizeof s.re); memset(s.im, 0, sizeof s.im); memset(s.e, 0, sizeof s.e);
  return out;
}
/* the plain loop: n_blocks blocks of a behind the channel's words -> the records of the call, the words renewed (law.K > 0) */
inline void dtmf_reference(const float4 *tab, const DtmfLaw &law, bool reset, uint32_t *words /* [DTMF_WORDS] */, const float *a, int n_blocks,
                           uint8_t *key_rec, uint8_t *new_rec, float *lo_rec, float *hi_rec) {
  DtmfState s;
  dtmf_load(s, words);
  dtmf_start(s, law.K, reset);
  for (int b = 0; b < n_blocks; b++) {
    const float *x = a + (size_t)b * BLOCK;
    for (int r = 0; r < PER_BLOCK; r++) {
      const float d = dtmf_quad(x[4 * r], x[4 * r + 1], x[4 * r + 2], x[4 * r + 3]);
      const uint32_t m = (uint32_t)PER_BLOCK * s.cnt + (uint32_t)r;
      const int j = r / PER_SUB;
      for (int t = 0; t < TONES; t++) dtmf_mac(tab, m * law.dphi[t], d, s.re[SUBS * t + j], s.im[SUBS * t + j]);
      s.e[j] = fmaf(d, d, s.e[j]);
    }
    s.cnt += 1u;
    s.g.t_blocks += 1u;
    const uint32_t out = s.cnt == law.K ? dtmf_frame(s, law) : DTMF_NONE;
    key_rec[b] = (uint8_t)s.g.cur;
    new_rec[b] = (uint8_t)out;
    lo_rec[b] = s.PL;
    hi_rec[b] = s.PH;
  }
  dtmf_store(s, words);
}

}  // namespace rdsp_dtmf

#endif
