/*
 * rdsp_tone_search.h -- the arithmetic of rdsp_engine_t's CTCSS tone search (include/rdsp.h has the definition), shared by the
 * kernel (rdsp_engine_tone_search.hip), the host entry points (rdsp_engine_tone_search_host.hip) and the host program of the
 * tests (tests/host/host_tone_search_check.cpp).  Compile with -ffp-contract=off: every product and sum below is rounded on its
 * own, the fused operations are written as fmaf.
 *
 * Per channel, a[n] the receiver's "demod" tap (rdsp_fm.h's y[n]), blocks of 128 samples counted from the detector's last reset:
 *   bank     n_tones frequencies in [60, 300] Hz, strictly ascending, 1 <= n_tones <= 64 (default: the 50 standard tones)
 *   dphi_t = (uint32) llround((double) tone_hz_t 2^32 32 / 44100.0)       the step per DECIMATED sample
 *   key    = FNV-1a (32 bits) over the little-endian bytes of n_tones and every dphi_t; 0 is replaced by 1
 *   d[b][q], q = 0 ... 3: the sum of a[128 b + 32 q ... + 31] by the meter's tree cut off after five levels (search_dec)
 *   m = 4 cnt + q; (c, s) = tune_phasor(tab, m dphi_t); re_t = fmaf(d, c, re_t), im_t = fmaf(d, s, im_t)  one chain per tone
 *   cnt += 1; cnt == K: P_t = fmaf(re_t, re_t, im_t im_t) scale (tone_scale of rdsp_tone.h); i = the lowest index of the largest
 *     P_t; next = the largest P_t over |t - i| > 1 (0 if none); found = P_i >= min2 && P_i >= ratio next;
 *     best1 = found ? i + 1 : 0, a2 = P_i; re = im = 0, cnt = 0
 * A wave computes d as the meter's tree: a lane adds its 4 consecutive samples as (a0 + a1) + (a2 + a3) (search_quad: levels 1
 * and 2), then 8 lanes exchange with strides 1, 2, 4 (levels 3 ... 5).
 *
 * A channel's state is SEARCH_WORDS = 200 words: K, key, cnt, best1, a2, next, 0, 0, then re[64], im[64], P[64] (floats but the
 * first four).  A detector whose stored K or key is not the one it is run with starts from zeros (search_start).
 */
#ifndef RDSP_TONE_SEARCH_H
#define RDSP_TONE_SEARCH_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rdsp_tone.h"
#include "rdsp_tune.h"

namespace rdsp_tone_search {

constexpr int BLOCK = 128, DEC = 32, PER_BLOCK = BLOCK / DEC;
constexpr int MAX_TONES = 64, STANDARD_TONES = 50;
enum { TS_K = 0, TS_KEY, TS_CNT, TS_BEST1, TS_A2, TS_NEXT, TS_RE = 8, TS_IM = TS_RE + MAX_TONES, TS_P = TS_IM + MAX_TONES, SEARCH_WORDS = TS_P + MAX_TONES };
constexpr float SEARCH_DEFAULT_MIN = 0.04f, SEARCH_DEFAULT_RATIO = 4.0f, SEARCH_MAX_RATIO = 1e6f;
constexpr uint8_t SEARCH_NONE = 255;

/* the 50 standard CTCSS tones, the EIA list */
constexpr float STANDARD_HZ[STANDARD_TONES] = {
    67.0f,  69.3f,  71.9f,  74.4f,  77.0f,  79.7f,  82.5f,  85.4f,  88.5f,  91.5f,  94.8f,  97.4f,  100.0f, 103.5f, 107.2f, 110.9f, 114.8f,
    118.8f, 123.0f, 127.3f, 131.8f, 136.5f, 141.3f, 146.2f, 151.4f, 156.7f, 159.8f, 162.2f, 165.5f, 167.9f, 171.3f, 173.8f, 177.3f, 179.9f,
    183.5f, 186.2f, 189.9f, 192.8f, 196.6f, 199.5f, 203.5f, 206.5f, 210.7f, 218.1f, 225.7f, 229.1f, 233.6f, 241.8f, 250.3f, 254.1f};

/* a group's settings (rdsp_engine_set_tone_search); K == 0: off */
struct SearchSet {
  int K;
  float min_amp, ratio;
};
/* what the kernel is handed of them */
struct SearchLaw {
  uint32_t K;
  float scale, min2, ratio;
};
/* the engine's bank as the kernel reads it: the steps (zeros from n_tones on) and its key */
struct SearchBank {
  uint32_t n_tones, key;
  uint32_t dphi[MAX_TONES];
};

/* the setters' limits (a NaN fails every comparison) */
inline bool search_ok(int K, float min_amp, float ratio) {
  return (K == 0 || (K >= rdsp_tone::TONE_MIN_K && K <= rdsp_tone::TONE_MAX_K)) && min_amp > 0.0f && min_amp <= 1.0f && ratio >= 1.0f &&
         ratio <= SEARCH_MAX_RATIO;
}
inline bool bank_ok(const float *hz, int n) {
  if (!hz || n < 1 || n > MAX_TONES) return false;
  for (int t = 0; t < n; t++)
    if (!(hz[t] >= rdsp_tone::TONE_MIN_HZ && hz[t] <= rdsp_tone::TONE_MAX_HZ) || (t > 0 && !(hz[t] > hz[t - 1]))) return false;
  return true;
}

/* host only, libm-free but for the rounding: every host and numpy compute the same bits */
inline uint32_t search_dphi(float tone_hz) {
  return (uint32_t)(unsigned long long)llround((double)tone_hz * 4294967296.0 * (double)DEC / rdsp_tune::TUNE_FS);
}
inline uint32_t fnv1a_word(uint32_t h, uint32_t w) {
  for (int k = 0; k < 4; k++) { h ^= (w >> (8 * k)) & 0xffu; h *= 16777619u; }
  return h;
}
inline SearchBank search_bank(const float *hz, int n) {
  SearchBank b;
  memset(&b, 0, sizeof b);
  b.n_tones = (uint32_t)n;
  uint32_t h = fnv1a_word(2166136261u, b.n_tones);
  for (int t = 0; t < n; t++) h = fnv1a_word(h, b.dphi[t] = search_dphi(hz[t]));
  b.key = h ? h : 1u;
  return b;
}
inline SearchLaw search_law(const SearchSet &s) {
  return {(uint32_t)s.K, s.K > 0 ? rdsp_tone::tone_scale(s.K) : 0.0f, s.min_amp * s.min_amp, s.ratio};
}
/* host only: what the boxcar of 32 samples leaves of a sinusoid at tone_hz, relative to its gain of 32 at 0 Hz */
inline double search_boxcar_gain(float tone_hz) {
  const double w = 3.141592653589793 * (double)tone_hz / rdsp_tune::TUNE_FS;
  return fabs(sin((double)DEC * w) / ((double)DEC * sin(w)));
}

/* levels 1 and 2 of the decimator's tree on a lane's four consecutive samples */
RDSP_HD float search_quad(float a0, float a1, float a2, float a3) { return (a0 + a1) + (a2 + a3); }
/* one decimated sample into one tone's chain; ph = m dphi */
RDSP_HD void search_mac(const float4 *tab, uint32_t ph, float d, float &re, float &im) {
  const float2 e = rdsp_tune::tune_phasor(tab, ph);
  re = fmaf(d, e.x, re);
  im = fmaf(d, e.y, im);
}
RDSP_HD float search_power(float re, float im, float scale) { return fmaf(re, re, im * im) * scale; }
/* the order of the arg-max: does (Pb, b) beat (Pa, a)?  The larger power, the lower index on a tie */
RDSP_HD bool search_beats(float Pb, int b, float Pa, int a) { return Pb > Pa || (Pb == Pa && b < a); }
RDSP_HD uint32_t search_best1(float Pi, int i, float next, const SearchLaw &law) {
  return Pi >= law.min2 && Pi >= law.ratio * next ? (uint32_t)i + 1u : 0u;
}

/* a channel's detector on the host: its 200 words */
struct SearchState {
  uint32_t K, key, cnt, best1;
  float a2, next;
  float re[MAX_TONES], im[MAX_TONES], P[MAX_TONES];
};
inline void search_load(SearchState &s, const uint32_t *w) {
  s.K = w[TS_K]; s.key = w[TS_KEY]; s.cnt = w[TS_CNT]; s.best1 = w[TS_BEST1];
  memcpy(&s.a2, &w[TS_A2], 4); memcpy(&s.next, &w[TS_NEXT], 4);
  memcpy(s.re, &w[TS_RE], MAX_TONES * 4); memcpy(s.im, &w[TS_IM], MAX_TONES * 4); memcpy(s.P, &w[TS_P], MAX_TONES * 4);
}
inline void search_store(const SearchState &s, uint32_t *w) {
  w[TS_K] = s.K; w[TS_KEY] = s.key; w[TS_CNT] = s.cnt; w[TS_BEST1] = s.best1; w[6] = 0u; w[7] = 0u;
  memcpy(&w[TS_A2], &s.a2, 4); memcpy(&w[TS_NEXT], &s.next, 4);
  memcpy(&w[TS_RE], s.re, MAX_TONES * 4); memcpy(&w[TS_IM], s.im, MAX_TONES * 4); memcpy(&w[TS_P], s.P, MAX_TONES * 4);
}
/* the detector a call begins with: zeros behind a reset, another K or another bank */
inline void search_start(SearchState &s, uint32_t K, uint32_t key, bool reset) {
  if (reset || s.K != K || s.key != key) memset(&s, 0, sizeof s);
  s.K = K; s.key = key;
}
/* d[b][q] on the host: the tree by halving */
inline float search_dec(const float *a /* [32] */) {
  float q[DEC / 4];
  for (int i = 0; i < DEC / 4; i++) q[i] = search_quad(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
  for (int n = DEC / 8; n >= 1; n >>= 1)
    for (int i = 0; i < n; i++) q[i] = q[2 * i] + q[2 * i + 1];
  return q[0];
}
/* the end of a window on the host: P, the arg-max, next, the decision; re, im and cnt to 0 */
inline void search_window(SearchState &s, const SearchBank &bank, const SearchLaw &law) {
  const int n = (int)bank.n_tones;
  for (int t = 0; t < n; t++) s.P[t] = search_power(s.re[t], s.im[t], law.scale);
  int i = 0;
  for (int t = 1; t < n; t++)
    if (search_beats(s.P[t], t, s.P[i], i)) i = t;
  float next = 0.0f;
  for (int t = 0; t < n; t++)
    if ((t < i - 1 || t > i + 1) && s.P[t] > next) next = s.P[t];
  s.best1 = search_best1(s.P[i], i, next, law);
  s.a2 = s.P[i]; s.next = next; s.cnt = 0u;
  memset(s.re, 0, sizeof s.re); memset(s.im, 0, sizeof s.im);
}
/* the plain loop: n_blocks blocks of a behind the channel's words -> the records of the call, the words renewed (law.K > 0) */
inline void search_reference(const float4 *tab, const SearchLaw &law, const SearchBank &bank, bool reset, uint32_t *words /* [SEARCH_WORDS] */,
                             const float *a, int n_blocks, uint8_t *best_rec, float *a2_rec, float *next_rec) {
  SearchState s;
  search_load(s, words);
  search_start(s, law.K, bank.key, reset);
  for (int b = 0; b < n_blocks; b++) {
    for (int q = 0; q < PER_BLOCK; q++) {
      const float d = search_dec(a + (size_t)b * BLOCK + (size_t)q * DEC);
      const uint32_t m = (uint32_t)PER_BLOCK * s.cnt + (uint32_t)q;
      for (uint32_t t = 0; t < bank.n_tones; t++) search_mac(tab, m * bank.dphi[t], d, s.re[t], s.im[t]);
    }
    s.cnt += 1u;
    if (s.cnt == law.K) search_window(s, bank, law);
    best_rec[b] = (uint8_t)(s.best1 - 1u);
    a2_rec[b] = s.a2;
    next_rec[b] = s.next;
  }
  search_store(s, words);
}

}  // namespace rdsp_tone_search

#endif
