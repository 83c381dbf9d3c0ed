/*
 * rdsp_tone.h -- the arithmetic of rdsp_engine_t's CTCSS tone squelch (include/rdsp.h has the definition), shared by the kernel
 * (rdsp_engine_tone.hip), the host entry points (rdsp_engine_tone_host.hip) and the host program of the tests
 * (tests/host/host_tone_check.cpp).  Compile with -ffp-contract=off: every product and sum below is rounded on its own, the one
 * fused operation is written as fmaf.
 *
 * Per channel, a[n] the receiver's "demod" tap (rdsp_fm.h's y[n]), blocks of 128 samples counted from the detector's last reset:
 *   dphi   = (uint32) llround((double) tone_hz 2^32 / 44100.0)          0: no tone
 *   (c, s) = tune_phasor(tab, ph + t dphi), t = 0 ... 127               rdsp_tune.h's table and interpolation
 *   Sr, Si = the meter's tree sums (adjacent pairs in index order, seven levels) of a[t] c and a[t] s, one rounded product each
 *   re += Sr, im += Si, ph += 128 dphi, cnt += 1
 *   cnt == K: a2 = fmaf(re, re, im im) scale, scale = (float)(4.0 / ((128.0 K) (128.0 K))); tone = a2 >= (tone ? off2 : on2);
 *             re = im = 0, cnt = 0
 * A wave computes the tree as the meter's does: a lane multiplies its 4 consecutive samples and adds them as (p0 + p1) + (p2 + p3)
 * (tone_quad: levels 1 and 2), then 32 lanes exchange with strides 1, 2, 4, 8, 16 (levels 3 ... 7).
 *
 * A channel's state is TONE_WORDS = 8 words: dphi, K, ph, re, im, cnt, tone, a2 (re, im and a2 floats).  A detector whose stored
 * dphi or K is not the one it is run with starts from zeros (tone_start).
 */
#ifndef RDSP_TONE_H
#define RDSP_TONE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rdsp_tune.h"

namespace rdsp_tone {

constexpr int BLOCK = 128;
enum { TN_DPHI = 0, TN_K, TN_PH, TN_RE, TN_IM, TN_CNT, TN_TONE, TN_A2, TONE_WORDS = 8 };
constexpr float TONE_MIN_HZ = 60.0f, TONE_MAX_HZ = 300.0f;
constexpr int TONE_MIN_K = 4, TONE_MAX_K = 512, TONE_DEFAULT_K = 128;
constexpr float TONE_DEFAULT_ON = 0.04f, TONE_DEFAULT_OFF = 0.025f;

/* a group's detector settings (rdsp_engine_set_tone_squelch) */
struct ToneSet {
  int K;
  float on_amp, off_amp;
};
/* what the kernel is handed of them */
struct ToneLaw {
  uint32_t K;
  float scale, on2, off2;
};
/* a channel's detector: its eight words */
struct ToneState {
  uint32_t dphi, K, ph;
  float re, im;
  uint32_t cnt, tone;
  float a2;
};

/* the setters' limits (a NaN fails every comparison) */
inline bool tone_ok(float hz) { return hz == 0.0f || (hz >= TONE_MIN_HZ && hz <= TONE_MAX_HZ); }
inline bool squelch_ok(int K, float on_amp, float off_amp) {
  return K >= TONE_MIN_K && K <= TONE_MAX_K && off_amp > 0.0f && off_amp <= on_amp && on_amp <= 1.0f;
}

/* host only, libm-free but for the rounding: every host and numpy compute the same bits */
inline uint32_t tone_dphi(float tone_hz) { return (uint32_t)(unsigned long long)llround((double)tone_hz * 4294967296.0 / rdsp_tune::TUNE_FS); }
inline float tone_scale(int K) { return (float)(4.0 / ((128.0 * (double)K) * (128.0 * (double)K))); }
inline ToneLaw tone_law(const ToneSet &s) { return {(uint32_t)s.K, tone_scale(s.K), s.on_amp * s.on_amp, s.off_amp * s.off_amp}; }
/* host only: the magnitude of the NFM de-emphasis y <- fmaf(a, u - y, y) at tone_hz, a the float of rdsp_fm.h's fm_deemph_a */
inline double tone_gain(float tone_hz, float a) {
  const double w = 6.283185307179586 * (double)tone_hz / rdsp_tune::TUNE_FS, r = 1.0 - (double)a;
  return (double)a / sqrt(1.0 - 2.0 * r * cos(w) + r * r);
}

/* the detector a call begins with: zeros behind a reset, another tone or another K */
RDSP_HD void tone_start(ToneState &s, uint32_t dphi, uint32_t K, bool reset) {
  if (reset || s.dphi != dphi || s.K != K) { s.ph = 0u; s.re = 0.0f; s.im = 0.0f; s.cnt = 0u; s.tone = 0u; s.a2 = 0.0f; }
  s.dphi = dphi; s.K = K;
}
/* levels 1 and 2 of both trees on four consecutive samples, the first of them at phase ph */
RDSP_HD void tone_quad(const float4 *tab, uint32_t ph, uint32_t dphi, float a0, float a1, float a2, float a3, float &qr, float &qi) {
  const float2 e0 = rdsp_tune::tune_phasor(tab, ph), e1 = rdsp_tune::tune_phasor(tab, ph + dphi);
  const float2 e2 = rdsp_tune::tune_phasor(tab, ph + 2u * dphi), e3 = rdsp_tune::tune_phasor(tab, ph + 3u * dphi);
  qr = (a0 * e0.x + a1 * e1.x) + (a2 * e2.x + a3 * e3.x);
  qi = (a0 * e0.y + a1 * e1.y) + (a2 * e2.y + a3 * e3.y);
}
/* the detector after a block whose tree sums are Sr, Si */
RDSP_HD void tone_step(ToneState &s, float Sr, float Si, const ToneLaw &law) {
  s.re = s.re + Sr;
  s.im = s.im + Si;
  s.ph += (uint32_t)BLOCK * s.dphi;
  s.cnt += 1u;
  if (s.cnt == law.K) {
    s.a2 = fmaf(s.re, s.re, s.im * s.im) * law.scale;
    s.tone = s.a2 >= (s.tone ? law.off2 : law.on2) ? 1u : 0u;
    s.re = 0.0f; s.im = 0.0f; s.cnt = 0u;
  }
}

/* a channel's words and back */
inline void tone_load(ToneState &s, const uint32_t *w) {
  s.dphi = w[TN_DPHI]; s.K = w[TN_K]; s.ph = w[TN_PH]; s.cnt = w[TN_CNT]; s.tone = w[TN_TONE];
  memcpy(&s.re, &w[TN_RE], 4); memcpy(&s.im, &w[TN_IM], 4); memcpy(&s.a2, &w[TN_A2], 4);
}
inline void tone_store(const ToneState &s, uint32_t *w) {
  w[TN_DPHI] = s.dphi; w[TN_K] = s.K; w[TN_PH] = s.ph; w[TN_CNT] = s.cnt; w[TN_TONE] = s.tone;
  memcpy(&w[TN_RE], &s.re, 4); memcpy(&w[TN_IM], &s.im, 4); memcpy(&w[TN_A2], &s.a2, 4);
}
/* one block on the host: the trees by halving, in place */
inline void tone_block_sums(const float4 *tab, uint32_t ph, uint32_t dphi, const float *a, float *Sr, float *Si) {
  float qr[BLOCK / 4], qi[BLOCK / 4];
  for (int i = 0; i < BLOCK / 4; i++)
    tone_quad(tab, ph + (uint32_t)(4 * i) * dphi, dphi, a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3], qr[i], qi[i]);
  for (int n = BLOCK / 8; n >= 1; n >>= 1)
    for (int i = 0; i < n; i++) { qr[i] = qr[2 * i] + qr[2 * i + 1]; qi[i] = qi[2 * i] + qi[2 * i + 1]; }
  *Sr = qr[0]; *Si = qi[0];
}
/* the plain loop: n_blocks blocks of a behind the channel's words -> the records of the call, the words renewed.  dphi == 0: the
 * words and the records are zeros */
inline void tone_reference(const float4 *tab, const ToneLaw &law, uint32_t dphi, bool reset, uint32_t *words /* [TONE_WORDS] */, const float *a,
                           int n_blocks, float *a2_rec, uint8_t *tone_rec) {
  ToneState s;
  tone_load(s, words);
  tone_start(s, dphi, law.K, reset);
  if (dphi == 0u) {
    memset(words, 0, TONE_WORDS * 4);
    for (int b = 0; b < n_blocks; b++) { a2_rec[b] = 0.0f; tone_rec[b] = 0; }
    return;
  }
  for (int b = 0; b < n_blocks; b++) {
    float Sr, Si;
    tone_block_sums(tab, s.ph, dphi, a + (size_t)b * BLOCK, &Sr, &Si);
    tone_step(s, Sr, Si, law);
    a2_rec[b] = s.a2;
    tone_rec[b] = (uint8_t)s.tone;
  }
  tone_store(s, words);
}

}  // namespace rdsp_tone

#endif
