/*
 * rdsp_voice.h -- the arithmetic of rdsp_engine_t's voice-rate audio (include/rdsp.h has the definition), shared by the kernel
 * (rdsp_engine_voice.hip), the host entry points (rdsp_engine_voice_host.hip) and the host program of the tests
 * (tests/host/host_voice_check.cpp).  Integers only behind the tap design.
 *
 * Per channel, x the stream of the LEFT words of its output row as a call leaves it (x[n] = 0 in front of the last reset),
 * R = 2 or 4, T = 16 R:
 *   q_k    = (int32) rint((double) h_k 2^18),  h = the prototype of a source at R x 44 100 Hz (rdsp_tune.h's ddc_taps(R, 1))
 *   acc[m] = sum_{k < T} q_k x[R m + R - 1 - k]                         exact in int64: |acc| < 2^34
 *   y[m]   = clamp((acc[m] + 2^17) >> 18, -32768, 32767)                arithmetic shift: floor, ties upwards
 * The sum is exact, so its order is free: no tile, lane or call size is in the bits.  A channel keeps the last VOICE_HIST = 60
 * left words of x (15 R at R = 4; R = 2 uses the newest 30), oldest first.
 */
#ifndef RDSP_VOICE_H
#define RDSP_VOICE_H

#include <math.h>
#include <stdint.h>

#include "rdsp_tune.h"

namespace rdsp_voice {

constexpr int BLOCK = 128;
constexpr int TAPS_PER_PHASE = rdsp_tune::DDC_TAPS_PER_PHASE; /* T = 16 R */
constexpr int MAX_R = 4;
constexpr int VOICE_HIST = (TAPS_PER_PHASE - 1) * MAX_R;     /* 60 words a channel, whatever R */
constexpr int SHIFT = 18;

RDSP_HD bool rate_ok(int R) { return R == 2 || R == 4; }

/* host only: the 16 R taps, no libm behind rint (rdsp_tune.h's design is + - * / sqrt in double) */
inline void voice_taps(int R, int32_t *out) {
  float h[TAPS_PER_PHASE * MAX_R];
  rdsp_tune::ddc_taps(R, 1.0, h);
  for (int k = 0; k < TAPS_PER_PHASE * R; k++) out[k] = (int32_t)rint((double)h[k] * 262144.0);
}

RDSP_HD int16_t voice_round_sat(int64_t acc) {
  const int64_t v = (acc + ((int64_t)1 << (SHIFT - 1))) >> SHIFT; /* floor: the shift is arithmetic */
  return (int16_t)(v < -32768 ? -32768 : v > 32767 ? 32767 : v);
}

/* The kernel's form of the exact sum: q = 256 hi + lo with lo in -128 ... 127, so acc = 256 sum hi x + sum lo x, both sums
 * of 16-bit products inside int32 (|hi| <= 513: |sum hi x| < 2^15 (sum |q| / 256 + T) < 2^27; |sum lo x| <= 2^15 2^7 T <= 2^28). */
RDSP_HD void voice_tap_split(int32_t q, int32_t *hi, int32_t *lo) {
  *lo = ((q + 128) & 255) - 128;
  *hi = (q - *lo) >> 8; /* exact: q - lo is a multiple of 256 */
}
RDSP_HD int64_t voice_acc_join(int32_t sum_hi, int32_t sum_lo) { return (int64_t)sum_hi * 256 + (int64_t)sum_lo; }
/* host only: the taps as the kernel reads them, [16][R / 2][2] words: for a < 16 and pair pp (the samples x[R j + 2 pp] in the
 * low half word, x[R j + 2 pp + 1] in the high one) the two taps that meet them, q[R a + R - 1 - 2 pp] low and q[R a + R - 2 - 2 pp]
 * high, as the word of their hi parts and the word of their lo parts */
inline void voice_tap_pairs(int R, const int32_t *q, uint32_t *out /* [16 R] */) {
  for (int a = 0; a < TAPS_PER_PHASE; a++)
    for (int pp = 0; pp < R / 2; pp++) {
      int32_t h0, l0, h1, l1;
      voice_tap_split(q[R * a + R - 1 - 2 * pp], &h0, &l0);
      voice_tap_split(q[R * a + R - 2 - 2 * pp], &h1, &l1);
      uint32_t *o = out + ((size_t)a * (size_t)(R / 2) + (size_t)pp) * 2;
      o[0] = ((uint32_t)h0 & 0xFFFFu) | ((uint32_t)h1 << 16);
      o[1] = ((uint32_t)l0 & 0xFFFFu) | ((uint32_t)l1 << 16);
    }
}

/* the plain loop: n left words x (n a multiple of R, at least VOICE_HIST for the history to be the call's alone -- shorter
 * calls are handled too) behind the channel's history -> n / R outputs, and the history renewed */
inline void voice_reference(const int32_t *q, int R, int32_t *hist /* [VOICE_HIST] */, const int16_t *x, size_t x_step, int n, int16_t *y) {
  const int T = TAPS_PER_PHASE * R;
  auto at = [&](int s) { return s < 0 ? (VOICE_HIST + s >= 0 ? hist[VOICE_HIST + s] : 0) : (int32_t)x[(size_t)s * x_step]; };
  for (int m = 0; m < n / R; m++) {
    int64_t acc = 0;
    for (int k = 0; k < T; k++) acc += (int64_t)q[k] * (int64_t)at(R * m + R - 1 - k);
    y[m] = voice_round_sat(acc);
  }
  int32_t next[VOICE_HIST];
  for (int j = 0; j < VOICE_HIST; j++) next[j] = at(n - VOICE_HIST + j);
  for (int j = 0; j < VOICE_HIST; j++) hist[j] = next[j];
}

}  // namespace rdsp_voice

#endif
