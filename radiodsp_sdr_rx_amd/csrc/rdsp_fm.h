/*
 * rdsp_fm.h -- the arithmetic of rdsp_engine_t's narrow-band FM detector (include/rdsp.h has the definition), shared by the
 * kernel (rdsp_engine_fm.hip), the host entry points (rdsp_engine_fm_host.hip) and the host program of the tests
 * (tests/host/host_fm_check.cpp).  A design of this build: neither the sketch nor the image has an FM mode.
 *
 * Include this header only from sources compiled with -ffp-contract=off: every fused operation here is written as one
 * (fmaf), and the bits of every other product, sum and quotient depend on its not being contracted.
 *
 * Per channel, x[n] = ((float) I, (float) Q) the receiver's int16 IQ row in counts, n counted from the last FM reset, x[n] = 0
 * for n < 0.  NFM ignores setInputGain, setIQgainBalance and the blanker: a discriminator does not care about amplitude.
 *   h      = rdsp_tune.h's ddc_taps(W, 1), T = 16 W taps (W = 2: 32, wide; W = 3: 48, narrow)
 *   z[n]   = sum_{k < T} h_k x[n - k]           per component ONE chain over k ascending from 0: z = fmaf(h_k, x[n - k], z)
 *   lvl[n] = sqrtf(fmaf(zI, zI, zQ zQ)) 2^-15   the square root correctly rounded; a full-scale complex carrier reads 1.0
 *   re     = fmaf(zI, pI, zQ pQ),  im = fmaf(zQ, pI, -(zI pQ)),  (pI, pQ) = z[n - 1]
 *   d[n]   = fm_atan2(im, re)                   below
 *   u[n]   = fminf(fmaxf(d[n] k, -1), 1),       k = (float)(44100.0 / (6.283185307179586 (double) deviation_hz))
 *   y[n]   = fmaf(a, u[n] - y[n - 1], y[n - 1]),  a = (float)(1.0 / (1.0 + 44100.0 (double) tau_us 1e-6));  tau_us == 0: y = u
 * Everything is a function of the sample index: no tile, lane, trip or call size is in the bits.
 *
 * fm_atan2(y, x), this build's own: ax = |x|, ay = |y|; both 0: the result is +0.  t = min(ax, ay) / max(ax, ay), one
 * correctly rounded quotient; s = t t; p = C6; p = fmaf(p, s, C_j) for j = 5 ... 0; r = t p; ay > ax: r = PI_2 - r; x < 0:
 * r = PI - r; the result carries the sign bit of y.  Measured by tests/host/host_fm_check.cpp against the double atan2 over every
 * t = j / 2^20 and a million drawn pairs: the worst error is 5.2e-7 rad (the bound of the definition is 2^-19 = 1.9e-6).
 *
 * A channel's state is FM_STATE_WORDS = 50 words: the newest 47 input pair words (I | Q << 16), oldest first (W = 2 uses the
 * newest 31); z[n - 1], two floats; y[n - 1].
 */
#ifndef RDSP_FM_H
#define RDSP_FM_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rdsp_tune.h"

namespace rdsp_fm {

constexpr int BLOCK = 128;
constexpr int TAPS_PER_W = rdsp_tune::DDC_TAPS_PER_PHASE; /* T = 16 W */
constexpr int MAX_W = 3, MAX_T = TAPS_PER_W * MAX_W;
constexpr int FM_HIST = MAX_T - 1;                                                        /* 47 pair words a channel, whatever W */
constexpr int FM_ST_Z = FM_HIST, FM_ST_Y = FM_HIST + 2, FM_STATE_WORDS = FM_HIST + 3;     /* 50 */
constexpr int FM_DEFAULT_W = 2;
constexpr float FM_DEFAULT_DEVIATION = 5000.0f, FM_DEFAULT_TAU = 750.0f;

RDSP_HD bool width_ok(int W) { return W == 2 || W == 3; }
RDSP_HD bool deviation_ok(float d) { return d >= 1000.0f && d <= 7500.0f; } /* a NaN fails both */
RDSP_HD bool tau_ok(float t) { return t == 0.0f || (t >= 25.0f && t <= 1000.0f); }

/* host only, libm-free: every host and numpy compute the same bits */
inline float fm_scale(float deviation_hz) { return (float)(44100.0 / (6.283185307179586 * (double)deviation_hz)); }
inline float fm_deemph_a(float tau_us) { return (float)(1.0 / (1.0 + 44100.0 * (double)tau_us * 1e-6)); }
inline void fm_taps(int W, float *out /* [16 W] */) { rdsp_tune::ddc_taps(W, 1.0, out); }

constexpr float FM_PI = 3.14159274101257324f, FM_PI_2 = 1.57079637050628662f;
/* atan(t) / t over s = t^2 in [0, 1]: a least-squares fit of this build, seven terms */
constexpr float FM_C0 = 0.9999961256980896f, FM_C1 = -0.3331736922264099f, FM_C2 = 0.19807817041873932f, FM_C3 = -0.132333442568779f,
                FM_C4 = 0.07962367683649063f, FM_C5 = -0.0336042158305645f, FM_C6 = 0.006811788771301508f;

RDSP_HD float fm_atan2(float y, float x) {
  const float ax = fabsf(x), ay = fabsf(y);
  const float mx = ax > ay ? ax : ay, mn = ax > ay ? ay : ax;
  if (mx == 0.0f) return 0.0f;
  const float t = mn / mx, s = t * t;
  float p = FM_C6;
  p = fmaf(p, s, FM_C5);
  p = fmaf(p, s, FM_C4);
  p = fmaf(p, s, FM_C3);
  p = fmaf(p, s, FM_C2);
  p = fmaf(p, s, FM_C1);
  p = fmaf(p, s, FM_C0);
  float r = t * p;
  if (ay > ax) r = FM_PI_2 - r;
  if (x < 0.0f) r = FM_PI - r;
  return copysignf(r, y);
}

/* the components of a pair word */
RDSP_HD float fm_i_of(uint32_t w) { return (float)(int16_t)(w & 0xffffu); }
RDSP_HD float fm_q_of(uint32_t w) { return (float)(int16_t)(w >> 16); }
/* one tap of the chain */
RDSP_HD void fm_mac(float &zi, float &zq, float h, float xi, float xq) {
  zi = fmaf(h, xi, zi);
  zq = fmaf(h, xq, zq);
}
RDSP_HD float fm_level(float zi, float zq) { return sqrtf(fmaf(zi, zi, zq * zq)) * 3.0517578125e-05f; }
/* u[n] of z[n] = (zi, zq) and z[n - 1] = (pi, pq) */
RDSP_HD float fm_detect(float zi, float zq, float pi, float pq, float k) {
  const float re = fmaf(zi, pi, zq * pq), im = fmaf(zq, pi, -(zi * pq));
  return fminf(fmaxf(fm_atan2(im, re) * k, -1.0f), 1.0f);
}
RDSP_HD float fm_deemph(float a, float u, float y1) { return fmaf(a, u - y1, y1); }

/* what a group's detector runs with (rdsp_engine_set_fm); tau_us == 0: the de-emphasis is bypassed, a is not used */
struct FmSet {
  int W;
  float deviation_hz, tau_us;
};

/* the plain loop: n pair words x (n >= 1) behind the channel's state -> n demodulated samples y and n levels, the state renewed */
inline void fm_reference(const float *h, int W, float k, float a, int deemph, uint32_t *state /* [FM_STATE_WORDS] */, const uint32_t *x, int n,
                         float *y, float *lvl) {
  const int T = TAPS_PER_W * W;
  auto at = [&](int s) { return s < 0 ? (FM_HIST + s >= 0 ? state[FM_HIST + s] : 0u) : x[s]; };
  float pi, pq, y1;
  memcpy(&pi, &state[FM_ST_Z], 4); memcpy(&pq, &state[FM_ST_Z + 1], 4); memcpy(&y1, &state[FM_ST_Y], 4);
  for (int m = 0; m < n; m++) {
    float zi = 0.0f, zq = 0.0f;
    for (int j = 0; j < T; j++) {
      const uint32_t w = at(m - j);
      fm_mac(zi, zq, h[j], fm_i_of(w), fm_q_of(w));
    }
    lvl[m] = fm_level(zi, zq);
    const float u = fm_detect(zi, zq, pi, pq, k);
    y1 = deemph ? fm_deemph(a, u, y1) : u;
    y[m] = y1;
    pi = zi; pq = zq;
  }
  uint32_t next[FM_HIST];
  for (int j = 0; j < FM_HIST; j++) next[j] = at(n - FM_HIST + j);
  for (int j = 0; j < FM_HIST; j++) state[j] = next[j];
  memcpy(&state[FM_ST_Z], &pi, 4); memcpy(&state[FM_ST_Z + 1], &pq, 4); memcpy(&state[FM_ST_Y], &y1, 4);
}

}  // namespace rdsp_fm

#endif
