/*
 * rdsp_noise.h -- the arithmetic of rdsp_engine_t's noise squelch (include/rdsp.h has the definition), shared by the kernel
 * (rdsp_engine_noise.hip), the host entry points (rdsp_engine_noise_host.hip) and the host program of the tests
 * (tests/host/host_noise_check.cpp).  Compile with -ffp-contract=off: every product and sum below is rounded on its own, the
 * fused operations are written as fmaf.
 *
 * Per channel, a[n] the receiver's "demod" tap (rdsp_fm.h's y[n]), blocks of 128 samples counted from the detector's last start:
 *   g      = noise_taps(tau_us): a 4500 ... 8000 Hz band-pass of 64 taps with the inverse of the de-emphasis folded in, 65 taps
 *   v_j    = sum_{k <= 64} g_k a[n0 + 4 j + 3 - k], j = 0 ... 31: ONE chain over k ascending from 0, v = fmaf(g_k, a[.], v)
 *   nz     = tree(v_j v_j) 2^-5              adjacent pairs in index order, five levels: the last five of the meter's exchange
 *   N     <- rdsp_meter::level_step(N, nz, rise, fall)
 *   the gate (open, hang) from N by noise_gate_step: the meter's gate with the sense reversed
 * Only every fourth output of the filter is computed: the mean square of a subsampled stationary signal is the same mean square.
 *
 * A channel's state is NOISE_WORDS = 68 words: key, N, open, hang, the newest 64 samples of the tap (oldest first).  A detector
 * whose stored key is not the one it is run with starts closed: N = 1, history zeros (noise_start).
 */
#ifndef RDSP_NOISE_H
#define RDSP_NOISE_H

#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rdsp_fm.h"
#include "rdsp_meter.h"

namespace rdsp_noise {

constexpr int BLOCK = 128;
constexpr int NOISE_PROTO = 64;             /* taps of the prototype */
constexpr int NOISE_TAPS = NOISE_PROTO + 1; /* with the compensation */
constexpr int NOISE_HIST = 64;              /* samples a channel keeps */
constexpr int NOISE_STEP = 4, NOISE_OUT = BLOCK / NOISE_STEP; /* every fourth output: 32 a block */
enum { NZ_KEY = 0, NZ_N, NZ_OPEN, NZ_HANG, NZ_HIST, NOISE_WORDS = NZ_HIST + NOISE_HIST };
constexpr float NZ_SCALE = 0.03125f; /* 1 / 32, exact */
constexpr double NOISE_KAISER_BETA = 6.0;
constexpr int NOISE_OFF = 0, NOISE_MEASURE = 1, NOISE_GATE = 2;
constexpr float NOISE_DEFAULT_OPEN = 0.01f, NOISE_DEFAULT_CLOSE = 0.025f, NOISE_DEFAULT_FALL = 0.75f, NOISE_DEFAULT_RISE = 0.125f;
constexpr int NOISE_DEFAULT_HANG = 8;

/* a group's detector settings (rdsp_engine_set_noise_squelch) */
struct NoiseSet {
  int mode;
  float open_n, close_n;
  int hang_blocks;
  float fall, rise;
};
/* a channel's detector without its history */
struct NoiseState {
  uint32_t key;
  float N;
  int32_t open, hang;
};

/* the setter's limits (a NaN fails every comparison) */
inline bool squelch_ok(int mode, float open_n, float close_n, int hang_blocks, float fall, float rise) {
  return mode >= NOISE_OFF && mode <= NOISE_GATE && open_n > 0.0f && open_n <= close_n && isfinite(close_n) && hang_blocks >= 0 &&
         hang_blocks <= rdsp_meter::HANG_MAX && rdsp_meter::coefficients_ok(fall, rise);
}
RDSP_HD uint32_t noise_key(int mode, int W, bool deemph) { return 0x80000000u | (uint32_t)mode << 24 | (uint32_t)W << 16 | (deemph ? 1u : 0u); }

/* host only, libm-free but for the square root (rdsp_tune.h's sine and I0 series): every host and numpy compute the same bits.
 * The prototype: hb_k = (sin(2 pi 8000 m / 44100) - sin(2 pi 4500 m / 44100)) / (pi m) w_k, m = k - 31.5, w the Kaiser window
 * of beta 6 -- the difference of two windowed sincs; with q = |2 k - 63| the sines are sin(pi 160 q / 882) and sin(pi 90 q / 882).
 * The tap sits behind y <- fmaf(a, u - y, y): g_k = (hb_k - r hb_{k-1}) / a, r = 1 - a, gives the band-pass of u. */
inline void noise_taps(float tau_us, float *out /* [NOISE_TAPS] */) {
  double hb[NOISE_PROTO + 2];
  const double i0b = rdsp_tune::ddc_i0(NOISE_KAISER_BETA);
  hb[0] = 0.0; hb[NOISE_PROTO + 1] = 0.0; /* hb[1 + k]: hb_{-1} and hb_64 are zeros */
  for (int k = 0; k < NOISE_PROTO; k++) {
    const int q = 2 * k - (NOISE_PROTO - 1) < 0 ? (NOISE_PROTO - 1) - 2 * k : 2 * k - (NOISE_PROTO - 1);
    const double u = (3.141592653589793 * (double)q) / 2.0;
    const double rho = (double)q / (double)(NOISE_PROTO - 1);
    const double s = rdsp_tune::ddc_sin_halfpi(160 * q, 441) - rdsp_tune::ddc_sin_halfpi(90 * q, 441);
    hb[1 + k] = (s / u) * (rdsp_tune::ddc_i0(NOISE_KAISER_BETA * sqrt(1.0 - rho * rho)) / i0b);
  }
  if (tau_us == 0.0f) {
    for (int k = 0; k < NOISE_TAPS; k++) out[k] = (float)hb[1 + k];
    return;
  }
  const double a = (double)rdsp_fm::fm_deemph_a(tau_us), r = 1.0 - a;
  for (int k = 0; k < NOISE_TAPS; k++) out[k] = (float)((hb[1 + k] - r * hb[k]) / a);
}

/* one tap of the chain */
RDSP_HD float noise_mac(float v, float g, float a) { return fmaf(g, a, v); }
RDSP_HD float noise_reading(float tree_sum) { return tree_sum * NZ_SCALE; }
/* the detector a call begins with: closed behind a reset or another key; true: the history is zeros too */
RDSP_HD bool noise_start(NoiseState &s, uint32_t key, bool reset) {
  const bool fresh = reset || s.key != key;
  if (fresh) { s.N = 1.0f; s.open = 0; s.hang = 0; }
  s.key = key;
  return fresh;
}
/* the gate after the level of a block: rdsp_meter's gate_step with the sense reversed */
RDSP_HD void noise_gate_step(NoiseState &g, const NoiseSet &s) {
  if (g.N <= s.open_n) { g.open = 1; g.hang = s.hang_blocks; }
  else if (g.open && g.N <= s.close_n) g.hang = s.hang_blocks;
  else if (g.open && g.hang > 0) g.hang--;
  else g.open = 0;
}
RDSP_HD void noise_step(NoiseState &g, float nz, const NoiseSet &s) {
  g.N = rdsp_meter::level_step(g.N, nz, s.rise, s.fall);
  noise_gate_step(g, s);
}

/* one block on the host: x[0 ... 63] the samples in front of it, x[64 ... 191] the block; the tree by halving */
inline float noise_block(const float *g, const float *x) {
  float q[NOISE_OUT];
  for (int j = 0; j < NOISE_OUT; j++) {
    float v = 0.0f;
    for (int k = 0; k < NOISE_TAPS; k++) v = noise_mac(v, g[k], x[NOISE_HIST + NOISE_STEP * j + 3 - k]);
    q[j] = v * v;
  }
  for (int n = NOISE_OUT / 2; n >= 1; n >>= 1)
    for (int i = 0; i < n; i++) q[i] = q[2 * i] + q[2 * i + 1];
  return noise_reading(q[0]);
}
/* the plain loop: n_blocks blocks of a behind the channel's words -> the records of the call, the words renewed.  set.mode == 0:
 * the words and the records are zeros */
inline void noise_reference(const float *g, const NoiseSet &set, uint32_t key, bool reset, uint32_t *words /* [NOISE_WORDS] */, const float *a,
                            int n_blocks, float *noise_rec, uint8_t *open_rec) {
  if (set.mode == NOISE_OFF) {
    memset(words, 0, NOISE_WORDS * 4);
    for (int b = 0; b < n_blocks; b++) { noise_rec[b] = 0.0f; open_rec[b] = 0; }
    return;
  }
  NoiseState s;
  s.key = words[NZ_KEY]; s.open = (int32_t)words[NZ_OPEN]; s.hang = (int32_t)words[NZ_HANG];
  memcpy(&s.N, &words[NZ_N], 4);
  float x[NOISE_HIST + BLOCK];
  if (noise_start(s, key, reset)) memset(x, 0, NOISE_HIST * 4);
  else memcpy(x, &words[NZ_HIST], NOISE_HIST * 4);
  for (int b = 0; b < n_blocks; b++) {
    memcpy(x + NOISE_HIST, a + (size_t)b * BLOCK, BLOCK * 4);
    noise_step(s, noise_block(g, x), set);
    noise_rec[b] = s.N;
    open_rec[b] = (uint8_t)s.open;
    memmove(x, x + BLOCK, NOISE_HIST * 4);
  }
  words[NZ_KEY] = s.key; words[NZ_OPEN] = (uint32_t)s.open; words[NZ_HANG] = (uint32_t)s.hang;
  memcpy(&words[NZ_N], &s.N, 4);
  memcpy(&words[NZ_HIST], x, NOISE_HIST * 4);
}

}  // namespace rdsp_noise

#endif
