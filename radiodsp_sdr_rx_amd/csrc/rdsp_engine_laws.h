/*
 * rdsp_engine_laws.h -- the engine's hang AGC (0xdb58) and ALS line enhancer (0xda24) as the image computes them: the one
 * copy of their stage bodies, for rdsp_engine_t's two tail kernels (rdsp_engine_tail.hip) and the chain's engine-law tail
 * stage (rdsp_tail_engine.hip).  The kernels keep their own lanes, LDS tiles, block loops, barriers and HBM layouts; the
 * pieces here take plain pointers and values.  Also: the truncating conversion, the gain look-up, the output word
 * (0xebfa), the constants of the AGC modes (0xdfe0) and of the constructor (0xdf14), and the host generator of the
 * soft-knee gain curve (0xdd40).
 *
 * Include this header only from sources compiled with -ffp-contract=off: every fused operation here is written as one
 * (fmaf / fma), and the bits of every other product and sum depend on its not being contracted.
 */
#ifndef RDSP_ENGINE_LAWS_H
#define RDSP_ENGINE_LAWS_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "rdsp_kernels.h"

namespace {

constexpr int ENGINE_ALS_DELAY = 3; /* the constructor's value, as are the RDSP_ENG_ALS_TAPS taps; the image has no setter */

__device__ __forceinline__ int trunc_s32(double x) { /* VCVT.S32.F64: toward zero, saturating, NaN -> 0 -- which is what v_cvt_i32_f64 does too */
  int r;
  asm("v_cvt_i32_f64 %0, %1" : "=v"(r) : "v"(x));
  return r;
}

/* 0xdb58's look-up: the envelope x 32767 toward zero, the high byte picks the entry, the low byte interpolates */
__device__ __forceinline__ float agc_lookup(const float *curve, float env) {
  const int idx = trunc_s32((double)env * 32767.0);
  int hi = (idx >> 8) & 0xff, hi1;
  if (hi > 127) { hi = 127; hi1 = 128; } else hi1 = hi + 1;
  const float frac = (float)(unsigned)(idx & 0xff) * 0.00390625f;
  const float t0 = curve[hi];
  return fmaf(frac, curve[hi1] - t0, t0);
}

/* one channel's AGC state, as 4 words in HBM: envelope, gain, hang counter (int), active flag (int) */
struct EngineAgcState {
  float env, g;
  int hang, active;
  __device__ __forceinline__ void load(const float *s) {
    env = s[0]; g = s[1]; hang = __float_as_int(s[2]); active = __float_as_int(s[3]);
  }
  __device__ __forceinline__ void store(float *s) const {
    s[0] = env; s[1] = g; s[2] = __int_as_float(hang); s[3] = __int_as_float(active);
  }
};

/* 0xdb58's envelope over one block row `a`, on one lane per channel: le[t] is the envelope sample t's gain is looked up
 * from (< 0: none yet in this block, the gain carried in); then the block's last look-up and the active flag.  Attack
 * (the hang counter is re-armed) / decay (counter at 0) / hold (count down): both candidate envelopes are formed and one
 * is selected -- the channels of a wave are in different states, and as branches every lane would walk all three arms.
 * The loop works on copies of env and hang: written through the reference, the selects come out as branches. */
__device__ __forceinline__ void agc_envelope(EngineAgcState &s, const EngineAgcSet &k, const float *curve, const float *a, float *le) {
  float env = s.env, last = -1.0f;
  int hang = s.hang;
  float anext = a[0];
  for (int t = 0; t < RDSP_BLOCK; t++) {
    float in = fabsf(anext);
    anext = a[t + 1 < RDSP_BLOCK ? t + 1 : RDSP_BLOCK - 1];
    if (in > 1.0f) in = 1.0f;
    const bool attack = env < in, decay = !attack && hang == 0;
    const float ea = fmaf(env, k.attack_a, in * k.attack_b), ed = fmaf(env, k.decay_a, in * k.decay_b);
    env = attack ? ea : (decay ? ed : env);
    hang = attack ? k.hang_time : (decay ? 0 : hang - 1);
    last = (attack || decay) ? env : last;
    le[t] = last;
  }
  s.env = env;
  s.hang = hang;
  if (last >= 0.0f) s.g = agc_lookup(curve, last);
  s.active = (double)s.g < 0.98999999999999999;
}

/* 0xdc10 on one sample x: the gain looked up from the envelope le (< 0: g_in, the gain carried into the block), x the
 * makeup gain, clamped to +-1 */
__device__ __forceinline__ float agc_gain_clamp(const EngineAgcSet &k, const float *curve, float le, float g_in, float x) {
  const float gg = le < 0.0f ? g_in : agc_lookup(curve, le);
  float y = (gg * k.makeup) * x;
  if (y > 1.0f) y = 1.0f;
  else if (y < -1.0f) y = -1.0f;
  return y;
}

/* 0xda24 over one block, on the four lanes (aq) of a channel's quad, the taps w in registers (the same in all four).
 * y[n] = sum_k w_k x[n - 3 - k] as one chain of 55 fused multiply-adds, e = x[n] - y; on every fourth sample of a block
 * (its first one included) w_k += (e x[n - 3 - k]) / 2.  The chain of one sample cannot be cut, but the four samples
 * between two tap moves see the same taps: each lane takes one, then every lane makes the move with the fourth lane's
 * error.  The line x in LDS holds H samples of history, then the block (block sample j at x[H + j]).  Quads of four
 * samples ending on a move: {-3 .. 0} (only 0 is this block's), {1 .. 4}, ..., {125 .. 128} (128 is the next block's
 * first: not computed here, no move).  out[j] gets the error (notch) or the prediction (peak); adaptive = 0: the taps
 * stay. */
template <int H>
__device__ __forceinline__ void als_block(float (&w)[RDSP_ENG_ALS_TAPS], const float *x, float *out, int aq, int notch, int adaptive) {
  static_assert(H >= 60, "the first quad reads x[H - 60]");
  for (int q = -1; q < RDSP_BLOCK / 4; q++) {
    const int m = H + 1 + 4 * q + aq;
    float y = 0.0f;
#pragma unroll
    for (int k = 0; k < RDSP_ENG_ALS_TAPS; k++) y = fmaf(w[k], x[m - ENGINE_ALS_DELAY - k], y);
    const float err = x[m < H + RDSP_BLOCK ? m : H + RDSP_BLOCK - 1] - y;
    if (m >= H && m < H + RDSP_BLOCK) out[m - H] = notch ? err : y;
    if (adaptive && q < RDSP_BLOCK / 4 - 1) {
      const float e3 = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, err), 0xFF, 0xF, 0xF, false)); /* quad_perm [3,3,3,3] */
      const float *xm = x + (H + 4 + 4 * q) - ENGINE_ALS_DELAY;
#pragma unroll
      for (int k = 0; k < RDSP_ENG_ALS_TAPS; k++) w[k] = fmaf(e3 * xm[-k], 0.5f, w[k]);
    }
  }
}

/* 0xebfa: x output gain x 32767 toward zero, the low half-word, on both outputs (L | R << 16) */
__device__ __forceinline__ int32_t engine_out_word(float y, float output_gain, int mute) {
  const uint32_t v = mute ? 0u : ((uint32_t)trunc_s32((double)(y * output_gain) * 32767.0) & 0xffffu);
  return (int32_t)(v | (v << 16));
}

inline float bits_f(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
inline uint32_t f_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

/* the AGC's constants: {attack a, attack b, decay a, decay b} as the image's bit patterns, the makeup gain after the
 * curve (the constructor's, the same in every set) and the hang time in samples.  Sets 1 .. 3 are setAGCmode's (0xdfe0:
 * fast / medium / slow); set 0 is what the constructor leaves (0xdf14: the medium attack with the slow decay and the
 * fast hang time) */
inline EngineAgcSet engine_agc_set(int set) {
  static const uint32_t k[4][4] = {{0x3f7d5732, 0x3c2a3380, 0x3f7ff928, 0x38db0000}, {0x3f79673b, 0x3cd318a0, 0x3f7fddca, 0x3a08d800},
                                   {0x3f7d5732, 0x3c2a3380, 0x3f7ff250, 0x395b0000}, {0x3f7eaab6, 0x3baaa500, 0x3f7ff928, 0x38db0000}};
  static const int hang[4] = {4410, 4410, 22050, 88200};
  if (set < 0 || set > 3) set = 0;
  return {bits_f(k[set][0]), bits_f(k[set][1]), bits_f(k[set][2]), bits_f(k[set][3]), 10.0f, hang[set]};
}
/* the constructor's values of the curve */
constexpr float ENGINE_AGC_THRESHOLD_DB = -60.0f, ENGINE_AGC_KNEE_DB = 2.0f;
constexpr uint32_t ENGINE_AGC_SLOPE_BITS = 0x3dcccccd;

/* expf of the C library the engine was linked against (newlib's e_expf.c, Sun's algorithm): the gain curve below is built
 * with it, and a different last bit in one of its 129 entries would be a different gain on every sample that uses it */
inline float engine_expf(float x) {
  const float ln2_hi = 6.9313812256e-01f, ln2_lo = 9.0580006145e-06f, inv_ln2 = 1.4426950216e+00f;
  const float P[5] = {1.6666667163e-01f, -2.7777778450e-03f, 6.6137559770e-05f, -1.6533901999e-06f, 4.1381369442e-08f};
  const uint32_t hx = f_bits(x) & 0x7fffffffu;
  const int neg = (int)(f_bits(x) >> 31);
  if (hx > 0x7f800000u) return x + x;
  if (hx == 0x7f800000u) return neg ? 0.0f : x;
  if (x > 8.8721679688e+01f) return INFINITY;
  if (x < -1.0397208405e+02f) return 0.0f;
  float hi = 0.0f, lo = 0.0f;
  int k = 0;
  if (hx > 0x3eb17218u) {
    if (hx < 0x3F851592u) { hi = neg ? x + ln2_hi : x - ln2_hi; lo = neg ? -ln2_lo : ln2_lo; k = neg ? -1 : 1; }
    else { k = (int)(inv_ln2 * x + (neg ? -0.5f : 0.5f)); const float t = (float)k; hi = x - t * ln2_hi; lo = t * ln2_lo; }
    x = hi - lo;
  } else if (hx < 0x31800000u) return 1.0f + x;
  const float t = x * x;
  const float c = x - t * (P[0] + t * (P[1] + t * (P[2] + t * (P[3] + t * P[4]))));
  if (k == 0) return 1.0f - ((x * c) / (c - 2.0f) - x);
  const float y = 1.0f - ((lo - (x * c) / (2.0f - c)) - hi);
  if (k >= -125) return bits_f(f_bits(y) + ((uint32_t)k << 23));
  return bits_f(f_bits(y) + ((uint32_t)(k + 100) << 23)) * 7.8886090522e-31f;
}

/* 0xdd40: soft-knee compressor curve over the envelope, 1/128 per entry (130 entries: the look-up reads entry hi + 1) */
inline void engine_agc_curve(float threshold_db, float knee_db, float slope, float *curve) {
  const double ln10ish = 2.3025, db_per_octave = 6.026; /* the library's own constants */
  const double T = (double)threshold_db, W = (double)knee_db;
  const float x_lo = engine_expf((float)(((T - W * 0.5) * ln10ish) / 20.0)), x_hi = engine_expf((float)(((T + W * 0.5) * ln10ish) / 20.0));
  for (int i = 0; i < 130; i++) {
    const float x = (float)i * 0.0078125f;
    if (x_lo > x) { curve[i] = 1.0f; continue; }
    int ex;
    const float m = frexpf(x, &ex);
    const float log2x = fmaf(m, fmaf(m, fmaf(m, 1.2314958572387695f, -4.1185250282287598f), 6.021970272064209f), -3.1339645385742188f) + (float)ex;
    const float xdb = (float)((double)log2x * db_per_octave);
    float gdb;
    if (x_hi >= x) {
      const double d = fma(W, 0.5, (double)(xdb - threshold_db));
      gdb = (float)(((((double)slope - 1.0) * d) * d) / (W + W) + (double)xdb) - xdb;
    } else {
      gdb = fmaf(xdb - threshold_db, slope, threshold_db) - xdb;
    }
    curve[i] = engine_expf((float)(((double)gdb * ln10ish) / 20.0));
  }
}

}  // namespace

#endif
