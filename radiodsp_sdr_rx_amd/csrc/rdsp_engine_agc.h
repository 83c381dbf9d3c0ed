/*
 * rdsp_engine_agc.h -- the engine's hang AGC as the image computes it, shared by rdsp_engine_t (rdsp_engine.hip) and the
 * chain's engine-law tail stage (rdsp_tail_engine.hip): the truncating conversion, the gain look-up (0xdb58), the
 * constants of the AGC modes (0xdfe0) and of the constructor (0xdf14), and the host generator of the soft-knee gain
 * curve (0xdd40).  Both sources are compiled with -ffp-contract=off: every fused operation here is written as one.
 */
#ifndef RDSP_ENGINE_AGC_H
#define RDSP_ENGINE_AGC_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

namespace {

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

inline float bits_f(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }
inline uint32_t f_bits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }

/* the AGC's constants: {attack a, attack b, decay a, decay b} as the image's bit patterns, and the hang time in samples.
 * Sets 1 .. 3 are setAGCmode's (0xdfe0: fast / medium / slow); set 0 is what the constructor leaves (0xdf14: the
 * medium attack with the slow decay and the fast hang time) */
struct EngineAgcSet { float attack_a, attack_b, decay_a, decay_b; int hang_time; };
inline EngineAgcSet engine_agc_set(int set) {
  static const uint32_t k[4][4] = {{0x3f7d5732, 0x3c2a3380, 0x3f7ff928, 0x38db0000}, {0x3f79673b, 0x3cd318a0, 0x3f7fddca, 0x3a08d800},
                                   {0x3f7d5732, 0x3c2a3380, 0x3f7ff250, 0x395b0000}, {0x3f7eaab6, 0x3baaa500, 0x3f7ff928, 0x38db0000}};
  static const int hang[4] = {4410, 4410, 22050, 88200};
  if (set < 0 || set > 3) set = 0;
  return {bits_f(k[set][0]), bits_f(k[set][1]), bits_f(k[set][2]), bits_f(k[set][3]), hang[set]};
}
constexpr float ENGINE_AGC_MAKEUP = 10.0f; /* the constructor's values of the curve and the gain after it */
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
