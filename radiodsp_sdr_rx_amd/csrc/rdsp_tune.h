/*
 * rdsp_tune.h -- the arithmetic of rdsp_engine_t's tuning pass (rdsp_engine_update_sources, include/rdsp.h): receiver
 * ch's row is its source row times e^{+j phi[n]}, phi a uint32 phase accumulator, requantized to int16.  Shared by the
 * kernel (rdsp_engine_tune.hip) and the host restatement of the tests (tests/host/host_tune_check.cpp), so both evaluate
 * the same operations in the same order; both are compiled with -ffp-contract=off, and every fused operation is an fmaf.
 *
 * The phasor: a table of TUNE_N entries {cos, sin of 2 pi k / TUNE_N, and the steps to entry k + 1}, generated on the host
 * (libm in double, rounded to float), and linear interpolation by the low TUNE_FRAC_BITS of the phase.  The chord's error is
 * at most (2 pi / TUNE_N)^2 / 8 = 4.7e-6 at TUNE_N = 1024, below 2^-17 with the rounding of the table and of the fmaf
 * (tests/test_engine_tuning.py sweeps it).  Phase 0 is entry 0 with a zero fraction: exactly (1, 0), so a receiver whose
 * shift is 0 gets its source's pairs unchanged, -32768 included.
 */
#ifndef RDSP_TUNE_H
#define RDSP_TUNE_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#ifndef RDSP_HD
#define RDSP_HD __host__ __device__ __forceinline__
#endif

namespace rdsp_tune {

constexpr int TUNE_BITS = 10;
constexpr int TUNE_N = 1 << TUNE_BITS;
constexpr int TUNE_FRAC_BITS = 32 - TUNE_BITS;
constexpr double TUNE_FS = 44100.0; /* the engine's only rate */
constexpr double TUNE_MAX_HZ = 22050.0; /* |station| must stay below it */

/* host only: the table, float4 {cos, sin, cos[k + 1] - cos[k], sin[k + 1] - sin[k]} (entry TUNE_N is entry 0) */
inline void tune_table(float4 *tab) {
  float c[TUNE_N + 1], s[TUNE_N + 1];
  for (int k = 0; k < TUNE_N; k++) {
    const double a = 2.0 * 3.14159265358979323846 * (double)k / (double)TUNE_N;
    c[k] = (float)cos(a);
    s[k] = (float)sin(a);
  }
  c[0] = 1.0f; s[0] = 0.0f;
  c[TUNE_N] = c[0]; s[TUNE_N] = s[0];
  for (int k = 0; k < TUNE_N; k++) tab[k] = make_float4(c[k], s[k], c[k + 1] - c[k], s[k + 1] - s[k]);
}

/* e^{+j 2 pi ph / 2^32} as (cos, sin) */
RDSP_HD float2 tune_phasor(const float4 *tab, uint32_t ph) {
  const float4 t = tab[ph >> TUNE_FRAC_BITS];
  const float f = (float)(ph & ((1u << TUNE_FRAC_BITS) - 1u)) * 0x1p-22f; /* exact: 22 bits */
  return make_float2(fmaf(f, t.z, t.x), fmaf(f, t.w, t.y));
}

/* round half to even, then saturate */
RDSP_HD uint32_t tune_q16(float v) {
  v = fminf(fmaxf(rintf(v), -32768.0f), 32767.0f);
  return (uint32_t)(uint16_t)(int16_t)(int)v;
}

/* one int16 pair (a word I | Q << 16) times (c + j s), rotated as the engine's shifter rotates */
RDSP_HD uint32_t tune_pair(uint32_t w, float2 cs) {
  const float i = (float)(int16_t)(uint16_t)(w & 0xffffu), q = (float)(int16_t)(uint16_t)(w >> 16);
  const float ir = fmaf(i, cs.x, -(q * cs.y));
  const float qr = fmaf(q, cs.x, i * cs.y);
  return tune_q16(ir) | tune_q16(qr) << 16;
}

/* phase of sample t of a call that starts at phase ph0; the accumulator after a call of n samples is tune_phase(ph0, dphi, n) */
RDSP_HD uint32_t tune_phase(uint32_t ph0, uint32_t dphi, uint32_t t) { return ph0 + t * dphi; }

/* host only: the step per sample that moves a station at station_hz (from the stream's centre) to the engine's IF */
inline uint32_t tune_dphi(float tuning_offset, double station_hz) {
  return (uint32_t)(unsigned long long)llround(((double)tuning_offset - station_hz) * 4294967296.0 / TUNE_FS);
}

/* the pass's arguments: receivers are visited in `order` (grouped by source); cpw receivers per workgroup */
struct TuneParams {
  const uint32_t *src; size_t src_stride;   /* [source][t] words I | Q << 16 */
  uint32_t *dst; size_t dst_stride;         /* [ch][t] */
  const int *order, *source_of;             /* [n_channels] */
  uint32_t *phase; const uint32_t *dphi;    /* [n_channels] */
  const float4 *tab;                        /* [TUNE_N] */
  int n_channels, cpw;
  uint32_t n_samples;                       /* a multiple of 4 */
};
constexpr int TUNE_THREADS = 256;
constexpr int TUNE_MAX_CPW = 8;

}  // namespace rdsp_tune

hipError_t rdsp_engine_tune_launch(const rdsp_tune::TuneParams &p, hipStream_t s);

#endif
