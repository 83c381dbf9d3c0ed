/*
 * rdsp_meter.h -- the arithmetic of rdsp_engine_t's signal meter and squelch (include/rdsp.h has the definition), shared by
 * the kernel (rdsp_engine_meter.hip) and the host program of the tests (tests/host/host_meter_check.cpp).  Compile with
 * -ffp-contract=off: every product and sum below is rounded on its own, the one fused operation is written as fmaf.
 *
 * Per channel and block of 128 samples a[0..127] of the demodulated row:
 *   ms  = tree sum of a[t] a[t] (adjacent pairs in index order, seven levels) x 2^-7
 *   pk  = max |a[t]| (fmaxf)
 *   L  <- fmaf(ms - L > 0 ? attack : decay, ms - L, L)
 *   the gate (open, hang) from L by gate_step
 * A wave computes the tree by an exchange reduction: a lane squares its 4 consecutive samples and adds them as (q0 + q1) +
 * (q2 + q3) (quad_sum: levels 1 and 2), then 32 lanes exchange with strides 1, 2, 4, 8, 16 (levels 3 ... 7).  Float addition
 * is commutative, so both partners of an exchange hold the same bits afterwards and the butterfly is the tree.
 */
#ifndef RDSP_METER_H
#define RDSP_METER_H

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#ifndef RDSP_HD
#define RDSP_HD __host__ __device__ __forceinline__
#endif

namespace rdsp_meter {

constexpr int BLOCK = 128;
constexpr float MS_SCALE = 0.0078125f; /* 1 / 128, exact */
constexpr float ATTACK_DEFAULT = 0.5f, DECAY_DEFAULT = 0.0625f;
constexpr int HANG_MAX = 65535;

/* a group's meter settings */
struct MeterSet {
  float attack, decay, open_ms, close_ms;
  int squelch, hang_blocks;
};
/* a channel's meter state: signal state, three words of a state blob */
struct MeterState {
  float level;
  int32_t open, hang;
};

/* levels 1 and 2 of the tree on four consecutive samples */
RDSP_HD float quad_sum(float a0, float a1, float a2, float a3) { return (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3); }
RDSP_HD float quad_peak(float a0, float a1, float a2, float a3) { return fmaxf(fmaxf(fabsf(a0), fabsf(a1)), fmaxf(fabsf(a2), fabsf(a3))); }
RDSP_HD float mean_square(float tree_sum) { return tree_sum * MS_SCALE; }

RDSP_HD float level_step(float level, float ms, float attack, float decay) {
  const float d = ms - level;
  return fmaf(d > 0.0f ? attack : decay, d, level);
}

/* the gate after the level of a block */
RDSP_HD void gate_step(MeterState &g, const MeterSet &s) {
  if (!s.squelch) { g.open = 1; g.hang = s.hang_blocks; }
  else if (g.level >= s.open_ms) { g.open = 1; g.hang = s.hang_blocks; }
  else if (g.open && g.level >= s.close_ms) g.hang = s.hang_blocks;
  else if (g.open && g.hang > 0) g.hang--;
  else g.open = 0;
}

/* one block of one channel on the host: the tree by halving, in place in q */
inline void block_measure(const float *a, float *ms, float *pk) {
  float q[BLOCK / 4], p = 0.0f;
  for (int i = 0; i < BLOCK / 4; i++) {
    q[i] = quad_sum(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]);
    p = fmaxf(p, quad_peak(a[4 * i], a[4 * i + 1], a[4 * i + 2], a[4 * i + 3]));
  }
  for (int n = BLOCK / 8; n >= 1; n >>= 1)
    for (int i = 0; i < n; i++) q[i] = q[2 * i] + q[2 * i + 1];
  *ms = mean_square(q[0]);
  *pk = p;
}
inline void block_step(MeterState &g, const MeterSet &s, const float *a, float *ms, float *pk) {
  block_measure(a, ms, pk);
  g.level = level_step(g.level, *ms, s.attack, s.decay);
  gate_step(g, s);
}

/* the setters' limits (NaN fails every comparison) */
inline bool coefficients_ok(float attack, float decay) { return attack > 0.0f && attack <= 1.0f && decay > 0.0f && decay <= 1.0f; }
inline bool squelch_ok(float open_ms, float close_ms, int hang_blocks) {
  return close_ms >= 0.0f && close_ms <= open_ms && isfinite(open_ms) && hang_blocks >= 0 && hang_blocks <= HANG_MAX;
}

}  // namespace rdsp_meter

#endif
