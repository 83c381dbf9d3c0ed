/*
 * rdsp_engine_dev.h -- the device pieces that more than one stage of rdsp_engine_t's kernels uses (rdsp_engine.hip maps
 * the image's addresses to the stages and their files): the table oscillator, the cascade on the lanes of a quad, the
 * conversion's division, the walk over a tile and the two roles a lane of a recursive kernel can have.
 *
 * Include this header only from sources compiled with -ffp-contract=off: every fused operation here is written as one
 * (fmaf / fma), and the bits of every other product and sum depend on its not being contracted.
 */
#ifndef RDSP_ENGINE_DEV_H
#define RDSP_ENGINE_DEV_H

#include <hip/hip_runtime.h>
#include <math.h>

#include "rdsp_engine_int.h"

namespace {

using namespace rdsp_eng;

constexpr int PITCH = BS + 1;
constexpr float TWO_PI_F = 6.2831854820251465f;   /* the float the image holds for 2 pi */
constexpr float RAD_PER_HZ = 0.00014247586659621447f; /* 2 pi / 44100, its float */
constexpr int FW = 256, FCH = 8, PW = 256; /* threads, channels per workgroup; PW: threads of the pipelined kernels (four waves, as FW) */

/* the oscillator: sin of a phase in [0, 2 pi) by linear interpolation in the 256-step table, through double as the image does */
/* trunc(RN(a / d)) for a >= 0 and d = the double of the image's 2 pi, without the division: k d is exact for k < 2^16 (a
 * 24-bit d), so floor(a / d) follows from two exact comparisons around the estimate a (1 / d); and the correctly rounded
 * quotient cannot lie across an integer from the true one, because a is either exactly k d or at least an ulp of a away
 * from it, which is more than half an ulp of the quotient (tests/test_host_logic.py walks every k and its neighbours) */
__device__ __forceinline__ int index_of_phase(double a) {
  const double d = (double)TWO_PI_F;
  int k = (int)(a * (1.0 / d));
  if ((double)k * d > a) k--;
  else if ((double)(k + 1) * d <= a) k++;
  return k;
}
__device__ __forceinline__ float table_sin(const float *sine, float ph) {
  const int idx = index_of_phase((double)ph * 65535.0);
  const int hi = (idx >> 8) & 0xff;
  const float lo = (float)(unsigned)(idx & 0xff);
  const float t0 = sine[hi], t1 = sine[hi + 1];
  return (float)fma((double)((t1 - t0) * lo), 0.00390625, (double)t0);
}
/* cos and sin of a phase, each argument wrapped into [0, 2 pi), from the table: the mixers' and the PLL's */
__device__ __forceinline__ void table_cos_sin(const float *sine, float ph, float &c, float &s) {
  float pc = (float)((double)ph + 1.5707963267948966);
  if (pc >= TWO_PI_F) pc -= TWO_PI_F;
  if (pc < 0.0f) pc += TWO_PI_F;
  c = table_sin(sine, pc);
  float ps = ph >= TWO_PI_F ? ph - TWO_PI_F : ph;
  if (ps < 0.0f) ps += TWO_PI_F;
  s = table_sin(sine, ps);
}
__device__ __forceinline__ float dpp_up1(float v) { /* lane s of a quad takes lane s - 1's value: quad_perm [0,0,1,2] */
  const int w = __builtin_bit_cast(int, v);
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(w, w, 0x90, 0xF, 0xF, false)); /* every lane has a source: `old` is never kept */
}
__device__ __forceinline__ float quick_root_guess(float p) { return __uint_as_float((__float_as_uint(p) >> 1) + 0x1fa00000u + 0x1b4000u + 3886u); }
__device__ __forceinline__ float quick_sqrt1(float p) { const float g = quick_root_guess(p); return (p / g + g) * 0.5f; }
__device__ __forceinline__ float quick_sqrt2(float p) { const float y = quick_sqrt1(p); return (p / y + y) * 0.5f; }

/* ---- stages of a cascade on neighbouring lanes --------------------------------------------------------------------
 * arm_biquad_cascade_df1_f32 runs section after section over the block; the result is the same when sample n enters
 * section s at step n + s.  Lane s of a quad holds section s of one row of the tile (its five coefficients and four
 * state words) and at step i works on sample i - s, taking its input from lane s - 1's previous output (one DPP move):
 * a block costs 131 steps of ONE section instead of 128 of four, and a row occupies four lanes. */
struct Section {
  float b0, b1, b2, a1, a2, x1, x2, y1, y2;
  __device__ __forceinline__ void load(const float *coef5, const float *state4, bool clear) {
    b0 = coef5[0]; b1 = coef5[1]; b2 = coef5[2]; a1 = coef5[3]; a2 = coef5[4];
    x1 = clear ? 0.0f : state4[0]; x2 = clear ? 0.0f : state4[1]; y1 = clear ? 0.0f : state4[2]; y2 = clear ? 0.0f : state4[3];
  }
  __device__ __forceinline__ void store(float *state4) const { state4[0] = x1; state4[1] = x2; state4[2] = y1; state4[3] = y2; }
  __device__ __forceinline__ float eval(float x) const { /* products rounded, summed left to right */
    float y = b0 * x;
    y = y + b1 * x1;
    y = y + b2 * x2;
    y = y + a1 * y1;
    y = y + a2 * y2;
    return y;
  }
  __device__ __forceinline__ void commit(float x, float y) { x2 = x1; x1 = x; y2 = y1; y1 = y; }
};
/* one block of one tile row through the cascade, in place; called by all four lanes of the row's quad */
/* LEAN: the form for the kernels that carry blanker / detector code beside it (fewer registers: two workgroups per CU) */
template <bool LEAN = false>
__device__ __forceinline__ void cascade_row(Section &sec, float *row, int s) {
  float yprev = 0.0f, xnext = row[0];
#pragma unroll 4
  for (int i = 0; i < BS + 3; i++) {
    const int n = i - s;
    const float up = dpp_up1(yprev);
    const float xin = xnext;
    xnext = row[i + 1 < BS ? i + 1 : BS - 1]; /* asked for a step ahead: the read's latency passes behind this step's arithmetic
                                               * (the row is also written below, so the compiler will not move the read itself) */
    const float x = s == 0 ? xin : up;
    const float y = sec.eval(x);
    const bool live = n >= 0 && n < BS;
    if (live) {
      sec.commit(x, y);
      yprev = y;
    }
    if constexpr (LEAN) {
      if (live && s == 3) row[n] = y;
    } else {
      row[(live && s == 3) ? n : BS] = y; /* the last section's lane writes the sample; every other lane the row's spare word */
    }
  }
}
/* the oscillator in two passes: the phase recursion alone (one lane per channel: a float add and the wrap), then cosine,
 * sine and the complex product for every sample of the tile in parallel -- they are pure functions of the phase */
__device__ __forceinline__ void phase_row(float &ph, float inc, float *out) {
  for (int t = 0; t < BS; t++) { /* both wrapped candidates are formed and one value selected: as branches the three cases cost
                                  * the lone wave more instructions (exec-mask bookkeeping) than the arithmetic */
    out[t] = ph;
    ph = ph + inc;
    const float down = ph - TWO_PI_F, up = ph + TWO_PI_F;
    ph = ph > TWO_PI_F ? down : (ph < 0.0f ? up : ph);
  }
}
__device__ __forceinline__ void rotate_sample(const float *sine, float ph, float &x, float &y) {
  float c, s;
  table_cos_sin(sine, ph, c, s);
  const float xi = x, yq = y;
  x = fmaf(xi, c, -(s * yq));
  y = fmaf(yq, c, xi * s);
}

/* v / 32767.0 correctly rounded without the division: q0 = v y, r = v - 32767 q0 (exact, fused), q = q0 + r y with
 * y = RN(1 / 32767) -- equal to the IEEE quotient for every int16 v (tests/test_host_logic.py tries all 65 536) */
__device__ __forceinline__ double over_32767(int v) {
  const double y = 1.0 / 32767.0, x = (double)v;
  const double q0 = x * y;
  return fma(fma(-q0, 32767.0, x), y, q0);
}

/* ---- what the kernels of every stage say the same way ------------------------------------------------------------------ */

/* the walk over a tile of ROWS rows of a block, on LANES lanes: in step j of TILE_STEPS a lane is on element
 * e = lane + LANES j, sample t = e & 127 of row r = e >> 7 -- consecutive lanes on consecutive samples of a row (coalesced
 * in HBM, conflict-free at the tiles' pitch).  The loop itself stays with the pass: with its body handed over as a
 * function object the compiler arranges the passes differently (docs/history.md) */
static_assert(BS == 128, "a tile row is a block of 128 samples");
struct TileAt {
  int r, t;
};
template <int LANES, int ROWS>
constexpr int TILE_STEPS = ROWS * BS / LANES;
template <int LANES>
__device__ __forceinline__ TileAt tile_at(int lane, int j) {
  const int e = lane + LANES * j;
  return {e >> 7, e & 127};
}

/* the cascade role: the lane's quad holds tile row `row` (of ROWS, RPC rows per channel: the rails), the lane its section
 * sct; ch is the row's channel -- the workgroup's last one where the row lies beyond them, and then `valid` is false:
 * such a quad computes like the others and stores nothing */
struct QuadRole {
  int row, sct, ch;
  bool valid;
};
template <int ROWS, int RPC>
__device__ __forceinline__ QuadRole quad_role(int tid, int c0, int n_channels) {
  static_assert(RPC == 1 || RPC == 2, "one row per channel, or its two rails");
  QuadRole q;
  q.row = (tid >> 2) & (ROWS - 1);
  q.sct = tid & 3;
  const int cl = RPC == 2 ? q.row >> 1 : q.row;
  q.ch = min(c0 + cl, n_channels - 1);
  q.valid = c0 + cl < n_channels;
  return q;
}
/* the serial role: lane `first` + sc owns channel c0 + sc's scalars and runs its true recursions (`on`); ch and valid as above */
struct SerialRole {
  bool on, valid;
  int sc, ch;
};
template <int CH>
__device__ __forceinline__ SerialRole serial_role(int tid, int first, int c0, int n_channels) {
  SerialRole r;
  r.on = tid >= first && tid < first + CH;
  r.sc = (tid - first) & (CH - 1);
  r.ch = min(c0 + r.sc, n_channels - 1);
  r.valid = r.on && c0 + r.sc < n_channels;
  return r;
}

}  // namespace

#endif
