/*
 * rdsp_tail_engine.hip -- the chain's tail stage under RDSP_TAIL_ENGINE (gfx950): the reference engine's own laws for
 * A9 and A8, in the engine's order, bit for bit with AudioSDR::update's stage taps:
 *
 *   rdsp_tail_engine_kernel   hang AGC (0xdb58: peak envelope with attack / hang / decay, gain by the 130-entry curve,
 *                             x makeup, clamped to +-1), then the ALS line enhancer (0xda24: 55 taps, delay 3, mu 0.5,
 *                             the taps move on the first and every fourth sample of a block), then x output gain and
 *                             the chain's pack -- or the floats alone (rdsp_chain_run_tail_f32)
 *
 * Layout: one wave per workgroup, 16 channels per wave (4096 channels: 256 waves, one per CU).  Both laws are serial in
 * time, so the parallel axes are channels and, where a recursion allows it, samples:
 *   - the AGC's envelope is the only true recursion of the AGC: it runs on one lane per channel and leaves for every
 *     sample the envelope its gain is looked up from (< 0: none yet in this block, the gain carried in); look-up, gain,
 *     clamp and pack are pure functions and run on all 64 lanes;
 *   - the ALS filter runs on a quad per channel: the four samples between two tap moves see the same taps, so each lane
 *     evaluates one sample's chain of 55 fused multiply-adds (the taps in registers, the same in all four lanes), and
 *     every lane then makes the move with the fourth lane's error (quad_perm DPP).
 * The stage bodies are rdsp_engine_laws.h's, the ones rdsp_engine_t's tail kernels (rdsp_engine_tail.hip) call; this kernel
 * runs them on the chain's buffers: float rows at any stride in, int16 L = R pairs (arm_float_to_q15 rounding) and float
 * pairs out, channel sub-batches by ch_base.
 * 180 VGPRs, no scratch.  (Holding the next block in registers through the current one took the kernel to 256 VGPRs
 * + 50 AGPRs: the ALS chain's 55 window loads are hoisted ahead of it.)  Measured cost: DESIGN.md 4.2b.
 *
 * Compiled with -ffp-contract=off, as rdsp_engine_laws.h requires.
 */
#include "rdsp_engine_laws.h"
#include "rdsp_kernels.h"
#include "rdsp_wave.h"

namespace {

constexpr int BS = RDSP_BLOCK;
constexpr int TCH = 16;                   /* channels per wave */
constexpr int H = RDSP_ENG_ALS_HIST;      /* ALS line: H samples of history, then the block */
constexpr int LP = H + BS + 4;            /* pitch of a channel's line in LDS */
constexpr int EP = TCH * BS / 64;         /* elements per lane and block (element e = lane + 64 j: row e / 128, sample e % 128) */

__global__ __launch_bounds__(64) void rdsp_tail_engine_kernel(const RdspTailEngineParams p) {
  __shared__ float line[TCH][LP];
  __shared__ float row[TCH][BS + 1];
  __shared__ float ge[TCH][BS + 1];
  __shared__ float curve[130];
  __shared__ float g_in[TCH];
  if (p.prio == 1) __builtin_amdgcn_s_setprio(1);
  else if (p.prio == 2) __builtin_amdgcn_s_setprio(2);
  else if (p.prio == 3) __builtin_amdgcn_s_setprio(3);
  const int tid = threadIdx.x;
  const int c0 = p.ch_base + blockIdx.x * TCH;
  for (int i = tid; i < 130; i += 64) curve[i] = p.curve[i];

  /* AGC role: lane sc < 16 carries channel c0 + sc's envelope */
  const bool ser = tid < TCH;
  const int sc = tid & (TCH - 1);
  const int sch = min(c0 + sc, p.n_channels - 1);
  float *sst = p.st + (size_t)sch * RDSP_ENG_ST_WORDS;
  EngineAgcState agc;
  agc.load(sst);

  /* ALS role: quad ac on channel c0 + ac, lane aq on every fourth sample */
  const int ac = tid >> 2, aq = tid & 3;
  const int ach = min(c0 + ac, p.n_channels - 1);
  float w[RDSP_ENG_ALS_TAPS];
  if (p.als_on) {
    const float *a = p.als + (size_t)ach * RDSP_ENG_ALS_WORDS;
    for (int i = aq; i < H; i += 4) line[ac][i] = p.als_clear ? 0.0f : a[i];
#pragma unroll
    for (int k = 0; k < RDSP_ENG_ALS_TAPS; k++) w[k] = p.als_clear ? 0.0f : a[H + k];
  }

  for (int b = 0; b < p.n_blocks; b++) {
    /* all of a block's loads in flight at once, then into LDS: rows past the launch's last channel read that channel
     * (computed on, never stored).  Loaded behind a per-row bound check instead, every load waited out its own HBM
     * round trip: 49 us per block at 4096 channels */
    float v[EP];
#pragma unroll
    for (int j = 0; j < EP; j++) {
      const int e = tid + 64 * j, r = e >> 7, t = e & 127;
      v[j] = p.in[(size_t)min(c0 + r, p.n_channels - 1) * p.in_stride + (size_t)b * BS + t];
    }
#pragma unroll
    for (int j = 0; j < EP; j++) {
      const int e = tid + 64 * j;
      row[e >> 7][e & 127] = v[j];
    }
    wg_sync<1>();
    if (p.agc_on) {
      if (ser) {
        g_in[sc] = agc.g;
        agc_envelope(agc, p.agc, curve, row[sc], ge[sc]);
      }
      wg_sync<1>();
#pragma unroll 4
      for (int j = 0; j < EP; j++) {
        const int e = tid + 64 * j, r = e >> 7, t = e & 127;
        row[r][t] = agc_gain_clamp(p.agc, curve, ge[r][t], g_in[r], row[r][t]);
      }
      wg_sync<1>();
    }
    if (p.als_on) {
      /* the line: the newest H samples before the block, then the block */
      float *x = line[ac], *rowp = row[ac];
      if (b > 0)
        for (int i = aq; i < H; i += 4) x[i] = x[i + BS];
      for (int i = aq; i < BS; i += 4) x[H + i] = rowp[i];
      wg_sync<1>();
      als_block<H>(w, x, rowp, aq, p.als_notch, 1);
      wg_sync<1>();
    }
#pragma unroll 4
    for (int j = 0; j < EP; j++) {
      const int e = tid + 64 * j, r = e >> 7, t = e & 127;
      if (c0 + r >= p.n_channels) continue;
      const float y = row[r][t];
      if (p.raw_out) {
        p.raw_out[(size_t)(c0 + r) * p.in_stride + (size_t)b * BS + t] = y;
      } else {
        const float v = y * p.out_gain;
        const size_t o = (size_t)(c0 + r) * p.out_stride + (size_t)b * BS + t;
        p.out_i16[o] = pack_lr(v, v);
        if (p.out_f32) p.out_f32[o] = make_float2(v, v);
      }
    }
    wg_sync<1>();
  }
  if (ser && c0 + sc < p.n_channels) agc.store(sst);
  if (p.als_on && c0 + ac < p.n_channels) {
    float *a = p.als + (size_t)ach * RDSP_ENG_ALS_WORDS;
    for (int i = aq; i < H; i += 4) a[i] = line[ac][i + BS]; /* the newest H samples of the last block */
    if (aq == 0) {
#pragma unroll
      for (int k = 0; k < RDSP_ENG_ALS_TAPS; k++) a[H + k] = w[k];
    }
  }
}

}  // namespace

extern "C" int rdsp_launch_tail_engine(const RdspTailEngineParams *p, hipStream_t stream) {
  if (p->n_blocks <= 0 || p->n_channels <= p->ch_base) return 0;
  const int grid = (p->n_channels - p->ch_base + TCH - 1) / TCH;
  hipLaunchKernelGGL(rdsp_tail_engine_kernel, dim3(grid), dim3(64), 0, stream, *p);
  return (int)hipGetLastError();
}

/* the host half of a launch's parameters: the AGC's constants of set `agc_set` (0: the constructor's, 1 .. 3:
 * setAGCmode's), the makeup gain and the gain curve -- generated here, under this file's -ffp-contract=off, the way
 * rdsp_engine_t generates them */
extern "C" void rdsp_tail_engine_constants(RdspTailEngineParams *p, int agc_set) {
  p->agc = engine_agc_set(agc_set);
  engine_agc_curve(ENGINE_AGC_THRESHOLD_DB, ENGINE_AGC_KNEE_DB, bits_f(ENGINE_AGC_SLOPE_BITS), p->curve);
}
