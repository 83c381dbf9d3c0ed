/*
 * rdsp_engine_tail.hip -- the tail stage of rdsp_engine_t (rdsp_engine.hip has the engine's narrative and the map of the
 * image's addresses): audio band-pass (0xd944), hang AGC (0xdb58, 0xdc10), ALS line enhancer (0xda24), output (0xebfa).
 * The AGC, the ALS filter and the output word are the pieces of rdsp_engine_laws.h, which the chain's engine-law tail
 * stage (rdsp_tail_engine.hip) calls too; the two kernels here keep their lanes, tiles and HBM layouts.
 * Compiled with -ffp-contract=off: every fused operation below is written as one (fmaf / fma).
 */
#include <hip/hip_runtime.h>
#include <math.h>

#include "rdsp_engine_dev.h"
#include "rdsp_engine_laws.h"
#include "rdsp_sync.h"

namespace {

static_assert(BS == RDSP_BLOCK, "the tail kernels hand rdsp_engine_laws.h rows of BS samples");

/* ---- tail: audio band-pass (0xd944), AGC (0xdb58), ALS (0xda24), output (0xebfa) -------------------------------------
 * Per block: the audio cascade with a quad per channel (wave 0); the AGC's envelope -- the only true recursion in it -- on
 * one lane per channel (wave 1), which leaves for every sample the envelope value its gain is looked up from (or "none
 * yet": the gain carried in); gain, clamp and pack are then pure functions and run on all lanes. */

/* block b of the workgroup's TCH channels comes into the tile, on LANES lanes */
template <int LANES, int TCH>
__device__ __forceinline__ void tail_load_block(const EngParams &p, int c0, int lane, int b, float (*ta)[PITCH]) {
  for (int j = 0; j < TILE_STEPS<LANES, TCH>; j++) {
    const auto [r, t] = tile_at<LANES>(lane, j);
    ta[r][t] = c0 + r < p.n_channels ? p.audio[(size_t)(c0 + r) * p.audio_stride + (size_t)b * BS + t] : 0.0f;
  }
}
/* block b leaves: gain by the curve and clamp (0xdc10; GAIN: where the tile does not hold them yet), then 0xebfa: x output
 * gain x 32767 toward zero, the low half-word, on both outputs */
template <int LANES, int TCH, bool GAIN>
__device__ __forceinline__ void tail_out_block(const EngParams &p, int c0, int lane, int b, const float (*ta)[PITCH], const float (*ge)[PITCH],
                                               const float *g_in, const float *curve) {
  for (int j = 0; j < TILE_STEPS<LANES, TCH>; j++) {
    const auto [r, t] = tile_at<LANES>(lane, j);
    float y = ta[r][t];
    if (GAIN && p.agc_on) y = agc_gain_clamp(p.agc, curve, ge[r][t], g_in[r], y);
    if (c0 + r < p.n_channels) p.out[(size_t)(c0 + r) * p.out_stride + (size_t)b * BS + t] = engine_out_word(y, p.output_gain, p.mute);
  }
}

/* With the ALS filter: 16 channels per workgroup of four waves, the passes of a block one after the other; the filter's
 * 55-tap chain on the lanes of a quad (the four samples between two tap moves), taps in registers. */
constexpr int ACH = 16;
__global__ __launch_bounds__(FW, 2) void rdsp_engine_tail_kernel(const EngParams p) {
  __shared__ float ta[ACH][PITCH];
  __shared__ float ge[ACH][PITCH];
  __shared__ float curve[130];
  __shared__ float g_in[ACH];
  constexpr int LP = 260;                 /* pitch of a channel's 256-sample ALS line */
  __shared__ float line[ACH][LP];
  const int tid = threadIdx.x, c0 = blockIdx.x * ACH;
  /* quad q.row on channel c0 + q.row: wave 0's quads run its audio cascade (lane = section), wave 1's its ALS filter (the
   * lane works on every fourth sample) */
  const QuadRole q = quad_role<ACH, 1>(tid, c0, p.n_channels);
  const bool casc = tid < 4 * ACH, als_lane = (tid >> 6) == 1;
  float w[RDSP_ENG_ALS_TAPS];
  Section aud;
  aud.load(p.sets + 20 * p.audio_set + 5 * q.sct, p.st + (size_t)q.ch * NF + ST_AUDIO + 4 * q.sct, (p.resets & RESET_AUDIO) != 0);
  const SerialRole ser = serial_role<ACH>(tid, 64, c0, p.n_channels);
  float *sst = p.st + (size_t)ser.ch * NF + ST_AGC_ENV;
  EngineAgcState agc;
  agc.load(sst);
  for (int i = tid; i < 130; i += FW) curve[i] = p.curve[i];
  if (als_lane) {
    const float *a = p.als + (size_t)q.ch * ALS_WORDS;
    const bool clear = (p.resets & RESET_ALS) != 0;
    for (int i = q.sct; i < 256; i += 4) line[q.row][i] = clear ? 0.0f : a[i];
#pragma unroll
    for (int k = 0; k < RDSP_ENG_ALS_TAPS; k++) w[k] = clear ? 0.0f : a[256 + k];
  }
  for (int b = 0; b < p.n_blocks; b++) {
    __syncthreads();
    tail_load_block<FW, ACH>(p, c0, tid, b, ta);
    __syncthreads();
    if (p.audio_on) {
      if (casc) cascade_row<true>(aud, ta[q.row], q.sct);
      __syncthreads();
    }
    if (p.agc_on) {
      if (ser.on) {
        g_in[ser.sc] = agc.g;
        agc_envelope(agc, p.agc, curve, ta[ser.sc], ge[ser.sc]);
      }
      __syncthreads();
      for (int j = 0; j < TILE_STEPS<FW, ACH>; j++) {
        const auto [r, t] = tile_at<FW>(tid, j); /* in place: the ALS filter takes the block from the tile */
        ta[r][t] = agc_gain_clamp(p.agc, curve, ge[r][t], g_in[r], ta[r][t]);
      }
      __syncthreads();
    }
    /* the line: the previous block, then this one (samples 128 .. 255) */
    if (als_lane) {
      float *x = line[q.row], *rowp = ta[q.row];
      for (int i = q.sct; i < 128; i += 4) { x[i] = x[i + 128]; x[i + 128] = rowp[i]; }
      wg_sync<1>();
      als_block<128>(w, x, rowp, q.sct, p.als_notch, p.als_adaptive);
    }
    __syncthreads();
    tail_out_block<FW, ACH, false>(p, c0, tid, b, ta, ge, g_in, curve);
  }
  if (casc && q.valid) aud.store(p.st + (size_t)q.ch * NF + ST_AUDIO + 4 * q.sct);
  if (ser.valid) agc.store(sst);
  if (als_lane && q.valid) {
    float *a = p.als + (size_t)q.ch * ALS_WORDS;
    for (int i = q.sct; i < 256; i += 4) a[i] = line[q.row][i];
    if (q.sct == 0) {
#pragma unroll
      for (int k = 0; k < RDSP_ENG_ALS_TAPS; k++) a[256 + k] = w[k];
    }
  }
}

/* The tail stage without the ALS filter, 8 channels per workgroup, as a pipeline of waves (see
 * rdsp_engine_front_pipe_kernel): waves 2 and 3 bring block s in and send block s - 3 out (gain by the curve, clamp, pack),
 * wave 0 runs the audio cascade of block s - 1, wave 1 the AGC's envelope of block s - 2. */
constexpr int TCH = 8;
__global__ __launch_bounds__(PW, 2) void rdsp_engine_tail_pipe_kernel(const EngParams p) {
  __shared__ float ta[4][TCH][PITCH];
  __shared__ float ge[4][TCH][PITCH];
  __shared__ float g_in[4][TCH];
  __shared__ float curve[130];
  const int tid = threadIdx.x, wave = tid >> 6, c0 = blockIdx.x * TCH;
  const QuadRole q = quad_role<TCH, 1>(tid, c0, p.n_channels);
  const bool casc = wave == 0 && tid < 4 * TCH;
  Section aud;
  aud.load(p.sets + 20 * p.audio_set + 5 * q.sct, p.st + (size_t)q.ch * NF + ST_AUDIO + 4 * q.sct, (p.resets & RESET_AUDIO) != 0);
  const SerialRole ser = serial_role<TCH>(tid, 64, c0, p.n_channels);
  float *sst = p.st + (size_t)ser.ch * NF + ST_AGC_ENV;
  EngineAgcState agc;
  agc.load(sst);
  for (int i = tid; i < 130; i += PW) curve[i] = p.curve[i];
  const int wl = tid - 128;
  __syncthreads();
  for (int step = 0; step < p.n_blocks + 3; step++) {
    if (wave >= 2) {
      if (step < p.n_blocks) tail_load_block<PW - 128, TCH>(p, c0, wl, step, ta[step & 3]);
      const int b = step - 3;
      if (b >= 0) tail_out_block<PW - 128, TCH, true>(p, c0, wl, b, ta[b & 3], ge[b & 3], g_in[b & 3], curve);
    } else if (wave == 0) {
      const int b = step - 1;
      if (casc && p.audio_on && b >= 0 && b < p.n_blocks) cascade_row(aud, ta[b & 3][q.row], q.sct);
    } else {
      const int b = step - 2;
      if (ser.on && p.agc_on && b >= 0 && b < p.n_blocks) {
        g_in[b & 3][ser.sc] = agc.g;
        agc_envelope(agc, p.agc, curve, ta[b & 3][ser.sc], ge[b & 3][ser.sc]);
      }
    }
    __syncthreads();
  }
  if (casc && q.valid) aud.store(p.st + (size_t)q.ch * NF + ST_AUDIO + 4 * q.sct);
  if (ser.valid) agc.store(sst);
}

}  // namespace

namespace rdsp_eng {
/* which kernel: with the ALS filter 16 channels per workgroup and the passes in sequence, without it 8 and the pipeline
 * (measured: 8 channels are 12 % faster than 16 without the ALS filter, half as fast with it) */
void engine_launch_tail(const EngParams &p, bool als, hipStream_t s) {
  const int tch = als ? ACH : TCH;
  const dim3 g((unsigned)((p.n_channels + tch - 1) / tch));
  if (als) hipLaunchKernelGGL(rdsp_engine_tail_kernel, g, dim3(FW), 0, s, p);
  else hipLaunchKernelGGL(rdsp_engine_tail_pipe_kernel, g, dim3(PW), 0, s, p);
}
}  // namespace rdsp_eng
