/*
 * rdsp_engine_tone.hip -- rdsp_engine_t's CTCSS tone squelch (include/rdsp.h has the definition, rdsp_tone.h the arithmetic): the
 * kernel an NFM group launches behind its meter kernel.  It reads the group's demodulated rows once, writes two records a block
 * and, with the meter on, closes the blocks the carrier gate left open that do not carry the receiver's tone.  Compiled with the
 * engine's flags (-ffp-contract=off).
 *
 * rdsp_engine_tone_kernel has the meter kernel's shape: one wave per channel, four channels a workgroup.  The workgroup first
 * copies the phasor table into LDS, 16 KiB, with one barrier behind the fill; a wave past the last channel leaves behind it.
 * (Reading the table from global memory through the cache instead, with no LDS and no barrier, was built first and measured
 * 0.009 ms more a call of 4096 receivers x 32 blocks: docs/engine.md.)  A half-wave holds one block: lane l of 32 loads samples
 * 4 l ... 4 l + 3 in one 16-byte load, takes their four phasors from the table -- 16-byte LDS reads, a lane's four entries a few
 * apart and a half-wave's within a few hundred --, multiplies and adds them as levels 1 and 2 of both trees, and the 32 lanes
 * exchange with strides 1, 2 (quad permutes), 4, 8 (row mirrors) and 16 (a swizzle inside the half-wave): levels 3 ... 7.  Eight blocks are loaded before the first is reduced.  The window recursion then runs wave-uniform
 * over those blocks in block order; lane j keeps block j's records and lanes 0 ... 7 write them; a block the tone closes has its
 * 128 audio words overwritten with zeros by the half-wave that held it, 16 bytes a lane.  A channel without a tone (dphi == 0)
 * writes zero words and zero records and leaves the gate alone.
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_meter.h"
#include "rdsp_engine_tone.h"
#include "rdsp_wave.h"

using namespace rdsp_eng;
using namespace rdsp_tone;

namespace {
constexpr int TW = 256, TCH = TW / 64; /* the meter's workgroup: four waves, four channels */
constexpr int TSTEP = 8;               /* blocks in flight per wave */

__device__ __forceinline__ float swap16(float v) { /* lane ^ 16 inside each 32 lanes: and 0x1f, or 0, xor 0x10 */
  return __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));
}
/* levels 3 ... 7 of the tree over the 32 lanes of a half-wave, the result in every one of them: the meter's exchange */
__device__ __forceinline__ float half_allsum(float v) {
  v += dpp_f<0xB1>(v);  /* quad_perm [1,0,3,2] */
  v += dpp_f<0x4E>(v);  /* quad_perm [2,3,0,1] */
  v += dpp_f<0x141>(v); /* row_half_mirror */
  v += dpp_f<0x140>(v); /* row_mirror */
  v += swap16(v);
  return v;
}
__device__ __forceinline__ float lane_value(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
}  // namespace

__global__ __launch_bounds__(TW) void rdsp_engine_tone_kernel(const ToneParams p) {
  const int lane = (int)threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
  const int ch = (int)blockIdx.x * TCH + ((int)threadIdx.x >> 6);
  __shared__ float4 tab[rdsp_tune::TUNE_N];
  for (int i = (int)threadIdx.x; i < rdsp_tune::TUNE_N; i += TW) tab[i] = p.tab[i];
  __syncthreads(); /* the only barrier: every wave of the workgroup filled its quarter */
  if (ch >= p.n_channels) return;
  uint32_t *w = p.state + (size_t)ch * TONE_WORDS;
  float *a2_rec = p.a2 + (size_t)ch * p.rec_stride;
  uint8_t *tone_rec = p.tone + (size_t)ch * p.rec_stride;
  const uint32_t dphi = uniform(p.dphi[ch]);
  if (dphi == 0u) { /* no tone: zero words, zero records, the gate is the meter's */
    for (int b = lane; b < p.n_blocks; b += 64) { a2_rec[b] = 0.0f; tone_rec[b] = 0; }
    if (lane < TONE_WORDS) w[lane] = 0u;
    return;
  }
  ToneState st;
  st.dphi = uniform(w[TN_DPHI]); st.K = uniform(w[TN_K]); st.ph = uniform(w[TN_PH]);
  st.re = __uint_as_float(uniform(w[TN_RE])); st.im = __uint_as_float(uniform(w[TN_IM]));
  st.cnt = uniform(w[TN_CNT]); st.tone = uniform(w[TN_TONE]); st.a2 = __uint_as_float(uniform(w[TN_A2]));
  tone_start(st, dphi, p.law.K, p.reset != 0);
  const float4 *row = (const float4 *)(p.audio + (size_t)ch * p.audio_stride);
  const bool gated = p.open != nullptr;
  uint8_t *open_rec = gated ? p.open + (size_t)ch * p.open_stride : nullptr;
  int32_t *out = p.out + (size_t)ch * p.out_stride;
  int any = 0;
  for (int b0 = 0; b0 < p.n_blocks; b0 += TSTEP) {
    float4 v[TSTEP / 2];
#pragma unroll
    for (int k = 0; k < TSTEP / 2; k++) {
      const int b = b0 + 2 * k + half;
      v[k] = b < p.n_blocks ? row[(size_t)b * (BLOCK / 4) + l32] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    int was_open = 0; /* lane j: the carrier gate's record of block b0 + j */
    if (gated && lane < TSTEP && b0 + lane < p.n_blocks) was_open = open_rec[b0 + lane];
    float sr[TSTEP / 2], si[TSTEP / 2];
#pragma unroll
    for (int k = 0; k < TSTEP / 2; k++) {
      const uint32_t ph = st.ph + (uint32_t)((2 * k + half) * BLOCK + 4 * l32) * dphi; /* of the lane's first sample */
      float qr, qi;
      tone_quad(tab, ph, dphi, v[k].x, v[k].y, v[k].z, v[k].w, qr, qi);
      sr[k] = half_allsum(qr);
      si[k] = half_allsum(qi);
    }
    float rec_a2 = 0.0f;
    int rec_tone = 0, rec_open = 0;
#pragma unroll
    for (int j = 0; j < TSTEP; j++) {
      if (b0 + j < p.n_blocks) { /* wave-uniform */
        tone_step(st, lane_value(sr[j >> 1], 32 * (j & 1)), lane_value(si[j >> 1], 32 * (j & 1)), p.law);
        if (lane == j) { rec_a2 = st.a2; rec_tone = (int)st.tone; }
        if (gated) {
          const int carrier = __builtin_amdgcn_readlane(was_open, j), both = carrier & (int)st.tone;
          any |= both;
          if (lane == j) rec_open = both;
          if (carrier && !both && half == (j & 1)) { /* newly closed: the half-wave that held the block */
            int32_t *o = out + (size_t)(b0 + j) * BLOCK + 4 * l32;
            if (p.out_vec) *(int4 *)o = make_int4(0, 0, 0, 0);
            else { o[0] = 0; o[1] = 0; o[2] = 0; o[3] = 0; }
          }
        }
      }
    }
    if (lane < TSTEP && b0 + lane < p.n_blocks) {
      a2_rec[b0 + lane] = rec_a2; tone_rec[b0 + lane] = (uint8_t)rec_tone;
      if (gated) open_rec[b0 + lane] = (uint8_t)rec_open;
    }
  }
  if (lane == 0) {
    w[TN_DPHI] = st.dphi; w[TN_K] = st.K; w[TN_PH] = st.ph; w[TN_RE] = __float_as_uint(st.re); w[TN_IM] = __float_as_uint(st.im);
    w[TN_CNT] = st.cnt; w[TN_TONE] = st.tone; w[TN_A2] = __float_as_uint(st.a2);
    if (gated) p.meter_words[(size_t)ch * MT_WORDS + MT_ANY] = __int_as_float(any);
  }
}

hipError_t rdsp_engine_tone_launch(const ToneParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1) return hipSuccess;
  hipLaunchKernelGGL(rdsp_engine_tone_kernel, dim3((unsigned)((p.n_channels + TCH - 1) / TCH)), dim3(TW), 0, s, p);
  return hipGetLastError();
}
