/*
 * rdsp_engine_tone_search.hip -- rdsp_engine_t's CTCSS tone search (include/rdsp.h has the definition, rdsp_tone_search.h the
 * arithmetic): the kernel an NFM group with a search window launches behind its tone-squelch kernel.  It reads the group's
 * demodulated rows once and writes three records a block and its own state words; the audio, the meter's records and the active
 * list are not touched.  Compiled with the engine's flags (-ffp-contract=off).
 *
 * rdsp_engine_tone_search_kernel has the tone kernel's shape: one wave per channel, four channels a workgroup, the phasor table
 * a 16 KiB LDS copy behind the only barrier; a wave past the last channel leaves behind it.  Eight blocks a trip: a half-wave
 * holds a block, lane l of 32 loads samples 4 l ... 4 l + 3 in one 16-byte load and adds them as levels 1 and 2 of the
 * decimator's tree; the exchanges with strides 1, 2 (quad permutes) and 4 (row_half_mirror) are levels 3 ... 5, after which the
 * eight lanes 8 q ... 8 q + 7 of a half-wave all hold d[b][q].  Lane t of 64 IS tone t of the bank: its re, im, P and step live
 * in registers across the call, and its phase m dphi_t advances by dphi_t a decimated sample (the uint32 wraps as the product
 * does).  The trip's 32 decimated values reach every lane as wave-uniform operands by readlane, in m order: one table look-up
 * and two fmaf each.  The end of a window is wave-uniform: the arg-max is a butterfly over (P, index) in the order of
 * search_beats, which is total, so every lane ends with the same pair; `next` is a second butterfly once i is known.  Lanes at
 * or above n_tones run with a step of 0 and are masked where they could show: P = 0 there, and zeros are stored.
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_tone_search.h"
#include "rdsp_wave.h"

using namespace rdsp_eng;
using namespace rdsp_tone_search;

namespace {
constexpr int SW = 256, SCH = SW / 64; /* the tone kernel's workgroup: four waves, four channels */
constexpr int SSTEP = 8;               /* blocks in flight per wave */

/* levels 3 ... 5 of the tree over eight lanes, the result in every one of them */
__device__ __forceinline__ float oct_allsum(float v) {
  v += dpp_f<0xB1>(v);  /* quad_perm [1,0,3,2] */
  v += dpp_f<0x4E>(v);  /* quad_perm [2,3,0,1] */
  v += dpp_f<0x141>(v); /* row_half_mirror */
  return v;
}
__device__ __forceinline__ float lane_value(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}
__device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
}  // namespace

__global__ __launch_bounds__(SW) void rdsp_engine_tone_search_kernel(const ToneSearchParams p) {
  const int lane = (int)threadIdx.x & 63, half = lane >> 5, l32 = lane & 31;
  const int ch = (int)blockIdx.x * SCH + ((int)threadIdx.x >> 6);
  __shared__ float4 tab[rdsp_tune::TUNE_N];
  for (int i = (int)threadIdx.x; i < rdsp_tune::TUNE_N; i += SW) tab[i] = p.tab[i];
  __syncthreads(); /* the only barrier: every wave of the workgroup filled its quarter */
  if (ch >= p.n_channels) return;
  uint32_t *w = p.state + (size_t)ch * SEARCH_WORDS;
  const bool active = lane < (int)p.n_tones;
  const uint32_t dphi = p.dphi[lane];
  const SearchLaw law = p.law;
  /* the detector the call begins with (search_start) */
  const bool fresh = p.reset != 0 || uniform(w[TS_K]) != law.K || uniform(w[TS_KEY]) != p.bank_key;
  uint32_t cnt = fresh ? 0u : uniform(w[TS_CNT]), best1 = fresh ? 0u : uniform(w[TS_BEST1]);
  float a2 = fresh ? 0.0f : __uint_as_float(uniform(w[TS_A2])), next = fresh ? 0.0f : __uint_as_float(uniform(w[TS_NEXT]));
  float re = fresh ? 0.0f : __uint_as_float(w[TS_RE + lane]), im = fresh ? 0.0f : __uint_as_float(w[TS_IM + lane]);
  float P = fresh ? 0.0f : __uint_as_float(w[TS_P + lane]);
  uint32_t ph = ((uint32_t)PER_BLOCK * cnt) * dphi;
  const float4 *row = (const float4 *)(p.audio + (size_t)ch * p.audio_stride);
  uint8_t *best_rec = p.best + (size_t)ch * p.rec_stride;
  float *a2_rec = p.a2 + (size_t)ch * p.rec_stride, *next_rec = p.next + (size_t)ch * p.rec_stride;
  for (int b0 = 0; b0 < p.n_blocks; b0 += SSTEP) {
    float d[SSTEP / 2];
#pragma unroll
    for (int k = 0; k < SSTEP / 2; k++) {
      const int b = b0 + 2 * k + half;
      const float4 v = b < p.n_blocks ? row[(size_t)b * (BLOCK / 4) + l32] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      d[k] = oct_allsum(search_quad(v.x, v.y, v.z, v.w));
    }
    uint32_t rec_best = 0u;
    float rec_a2 = 0.0f, rec_next = 0.0f;
#pragma unroll
    for (int j = 0; j < SSTEP; j++) {
      if (b0 + j < p.n_blocks) { /* wave-uniform */
#pragma unroll
        for (int q = 0; q < PER_BLOCK; q++) {
          search_mac(tab, ph, lane_value(d[j >> 1], 32 * (j & 1) + 8 * q), re, im);
          ph += dphi;
        }
        cnt += 1u;
        if (cnt == law.K) { /* wave-uniform */
          P = active ? search_power(re, im, law.scale) : 0.0f;
          float bp = P;
          int bi = lane;
#pragma unroll
          for (int s = 1; s < 64; s <<= 1) {
            const float op = __shfl_xor(bp, s);
            const int oi = __shfl_xor(bi, s);
            if (search_beats(op, oi, bp, bi)) { bp = op; bi = oi; }
          }
          const int i = (int)uniform((uint32_t)bi);
          float nx = (lane < i - 1 || lane > i + 1) ? P : 0.0f;
#pragma unroll
          for (int s = 1; s < 64; s <<= 1) {
            const float o = __shfl_xor(nx, s);
            nx = o > nx ? o : nx;
          }
          a2 = __uint_as_float(uniform(__float_as_uint(bp)));
          next = __uint_as_float(uniform(__float_as_uint(nx)));
          best1 = search_best1(a2, i, next, law);
          re = 0.0f; im = 0.0f; cnt = 0u; ph = 0u;
        }
        if (lane == j) { rec_best = best1; rec_a2 = a2; rec_next = next; }
      }
    }
    if (lane < SSTEP && b0 + lane < p.n_blocks) {
      best_rec[b0 + lane] = (uint8_t)(rec_best - 1u);
      a2_rec[b0 + lane] = rec_a2;
      next_rec[b0 + lane] = rec_next;
    }
  }
  w[TS_RE + lane] = active ? __float_as_uint(re) : 0u;
  w[TS_IM + lane] = active ? __float_as_uint(im) : 0u;
  w[TS_P + lane] = active ? __float_as_uint(P) : 0u;
  if (lane == 0) {
    w[TS_K] = law.K; w[TS_KEY] = p.bank_key; w[TS_CNT] = cnt; w[TS_BEST1] = best1;
    w[TS_A2] = __float_as_uint(a2); w[TS_NEXT] = __float_as_uint(next); w[6] = 0u; w[7] = 0u;
  }
}

hipError_t rdsp_engine_tone_search_launch(const ToneSearchParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1) return hipSuccess;
  hipLaunchKernelGGL(rdsp_engine_tone_search_kernel, dim3((unsigned)((p.n_channels + SCH - 1) / SCH)), dim3(SW), 0, s, p);
  return hipGetLastError();
}
