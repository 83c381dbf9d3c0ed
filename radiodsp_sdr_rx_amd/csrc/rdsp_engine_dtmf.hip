/*
 * rdsp_engine_dtmf.hip -- rdsp_engine_t's DTMF decoder (include/rdsp.h has the definition, rdsp_dtmf.h the arithmetic): the kernel
 * an NFM group with a DTMF frame length launches behind its other detector kernels.  It reads the group's demodulated rows once
 * and writes four records a block and its own state words; the audio, the meter's records, the gates and the active list are
 * not touched.  Compiled with the engine's flags (-ffp-contract=off).
 *
 * rdsp_engine_dtmf_kernel has the tone-search kernel's shape: one wave per channel, four channels a workgroup, the phasor table
 * a 16 KiB LDS copy behind the only barrier; a wave past the last channel leaves behind it.  Eight blocks a trip: a half-wave
 * holds a block, lane l of 32 loads samples 4 l ... 4 l + 3 in one 16-byte load and adds them as dtmf_quad, so lane 32 h + r
 * holds d[b][r] of the trip's block 2 k + h.  Lane 8 t + j of 64 IS sub-chain j of tone t: its re, im, e (the same in every
 * tone's lane j) and its phase live in registers across the call; the phase (32 cnt + 4 j) dphi_t advances by dphi_t a decimated
 * sample and by 28 dphi_t more to the next block (the uint32 wraps as the product does).  A block's four decimated samples
 * 4 j ... 4 j + 3 reach the lane by four lane permutes: one table look-up and three fmaf each.  The end of a frame is
 * wave-uniform: the sums over j are oct_allsum's three DPP steps (the tree of dtmf_tree8: float addition commutes), the two
 * groups' arg-max and second are butterflies over lane bits 3 and 4 in the order of dtmf_beats, which is total, so a half-wave
 * ends with the same pair; the decision and the digit logic are scalar work on lane 0's and lane 32's values.  Lane l of 16
 * holds ring[l].
 */
#include <hip/hip_runtime.h>

#include "rdsp_engine_dtmf.h"
#include "rdsp_wave.h"

using namespace rdsp_eng;
using namespace rdsp_dtmf;

namespace {
constexpr int DW = 256, DCH = DW / 64; /* the tone kernel's workgroup: four waves, four channels */
constexpr int DSTEP = 8;               /* blocks in flight per wave */

/* dtmf_tree8 over the eight lanes of a tone, the result in every one of them */
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

__global__ __launch_bounds__(DW) void rdsp_engine_dtmf_kernel(const DtmfParams p) {
  const int lane = (int)threadIdx.x & 63, half = lane >> 5, l32 = lane & 31, tone = lane >> 3, sub = lane & 7;
  const int ch = (int)blockIdx.x * DCH + ((int)threadIdx.x >> 6);
  __shared__ float4 tab[rdsp_tune::TUNE_N];
  for (int i = (int)threadIdx.x; i < rdsp_tune::TUNE_N; i += DW) tab[i] = p.tab[i];
  __syncthreads(); /* the only barrier: every wave of the workgroup filled its quarter */
  if (ch >= p.n_channels) return;
  uint32_t *w = p.state + (size_t)ch * DTMF_WORDS;
  const DtmfLaw law = p.law;
  uint32_t dphi = 0u;
#pragma unroll
  for (int t = 0; t < TONES; t++) dphi = tone == t ? law.dphi[t] : dphi;
  /* the detector the call begins with (dtmf_start) */
  const bool fresh = p.reset != 0 || uniform(w[DT_K]) != law.K;
  uint32_t cnt = fresh ? 0u : uniform(w[DT_CNT]);
  DtmfDigit g;
  g.last = fresh ? DTMF_NONE : dtmf_minus1(uniform(w[DT_LAST1]));
  g.run = fresh ? 0u : uniform(w[DT_RUN]);
  g.cur = fresh ? DTMF_NONE : dtmf_minus1(uniform(w[DT_CUR1]));
  g.miss = fresh ? 0u : uniform(w[DT_MISS]);
  g.n_digits = fresh ? 0u : uniform(w[DT_NDIGITS]);
  g.t_blocks = fresh ? 0u : uniform(w[DT_TBLOCKS]);
  float PL = fresh ? 0.0f : __uint_as_float(uniform(w[DT_PL])), PH = fresh ? 0.0f : __uint_as_float(uniform(w[DT_PH]));
  uint32_t ring = fresh || lane >= RING ? 0u : w[DT_RING + lane];
  float re = fresh ? 0.0f : __uint_as_float(w[DT_RE + lane]), im = fresh ? 0.0f : __uint_as_float(w[DT_IM + lane]);
  float e = fresh ? 0.0f : __uint_as_float(w[DT_E + sub]);
  uint32_t ph = ((uint32_t)PER_BLOCK * cnt + (uint32_t)(PER_SUB * sub)) * dphi;
  const float4 *row = (const float4 *)(p.audio + (size_t)ch * p.audio_stride);
  uint8_t *key_rec = p.key + (size_t)ch * p.rec_stride, *new_rec = p.fresh + (size_t)ch * p.rec_stride;
  float *lo_rec = p.lo + (size_t)ch * p.rec_stride, *hi_rec = p.hi + (size_t)ch * p.rec_stride;
  for (int b0 = 0; b0 < p.n_blocks; b0 += DSTEP) {
    float d[DSTEP / 2];
#pragma unroll
    for (int k = 0; k < DSTEP / 2; k++) {
      const int b = b0 + 2 * k + half;
      const float4 v = b < p.n_blocks ? row[(size_t)b * (BLOCK / 4) + l32] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      d[k] = dtmf_quad(v.x, v.y, v.z, v.w);
    }
    uint32_t rec_key = DTMF_NONE, rec_new = DTMF_NONE;
    float rec_lo = 0.0f, rec_hi = 0.0f;
#pragma unroll
    for (int j = 0; j < DSTEP; j++) {
      if (b0 + j < p.n_blocks) { /* wave-uniform */
#pragma unroll
        for (int i = 0; i < PER_SUB; i++) {
          const float x = __shfl(d[j >> 1], 32 * (j & 1) + PER_SUB * sub + i);
          dtmf_mac(tab, ph, x, re, im);
          e = fmaf(x, x, e);
          ph += dphi;
        }
        ph += (uint32_t)(PER_BLOCK - PER_SUB) * dphi;
        cnt += 1u;
        g.t_blocks += 1u;
        uint32_t out = DTMF_NONE;
        if (cnt == law.K) { /* wave-uniform */
          const float P = dtmf_power(oct_allsum(re), oct_allsum(im), law.scale);
          const float E = oct_allsum(e) * law.escale;
          float bp = P;
          int bi = tone;
#pragma unroll
          for (int s = 8; s < 32; s <<= 1) {
            const float op = __shfl_xor(bp, s);
            const int oi = __shfl_xor(bi, s);
            if (dtmf_beats(op, oi, bp, bi)) { bp = op; bi = oi; }
          }
          float sec = tone == bi ? 0.0f : P;
#pragma unroll
          for (int s = 8; s < 32; s <<= 1) {
            const float o = __shfl_xor(sec, s);
            sec = o > sec ? o : sec;
          }
          PL = lane_value(bp, 0); PH = lane_value(bp, 32);
          const int iL = __builtin_amdgcn_readlane(bi, 0), iH = __builtin_amdgcn_readlane(bi, 32);
          const uint32_t sym = dtmf_symbol(PL, iL, lane_value(sec, 0), PH, iH, lane_value(sec, 32), lane_value(E, 0), law);
          out = dtmf_digit(g, sym, law);
          if (out != DTMF_NONE && lane == (int)((g.n_digits - 1u) % RING)) ring = dtmf_ring_word(out, g.t_blocks);
          re = 0.0f; im = 0.0f; e = 0.0f; cnt = 0u;
          ph = (uint32_t)(PER_SUB * sub) * dphi;
        }
        if (lane == j) { rec_key = g.cur; rec_new = out; rec_lo = PL; rec_hi = PH; }
      }
    }
    if (lane < DSTEP && b0 + lane < p.n_blocks) {
      key_rec[b0 + lane] = (uint8_t)rec_key;
      new_rec[b0 + lane] = (uint8_t)rec_new;
      lo_rec[b0 + lane] = rec_lo;
      hi_rec[b0 + lane] = rec_hi;
    }
  }
  w[DT_RE + lane] = __float_as_uint(re);
  w[DT_IM + lane] = __float_as_uint(im);
  if (lane < SUBS) w[DT_E + lane] = __float_as_uint(e);
  if (lane < RING) w[DT_RING + lane] = ring;
  if (lane == 0) {
    w[DT_K] = law.K; w[DT_CNT] = cnt; w[DT_LAST1] = dtmf_plus1(g.last); w[DT_RUN] = g.run; w[DT_CUR1] = dtmf_plus1(g.cur);
    w[DT_MISS] = g.miss; w[DT_NDIGITS] = g.n_digits; w[DT_TBLOCKS] = g.t_blocks;
    w[DT_PL] = __float_as_uint(PL); w[DT_PH] = __float_as_uint(PH);
#pragma unroll
    for (int k = DT_PH + 1; k < DT_RING; k++) w[k] = 0u;
  }
}

hipError_t rdsp_engine_dtmf_launch(const DtmfParams &p, hipStream_t s) {
  if (p.n_channels < 1 || p.n_blocks < 1) return hipSuccess;
  hipLaunchKernelGGL(rdsp_engine_dtmf_kernel, dim3((unsigned)((p.n_channels + DCH - 1) / DCH)), dim3(DW), 0, s, p);
  return hipGetLastError();
}
